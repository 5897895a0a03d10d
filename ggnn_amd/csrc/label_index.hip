// Label index: the label column in CSR form over the global base ids, and the exact search of a
// label's own rows through it ("Label index").
//
//   keys[L]       the distinct labels, ascending (signed)
//   offsets[L+1]  uint32 positions into rows, offsets[0] = 0, offsets[L] = N
//   rows[N]       base ids sorted by (label, id): within a label the ids ascend
//
// label_index_scan_kernel / label_index_scan_lds_kernel are bf_query_kernel / bf_query_lds_kernel
// (bf_query.hip) reading rows through the index: one wave per (query, slice) finds the query's label in
// `keys` (scalar binary search), walks its slice of the segment [offsets[j], offsets[j + 1]) in batches
// of ROWS * STEPS positions, takes the batch's ids with ONE coalesced dword per lane -- the load of
// batch b + 1 is issued in front of the rows of batch b, so that the dependent chain id -> row is
// exposed once per segment -- hands every lane group its row id by a cross-lane read, and computes and
// ranks the distances with the scan's own sequence (partial / group_sum / finish_cos, candidates in
// position order, push_best_stable keyed by the ROW ID).  Positions ascend with the ids, so the result
// is bit for bit what the scan of the whole base gives under the same label: that scan visits the same
// rows in the same order and skips the others.  Label -1 keeps its meaning: the segment is the whole
// base and position p is row p, with no indirection.  A label that is not a key has an empty segment.
//
// Slices cut a segment by position in ascending order; launch_merge_results_subset ("lower part first
// on ties") keeps the tie rule.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "hooks.hpp"
#include "label_index.hpp"

namespace ggnn_amd {

// ---- the index (host) ---------------------------------------------------------------------------------
// One sort of n 64-bit words (label with the sign bit flipped, then the id): the order of a stable
// sort by label, without its second buffer of pairs.
void label_index_build(const int32_t* labels, uint64_t n, int32_t* keys, uint32_t* offsets,
                       int32_t* rows, uint32_t* n_keys)
{
  GGNN_REQUIRE(n >= 1 && n <= kMaxLabeledShardRows, GGNN_INVALID_ARGUMENT,
               "a label index needs between 1 and 2^30 labels");
  GGNN_REQUIRE(labels && keys && offsets && rows && n_keys, GGNN_INVALID_ARGUMENT,
               "label_index_build: null pointer");
  std::vector<uint64_t> order(n);
  for (uint64_t i = 0; i < n; ++i)
    order[i] = (static_cast<uint64_t>(static_cast<uint32_t>(labels[i]) ^ 0x80000000u) << 32) | i;
  std::sort(order.begin(), order.end());
  uint32_t L = 0;
  for (uint64_t p = 0; p < n; ++p) {
    const int32_t label = static_cast<int32_t>(static_cast<uint32_t>(order[p] >> 32) ^ 0x80000000u);
    if (p == 0 || label != keys[L - 1]) {
      keys[L] = label;
      offsets[L] = static_cast<uint32_t>(p);
      ++L;
    }
    rows[p] = static_cast<int32_t>(order[p] & 0xffffffffu);
  }
  offsets[L] = static_cast<uint32_t>(n);
  *n_keys = L;
}

// ---- the scan through the index -------------------------------------------------------------------------
struct LabelIndexArgs {
  const void* base;
  const void* query;
  int32_t* ids;  // [slices x Nq x K] partial results (or final when slices == 1)
  float* dists;
  uint32_t D, Nq, N_base, K, slices;
  const int32_t* keys;
  uint32_t n_keys;
  const uint32_t* offsets;
  const int32_t* rows;
  const int32_t* query_labels;
};

// (label_index_find and label_index_batch: label_index.hpp, shared with label_spans.hip)

// the positions [begin, end) of one (query, slice) wave, scalar; direct: position p is row p (label -1)
struct LabelIndexSpan {
  uint32_t begin, end;
  bool direct;
};
GGNN_DEV LabelIndexSpan label_index_wave_span(const LabelIndexArgs& a, const uint32_t n,
                                              const uint32_t slice)
{
  const int32_t L = __builtin_amdgcn_readfirstlane(a.query_labels[n]);
  uint32_t lo = 0, hi = a.N_base;
  const bool direct = L == -1;
  if (!direct) {
    // scalar control flow: every value of the search is made wave-uniform
    uint32_t x = 0, y = a.n_keys;
    while (x < y) {
      const uint32_t mid = (x + y) >> 1;
      const int32_t key = __builtin_amdgcn_readfirstlane(a.keys[mid]);
      if (key < L)
        x = mid + 1;
      else
        y = mid;
    }
    lo = hi = 0;
    if (x < a.n_keys && __builtin_amdgcn_readfirstlane(a.keys[x]) == L) {
      lo = __builtin_amdgcn_readfirstlane(a.offsets[x]);
      hi = __builtin_amdgcn_readfirstlane(a.offsets[x + 1]);
      // (an index is at most N_base positions long: never read rows[] behind it)
      hi = min(hi, a.N_base);
      lo = min(lo, hi);
    }
  }
  const uint32_t len = hi - lo;
  // multiple of ROWS * STEPS for every configuration, as bf_slice_rows
  uint32_t per = (len + a.slices - 1) / a.slices;
  per = (per + 63u) & ~63u;
  const uint32_t first = min(len, slice * per);
  return LabelIndexSpan{lo + first, lo + min(len, first + per), direct};
}

// this lane's row id for position p0 + lane of a batch of B positions: one coalesced dword, or the
// position itself.  -1: no row (behind the span, or an id outside the base: never addressed)
template <int B>
GGNN_DEV int label_index_ids(const LabelIndexArgs& a, const LabelIndexSpan& sp, const uint32_t p0)
{
  const uint32_t p = p0 + threadIdx.x;
  if (static_cast<int>(threadIdx.x) >= B || p >= sp.end)
    return -1;
  const int id = sp.direct ? static_cast<int>(p) : a.rows[p];
  return static_cast<uint32_t>(id) < a.N_base ? id : -1;
}

template <typename BaseT, int LPR, int NCH, int R, int MODE>
__global__ void __launch_bounds__(kWave) label_index_scan_kernel(const LabelIndexArgs a)
{
  constexpr int ROWS = kWave / LPR;
  constexpr int STEPS = StepsOf<LPR, NCH>::value;
  constexpr int B = ROWS * STEPS;
  using DE = DistEngine<BaseT, LPR, NCH>;
  __shared__ float s_d[B];

  const int lane = threadIdx.x;
  const uint32_t bid = block_linear_index();
  if (bid >= a.Nq * a.slices)
    return;
  const uint32_t n = bid / a.slices;
  const uint32_t slice = bid % a.slices;
  const BaseT* base = static_cast<const BaseT*>(a.base);
  const BaseT* query = static_cast<const BaseT*>(a.query);

  DE de;
  de.template load_query<MODE>(base, a.D, query + static_cast<size_t>(n) * a.D);

  SortedList<R> best;  // only key/dist/BEST are used
  best.BEST = a.K;
  best.SORTED = a.K;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    best.key[r] = kEmptyKey;
    best.dist[r] = inf_f();
  }

  const LabelIndexSpan sp = label_index_wave_span(a, n, slice);
  int idn = label_index_ids<B>(a, sp, sp.begin);
  for (uint32_t p0 = sp.begin; p0 < sp.end; p0 += B) {
    const int idv = idn;
    idn = label_index_ids<B>(a, sp, p0 + B);  // the next batch's ids, in front of this batch's rows
    label_index_batch<BaseT, LPR, NCH, MODE>(de, idv, s_d);
    // visit the batch in position order = ascending ids (bf_query_layer.cu:52-57)
    const float cd = (lane < B && idv >= 0) ? s_d[lane] : inf_f();
    unsigned long long m = __ballot(cd < best.dist_at(a.K - 1));
    while (m) {
      const int j = __ffsll(static_cast<long long>(m)) - 1;
      m &= m - 1;
      const float d = rdlanef(cd, j);
      if (d < best.dist_at(a.K - 1))
        best.push_best_stable(rdlane(idv, j), d);
    }
  }

  const size_t out = (static_cast<size_t>(slice) * a.Nq + n) * a.K;  // [slices, Nq, K]
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t i = r * kWave + lane;
    if (i < a.K) {
      a.ids[out + i] = best.key[r];
      a.dists[out + i] = best.dist[r];
    }
  }
}

// k > 256: the K-best list lives in LDS (dists [K] | ids [K]), as in bf_query_lds_kernel
template <typename BaseT, int LPR, int NCH, int MODE>
__global__ void __launch_bounds__(kWave) label_index_scan_lds_kernel(const LabelIndexArgs a)
{
  constexpr int ROWS = kWave / LPR;
  constexpr int STEPS = StepsOf<LPR, NCH>::value;
  constexpr int B = ROWS * STEPS;
  using DE = DistEngine<BaseT, LPR, NCH>;
  extern __shared__ __attribute__((aligned(16))) int lds_raw[];
  float* best_d = reinterpret_cast<float*>(lds_raw);
  int* best_i = lds_raw + a.K;
  float* s_d = reinterpret_cast<float*>(lds_raw + 2 * a.K);

  const int lane = threadIdx.x;
  const uint32_t bid = block_linear_index();
  if (bid >= a.Nq * a.slices)
    return;
  const uint32_t n = bid / a.slices;
  const uint32_t slice = bid % a.slices;
  const BaseT* base = static_cast<const BaseT*>(a.base);
  DE de;
  de.template load_query<MODE>(base, a.D,
                               static_cast<const BaseT*>(a.query) + static_cast<size_t>(n) * a.D);
  for (uint32_t i = lane; i < a.K; i += kWave) {
    best_d[i] = inf_f();
    best_i[i] = kEmptyKey;
  }
  __syncthreads();

  const LabelIndexSpan sp = label_index_wave_span(a, n, slice);
  int idn = label_index_ids<B>(a, sp, sp.begin);
  for (uint32_t p0 = sp.begin; p0 < sp.end; p0 += B) {
    const int idv = idn;
    idn = label_index_ids<B>(a, sp, p0 + B);
    label_index_batch<BaseT, LPR, NCH, MODE>(de, idv, s_d);
    const float cd = (lane < B && idv >= 0) ? s_d[lane] : inf_f();
    unsigned long long m = __ballot(cd < best_d[a.K - 1]);
    while (m) {
      const int j = __ffsll(static_cast<long long>(m)) - 1;
      m &= m - 1;
      const float d = rdlanef(cd, j);
      if (!(d < best_d[a.K - 1]))
        continue;
      // stable insert (k_best_list.cuh:77-109): chunks from the right so that every entry is
      // read before it is overwritten
      const int id = rdlane(idv, j);
      for (int c0 = (static_cast<int>(a.K) - 1) / kWave * kWave; c0 >= 0; c0 -= kWave) {
        const int k = c0 + lane;
        const bool own = k < static_cast<int>(a.K);
        const float cur = own ? best_d[k] : inf_f();
        const float prev = (own && k > 0) ? best_d[k - 1] : -inf_f();
        const int previ = (own && k > 0) ? best_i[k - 1] : kEmptyKey;
        __syncthreads();
        if (own && d < cur) {
          const bool first = !(d < prev);
          best_d[k] = first ? d : prev;
          best_i[k] = first ? id : previ;
        }
        __syncthreads();
      }
    }
  }
  __syncthreads();
  const size_t out = (static_cast<size_t>(slice) * a.Nq + n) * a.K;
  for (uint32_t i = lane; i < a.K; i += kWave) {
    a.ids[out + i] = best_i[i];
    a.dists[out + i] = best_d[i];
  }
}

template <typename BaseT, int LPR, int NCH, int MODE>
static void launch_label_index_r(const LabelIndexArgs& args, hipStream_t stream)
{
  const dim3 grid = grid_for(static_cast<uint64_t>(args.Nq) * args.slices);
  if (args.K <= 64)
    hipLaunchKernelGGL((label_index_scan_kernel<BaseT, LPR, NCH, 1, MODE>), grid, dim3(kWave), 0,
                       stream, args);
  else if (args.K <= 128)
    hipLaunchKernelGGL((label_index_scan_kernel<BaseT, LPR, NCH, 2, MODE>), grid, dim3(kWave), 0,
                       stream, args);
  else if (args.K <= 256)
    hipLaunchKernelGGL((label_index_scan_kernel<BaseT, LPR, NCH, 4, MODE>), grid, dim3(kWave), 0,
                       stream, args);
  else
    hipLaunchKernelGGL((label_index_scan_lds_kernel<BaseT, LPR, NCH, MODE>), grid, dim3(kWave),
                       (2 * args.K + 64) * sizeof(int), stream, args);
}

void launch_label_index_scan(const LabelIndexLaunch& a, hipStream_t stream)
{
  if (a.Nq == 0)
    return;
  GGNN_REQUIRE(a.keys != nullptr && a.offsets != nullptr && a.rows != nullptr,
               GGNN_INVALID_ARGUMENT, "the label index is missing");
  GGNN_REQUIRE(a.query_labels != nullptr, GGNN_INVALID_ARGUMENT, "the query label array is null");
  GGNN_REQUIRE(a.n_keys >= 1 && a.n_keys <= a.N_base, GGNN_INVALID_ARGUMENT,
               "a label index has between 1 and N_base keys");
  GGNN_REQUIRE(a.N_base <= kMaxLabeledShardRows, GGNN_UNSUPPORTED,
               "label filters need at most 2^30 base vectors per scan");
  check_vector_layout(a.base, a.D, a.dtype);
  check_vector_layout(a.query, a.D, a.dtype);
  GGNN_REQUIRE(a.k_query >= 1 && a.k_query <= 6000, GGNN_INVALID_ARGUMENT,
               "KQuery must be in [1, 6000]");

  // enough waves to fill the chip: the longest segment the call can touch (label -1: the base) is cut
  // into slices when there are few queries, as launch_bf_query does; hook LABEL_INDEX_SLICES forces a
  // count
  const uint32_t longest = a.N_base;
  uint32_t slices = 1;
  const uint32_t target_waves = 256 * 16;
  if (a.Nq < target_waves)
    slices = std::min((target_waves + a.Nq - 1) / a.Nq, std::max(1u, longest / 4096u));
  const int64_t forced = hook(kHookLabelIndexSlices);
  if (forced > 0)
    slices = static_cast<uint32_t>(std::min<int64_t>(forced, 64));
  slices = std::max(1u, std::min(slices, 64u));

  int32_t* tmp_ids = nullptr;
  float* tmp_dists = nullptr;
  if (slices > 1) {
    const size_t part = static_cast<size_t>(a.Nq) * slices * a.k_query;
    GGNN_HIP_CHECK(
        hipMallocAsync(reinterpret_cast<void**>(&tmp_ids), 2 * part * sizeof(int32_t), stream));
    tmp_dists = reinterpret_cast<float*>(tmp_ids + part);
  }

  LabelIndexArgs args{};
  args.base = a.base;
  args.query = a.query;
  args.D = a.D;
  args.Nq = a.Nq;
  args.N_base = a.N_base;
  args.K = a.k_query;
  args.slices = slices;
  args.keys = a.keys;
  args.n_keys = a.n_keys;
  args.offsets = a.offsets;
  args.rows = a.rows;
  args.query_labels = a.query_labels;
  args.ids = slices > 1 ? tmp_ids : a.ids;
  args.dists = slices > 1 ? tmp_dists : a.dists;

#define GGNN_LAUNCH_LI(T, LPR, NCH)                          \
  do {                                                       \
    if (a.measure == GGNN_EUCLIDEAN)                         \
      launch_label_index_r<T, LPR, NCH, kL2>(args, stream);  \
    else                                                     \
      launch_label_index_r<T, LPR, NCH, kCos>(args, stream); \
  } while (0)
  GGNN_DISPATCH_DIST(a.dtype, a.D, GGNN_LAUNCH_LI);
#undef GGNN_LAUNCH_LI
  GGNN_HIP_CHECK(hipGetLastError());
  if (slices > 1) {
    // slices are in ascending position = ascending id order, so "lower part first" on ties keeps Q2
    launch_merge_results_subset(a.Nq, a.k_query, slices, a.k_query, 0, tmp_ids, tmp_dists, a.ids,
                                a.dists, nullptr, nullptr, stream);
    GGNN_HIP_CHECK(hipFreeAsync(tmp_ids, stream));
  }
}

// ---- classify: which queries of a batch the index answers ------------------------------------------------
// routed iff label != -1 and the label's segment has at most `cutoff` positions (a label no row carries:
// length 0, routed).  Two launches, no atomics, so the lists are the same for the same input: a flag word
// per 64 queries (one ballot), then ONE workgroup turns the words into the two order-preserving lists
// with a running prefix.
__global__ void __launch_bounds__(kWave)
    label_index_classify_kernel(const int32_t* keys, uint32_t n_keys, const uint32_t* offsets,
                                const int32_t* query_labels, uint32_t Nq, uint32_t cutoff,
                                unsigned long long* flags)
{
  const uint32_t w = block_linear_index();
  const uint32_t n = w * kWave + threadIdx.x;
  bool routed = false;
  if (n < Nq) {
    const int32_t L = query_labels[n];
    if (L != -1) {
      const uint32_t j = label_index_find(keys, n_keys, L);
      const uint32_t len = j < n_keys ? offsets[j + 1] - offsets[j] : 0u;
      routed = len <= cutoff;
    }
  }
  const unsigned long long m = __ballot(routed);
  if (threadIdx.x == 0 && w * kWave < Nq)
    flags[w] = m;
}

constexpr int kCompactThreads = 1024;
__global__ void __launch_bounds__(kCompactThreads)
    label_index_compact_kernel(const unsigned long long* flags, uint32_t Nq, uint32_t* routed_list,
                               uint32_t* rest_list, uint32_t* counts)
{
  __shared__ uint32_t s_wave[kCompactThreads / kWave];
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid % kWave, wid = tid / kWave;
  const uint32_t words = (Nq + kWave - 1) / kWave;
  uint32_t base_routed = 0, base_all = 0;  // the same in every thread
  for (uint32_t w0 = 0; w0 < words; w0 += kCompactThreads) {
    const uint32_t w = w0 + tid;
    const unsigned long long word = w < words ? flags[w] : 0ull;
    const uint32_t valid = w < words ? min(static_cast<uint32_t>(kWave), Nq - w * kWave) : 0u;
    const uint32_t mine = __popcll(word);
    // inclusive prefix inside the wave, then over the waves
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d);
      if (lane >= static_cast<uint32_t>(d))
        incl += up;
    }
    if (lane == kWave - 1)
      s_wave[wid] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t i = 0; i < kCompactThreads / kWave; ++i) {
      const uint32_t c = s_wave[i];
      before += i < wid ? c : 0u;
      total += c;
    }
    __syncthreads();
    // every word in front of this one inside the chunk is full (only the batch's last is not)
    uint32_t r = base_routed + before + incl - mine;
    uint32_t o = (base_all + tid * kWave) - r;
    for (uint32_t b = 0; b < valid; ++b) {
      const uint32_t q = w * kWave + b;
      if ((word >> b) & 1ull)
        routed_list[r++] = q;
      else
        rest_list[o++] = q;
    }
    base_routed += total;
    base_all = min(Nq, base_all + kCompactThreads * kWave);
  }
  if (tid == 0) {
    counts[0] = base_routed;
    counts[1] = Nq - base_routed;
  }
}

void launch_label_index_classify(const int32_t* keys, uint32_t n_keys, const uint32_t* offsets,
                                 const int32_t* query_labels, uint32_t Nq, uint32_t cutoff,
                                 uint32_t* routed_list, uint32_t* rest_list, uint32_t* counts,
                                 hipStream_t stream)
{
  GGNN_REQUIRE(counts != nullptr, GGNN_INVALID_ARGUMENT, "label_index_classify: null pointer");
  if (!Nq) {
    GGNN_HIP_CHECK(hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), stream));
    return;
  }
  GGNN_REQUIRE(keys && offsets && query_labels && routed_list && rest_list, GGNN_INVALID_ARGUMENT,
               "label_index_classify: null pointer");
  GGNN_REQUIRE(n_keys >= 1, GGNN_INVALID_ARGUMENT, "a label index has at least one key");
  const uint32_t words = (Nq + kWave - 1) / kWave;
  ScratchGuard flags{scratch_alloc(words * sizeof(unsigned long long), stream), stream};
  hipLaunchKernelGGL(label_index_classify_kernel, grid_for(words), dim3(kWave), 0, stream, keys,
                     n_keys, offsets, query_labels, Nq, cutoff,
                     static_cast<unsigned long long*>(flags.p));
  GGNN_HIP_CHECK(hipGetLastError());
  launch_label_index_compact(static_cast<const unsigned long long*>(flags.p), Nq, routed_list,
                             rest_list, counts, stream);
}

void launch_label_index_compact(const unsigned long long* flags, uint32_t Nq, uint32_t* routed_list,
                                uint32_t* rest_list, uint32_t* counts, hipStream_t stream)
{
  hipLaunchKernelGGL(label_index_compact_kernel, dim3(1), dim3(kCompactThreads), 0, stream, flags,
                     Nq, routed_list, rest_list, counts);
  GGNN_HIP_CHECK(hipGetLastError());
}

}  // namespace ggnn_amd
