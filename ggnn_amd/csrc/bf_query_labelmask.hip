// bf_query under label-mask filters: the exhaustive scan of bf_query.hip restricted to the rows whose
// label, read as 32 tag bits, passes one of the query's (mask, value, any) clauses and whose bit of the
// query's filter row is set (LabelMaskSpec, common.hpp; LabelMaskFilter in traversal.hpp is the
// traversal's form of the same predicate, and its constructor and passes() serve both).
//
// Kernel templates of their own -- the scan of bf_query_kernel / bf_query_lds_kernel word for word,
// with TWO coalesced words per batch of 64 rows in front of the rows: the row's label and its word of
// the bitset.  A denied row's distance becomes +inf before the ballot.  There is no matrix-core form:
// every label-mask call scans.
#include <cstdlib>

#include "hooks.hpp"
#include "traversal.hpp"

namespace ggnn_amd {

struct BfLabelMaskArgs {
  const void* base;
  const void* query;
  int32_t* ids;  // [slices x Nq x K] partial results (or final when slices == 1)
  float* dists;
  uint32_t D, Nq, N_base, K, slices, rows_per_slice;
  const uint32_t* filter_bits;  // the filter table, or null
  uint32_t filter_bit_offset;   // first global id of this base, in the table and in the column
  FilterTable filter_table;
  LabelMaskSpec mask;
};

// the predicate of one (query, slice) wave: scalar, set up once (LabelMaskFilter's constructor)
struct BfLabelMask {
  const LabelMaskFilter f;
  GGNN_DEV BfLabelMask(const BfLabelMaskArgs& a, const uint32_t n)
      : f(a.filter_bits, a.filter_bit_offset, a.filter_table, a.mask, n)
  {
  }
  // this lane's two words for row i0 + lane of a batch (rows at and above `end`: none, denied below
  // by the caller's count)
  GGNN_DEV void request(const uint32_t i0, const uint32_t end, uint32_t& word, uint32_t& bword) const
  {
    const uint32_t row = i0 + threadIdx.x;
    word = row < end ? filter_word_at(f.labels, row << 2) : 0u;
    bword = row < end ? filter_word_at(f.bits, ((row + f.offset) >> 3) & f.imask) : 0u;
  }
  GGNN_DEV bool allowed(const uint32_t i0, const uint32_t word, const uint32_t bword) const
  {
    return f.passes(word) && ((bword >> ((i0 + threadIdx.x + f.offset) & 31u)) & 1u);
  }
};

// the distances of one batch of ROWS * STEPS rows into s_d (bf_query.hip)
template <typename BaseT, int LPR, int NCH, int MODE, class DE>
GGNN_DEV void bf_labelmask_batch(const DE& de, const uint32_t i0, const uint32_t begin,
                                const uint32_t end, float* s_d)
{
  constexpr int ROWS = kWave / LPR;
  constexpr int STEPS = StepsOf<LPR, NCH>::value;
  using Chunk = typename DE::Chunk;
  const int grp = threadIdx.x / LPR;
  Chunk v[STEPS][NCH];
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    const uint32_t row = i0 + s * ROWS + grp;
    const bool valid = row < end;
    const BaseT* rp = de.row_ptr(valid ? row : begin);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      v[s][c] = ChunkOf<BaseT>::zero();
      if (valid && de.chunk_valid(c))
        v[s][c] = de.load_chunk(rp, c);
    }
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    float x, y;
    de.template partial<MODE>(v[s], x, y);
    x = group_sum<LPR>(x);
    if (MODE == kCos)
      y = group_sum<LPR>(y);
    if (de.g == 0)
      s_d[s * ROWS + grp] = (MODE == kCos) ? de.finish_cos(x, y) : x;
  }
  __syncthreads();
}

template <typename BaseT, int LPR, int NCH, int R, int MODE>
__global__ void __launch_bounds__(kWave) bf_query_labelmask_kernel(const BfLabelMaskArgs a)
{
  constexpr int ROWS = kWave / LPR;
  constexpr int STEPS = StepsOf<LPR, NCH>::value;
  using DE = DistEngine<BaseT, LPR, NCH>;
  __shared__ float s_d[ROWS * STEPS];

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

  const uint32_t begin = slice * a.rows_per_slice;
  const uint32_t end = min(a.N_base, begin + a.rows_per_slice);
  const BfLabelMask filt(a, n);
  for (uint32_t i0 = begin; i0 < end; i0 += ROWS * STEPS) {
    uint32_t word, bword;
    filt.request(i0, end, word, bword);
    bf_labelmask_batch<BaseT, LPR, NCH, MODE>(de, i0, begin, end, s_d);
    // visit the batch in base order (bf_query_layer.cu:52-57); a denied row never enters the list
    const uint32_t cnt = min((uint32_t)(ROWS * STEPS), end - i0);
    const float cd = (lane < (int)cnt && filt.allowed(i0, word, bword)) ? s_d[lane] : inf_f();
    unsigned long long m = __ballot(cd < best.dist_at(a.K - 1));
    while (m) {
      const int j = __ffsll(static_cast<long long>(m)) - 1;
      m &= m - 1;
      const float d = rdlanef(cd, j);
      if (d < best.dist_at(a.K - 1))
        best.push_best_stable(static_cast<int>(i0 + j), d);
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
__global__ void __launch_bounds__(kWave) bf_query_labelmask_lds_kernel(const BfLabelMaskArgs a)
{
  constexpr int ROWS = kWave / LPR;
  constexpr int STEPS = StepsOf<LPR, NCH>::value;
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

  const uint32_t begin = slice * a.rows_per_slice;
  const uint32_t end = min(a.N_base, begin + a.rows_per_slice);
  const BfLabelMask filt(a, n);
  for (uint32_t i0 = begin; i0 < end; i0 += ROWS * STEPS) {
    uint32_t word, bword;
    filt.request(i0, end, word, bword);
    bf_labelmask_batch<BaseT, LPR, NCH, MODE>(de, i0, begin, end, s_d);
    const uint32_t cnt = min((uint32_t)(ROWS * STEPS), end - i0);
    const float cd = (lane < (int)cnt && filt.allowed(i0, word, bword)) ? s_d[lane] : inf_f();
    unsigned long long m = __ballot(cd < best_d[a.K - 1]);
    while (m) {
      const int j = __ffsll(static_cast<long long>(m)) - 1;
      m &= m - 1;
      const float d = rdlanef(cd, j);
      if (!(d < best_d[a.K - 1]))
        continue;
      // stable insert (k_best_list.cuh:77-109): chunks from the right so that every entry is
      // read before it is overwritten
      const int id = static_cast<int>(i0 + j);
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
static void launch_bf_labelmask_r(const BfLabelMaskArgs& args, hipStream_t stream)
{
  const dim3 grid = grid_for(static_cast<uint64_t>(args.Nq) * args.slices);
  if (args.K <= 64)
    hipLaunchKernelGGL((bf_query_labelmask_kernel<BaseT, LPR, NCH, 1, MODE>), grid, dim3(kWave), 0,
                       stream, args);
  else if (args.K <= 128)
    hipLaunchKernelGGL((bf_query_labelmask_kernel<BaseT, LPR, NCH, 2, MODE>), grid, dim3(kWave), 0,
                       stream, args);
  else if (args.K <= 256)
    hipLaunchKernelGGL((bf_query_labelmask_kernel<BaseT, LPR, NCH, 4, MODE>), grid, dim3(kWave), 0,
                       stream, args);
  else
    hipLaunchKernelGGL((bf_query_labelmask_lds_kernel<BaseT, LPR, NCH, MODE>), grid, dim3(kWave),
                       (2 * args.K + 64) * sizeof(int), stream, args);
}

void bf_slice_rows(uint32_t N_base, uint32_t& slices, uint32_t& rows_per_slice);

// launch_bf_query (bf_query.hip) of a launch with label masks
void launch_bf_query_labelmask(const BfLaunch& a, hipStream_t stream)
{
  const LabelMaskSpec& mask = a.label_masks;
  GGNN_REQUIRE(mask.labels != nullptr && mask.masks != nullptr, GGNN_INVALID_ARGUMENT,
               "the label column or the label masks are missing");
  GGNN_REQUIRE(mask.n_masks >= 1 && mask.n_masks <= kMaxLabelMasks, GGNN_INVALID_ARGUMENT,
               "a query has 1 or 2 label mask clauses");
  GGNN_REQUIRE(!a.label_sets.labels && !a.label_ranges.labels, GGNN_INVALID_ARGUMENT,
               "label masks cannot be combined with label sets or label ranges in one launch");
  GGNN_REQUIRE(!a.filter_table.query_labels, GGNN_INVALID_ARGUMENT,
               "label masks exclude the one-label form");
  GGNN_REQUIRE(!a.filter_table.ids || !a.filter_table.num_filters ||
                   (a.filter_bits && a.filter_table.words),
               GGNN_INVALID_ARGUMENT, "filter ids into a table need the table");
  GGNN_REQUIRE(a.dtype != GGNN_I8, GGNN_UNSUPPORTED, "label masks are not built for int8 rows");
  GGNN_REQUIRE(a.N_base <= kMaxLabeledShardRows, GGNN_UNSUPPORTED,
               "label filters need at most 2^30 base vectors per scan");
  check_vector_layout(a.base, a.D, a.dtype);
  check_vector_layout(a.query, a.D, a.dtype);
  GGNN_REQUIRE(a.k_query >= 1 && a.k_query <= 6000, GGNN_INVALID_ARGUMENT,
               "KQuery must be in [1, 6000]");

  // enough waves to fill the chip: split the base into slices when there are few queries
  uint32_t slices = 1;
  const uint32_t target_waves = 256 * 16;
  if (a.Nq < target_waves)
    slices = std::min((target_waves + a.Nq - 1) / a.Nq, std::max(1u, a.N_base / 4096u));
  uint32_t rows_per_slice = 0;
  bf_slice_rows(a.N_base, slices, rows_per_slice);

  int32_t* tmp_ids = nullptr;
  float* tmp_dists = nullptr;
  if (slices > 1) {
    const size_t part = static_cast<size_t>(a.Nq) * slices * a.k_query;
    GGNN_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&tmp_ids), 2 * part * sizeof(int32_t), stream));
    tmp_dists = reinterpret_cast<float*>(tmp_ids + part);
  }

  BfLabelMaskArgs args{};
  args.base = a.base;
  args.query = a.query;
  args.D = a.D;
  args.Nq = a.Nq;
  args.N_base = a.N_base;
  args.K = a.k_query;
  args.slices = slices;
  args.rows_per_slice = rows_per_slice;
  args.filter_bits = a.filter_bits;
  args.filter_bit_offset = a.filter_bit_offset;
  args.filter_table = a.filter_table;
  args.mask = mask;
  args.ids = slices > 1 ? tmp_ids : a.ids;
  args.dists = slices > 1 ? tmp_dists : a.dists;

#define GGNN_LAUNCH_BF(T, LPR, NCH)                            \
  do {                                                         \
    if (a.measure == GGNN_EUCLIDEAN)                           \
      launch_bf_labelmask_r<T, LPR, NCH, kL2>(args, stream);    \
    else                                                       \
      launch_bf_labelmask_r<T, LPR, NCH, kCos>(args, stream);   \
  } while (0)
  if (dtype_is_16bit(a.dtype))
    GGNN_DISPATCH_DIST_16(a.dtype, a.D, GGNN_LAUNCH_BF);
  else
    GGNN_DISPATCH_DIST_32_8(a.dtype, a.D, GGNN_LAUNCH_BF);
#undef GGNN_LAUNCH_BF
  GGNN_HIP_CHECK(hipGetLastError());
  if (slices > 1) {
    // slices are in ascending base order, so "lower part first" on ties keeps Q2
    launch_merge_results_subset(a.Nq, a.k_query, slices, a.k_query, 0, tmp_ids, tmp_dists, a.ids,
                                a.dists, nullptr, nullptr, stream);
    GGNN_HIP_CHECK(hipFreeAsync(tmp_ids, stream));
  }
}

}  // namespace ggnn_amd
