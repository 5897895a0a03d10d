// bf_range: exact range search -- every base row within radius r of a query (BfRangeLaunch,
// common.hpp).
//
// The scan of bf_query.hip without its K-best list: one wave64 per (query, base slice), the same
// batch loop (16 B/lane chunk loads, partial / group_sum / finish_cos into s_d, one filter word per
// batch in front of the rows), so a pair's distance is bit for bit the one bf_query reports.  Three
// launches on one stream, nothing waits for the host and no atomic decides a position:
//   count   FILL = false: every wave counts its hits, one uint32 per (query, slice)
//   prefix  the counts become exclusive uint64 offsets per (query, slice), and lims[Nq + 1]
//   fill    FILL = true: the same predicate on the same bits; lane j of a batch writes its row at
//           offset + popcount(hits below j), so a query's rows stand in ascending id without a sort.
//           A wave leaves at once when lims[Nq] exceeds the capacity: ids / dists stay untouched.
// Count and fill are one kernel body with one `if constexpr`: they cannot disagree.
#include <algorithm>

#include "bf_common.hpp"
#include "hooks.hpp"
#include "traversal.hpp"

namespace ggnn_amd {

// a.ids / a.dists are the CSR outputs; K, qlist and qcount are not used
struct BfRangeArgs : BfFilteredArgs {
  const float* radii;       // [Nq]
  uint32_t* counts;         // [Nq x slices], written by the count pass
  const uint64_t* offsets;  // [Nq x slices] exclusive, read by the fill pass
  const uint64_t* lims;     // [Nq + 1], read by the fill pass
  uint64_t capacity;
};

template <typename BaseT, int LPR, int NCH, int MODE, bool FILT, bool LAB, bool FILL>
__global__ void __launch_bounds__(kWave) bf_range_kernel(const BfRangeArgs a)
{
  static_assert(FILT || !LAB, "label kernels are filtered kernels");
  constexpr int ROWS = kWave / LPR;
  constexpr int STEPS = StepsOf<LPR, NCH>::value;
  using DE = DistEngine<BaseT, LPR, NCH>;
  using Chunk = typename DE::Chunk;
  __shared__ float s_d[ROWS * STEPS];

  const int lane = threadIdx.x;
  const uint32_t bid = block_linear_index();
  if (bid >= a.Nq * a.slices)
    return;
  const uint32_t n = bid / a.slices;
  const uint32_t slice = bid % a.slices;
  uint64_t offset = 0;
  if constexpr (FILL) {
    // the total does not fit: nothing is written (wave-uniform)
    if (a.lims[a.Nq] > a.capacity)
      return;
    offset = a.offsets[bid];
  }
  const float r = a.radii[n];
  const BaseT* base = static_cast<const BaseT*>(a.base);
  const BaseT* query = static_cast<const BaseT*>(a.query);

  DE de;
  de.template load_query<MODE>(base, a.D, query + static_cast<size_t>(n) * a.D);
  const int grp = lane / LPR;

  uint32_t count = 0;
  const uint32_t begin = slice * a.rows_per_slice;
  const uint32_t end = min(a.N_base, begin + a.rows_per_slice);
  const uint32_t* fbits = bf_wave_filter<(FILT && !LAB)>(a, n);
  const BfLabelFilter flab = bf_wave_labels<LAB>(a, n);
  for (uint32_t i0 = begin; i0 < end; i0 += ROWS * STEPS) {
    const uint32_t fword = bf_word<FILT, LAB>(a, fbits, flab, i0, end);
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
    const uint32_t cnt = min((uint32_t)(ROWS * STEPS), end - i0);
    // NaN on either side of <= is no hit: a NaN radius admits nothing, +inf every non-NaN distance
    const float d = lane < (int)cnt ? s_d[lane] : inf_f();
    const bool hit = lane < (int)cnt && bf_allowed<FILT, LAB>(a, flab, fword, i0) && d <= r;
    const unsigned long long m = __ballot(hit);
    if constexpr (FILL) {
      const uint64_t pos = offset + __popcll(m & ((1ull << lane) - 1ull));
      // (pos < lims[Nq] <= capacity whenever the inputs are those of the count pass)
      if (hit && pos < a.capacity) {
        a.ids[pos] = static_cast<int32_t>(i0 + lane);
        a.dists[pos] = d;
      }
      offset += __popcll(m);
    }
    else
      count += __popcll(m);
  }
  if constexpr (!FILL) {
    if (lane == 0)
      a.counts[bid] = count;
  }
}

// counts [Nq x slices] -> exclusive offsets [Nq x slices] and lims [Nq + 1].  One workgroup: 1024
// queries per round (their slices summed by one thread each, an exclusive scan of the sums in LDS),
// the carry handed from round to round.  Launches have at most a few thousand (query, slice) pairs
// when slices > 1 and one count per query otherwise.
constexpr int kPrefixThreads = 1024;
__global__ void __launch_bounds__(kPrefixThreads)
    bf_range_prefix_kernel(const uint32_t* counts, uint32_t Nq, uint32_t slices, uint64_t* offsets,
                           uint64_t* lims)
{
  __shared__ uint64_t s_sum[kPrefixThreads];
  __shared__ uint64_t s_carry;
  const uint32_t t = threadIdx.x;
  if (t == 0)
    s_carry = 0;
  __syncthreads();
  for (uint32_t n0 = 0; n0 < Nq; n0 += kPrefixThreads) {
    const uint32_t n = n0 + t;
    uint64_t own = 0;
    if (n < Nq)
      for (uint32_t s = 0; s < slices; ++s)
        own += counts[static_cast<size_t>(n) * slices + s];
    // inclusive scan (Hillis-Steele)
    s_sum[t] = own;
    __syncthreads();
    for (uint32_t step = 1; step < kPrefixThreads; step <<= 1) {
      const uint64_t add = t >= step ? s_sum[t - step] : 0;
      __syncthreads();
      s_sum[t] += add;
      __syncthreads();
    }
    const uint64_t carry = s_carry;
    uint64_t off = carry + s_sum[t] - own;
    if (n < Nq) {
      lims[n] = off;
      for (uint32_t s = 0; s < slices; ++s) {
        offsets[static_cast<size_t>(n) * slices + s] = off;
        off += counts[static_cast<size_t>(n) * slices + s];
      }
    }
    __syncthreads();
    if (t == kPrefixThreads - 1)
      s_carry = carry + s_sum[t];
    __syncthreads();
  }
  if (t == 0)
    lims[Nq] = s_carry;
}

template <typename BaseT, int LPR, int NCH, int MODE, bool FILL>
static void launch_bf_range_r(const BfRangeArgs& args, hipStream_t stream)
{
  const dim3 grid = grid_for(static_cast<uint64_t>(args.Nq) * args.slices);
  if (args.filter_bits && args.filter_table.query_labels)
    hipLaunchKernelGGL((bf_range_kernel<BaseT, LPR, NCH, MODE, true, true, FILL>), grid,
                       dim3(kWave), 0, stream, args);
  else if (args.filter_bits)
    hipLaunchKernelGGL((bf_range_kernel<BaseT, LPR, NCH, MODE, true, false, FILL>), grid,
                       dim3(kWave), 0, stream, args);
  else
    hipLaunchKernelGGL((bf_range_kernel<BaseT, LPR, NCH, MODE, false, false, FILL>), grid,
                       dim3(kWave), 0, stream, args);
}

static void launch_bf_range_pass(const BfRangeLaunch& a, const BfRangeArgs& args, bool fill,
                                 hipStream_t stream)
{
#define GGNN_LAUNCH_BF_RANGE(T, LPR, NCH)                                \
  do {                                                                   \
    if (a.measure == GGNN_EUCLIDEAN) {                                   \
      if (fill)                                                          \
        launch_bf_range_r<T, LPR, NCH, kL2, true>(args, stream);         \
      else                                                               \
        launch_bf_range_r<T, LPR, NCH, kL2, false>(args, stream);        \
    }                                                                    \
    else {                                                               \
      if (fill)                                                          \
        launch_bf_range_r<T, LPR, NCH, kCos, true>(args, stream);        \
      else                                                               \
        launch_bf_range_r<T, LPR, NCH, kCos, false>(args, stream);       \
    }                                                                    \
  } while (0)
  GGNN_DISPATCH_DIST(a.dtype, a.D, GGNN_LAUNCH_BF_RANGE);
#undef GGNN_LAUNCH_BF_RANGE
  GGNN_HIP_CHECK(hipGetLastError());
}

void launch_bf_range_query(const BfRangeLaunch& a_in, hipStream_t stream)
{
  GGNN_REQUIRE(a_in.lims != nullptr, GGNN_INVALID_ARGUMENT, "range query: lims is null");
  GGNN_REQUIRE(a_in.capacity == 0 || (a_in.ids != nullptr && a_in.dists != nullptr),
               GGNN_INVALID_ARGUMENT, "range query: ids / dists are null with capacity > 0");
  if (a_in.Nq == 0) {
    GGNN_HIP_CHECK(hipMemsetAsync(a_in.lims, 0, sizeof(uint64_t), stream));
    return;
  }
  GGNN_REQUIRE(a_in.base != nullptr && a_in.query != nullptr && a_in.radii != nullptr,
               GGNN_INVALID_ARGUMENT, "range query: null pointer");
  GGNN_REQUIRE(a_in.N_base >= 1, GGNN_INVALID_ARGUMENT, "range query: the base is empty");
  // what a filtered launch must bring (launch_bf_query's rules)
  GGNN_REQUIRE(!a_in.filter_table.query_labels || (a_in.filter_bits && !a_in.filter_table.ids),
               GGNN_INVALID_ARGUMENT,
               "query labels need the label column and exclude filter ids");
  GGNN_REQUIRE(!a_in.filter_table.query_labels || a_in.N_base <= kMaxLabeledShardRows,
               GGNN_UNSUPPORTED, "label filters need at most 2^30 base vectors per scan");
  const bool table = a_in.filter_bits && a_in.filter_table.ids;
  GGNN_REQUIRE(!table || (a_in.filter_table.words != 0 && a_in.filter_table.num_filters != 0),
               GGNN_INVALID_ARGUMENT, "filter ids need a filter table");
  GGNN_REQUIRE(!a_in.filter_bits || a_in.filter_table.query_labels ||
                   static_cast<uint64_t>(a_in.filter_bit_offset) + a_in.N_base <= 0xffffffffull,
               GGNN_INVALID_ARGUMENT, "filter_bit_offset + N_base must fit 32 bits");
  check_vector_layout(a_in.base, a_in.D, a_in.dtype);
  check_vector_layout(a_in.query, a_in.D, a_in.dtype);
  BfRangeLaunch a = a_in;
  ScratchGuard consts{table ? filter_consts_scratch(a.filter_table, stream) : nullptr, stream};
  if (consts.p)
    a.filter_table.consts = static_cast<const uint32_t*>(consts.p);

  // slices as launch_bf_query chooses them; hook BF_RANGE_SLICES forces the count
  uint32_t slices = 1;
  const int64_t forced = hook(kHookBfRangeSlices);
  if (forced > 0)
    slices = static_cast<uint32_t>(std::min<int64_t>(forced, 64));
  else {
    const uint32_t target_waves = 256 * 16;
    if (a.Nq < target_waves)
      slices = std::min((target_waves + a.Nq - 1) / a.Nq, std::max(1u, a.N_base / 4096u));
  }
  uint32_t rows_per_slice = 0;
  bf_slice_rows(a.N_base, slices, rows_per_slice);

  // counts [Nq x slices] uint32 behind offsets [Nq x slices] uint64, one block of scratch
  const size_t pairs = static_cast<size_t>(a.Nq) * slices;
  ScratchGuard scratch{scratch_alloc(pairs * (sizeof(uint64_t) + sizeof(uint32_t)), stream), stream};
  uint64_t* offsets = static_cast<uint64_t*>(scratch.p);
  uint32_t* counts = reinterpret_cast<uint32_t*>(offsets + pairs);

  BfRangeArgs args{};
  args.base = a.base;
  args.query = a.query;
  args.ids = a.ids;
  args.dists = a.dists;
  args.D = a.D;
  args.Nq = a.Nq;
  args.N_base = a.N_base;
  args.slices = slices;
  args.rows_per_slice = rows_per_slice;
  args.filter_bits = a.filter_bits;
  args.filter_bit_offset = a.filter_bit_offset;
  args.filter_table = a.filter_table;
  args.radii = a.radii;
  args.counts = counts;
  args.offsets = offsets;
  args.lims = a.lims;
  args.capacity = a.capacity;

  launch_bf_range_pass(a, args, /*fill=*/false, stream);
  hipLaunchKernelGGL(bf_range_prefix_kernel, dim3(1), dim3(kPrefixThreads), 0, stream, counts, a.Nq,
                     slices, offsets, a.lims);
  GGNN_HIP_CHECK(hipGetLastError());
  // (capacity 0: the count-only call, and a total of 0 needs no fill)
  if (a.capacity != 0)
    launch_bf_range_pass(a, args, /*fill=*/true, stream);
}

}  // namespace ggnn_amd
