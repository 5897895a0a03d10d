// bf_range for uint8 / int8 rows under squared L2: the verdict of every (query, row) pair comes from
// the integer matrix cores (v_mfma_i32_32x32x32_i8), exactly.  Separate translation unit, compiled like
// bf_i8.hip with -mllvm -amdgpu-mfma-vgpr-form (Makefile): the accumulators and the per-query offset
// block that is their C operand stay in ordinary VGPRs.
//
// Arithmetic contract (why these are the scan's verdicts and the scan's bits).  The scan
// (bf_range_kernel, DistEngine::partial + group_sum, traversal.hpp) forms in every lane the exact
// integer partial (qq + bb) - 2 ab over the lane's chunks -- at most 256 elements, so below 2^24 --
// converts it to float32 and adds the lanes' values IN FLOAT32, as a tree.  With d the pair's exact
// integer distance:
//   * d < 2^24: every partial sum of the tree is an integer below 2^24, nothing rounds, the scan
//     reports exactly (float)d;
//   * d >= 2^24: the scan's value may be rounded, differently per row layout; rounding is monotonic
//     and 2^24 is representable, so the scan's value is still >= 2^24;
//   * d >= 2^24 needs D > 258 (255^2 * 258 < 2^24; int8 rows are the uint8 rows x ^ 0x80).
// For a query with radius r therefore
//   r NaN or r < 0            no hits                                               R = -1
//   r < 2^24                  hit iff the filter admits the row and d <= R,         R = floor(r)
//                             value (float)d: the scan's verdict and bits at any D <= 4096 (a pair with
//                             d >= 2^24 is no hit here and none in the scan, whose value is >= 2^24 > r)
//   r >= 2^24, D <= 258       every admitted row, value (float)d                    R = 2^24
//   r >= 2^24, D > 258        the integer path cannot reproduce the scan's rounded values: the prep
//                             kernel raises the fallback flag, the passes below leave at once and the
//                             scan passes of bf_range.hip -- always enqueued behind, gated by the flag
//                             -- answer the WHOLE call (fell_back = 1)
// No error bound, no candidate buffer, no exact re-evaluation, no compaction, no budget.
//
// Passes, one stream, nothing waits for the host, no atomic decides a position:
//   norms    bf_range_i8_norms_kernel: int32 |b'|^2 per base row (b' = b ^ 0x80 for uint8: squared L2
//            does not change under a common shift; b itself for int8).  Integers, because the float
//            norms of row_norms_kernel stop being exact above 2^24 (D > 1024 at |x| = 128)
//   prep     bf_range_i8_prep_kernel: per query |q'|^2, R, and the fallback flag
//   count    bf_range_i8_kernel<FILL = false>: hits per (query, part), a part being a contiguous,
//            32-aligned row range; parts ascend with the rows
//   prefix   bf_range_prefix_kernel (bf_range.hip): offsets per (query, part) and lims
//   fill     bf_range_i8_kernel<FILL = true>: the same predicate on the same bits; the lane that owns
//            a verdict writes (id, (float)d) at offset + hits so far + set bits below it: ascending id
//
// The tile kernel.  256 threads; wave w owns 64 queries as two 32-query sets that share every B
// operand read from LDS (the bf_i8v2 idea); the workgroup walks its part in 32-row tiles, double
// buffered in LDS at kBfI8RowStride with the row's norm (and label) in the spare bytes of its row.
//   * D <= 128: a stage is FOUR tiles (one barrier per 32 MFMAs of a wave, not per 8; two tiles under
//     a bitset, see bf_range_i8_stage_tiles), the query
//     operand lives in registers (4 x 16 bytes per set), a tile is 4 MFMAs per set, columns past D
//     are zero in the query operand (the base side repeats its last 16 columns against those zeros).
//   * D > 128 (CHUNKED): a stage is one tile x one 128-byte column chunk, all chunks of a tile go into
//     the same i32 accumulators (|q'.b'| <= 128^2 * 4096 = 2^26), the next chunk of the query operand
//     is requested from global memory before the MFMAs of this one.
// Verdict.  d <= R  <=>  2 q'.b' >= c + |b'|^2 with c = |q'|^2 - R.  With hq = c >> 1 and e = c & 1
// the accumulators start at -hq (the C operand of a tile's first MFMA, as bf_i8v2 folds its bound), so
//     acc = q'.b' - hq      and      d <= R  <=>  2 acc - |b'|^2 >= e.
//   fast path: a lane (= one row, 16 queries per set) has no hit unless max(acc) >= ceil(|b'|^2 / 2):
//     eight v_max3_i32 over the 16 accumulators and one compare per set and tile.  May pass a few
//     non-hits (e), never drops a hit.
//   exact path, only for sets whose ballot is non-zero: 2 acc - |b'|^2 >= e per element, the filter,
//     one ballot per accumulator register (32 row verdicts of two queries); d = R + e - (2 acc - |b'|^2).
//   Queries without hits (R = -1, padding) get hq = 2^29: acc < 0.  Rows past the end of a part get
//   the norm 2^28: above every 2 acc.  Neither needs a mask, and nothing overflows:
//   |q'.b'| <= 2^26, -2^23 <= hq <= 2^29, so |2 acc - |b'|^2| < 2^31.
// Lane q of a wave keeps the count of the wave's query q (64 lanes, 64 queries).
#include <algorithm>

#include "bf_common.hpp"
#include "bf_thread_filter.hpp"
#include "hooks.hpp"

namespace ggnn_amd {

constexpr int kRangeI8Queries = 256;     // per workgroup: 4 waves x 2 sets x 32
constexpr int kRangeI8DeadC = 1 << 30;   // c of a query without hits (hq = 2^29, e = 0)
constexpr int kRangeI8PadNorm = 1 << 28;  // norm of a row past the end of its part

struct BfRangeI8Args {
  const void* base;
  const void* query;
  const int32_t* bnorm;   // [N_base] |b'|^2
  const int32_t* qnorm;   // [Nq] |q'|^2
  const int32_t* qR;      // [Nq] R (-1: no hits)
  const uint32_t* flag;   // != 0: the scan answers the call
  uint32_t D, Nq, N_base, parts, rows_per_part;
  uint32_t* counts;         // [Nq x parts], written by the count pass
  const uint64_t* offsets;  // [Nq x parts] exclusive, read by the fill pass
  const uint64_t* lims;     // [Nq + 1], read by the fill pass
  uint64_t capacity;
  int32_t* ids;
  float* dists;
};
struct BfRangeI8FilteredArgs : BfRangeI8Args {
  const uint32_t* filter_bits;  // bitset / filter table / label column (BfRangeLaunch)
  uint32_t filter_bit_offset;   // kBfBits: a multiple of 32
  FilterTable filter_table;
};
template <int FM>
using BfRangeI8ArgsOf = std::conditional_t<FM != kBfNoFilter, BfRangeI8FilteredArgs, BfRangeI8Args>;

// LDS words of the filter area: the layout of bf_filter_lds_words for two blocks of 128 queries --
// kBfBits [2 buffers][tiles per stage][256] verdict words, kBfLabels [256] query labels (the row
// labels sit beside the norms in the tile rows)
constexpr uint32_t bf_range_i8_filter_words(int fm, uint32_t tiles_per_stage)
{
  return 2u * bf_filter_lds_words(fm, fm == kBfBits ? tiles_per_stage : 1u);
}

constexpr int bf_range_i8_stage_tiles(bool chunked, int fm)
{
  return chunked ? 1 : fm == kBfBits ? 2 : 4;
}

// |x'|^2 of one row by 16 lanes (g = lane of the group), every lane of the group gets the sum
template <bool SIGNED>
GGNN_DEV int i8_row_norm(const uint8_t* row, uint32_t D, uint32_t g)
{
  constexpr uint32_t kFlip = SIGNED ? 0u : 0x80808080u;
  int acc = 0;
  for (uint32_t e0 = g * 16; e0 < D; e0 += 256) {
    const uint4 v = *reinterpret_cast<const uint4*>(row + e0);
    const int x = static_cast<int>(v.x ^ kFlip), y = static_cast<int>(v.y ^ kFlip);
    const int z = static_cast<int>(v.z ^ kFlip), w = static_cast<int>(v.w ^ kFlip);
    acc = __builtin_amdgcn_sdot4(x, x, acc, false);
    acc = __builtin_amdgcn_sdot4(y, y, acc, false);
    acc = __builtin_amdgcn_sdot4(z, z, acc, false);
    acc = __builtin_amdgcn_sdot4(w, w, acc, false);
  }
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1)
    acc += __shfl_xor(acc, o);
  return acc;
}

// norms of the base rows; also clears the fallback flag for the prep kernel behind it
template <bool SIGNED>
__global__ void __launch_bounds__(256) bf_range_i8_norms_kernel(const uint8_t* base, uint32_t N,
                                                               uint32_t D, int32_t* bnorm,
                                                               uint32_t* flag)
{
  if (blockIdx.x == 0 && threadIdx.x == 0)
    *flag = 0u;
  const uint32_t g = threadIdx.x & 15;
  for (uint64_t row = static_cast<uint64_t>(blockIdx.x) * 16 + (threadIdx.x >> 4); row < N;
       row += static_cast<uint64_t>(gridDim.x) * 16) {
    const int n = i8_row_norm<SIGNED>(base + row * D, D, g);
    if (g == 0)
      bnorm[row] = n;
  }
}

// per query: |q'|^2, R, the fallback flag (see the top of this file)
template <bool SIGNED>
__global__ void __launch_bounds__(256) bf_range_i8_prep_kernel(const uint8_t* query,
                                                              const float* radii, uint32_t Nq,
                                                              uint32_t D, int32_t* qnorm, int32_t* qR,
                                                              uint32_t* flag, uint32_t* fell_back)
{
  const uint32_t g = threadIdx.x & 15;
  const uint32_t n = blockIdx.x * 16 + (threadIdx.x >> 4);
  if (n >= Nq)
    return;
  const int qn = i8_row_norm<SIGNED>(query + static_cast<size_t>(n) * D, D, g);
  if (g != 0)
    return;
  const float r = radii[n];
  int R = -1;
  if (r >= 0.f) {  // (NaN: no)
    if (r < 16777216.f)
      R = static_cast<int>(r);  // floor: r >= 0
    else if (D <= 258)
      R = 1 << 24;  // above every distance
    else {
      atomicOr(flag, 1u);
      if (fell_back)
        atomicOr(fell_back, 1u);
    }
  }
  qnorm[n] = qn;
  qR[n] = R;
}

// the scan passes wrote lims of their own: they become the call's if the scan answered
__global__ void __launch_bounds__(256) bf_range_i8_take_lims_kernel(const uint32_t* flag,
                                                                   const uint64_t* from, uint32_t n,
                                                                   uint64_t* lims)
{
  if (*flag == 0)
    return;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
    lims[i] = from[i];
}

template <bool SIGNED, int FM, bool FILL, bool CHUNKED>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
    bf_range_i8_kernel(const BfRangeI8ArgsOf<FM> a)
{
  constexpr uint32_t kFlip = SIGNED ? 0u : 0x80808080u;
  // tiles per stage (under a bitset every thread also carries one verdict word per tile of the stage in
  // flight: with four the fill kernel does not fit 256 registers)
  constexpr int TPS = bf_range_i8_stage_tiles(CHUNKED, FM);
  constexpr uint32_t SR = TPS * kBfTileRows;
  constexpr uint32_t stage_bytes = SR * kBfI8RowStride;
  // LEAN: the accumulator offsets -hq are read from LDS into the accumulators for every tile instead
  // of living in 32 VGPRs (bf_i8v2_kernel's register diet).  The chunked kernels, which hold two sets of
  // query operands, and the fill kernels, whose writes need address registers, do not stay inside 256
  // registers without a private segment otherwise; the count kernels of D <= 128 keep the registers
  constexpr bool LEAN = CHUNKED || FILL;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_b[];
  int* cq_l = reinterpret_cast<int*>(lds_b + 2 * stage_bytes);  // [256] c = |q'|^2 - R
  int* nh_l = cq_l + kRangeI8Queries;                           // [256] -hq = -(c >> 1)
  int* R_l = nh_l + kRangeI8Queries;                            // [256]
  // (fill pass: the 256 offsets of this (query block, part))
  uint64_t* off_l = reinterpret_cast<uint64_t*>(R_l + kRangeI8Queries);
  [[maybe_unused]] uint32_t* filt_l = reinterpret_cast<uint32_t*>(off_l + kRangeI8Queries);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;  // matrix layout: base row j of the tile, half h
  if (*a.flag != 0u)  // a radius sent the call to the scan (uniform)
    return;
  if constexpr (FILL) {
    if (a.lims[a.Nq] > a.capacity)  // the total does not fit: nothing is written (uniform)
      return;
  }
  const uint8_t* base = static_cast<const uint8_t*>(a.base);
  const uint8_t* query = static_cast<const uint8_t*>(a.query);
  const uint32_t part = blockIdx.y;
  const uint32_t begin = min(a.N_base, part * a.rows_per_part);
  const uint32_t end = min(a.N_base, begin + a.rows_per_part);
  const uint32_t qw = (blockIdx.x * 4 + wave) * 64;  // first query of this wave
  const uint32_t nch = CHUNKED ? (a.D + 127u) / 128u : 1u;
  const uint32_t nstages = (end - begin + SR - 1) / SR;
  const uint32_t nsteps = nstages * nch;

  // ---- lane = query state: entry tid of the per-query arrays is query qw + lane ----
  const uint32_t my_q = qw + lane;
  const bool my_valid = my_q < a.Nq;
  {
    const int R = my_valid ? a.qR[my_q] : -1;
    const int cq = R >= 0 ? a.qnorm[my_q] - R : kRangeI8DeadC;
    cq_l[tid] = cq;
    nh_l[tid] = -(cq >> 1);
    R_l[tid] = R;
    if constexpr (FILL)
      off_l[tid] = my_valid ? a.offsets[static_cast<size_t>(my_q) * a.parts + part] : 0ull;
    if constexpr (FM == kBfLabels)
      filt_l[tid] = static_cast<uint32_t>(my_valid ? a.filter_table.query_labels[my_q] : -1);
  }
  // kBfBits: the bitset row of this thread's query (padding queries have no hits anyway)
  [[maybe_unused]] const uint32_t* frow = nullptr;
  if constexpr (FM == kBfBits)
    frow = bf_thread_filter_row(a.filter_bits, a.filter_table, my_q, a.Nq);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();

  // ---- matrix layout state ----
  // accumulator register r of half h holds query row (r & 3) + 8 (r >> 2) + 4 h of its set
  // the offsets of set s2 as this lane's accumulators want them
  auto load_offsets = [&](int s2) __attribute__((always_inline)) -> i32x16 {
    const i32x4* p = reinterpret_cast<const i32x4*>(nh_l + wave * 64 + s2 * 32 + 4 * h);
    const i32x4 a0 = p[0], a1 = p[2], a2 = p[4], a3 = p[6];
    return i32x16{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3],
                  a2[0], a2[1], a2[2], a2[3], a3[0], a3[1], a3[2], a3[3]};
  };
  [[maybe_unused]] i32x16 cinit[2];  // (LEAN: unused)
  uint32_t ebits[2];                 // bit r: e of the query of register r
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    if constexpr (!LEAN)
      cinit[s2] = load_offsets(s2);
    ebits[s2] = 0u;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const i32x4 c4 = *reinterpret_cast<const i32x4*>(cq_l + wave * 64 + s2 * 32 + 8 * g + 4 * h);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        ebits[s2] |= static_cast<uint32_t>(c4[e] & 1) << (4 * g + e);
    }
  }
  // the query operand of chunk col0: 16 bytes at column col0 + 32 m + 16 h of query row j of the set
  // (always loaded, from a clamped address; zero past D and for padding queries)
  i32x4 aq[2][4];
  [[maybe_unused]] i32x4 aqn[2][4];
  const uint8_t* qrow[2];
  bool qv[2];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    const uint32_t qi = qw + s2 * 32 + j;
    qv[s2] = qi < a.Nq;
    qrow[s2] = query + static_cast<size_t>(qv[s2] ? qi : 0) * a.D;
  }
  auto query_load = [&](i32x4 (&dst)[2][4], uint32_t col0) __attribute__((always_inline)) {
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const uint32_t col = col0 + 32 * m + 16 * h;
        const uint4 v = *reinterpret_cast<const uint4*>(qrow[s2] + min(col, a.D - 16u));
        dst[s2][m] = i32x4{static_cast<int>(v.x ^ kFlip), static_cast<int>(v.y ^ kFlip),
                           static_cast<int>(v.z ^ kFlip), static_cast<int>(v.w ^ kFlip)};
      }
  };
  auto query_mask = [&](i32x4 (&dst)[2][4], const i32x4 (&src)[2][4], uint32_t col0)
                        __attribute__((always_inline)) {
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const bool ok = qv[s2] && col0 + 32 * m + 16 * h < a.D;
        dst[s2][m] = ok ? src[s2][m] : i32x4{0, 0, 0, 0};
      }
  };

  // ---- staging: a stage is SR rows x 128 bytes = 8 TPS pieces of 16 bytes per row, TPS per thread;
  // threads 0 .. SR - 1 carry the row constants.  Every load is unconditional with a clamped address
  // (bf_i8v2_kernel says why): rows past the end of the part repeat its last row and get the padding
  // norm when the stage is stored, columns past D repeat the last 16 and meet zeros in the query
  uint4 sv[TPS];
  int sbn = 0;
  [[maybe_unused]] uint32_t slab = 0u;
  [[maybe_unused]] uint32_t sfw[TPS];
  auto stage_load = [&](uint32_t row0, uint32_t col0) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < TPS; ++e) {
      const uint32_t p = tid + 256 * e, srow = p >> 3, scol = 16 * (p & 7);
      const uint32_t r = min(row0 + srow, end - 1), c = min(col0 + scol, a.D - 16u);
      sv[e] = *reinterpret_cast<const uint4*>(base + static_cast<size_t>(r) * a.D + c);
    }
    const uint32_t crow = min(row0 + (tid & (SR - 1)), end - 1);
    sbn = a.bnorm[crow];
    if constexpr (FM == kBfLabels)
      slab = filter_word_at(a.filter_bits + a.filter_bit_offset, crow << 2);
    if constexpr (FM == kBfBits) {
      // tiles start at multiples of 32 and so does the bit offset: one word per (query, tile)
#pragma unroll
      for (int t = 0; t < TPS; ++t)
        sfw[t] = frow[(min(row0 + t * kBfTileRows, end - 1) + a.filter_bit_offset) >> 5];
    }
  };
  auto stage_store = [&](uint32_t buf, uint32_t row0) __attribute__((always_inline)) {
    uint8_t* t = lds_b + buf * stage_bytes;
#pragma unroll
    for (int e = 0; e < TPS; ++e) {
      const uint32_t p = tid + 256 * e, srow = p >> 3, scol = 16 * (p & 7);
      *reinterpret_cast<uint4*>(t + srow * kBfI8RowStride + scol) =
          make_uint4(sv[e].x ^ kFlip, sv[e].y ^ kFlip, sv[e].z ^ kFlip, sv[e].w ^ kFlip);
    }
    if (tid < static_cast<int>(SR)) {
      int* rc = reinterpret_cast<int*>(t + tid * kBfI8RowStride + 128);
      rc[0] = (row0 + tid < end) ? sbn : kRangeI8PadNorm;
      if constexpr (FM == kBfLabels)
        rc[1] = static_cast<int>(slab);
    }
    if constexpr (FM == kBfBits) {
#pragma unroll
      for (int tl = 0; tl < TPS; ++tl)
        filt_l[(buf * TPS + tl) * kRangeI8Queries + tid] = sfw[tl];
    }
  };

  uint32_t cnt = 0;  // hits of query qw + lane so far
  // exact verdicts of one set of one tile; wave-uniform control flow throughout
  auto exact = [&](const i32x16& acc, const int s2, const int bnv, const int* rowc, const uint32_t buf,
                   const int t, const uint32_t rowid) __attribute__((always_inline)) {
    [[maybe_unused]] const int row_label = (FM == kBfLabels) ? rowc[1] : 0;
    const int qbase_l = wave * 64 + s2 * 32;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      [[maybe_unused]] i32x4 f4 = i32x4{0, 0, 0, 0};  // verdict words / labels of four queries
      if constexpr (FM == kBfBits)
        f4 = *reinterpret_cast<const i32x4*>(filt_l + (buf * TPS + t) * kRangeI8Queries + qbase_l +
                                             8 * g + 4 * h);
      if constexpr (FM == kBfLabels)
        f4 = *reinterpret_cast<const i32x4*>(filt_l + qbase_l + 8 * g + 4 * h);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * g + e;
        const int qa = s2 * 32 + e + 8 * g, qb = qa + 4;  // queries of the wave in lanes 0..31 / 32..63
        const int tv = 2 * acc[r] - bnv;
        const int ev = static_cast<int>((ebits[s2] >> r) & 1u);
        bool hit = tv >= ev;
        if constexpr (FM == kBfBits)
          hit = hit && ((static_cast<uint32_t>(f4[e]) >> j) & 1u);
        if constexpr (FM == kBfLabels)
          hit = hit && (f4[e] == -1 || f4[e] == row_label);
        const unsigned long long m = __ballot(hit);
        if (m) {
          const uint32_t m_lo = static_cast<uint32_t>(m), m_hi = static_cast<uint32_t>(m >> 32);
          if constexpr (FILL) {
            const uint32_t run_a = __builtin_amdgcn_readlane(static_cast<int>(cnt), qa);
            const uint32_t run_b = __builtin_amdgcn_readlane(static_cast<int>(cnt), qb);
            const uint32_t half = h ? m_hi : m_lo;
            if ((half >> j) & 1u) {
              const int ql = wave * 64 + (h ? qb : qa);
              const uint64_t pos = off_l[ql] + (h ? run_b : run_a) + __popc(half & ((1u << j) - 1u));
              // (pos < lims[Nq] <= capacity whenever the inputs are those of the count pass)
              if (pos < a.capacity) {
                a.ids[pos] = static_cast<int32_t>(rowid);
                a.dists[pos] = static_cast<float>(R_l[ql] + ev - tv);
              }
            }
          }
          cnt += lane == qa ? __popc(m_lo) : lane == qb ? __popc(m_hi) : 0u;
        }
      }
    }
  };

  if (nsteps) {
    stage_load(begin, 0);
    stage_store(0, begin);
  }
  query_load(aqn, 0);
  query_mask(aq, aqn, 0);
  __syncthreads();

  i32x16 acc[2];
  uint32_t st = 0, c = 0;
  for (uint32_t p = 0; p < nsteps; ++p) {
    // the step after this one: the next chunk of the stage, else the first chunk of the next stage
    const bool last_c = c + 1 == nch;
    const uint32_t n_st = last_c ? st + 1 : st, n_c = last_c ? 0u : c + 1;
    const bool has_next = p + 1 < nsteps;
    const uint32_t row0 = begin + st * SR;
    if (has_next)
      stage_load(begin + n_st * SR, n_c * 128);
    if constexpr (CHUNKED) {
      if (has_next)
        query_load(aqn, n_c * 128);
    }
    const uint32_t buf = p & 1;
    const uint8_t* blk = lds_b + buf * stage_bytes;
#pragma unroll
    for (int t = 0; t < TPS; ++t) {
      if (row0 + t * kBfTileRows >= end)
        break;  // uniform
      const uint8_t* trow = blk + (t * kBfTileRows + j) * kBfI8RowStride;
      i32x4 b[4];
#pragma unroll
      for (int m = 0; m < 4; ++m)
        b[m] = *reinterpret_cast<const i32x4*>(trow + 32 * m + 16 * h);
      if (!CHUNKED || c == 0) {
        acc[0] = LEAN ? load_offsets(0) : cinit[0];
        acc[1] = LEAN ? load_offsets(1) : cinit[1];
      }
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(aq[0][m], b[m], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(aq[1][m], b[m], acc[1], 0, 0, 0);
      }
      if (!CHUNKED || last_c) {
        const int* rowc = reinterpret_cast<const int*>(trow + 128);
        const int bnv = rowc[0];
        const int b0 = (bnv + 1) >> 1;
        int mx0 = acc[0][0], mx1 = acc[1][0];
#pragma unroll
        for (int r = 1; r < 16; r += 2) {
          mx0 = max(max(mx0, acc[0][r]), acc[0][(r + 1) & 15]);
          mx1 = max(max(mx1, acc[1][r]), acc[1][(r + 1) & 15]);
        }
        const uint32_t rowid = row0 + t * kBfTileRows + j;
        if (__any(mx0 >= b0))
          exact(acc[0], 0, bnv, rowc, buf, t, rowid);
        if (__any(mx1 >= b0))
          exact(acc[1], 1, bnv, rowc, buf, t, rowid);
      }
    }
    if (has_next)
      stage_store((p + 1) & 1, begin + n_st * SR);
    __syncthreads();
    if constexpr (CHUNKED) {
      if (has_next)
        query_mask(aq, aqn, n_c * 128);
    }
    st = n_st;
    c = n_c;
  }
  if constexpr (!FILL) {
    if (my_valid)
      a.counts[static_cast<size_t>(my_q) * a.parts + part] = cnt;
  }
}

// ---- host -----------------------------------------------------------------------------------------
static int bf_range_i8_filter_mode(const BfRangeLaunch& a)
{
  return !a.filter_bits ? kBfNoFilter : a.filter_table.query_labels ? kBfLabels : kBfBits;
}

bool bf_range_i8_supported(const BfRangeLaunch& a)
{
  const int64_t mode = hook(kHookBfRangeI8);
  if (hook(kHookBfRangePath) == 1 || mode == 1)
    return false;
  if (a.dtype != GGNN_U8 && a.dtype != GGNN_I8)
    return false;
  if (a.measure != GGNN_EUCLIDEAN)
    return false;  // cosine: float norms and dots, not exact above D = 256 -- the scan
  if (a.D == 0 || a.D % 16 != 0 || a.D > 4096)
    return false;
  if (bf_range_i8_filter_mode(a) == kBfBits && a.filter_bit_offset % 32 != 0)
    return false;  // a tile's verdicts must be one word of the bitset
  if (mode == 2)
    return true;
  // count-only and full calls alike: there is no budget to overflow.  From the sweep of DESIGN.md 4.6:
  // at N = 65536 the tiles win all four figures from 256 queries on; at N = 4096 a count-only call of
  // 1024 queries is slower than the scan's single pass (0.165 against 0.103 ms)
  return a.Nq >= 256 && a.N_base >= 65536;
}

// dynamic LDS of a tile workgroup: two stages, c / -hq / R / offsets of 256 queries, the filter area
size_t bf_range_i8_lds_bytes(uint32_t D, int fm)
{
  const uint32_t tps = bf_range_i8_stage_tiles(D > 128, fm);
  return 2 * tps * kBfTileRows * kBfI8RowStride +
         kRangeI8Queries * (3 * sizeof(int) + sizeof(uint64_t)) +
         bf_range_i8_filter_words(fm, tps) * sizeof(uint32_t);
}

template <bool SIGNED, int FM>
static void launch_bf_range_i8_tiles(const BfRangeLaunch& a, BfRangeI8ArgsOf<FM> t, bool fill,
                                     uint32_t qblocks, hipStream_t stream)
{
  if constexpr (FM != kBfNoFilter) {
    t.filter_bits = a.filter_bits;
    t.filter_bit_offset = a.filter_bit_offset;
    t.filter_table = a.filter_table;
  }
  const bool chunked = a.D > 128;
  const void* kern =
      fill ? (chunked ? reinterpret_cast<const void*>(&bf_range_i8_kernel<SIGNED, FM, true, true>)
                      : reinterpret_cast<const void*>(&bf_range_i8_kernel<SIGNED, FM, true, false>))
           : (chunked ? reinterpret_cast<const void*>(&bf_range_i8_kernel<SIGNED, FM, false, true>)
                      : reinterpret_cast<const void*>(&bf_range_i8_kernel<SIGNED, FM, false, false>));
  void* kargs[] = {&t};
  GGNN_HIP_CHECK(hipLaunchKernel(kern, dim3(qblocks, t.parts), dim3(256), kargs,
                                 bf_range_i8_lds_bytes(a.D, FM), stream));
}

template <bool SIGNED>
static void launch_bf_range_i8_t(const BfRangeLaunch& a, hipStream_t stream)
{
  const int fm = bf_range_i8_filter_mode(a);
  const uint32_t qblocks = (a.Nq + kRangeI8Queries - 1) / kRangeI8Queries;
  // parts per query: one round of resident workgroups (two per CU: two waves per SIMD); hook
  // BF_RANGE_SLICES forces the count
  uint32_t parts = std::clamp(256u * 2u / qblocks, 1u, 64u);
  if (const int64_t forced = hook(kHookBfRangeSlices); forced > 0)
    parts = static_cast<uint32_t>(std::min<int64_t>(forced, 64));
  uint32_t rows_per_part = (a.N_base + parts - 1) / parts;
  rows_per_part = (rows_per_part + kBfTileRows - 1) / kBfTileRows * kBfTileRows;
  parts = (a.N_base + rows_per_part - 1) / rows_per_part;
  const size_t pairs = static_cast<size_t>(a.Nq) * parts;

  auto pad4 = [](size_t words) { return (words + 3) / 4 * 4; };
  const size_t n_b = pad4(a.N_base), n_q = pad4(a.Nq), n_pairs = pad4(pairs);
  const size_t n_lims = pad4(2 * (static_cast<size_t>(a.Nq) + 1));
  // [row norms][query norms][R][flag][counts][offsets (uint64)][the scan's lims (uint64)]
  const size_t words = n_b + 2 * n_q + 4 + n_pairs + 2 * n_pairs + n_lims;
  ScratchGuard scratch{scratch_alloc(words * 4, stream), stream};
  int32_t* bnorm = static_cast<int32_t*>(scratch.p);
  int32_t* qnorm = bnorm + n_b;
  int32_t* qR = qnorm + n_q;
  uint32_t* flag = reinterpret_cast<uint32_t*>(qR + n_q);
  uint32_t* counts = flag + 4;
  uint64_t* offsets = reinterpret_cast<uint64_t*>(counts + n_pairs);
  uint64_t* scan_lims = offsets + n_pairs;

  const uint8_t* base = static_cast<const uint8_t*>(a.base);
  const uint8_t* query = static_cast<const uint8_t*>(a.query);
  hipLaunchKernelGGL((bf_range_i8_norms_kernel<SIGNED>),
                     dim3(std::clamp((a.N_base + 15u) / 16u, 1u, 4096u)), dim3(256), 0, stream, base,
                     a.N_base, a.D, bnorm, flag);
  hipLaunchKernelGGL((bf_range_i8_prep_kernel<SIGNED>), dim3((a.Nq + 15) / 16), dim3(256), 0, stream,
                     query, a.radii, a.Nq, a.D, qnorm, qR, flag, a.fell_back);
  GGNN_HIP_CHECK(hipGetLastError());

  BfRangeI8FilteredArgs t{};
  t.base = a.base;
  t.query = a.query;
  t.bnorm = bnorm;
  t.qnorm = qnorm;
  t.qR = qR;
  t.flag = flag;
  t.D = a.D;
  t.Nq = a.Nq;
  t.N_base = a.N_base;
  t.parts = parts;
  t.rows_per_part = rows_per_part;
  t.counts = counts;
  t.offsets = offsets;
  t.lims = a.lims;
  t.capacity = a.capacity;
  t.ids = a.ids;
  t.dists = a.dists;
  auto tile_pass = [&](bool fill) {
    if (fm == kBfBits)
      launch_bf_range_i8_tiles<SIGNED, kBfBits>(a, t, fill, qblocks, stream);
    else if (fm == kBfLabels)
      launch_bf_range_i8_tiles<SIGNED, kBfLabels>(a, t, fill, qblocks, stream);
    else
      launch_bf_range_i8_tiles<SIGNED, kBfNoFilter>(a, static_cast<const BfRangeI8Args&>(t), fill,
                                                    qblocks, stream);
  };
  tile_pass(false);
  launch_bf_range_prefix(counts, a.Nq, parts, offsets, a.lims, stream);
  if (a.capacity != 0)
    tile_pass(true);

  // the scan passes, gated by the flag: they answer the call iff a radius asked for them
  BfRangeLaunch fb = a;
  fb.lims = scan_lims;
  launch_bf_range_scan(fb, flag, stream);
  launch_bf_range_i8_take_lims(flag, scan_lims, a.Nq + 1, a.lims, stream);
}

// (bf_common.hpp: shared with bf_range_i8_cos.hip)
void launch_bf_range_i8_take_lims(const uint32_t* flag, const uint64_t* from, uint32_t n, uint64_t* lims,
                                  hipStream_t stream)
{
  hipLaunchKernelGGL(bf_range_i8_take_lims_kernel, dim3(std::min((n + 255) / 256, 1024u)), dim3(256), 0,
                     stream, flag, from, n, lims);
  GGNN_HIP_CHECK(hipGetLastError());
}

// the int32 row norms alone (bf_common.hpp): shared with the wide-row kernel of bf_query
void launch_bf_i8_row_norms(const void* rows, uint32_t N, uint32_t D, bool is_signed, int32_t* norms,
                            uint32_t* scratch_word, hipStream_t stream)
{
  const dim3 grid(std::clamp((N + 15u) / 16u, 1u, 4096u));
  const uint8_t* r = static_cast<const uint8_t*>(rows);
  if (is_signed)
    hipLaunchKernelGGL((bf_range_i8_norms_kernel<true>), grid, dim3(256), 0, stream, r, N, D, norms,
                       scratch_word);
  else
    hipLaunchKernelGGL((bf_range_i8_norms_kernel<false>), grid, dim3(256), 0, stream, r, N, D, norms,
                       scratch_word);
  GGNN_HIP_CHECK(hipGetLastError());
}

void launch_bf_range_query_i8(const BfRangeLaunch& a, hipStream_t stream)
{
  if (a.dtype == GGNN_I8)
    launch_bf_range_i8_t<true>(a, stream);
  else if (a.dtype == GGNN_U8)
    launch_bf_range_i8_t<false>(a, stream);
  else
    throw Error(GGNN_UNSUPPORTED, "range search: the integer tile kernels take uint8 / int8 rows");
}

}  // namespace ggnn_amd
