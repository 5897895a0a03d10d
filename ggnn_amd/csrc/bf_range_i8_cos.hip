// bf_range for uint8 / int8 rows under cosine: the verdict of every (query, row) pair comes from the
// exact integer dot product of the integer matrix cores (v_mfma_i32_32x32x32_i8), a conservative float
// pre-test and the scan's own expression on the outputs that pass it.  Separate translation unit,
// compiled like bf_range_i8.hip with -mllvm -amdgpu-mfma-vgpr-form (Makefile).
//
// Arithmetic contract (why these are the scan's verdicts and the scan's bits).  The scan's value of a
// pair (bf_range_kernel, DistEngine::partial / finish_cos, traversal.hpp) is
//     value = (qn * bn > 0) ? fabsf(1 - dot / sqrtf(qn * bn)) : 1        (float32, operation by operation)
// with dot = (float) sum o q, bn = (float) sum o^2, qn = (float) sum q^2: three integers that the scan
// holds exactly while they stay below 2^24 (always for uint8 at D <= 258 and int8 at D < 1024).  A pair is
// a hit iff the filter admits the row and value <= r; a NaN radius and a negative one admit nothing, +inf
// admits every admitted row.
//   * The 2^24 rule.  If any base row has sum o^2 >= 2^24 (the records pass leaves the maximum in a device
//     word) or any query whose radius can have hits (r >= 0) has sum q^2 >= 2^24, the prep kernel raises
//     the fallback flag: the tile passes leave at once and the scan passes of bf_range.hip -- always
//     enqueued behind, gated by the flag -- answer the WHOLE call (fell_back = 1).  |dot| < 2^24 follows
//     from the two norms (Cauchy-Schwarz).
//   * The exact dot.  int8 rows enter the signed instruction as they are.  uint8 rows enter flipped
//     (x' = x ^ 0x80 = x - 128), and  sum o q = q'.b' + 128 sum b' + (128 sum q' + 16384 D):  the query's
//     term is the accumulators' initial block, the row's term a word of the row's record in LDS (the
//     records of bf_i8cos_records_kernel, bf_common.hpp).  Every intermediate is below 2^31.
//   * Two-level verdict.  Every output meets  fmaf((float)dot, rinv[row], -c[query]) >= 0  first, with
//     rinv = fl(1 / sqrtf(bn)) (0 for a zero row) and, u = 2^-24,
//         c = ((1 - r) - 16 u) * sqrtf(qn);   c = +inf for a query without hits;   c = -inf for r >= 3.
//     This is the pre-test of bf_i8_cos.hip with T := r, constant for the whole call; that file's header
//     proves that no pair with value <= T fails it (9 u needed, 16 u given, independent of D).  Its two
//     assumptions on T hold for a radius as well: where it uses "T is 0 or >= 2^-24" only the half ulp of
//     T matters, which is <= u T for a normal r and 2^-150 for a subnormal one; where it uses T <= 2, a
//     radius in (2, 3) costs 3 u instead of 2 u (10 u of 16), and from r >= 3 on every value is a hit
//     (value <= 2 + 4 u), which c = -inf says -- as it must for r = +inf, where (1 - r) * 0 is a NaN.
//     Outputs that pass are evaluated with the scan's expression, uncontracted, by the lane that holds
//     the row; the filter and value <= r decide.  Count and fill apply the same predicate to the same bits.
//   * Zero row, zero query: value = 1, a hit iff r >= 1.  The pre-test passes both (0 >= c with c <= -0
//     for r >= 1; c = +-0 for a zero query): see the sibling's header.
//   * Rows past the end of a part carry the record rinv = NaN: every fmaf is a NaN, no compare holds.
//     Dead queries (no hits, padding) carry -c = -inf.  No masks in the steady state.
//
// Passes, one stream, nothing waits for the host, no atomic decides a position:
//   records  launch_bf_i8_cos_records on the base (with the maximum norm) and on the queries
//   prep     bf_range_i8cos_prep_kernel: -c per query, the fallback flag
//   count    bf_range_i8cos_kernel<FILL = false>: hits per (query, part), a part being a contiguous,
//            32-aligned row range; parts ascend with the rows
//   prefix   bf_range_prefix_kernel (bf_range.hip)
//   fill     bf_range_i8cos_kernel<FILL = true>: the lane that owns a verdict bit writes (id, value) at
//            offset + hits so far + set bits below it: ascending id
//   then the gated scan passes and bf_range_i8_take_lims_kernel (bf_range_i8.hip).
//
// The tile kernel.  bf_range_i8_kernel's geometry: 256 threads; wave w owns 64 queries as two 32-query
// sets that share every B operand read from LDS; 32-row tiles, double buffered at kBfI8RowStride with the
// row's record (rinv, sum o^2, row term, label) in the spare 16 bytes of its row.
//   * D <= 128: a stage is four tiles (two under a bitset), the query operand is resident in registers.
//   * D > 128 (CHUNKED): a stage is one tile x one 128-byte column chunk, all chunks of a tile go into the
//     same i32 accumulators, the next chunk of the query operand is requested in front of the MFMAs.
//   Epilogue per set and tile: one integer add (uint8), one convert and one fmaf per output, eight
//   v_max3_f32, one compare, one ballot.  -c lives in 32 registers in matrix order in the count kernels of
//   D <= 128; the chunked kernels (two sets of query operands) and the fill kernels (address registers)
//   read it from LDS per tile, as bf_range_i8_kernel's LEAN forms read their offsets.  The query terms
//   of uint8 are read from LDS into the accumulators for every tile.
// Lane q of a wave keeps the count of the wave's query q (64 lanes, 64 queries).
#include <algorithm>

#include "bf_common.hpp"
#include "bf_thread_filter.hpp"
#include "hooks.hpp"

namespace ggnn_amd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kRangeI8cQueries = 256;                    // per workgroup: 4 waves x 2 sets x 32
constexpr float kRangeI8cSlack = 9.5367431640625e-7f;    // 16 u = 2^-20 (bf_i8_cos.hip's derivation)
constexpr int kRangeI8cPadRinv = 0x7fc00000;             // rinv of a row past the end of its part: NaN

struct BfRangeI8CosArgs {
  const void* base;
  const void* query;
  const int4* brec;      // [N_base] records of the base rows (bf_common.hpp, BfI8CosArgs)
  const int4* qrec;      // [Nq] records of the queries
  const float* nc;       // [Nq] -c
  const float* radii;    // [Nq]
  const uint32_t* flag;  // != 0: the scan answers the call
  uint32_t D, Nq, N_base, parts, rows_per_part;
  uint32_t* counts;         // [Nq x parts], written by the count pass
  const uint64_t* offsets;  // [Nq x parts] exclusive, read by the fill pass
  const uint64_t* lims;     // [Nq + 1], read by the fill pass
  uint64_t capacity;
  int32_t* ids;
  float* dists;
};
struct BfRangeI8CosFilteredArgs : BfRangeI8CosArgs {
  const uint32_t* filter_bits;  // bitset / filter table / label column (BfRangeLaunch)
  uint32_t filter_bit_offset;   // kBfBits: a multiple of 32
  FilterTable filter_table;
};
template <int FM>
using BfRangeI8CosArgsOf =
    std::conditional_t<FM != kBfNoFilter, BfRangeI8CosFilteredArgs, BfRangeI8CosArgs>;

constexpr int bf_range_i8cos_stage_tiles(bool chunked, int fm)
{
  return chunked ? 1 : fm == kBfBits ? 2 : 4;
}
// LDS words of the filter area: kBfBits [2 buffers][tiles per stage][256] verdict words, kBfLabels [256]
// query labels (the row labels sit in the records)
constexpr uint32_t bf_range_i8cos_filter_words(int fm, uint32_t tiles_per_stage)
{
  return fm == kBfBits ? 2u * tiles_per_stage * kRangeI8cQueries : fm == kBfLabels ? kRangeI8cQueries : 0u;
}

// per query: -c, and the fallback flag (see the top of this file)
__global__ void __launch_bounds__(256) bf_range_i8cos_prep_kernel(const int4* qrec, const float* radii,
                                                                 const uint32_t* norm_max, uint32_t Nq,
                                                                 float* nc, uint32_t* flag,
                                                                 uint32_t* fell_back)
{
  const uint32_t n = blockIdx.x * 256 + threadIdx.x;
  if (n >= Nq)
    return;
  const float r = radii[n];
  const uint32_t qn = static_cast<uint32_t>(qrec[n].y);
  bool scan = n == 0 && *norm_max >= (1u << 24);
  float v = -inf_f();  // no hits: c = +inf
  if (r >= 0.f) {      // (NaN: no)
    scan = scan || qn >= (1u << 24);
    v = r >= 3.f ? inf_f() : -(((1.0f - r) - kRangeI8cSlack) * sqrtf(static_cast<float>(qn)));
  }
  nc[n] = v;
  if (scan) {
    atomicOr(flag, 1u);
    if (fell_back)
      atomicOr(fell_back, 1u);
  }
}

template <bool SIGNED, int FM, bool FILL, bool CHUNKED>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
    bf_range_i8cos_kernel(const BfRangeI8CosArgsOf<FM> a)
{
  constexpr uint32_t kFlip = SIGNED ? 0u : 0x80808080u;
  // tiles per stage (under a bitset every thread also carries one verdict word per tile in flight)
  constexpr int TPS = bf_range_i8cos_stage_tiles(CHUNKED, FM);
  constexpr uint32_t SR = TPS * kBfTileRows;
  constexpr uint32_t stage_bytes = SR * kBfI8RowStride;
  constexpr bool NCREG = !CHUNKED && !FILL;  // -c in registers, matrix order
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_b[];
  float* nc_l = reinterpret_cast<float*>(lds_b + 2 * stage_bytes);  // [256] -c
  int* hq_l = reinterpret_cast<int*>(nc_l + kRangeI8cQueries);      // [256] uint8: 128 sum q' + 16384 D
  float* qn_l = reinterpret_cast<float*>(hq_l + kRangeI8cQueries);  // [256] (float) sum q^2
  float* r_l = qn_l + kRangeI8cQueries;                             // [256] radius (NaN: padding)
  // (fill pass: the 256 offsets of this (query block, part))
  uint64_t* off_l = reinterpret_cast<uint64_t*>(r_l + kRangeI8cQueries);
  [[maybe_unused]] uint32_t* filt_l = reinterpret_cast<uint32_t*>(off_l + kRangeI8cQueries);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;  // matrix layout: base row j of the tile, half h
  if (*a.flag != 0u)  // the 2^24 rule sent the call to the scan (uniform)
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
    const int4 qr = my_valid ? a.qrec[my_q] : make_int4(0, 0, 0, 0);
    nc_l[tid] = my_valid ? a.nc[my_q] : -inf_f();
    hq_l[tid] = SIGNED ? 0 : qr.z + 16384 * static_cast<int>(a.D);
    qn_l[tid] = static_cast<float>(qr.y);
    r_l[tid] = my_valid ? a.radii[my_q] : __int_as_float(kRangeI8cPadRinv);
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
  // accumulator register r of half h holds query row (r & 3) + 8 (r >> 2) + 4 h of its set: the four
  // queries of register group g stand at  wave * 64 + s2 * 32 + 8 g + 4 h  of the per-query arrays
  const int qlane0 = wave * 64 + 4 * h;
  auto load_terms = [&](int s2) __attribute__((always_inline)) -> i32x16 {
    const i32x4* p = reinterpret_cast<const i32x4*>(hq_l + qlane0 + s2 * 32);
    const i32x4 a0 = p[0], a1 = p[2], a2 = p[4], a3 = p[6];
    return i32x16{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3],
                  a2[0], a2[1], a2[2], a2[3], a3[0], a3[1], a3[2], a3[3]};
  };
  [[maybe_unused]] f32x4 ncr[2][4];  // (NCREG: -c of the wave's 64 queries as the accumulators want it)
  if constexpr (NCREG) {
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        ncr[s2][g] = *reinterpret_cast<const f32x4*>(nc_l + qlane0 + s2 * 32 + 8 * g);
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
  // threads 0 .. SR - 1 carry the row records.  Every load is unconditional with a clamped address: rows
  // past the end of the part repeat its last row and get the padding record when the stage is stored,
  // columns past D repeat the last 16 and meet zeros in the query operand
  uint4 sv[TPS];
  int4 srec = make_int4(0, 0, 0, 0);
  [[maybe_unused]] uint32_t sfw[TPS];
  auto stage_load = [&](uint32_t row0, uint32_t col0) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < TPS; ++e) {
      const uint32_t p = tid + 256 * e, srow = p >> 3, scol = 16 * (p & 7);
      const uint32_t r = min(row0 + srow, end - 1), c = min(col0 + scol, a.D - 16u);
      sv[e] = *reinterpret_cast<const uint4*>(base + static_cast<size_t>(r) * a.D + c);
    }
    const uint32_t crow = min(row0 + (tid & (SR - 1)), end - 1);
    srec = a.brec[crow];
    if constexpr (FM == kBfLabels)
      srec.w = static_cast<int>(filter_word_at(a.filter_bits + a.filter_bit_offset, crow << 2));
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
    if (tid < static_cast<int>(SR))
      *reinterpret_cast<int4*>(t + tid * kBfI8RowStride + 128) =
          (row0 + tid < end) ? srec : make_int4(kRangeI8cPadRinv, 0, 0, 0);
    if constexpr (FM == kBfBits) {
#pragma unroll
      for (int tl = 0; tl < TPS; ++tl)
        filt_l[(buf * TPS + tl) * kRangeI8cQueries + tid] = sfw[tl];
    }
  };

  uint32_t cnt = 0;  // hits of query qw + lane so far
  // exact verdicts of one set of one tile; wave-uniform control flow throughout
  auto exact = [&](const i32x16& acc, const int s2, const int4 rec, const uint32_t buf, const int t,
                   const uint32_t rowid) __attribute__((always_inline)) {
    const float rinv = __int_as_float(rec.x), bnf = static_cast<float>(rec.y);
    const int qbase_l = wave * 64 + s2 * 32;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int q4 = qbase_l + 8 * g + 4 * h;  // the four queries of this register group
      const f32x4 nc4 = *reinterpret_cast<const f32x4*>(nc_l + q4);
      const f32x4 qn4 = *reinterpret_cast<const f32x4*>(qn_l + q4);
      const f32x4 r4 = *reinterpret_cast<const f32x4*>(r_l + q4);
      [[maybe_unused]] i32x4 f4 = i32x4{0, 0, 0, 0};  // verdict words / labels of four queries
      if constexpr (FM == kBfBits)
        f4 = *reinterpret_cast<const i32x4*>(filt_l + (buf * TPS + t) * kRangeI8cQueries + q4);
      if constexpr (FM == kBfLabels)
        f4 = *reinterpret_cast<const i32x4*>(filt_l + q4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * g + e;
        const int qa = s2 * 32 + e + 8 * g, qb = qa + 4;  // queries of the wave in lanes 0..31 / 32..63
        const float dotf = static_cast<float>(SIGNED ? acc[r] : acc[r] + rec.z);
        const bool pre = fmaf(dotf, rinv, nc4[e]) >= 0.0f;
        if (!__any(pre))
          continue;
        // finish_cos, operation by operation
        const float norm_sqr = qn4[e] * bnf;
        const float v = (norm_sqr > 0.0f) ? fabsf(1.0f - dotf / sqrtf(norm_sqr)) : 1.0f;
        bool hit = pre && v <= r4[e];
        if constexpr (FM == kBfBits)
          hit = hit && ((static_cast<uint32_t>(f4[e]) >> j) & 1u);
        if constexpr (FM == kBfLabels)
          hit = hit && (f4[e] == -1 || f4[e] == rec.w);
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
                a.dists[pos] = v;
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
        // (int8: a block of zeros, read like the uint8 terms)
        acc[0] = load_terms(0);
        acc[1] = load_terms(1);
      }
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(aq[0][m], b[m], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(aq[1][m], b[m], acc[1], 0, 0, 0);
      }
      if (!CHUNKED || last_c) {
        const int4 rec = *reinterpret_cast<const int4*>(trow + 128);
        const float rinv = __int_as_float(rec.x);
        const uint32_t rowid = row0 + t * kBfTileRows + j;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          float f[16];
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            f32x4 n4;
            if constexpr (NCREG)
              n4 = ncr[s2][g];
            else
              n4 = *reinterpret_cast<const f32x4*>(nc_l + qlane0 + s2 * 32 + 8 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int r = 4 * g + e;
              f[r] = fmaf(static_cast<float>(SIGNED ? acc[s2][r] : acc[s2][r] + rec.z), rinv, n4[e]);
            }
          }
          // (a row past the end: sixteen NaNs, their maximum a NaN, the compare false)
          float mx = f[0];
#pragma unroll
          for (int r = 1; r < 16; r += 2)
            mx = fmaxf(fmaxf(mx, f[r]), f[(r + 1) & 15]);
          if (__any(mx >= 0.0f))
            exact(acc[s2], s2, rec, buf, t, rowid);
        }
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
static int bf_range_i8cos_filter_mode(const BfRangeLaunch& a)
{
  return !a.filter_bits ? kBfNoFilter : a.filter_table.query_labels ? kBfLabels : kBfBits;
}

bool bf_range_i8_cos_supported(const BfRangeLaunch& a)
{
  const int64_t mode = hook(kHookBfRangeI8Cos);
  if (hook(kHookBfRangePath) == 1 || mode == 1)
    return false;
  if (a.dtype != GGNN_U8 && a.dtype != GGNN_I8)
    return false;
  if (a.measure != GGNN_COSINE)
    return false;  // squared L2: bf_range_i8.hip
  if (a.D < 16 || a.D % 16 != 0 || a.D > 4096)
    return false;
  if (bf_range_i8cos_filter_mode(a) == kBfBits && a.filter_bit_offset % 32 != 0)
    return false;  // a tile's verdicts must be one word of the bitset
  if (mode == 2)
    return true;
  // From the sweep of DESIGN.md 4.6 (unfiltered calls): the tiles win all four figures at 1024 x 65536 and
  // at 10k x 1M; at 256 x 65536 and 1024 x 4096 they lose the count-only call.  Filtered calls were not
  // measured: they stay under the hook
  return bf_range_i8cos_filter_mode(a) == kBfNoFilter && a.Nq >= 1024 && a.N_base >= 65536;
}

// dynamic LDS of a tile workgroup: two stages, -c / query term / norm / radius / offset of 256 queries,
// the filter area
size_t bf_range_i8_cos_lds_bytes(uint32_t D, int fm)
{
  const uint32_t tps = bf_range_i8cos_stage_tiles(D > 128, fm);
  return 2 * tps * kBfTileRows * kBfI8RowStride +
         kRangeI8cQueries * (4 * sizeof(int) + sizeof(uint64_t)) +
         bf_range_i8cos_filter_words(fm, tps) * sizeof(uint32_t);
}

template <bool SIGNED, int FM>
static void launch_bf_range_i8cos_tiles(const BfRangeLaunch& a, BfRangeI8CosArgsOf<FM> t, bool fill,
                                        uint32_t qblocks, hipStream_t stream)
{
  if constexpr (FM != kBfNoFilter) {
    t.filter_bits = a.filter_bits;
    t.filter_bit_offset = a.filter_bit_offset;
    t.filter_table = a.filter_table;
  }
  const bool chunked = a.D > 128;
  const void* kern =
      fill ? (chunked ? reinterpret_cast<const void*>(&bf_range_i8cos_kernel<SIGNED, FM, true, true>)
                      : reinterpret_cast<const void*>(&bf_range_i8cos_kernel<SIGNED, FM, true, false>))
           : (chunked ? reinterpret_cast<const void*>(&bf_range_i8cos_kernel<SIGNED, FM, false, true>)
                      : reinterpret_cast<const void*>(&bf_range_i8cos_kernel<SIGNED, FM, false, false>));
  void* kargs[] = {&t};
  GGNN_HIP_CHECK(hipLaunchKernel(kern, dim3(qblocks, t.parts), dim3(256), kargs,
                                 bf_range_i8_cos_lds_bytes(a.D, FM), stream));
}

template <bool SIGNED>
static void launch_bf_range_i8cos_t(const BfRangeLaunch& a, hipStream_t stream)
{
  const int fm = bf_range_i8cos_filter_mode(a);
  const uint32_t qblocks = (a.Nq + kRangeI8cQueries - 1) / kRangeI8cQueries;
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
  const size_t n_q = pad4(a.Nq), n_pairs = pad4(pairs);
  const size_t n_lims = pad4(2 * (static_cast<size_t>(a.Nq) + 1));
  // [row records][query records][-c][flag, largest row norm][counts][offsets (uint64)][the scan's lims]
  const size_t words = 4 * static_cast<size_t>(a.N_base) + 4 * static_cast<size_t>(a.Nq) + n_q + 4 +
                       n_pairs + 2 * n_pairs + n_lims;
  ScratchGuard scratch{scratch_alloc(words * 4, stream), stream};
  int4* brec = static_cast<int4*>(scratch.p);
  int4* qrec = brec + a.N_base;
  float* nc = reinterpret_cast<float*>(qrec + a.Nq);
  uint32_t* flag = reinterpret_cast<uint32_t*>(nc + n_q);
  uint32_t* norm_max = flag + 1;
  uint32_t* counts = flag + 4;
  uint64_t* offsets = reinterpret_cast<uint64_t*>(counts + n_pairs);
  uint64_t* scan_lims = offsets + n_pairs;

  GGNN_HIP_CHECK(hipMemsetAsync(flag, 0, 4 * sizeof(uint32_t), stream));
  launch_bf_i8_cos_records(a.base, a.N_base, a.D, SIGNED, brec, norm_max, stream);
  launch_bf_i8_cos_records(a.query, a.Nq, a.D, SIGNED, qrec, nullptr, stream);
  hipLaunchKernelGGL(bf_range_i8cos_prep_kernel, dim3((a.Nq + 255) / 256), dim3(256), 0, stream, qrec,
                     a.radii, norm_max, a.Nq, nc, flag, a.fell_back);
  GGNN_HIP_CHECK(hipGetLastError());

  BfRangeI8CosFilteredArgs t{};
  t.base = a.base;
  t.query = a.query;
  t.brec = brec;
  t.qrec = qrec;
  t.nc = nc;
  t.radii = a.radii;
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
      launch_bf_range_i8cos_tiles<SIGNED, kBfBits>(a, t, fill, qblocks, stream);
    else if (fm == kBfLabels)
      launch_bf_range_i8cos_tiles<SIGNED, kBfLabels>(a, t, fill, qblocks, stream);
    else
      launch_bf_range_i8cos_tiles<SIGNED, kBfNoFilter>(a, static_cast<const BfRangeI8CosArgs&>(t), fill,
                                                       qblocks, stream);
  };
  tile_pass(false);
  launch_bf_range_prefix(counts, a.Nq, parts, offsets, a.lims, stream);
  if (a.capacity != 0)
    tile_pass(true);

  // the scan passes, gated by the flag: they answer the call iff the 2^24 rule asked for them
  BfRangeLaunch fb = a;
  fb.lims = scan_lims;
  launch_bf_range_scan(fb, flag, stream);
  launch_bf_range_i8_take_lims(flag, scan_lims, a.Nq + 1, a.lims, stream);
}

void launch_bf_range_query_i8_cos(const BfRangeLaunch& a, hipStream_t stream)
{
  if (a.dtype == GGNN_I8)
    launch_bf_range_i8cos_t<true>(a, stream);
  else if (a.dtype == GGNN_U8)
    launch_bf_range_i8cos_t<false>(a, stream);
  else
    throw Error(GGNN_UNSUPPORTED, "range search: the integer cosine kernels take uint8 / int8 rows");
}

}  // namespace ggnn_amd
