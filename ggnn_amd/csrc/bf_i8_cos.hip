// bf_query, uint8 / int8 rows of 16 <= D <= 4096 bytes (D % 16 == 0) under cosine, K <= 16, no filter: the
// K-best search on v_mfma_i32_32x32x32_i8 with per-query sets in registers.  bf_i8w_kernel's pipeline
// (bf_i8_wide.hip: stages, streamed query operand, pending lists, bound exchange, seeding) with side data
// and an epilogue of its own.  Separate translation unit, compiled like bf_i8_wide.hip with
// -mllvm -amdgpu-mfma-vgpr-form (Makefile).
//
// Arithmetic contract.  The scan's value of a pair (DistEngine::partial / finish_cos, traversal.hpp) is
//     value = (qn * bn > 0) ? fabsf(1 - dot / sqrtf(qn * bn)) : 1        (float32, operation by operation)
// with dot = (float) sum o q, bn = (float) sum o^2, qn = (float) sum q^2: three integers, exact in the scan
// whenever they are below 2^24 (always for uint8 at D <= 258 and int8 at D <= 1024).
//   * The matrix instruction is signed.  int8 rows go in as they are and the accumulator is sum o q.
//     uint8 rows go in flipped (x' = x ^ 0x80 = x - 128), and
//         sum o q = q'.b' + 128 sum b' + (128 sum q' + 16384 D):
//     the query's term is the accumulators' initial block, the row's term a word beside the row in LDS.
//     Every intermediate is below 2^31 in magnitude (255^2 * 4096 < 2^28.1).
//   * The kernel keeps, per query and slice, the KPT (4 / 10 / 16) smallest rows by (value, id), `value`
//     evaluated by the expression above on the exact integers.  bf_rerank_kernel (exact_arith = 1) then
//     recomputes the scan's values of the union and orders it.
//   * The 2^24 rule.  A query with sum q^2 >= 2^24 is not certified; if any base row has sum o^2 >= 2^24
//     (bf_i8cos_records_kernel leaves the maximum in a device word) no query is:
//     bf_i8cos_uncertified_kernel appends them to the rescan list and launch_bf_rescan answers them.
//     |sum o q| < 2^24 follows from the two norms (Cauchy-Schwarz), also for every partial sum of the scan.
//     n_rescanned is the number of such queries.  No certificate, no error model in D, no measured constant.
//
// Two-level verdict.  `value` costs a correctly rounded square root and a division; the epilogue has
// room for two or three VALU operations per output.  So every output meets a conservative test first:
//     s = dot * rinv[row] >= c[query],     rinv = fl(1 / fl(sqrt(bn)))  (0 for a zero row),
// evaluated as one fused fmaf((float)dot, rinv, -c) >= 0, which has the sign of the real dot * rinv - c
// (a result that underflows is >= 0 or -0: a pass).  Rows that pass are evaluated exactly.  With T the
// largest value that can still enter the query's set (its K-th entry, or the bound the slices agree on;
// +inf: none yet) and u = 2^-24, c is, in float32,
//     c = ((1 - T) - 16 u) * sqrtf(qn),        c = -inf while T = +inf.
// Claim: every row with value <= T has dot * rinv >= c.  (dot, bn, qn < 2^24: the conversions are exact.)
//   Let x = dot / sqrt(qn bn) in the reals, |x| <= 1, for bn, qn > 0.
//   (1) Q = fl(dot / fl(sqrt(fl(qn bn)))) = x (1 + e), |e| <= 3 u: one rounding each of the product (half
//       of it under the root), the root and the quotient, 2.5 u + O(u^2).  Nothing underflows: |dot| >= 1
//       or dot = 0, and the root is in [1, 2^24].  So x >= Q - 3 u.
//   (2) value = |fl(1 - Q)| <= T implies fl(1 - Q) <= T, and by monotonic rounding 1 - Q <= T (1 + u):
//       T is a float32 that is 0 or >= 2^-24 (a value is), half its ulp is <= u T.  Dropping the lower
//       side of the absolute value only admits more rows: a quotient that rounds above 1 has value
//       Q - 1 > 0 and fails value <= T for T = 0 although it passes here.  With T <= 2:
//       x >= 1 - T - 2 u - 3 u.
//   (3) dot * rinv = x sqrt(qn) (1 + f), |f| <= 4 u: the root and the reciprocal of the table entry, u each
//       (2 u each would still do), no rounding in the fused test.  |x| <= 1, so
//       dot * rinv >= (x - 4 u) sqrt(qn) >= (1 - T - 9 u) sqrt(qn).
//   (4) The float32 c: fl(1 - T) <= 1 - T + u, the second subtraction adds <= 1.01 u, so the factor g is
//       <= 1 - T - 13.9 u and |g| <= 1 + 17 u; the root and the product are off by <= 2.01 u |g| sqrt(qn).
//       c <= (1 - T - 11.8 u) sqrt(qn) <= dot * rinv.  The sign of g does not matter: the margins are
//       absolute in units of sqrt(qn).  T > 1 gives a negative c.
//   Zero row (bn = 0): value = 1, dot = 0, rinv = 0, the test is 0 >= c; value <= T means T >= 1, then
//       g < 0 and c <= -0: it passes.  Zero query (qn = 0): every value is 1, so is T once the set is
//       full, c = g * 0 = -0, and every row passes (dot = 0): such a query takes the slow path on every
//       tile, correct and rare.  T = +inf would make c a NaN (inf * 0): hence the explicit -inf.
//   Rows that tie T pass as well (the test is value <= T, the insertion decides by id), and a stale,
//   larger T only makes c smaller.  Nothing here depends on D.
//
// The tile kernel.  bf_i8w_kernel's: 256 threads, a wave owns two 32-query sets that share every B operand;
// a stage is one 32-row tile x up to four 128-byte column chunks, double buffered at a row stride of 528
// bytes, the spare 16 bytes holding the row's record (rinv, sum o^2, row term); the query operand streamed
// one chunk ahead from bf_i8w_pack_kernel's copy (KPT = 16: loaded in front of its MFMAs, one operand set).
//   Epilogue, once per tile: per output one add (uint8 only), one convert and one fmaf against the block of
//   -c kept in LDS in matrix order, eight v_max3_f32 and one compare per set.  A set with a hit transposes
//   its passing outputs through LDS into the lane = query pending lists as (float bits of the exact value,
//   id) -- the value is evaluated there, by the lane that holds the row, with the query's norm from LDS.
//   Values are non-negative, so their bits order as integers: the sets, the seeds and the exchange area of
//   bf_i8_sets.hpp carry them as the integer kernels carry distances, "infinity" 0x7fffffff included.
//   -c is refreshed between tiles when T changed.
#include <algorithm>

#include "bf_i8_sets.hpp"
#include "hooks.hpp"

namespace ggnn_amd {

constexpr uint32_t kI8cStageChunks = 4;                       // 128-byte column chunks per stage
constexpr uint32_t kI8cStageCols = 128 * kI8cStageChunks;
constexpr uint32_t kI8cRowStride = kI8cStageCols + 16;        // + the row's record; 33 slots of 16 bytes
constexpr uint32_t kI8cStageBytes = kBfTileRows * kI8cRowStride;
constexpr float kI8cSlack = 9.5367431640625e-7f;              // 16 u = 2^-20 (the header's derivation)
constexpr int kI8cNone = 0x7fffffff;                          // "no value": above the bits of every float

// sum x^2 and (uint8) sum (x - 128) of one row, 16 lanes per row; every lane of the group gets the sums
template <bool SIGNED>
GGNN_DEV void i8cos_row_sums(const uint8_t* row, uint32_t D, uint32_t g, uint32_t& nn, int& sm)
{
  nn = 0;
  sm = 0;
  for (uint32_t col = 16 * g; col < D; col += 256) {  // (D % 16 == 0)
    const uint4 v = *reinterpret_cast<const uint4*>(row + col);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if constexpr (SIGNED)
        nn = static_cast<uint32_t>(__builtin_amdgcn_sdot4(static_cast<int>(w[e]), static_cast<int>(w[e]),
                                                          static_cast<int>(nn), false));
      else {
        nn = __builtin_amdgcn_udot4(w[e], w[e], nn, false);
        sm = __builtin_amdgcn_sdot4(static_cast<int>(w[e] ^ 0x80808080u), 0x01010101, sm, false);
      }
    }
  }
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) {
    nn += __shfl_xor(nn, o);
    sm += __shfl_xor(sm, o);
  }
}

// the records of N rows (BfI8CosArgs); norm_max, if given, receives the largest sum x^2
template <bool SIGNED>
__global__ void __launch_bounds__(256) bf_i8cos_records_kernel(const uint8_t* rows, uint32_t N, uint32_t D,
                                                              int4* rec, uint32_t* norm_max)
{
  const uint32_t g = threadIdx.x & 15;
  uint32_t mx = 0;
  for (uint64_t row = static_cast<uint64_t>(blockIdx.x) * 16 + (threadIdx.x >> 4); row < N;
       row += static_cast<uint64_t>(gridDim.x) * 16) {
    uint32_t nn;
    int sm;
    i8cos_row_sums<SIGNED>(rows + row * D, D, g, nn, sm);
    mx = max(mx, nn);
    if (g == 0) {
      const float rinv = nn ? 1.0f / sqrtf(static_cast<float>(nn)) : 0.0f;
      rec[row] = make_int4(__float_as_int(rinv), static_cast<int>(nn), 128 * sm, 0);
    }
  }
  if (norm_max) {
#pragma unroll
    for (int o = 32; o >= 16; o >>= 1)  // (the 16 lanes of a group agree)
      mx = max(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0 && mx)
      atomicMax(norm_max, mx);
  }
}

__global__ void __launch_bounds__(256) bf_i8cos_uncertified_kernel(const int4* qrec, const uint32_t* norm_max,
                                                                  uint32_t Nq, uint32_t* rescan_list,
                                                                  uint32_t* rescan_count)
{
  const uint32_t n = blockIdx.x * 256 + threadIdx.x;
  if (n < Nq && (*norm_max >= (1u << 24) || static_cast<uint32_t>(qrec[n].y) >= (1u << 24)))
    rescan_list[atomicAdd(rescan_count, 1u)] = n;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int KPT, bool SIGNED>
__global__ void __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(2))) bf_i8cos_kernel(const BfI8CosArgs a)
{
  constexpr uint32_t kFlip = SIGNED ? 0u : 0x80808080u;
  constexpr bool AHEAD = KPT < 16;  // the query operand is requested one chunk ahead (two register sets)
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_b[];
  int* hq_l = reinterpret_cast<int*>(lds_b + 2 * kI8cStageBytes);  // [4 waves][64] query terms, matrix order
  float* nc_l = reinterpret_cast<float*>(hq_l + 4 * 64);            // [4 waves][64] -c, matrix order
  float* qn_l = nc_l + 4 * 64;                                      // [4 waves][64] (float) sum q^2
  int* pc_l = reinterpret_cast<int*>(qn_l + 4 * 64);                // [4 waves][64] pending counts
  int* pd_l = pc_l + 4 * 64;                                        // [4 waves][kPend][64] pending value bits
  int* pi_l = pd_l + 4 * kI8v2Pend * 64;                            // [4 waves][kPend][64] pending id

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int j = lane & 31, h = lane >> 5;  // matrix layout: base row j of the tile, half h
  // bookkeeping layout: lane = query (lane & 31) of set (lane >> 5)
  const uint8_t* base = static_cast<const uint8_t*>(a.base);
  const uint32_t qw = (blockIdx.x * 4 + wave) * 64;
  const uint32_t begin = blockIdx.y * a.rows_per_slice;
  const uint32_t end = min(a.N_base, begin + a.rows_per_slice);
  const uint32_t nch = a.nch;
  int* hq_w = hq_l + wave * 64;
  float* nc_w = nc_l + wave * 64;
  float* qn_w = qn_l + wave * 64;
  int* pc_w = pc_l + wave * 64;
  int* pd_w = pd_l + wave * kI8v2Pend * 64;
  int* pi_w = pi_l + wave * kI8v2Pend * 64;

  // ---- lane = query state ----
  const uint32_t my_q = qw + lane;
  const bool my_valid = my_q < a.Nq;
  const int4 qr = my_valid ? a.qrec[my_q] : make_int4(0, 0, 0, 0);
  const float sqn = sqrtf(static_cast<float>(qr.y));
  int T = kI8cNone;  // float bits of the largest value that can still enter the set: candidates need value <= T
  const int sl4 = static_cast<int>((a.slices + 15) / 16 * 4);  // int4 groups per position
  int* gl_q = a.gthr ? reinterpret_cast<int*>(a.gthr) +
                           static_cast<size_t>(my_valid ? my_q : 0) * kI8MaxRanks * 4 * sl4
                     : nullptr;
  const bool gl_q_any = a.gthr != nullptr && a.rank_mask != 0;  // uniform: anything to exchange
  if (my_valid && a.seed && !a.seeding)
    T = min(T, a.seed[my_q]);
  // the query's K-best set: sorted ascending by (value bits, index), unused slots hold "infinity"
  int sd[KPT], si[KPT];
#pragma unroll
  for (int k = 0; k < KPT; ++k) {
    sd[k] = kI8cNone;
    si[k] = kI8cNone;
  }
  int T_seen = kI8cNone;
  bool bounds_stale = false;  // wave-uniform
  qn_w[lane] = static_cast<float>(qr.y);
  pc_w[lane] = 0;

  // ---- matrix layout state ----
  // query (lane & 31) of a set sits in accumulator register (q & 3) + 4 (q >> 3) of half (q >> 2) & 1
  const int my_slot = i8_offset_slot(lane);
  hq_w[my_slot] = SIGNED ? 0 : qr.z + 16384 * static_cast<int>(a.D);  // the accumulators' initial block
  // -c changes only here, and only between tiles; a query past Nq never passes (-c = -inf)
  auto refresh_bounds = [&]() {
    float nc = -inf_f();
    if (my_valid)
      nc = T == kI8cNone ? inf_f() : -(((1.0f - __int_as_float(T)) - kI8cSlack) * sqn);
    nc_w[my_slot] = nc;
    T_seen = T;
    bounds_stale = false;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  auto load_bounds = [&](int s2) __attribute__((always_inline)) -> f32x16 {
    const f32x4* p = reinterpret_cast<const f32x4*>(nc_w + s2 * 32 + 16 * h);
    const f32x4 a0 = p[0], a1 = p[1], a2 = p[2], a3 = p[3];
    return f32x16{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3],
                  a2[0], a2[1], a2[2], a2[3], a3[0], a3[1], a3[2], a3[3]};
  };

  // applies the pending candidates of all 64 queries in lockstep (bf_i8w_kernel's; the lists hold the
  // value bits themselves)
  auto flush = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int cnt = min(pc_w[lane], kI8v2Pend);
    pc_w[lane] = 0;
    for (int i = 0; __any(i < cnt); ++i) {
      const bool have = i < cnt;
      const int rd = have ? pd_w[i * 64 + lane] : kI8cNone;
      const int rid = have ? pi_w[i * 64 + lane] : kI8cNone;
      const unsigned long long rec =
          (static_cast<unsigned long long>(static_cast<unsigned>(rd)) << 32) | static_cast<unsigned>(rid);
      bool lt_prev = false;  // rec < entry k-1
      int pd_ = 0, pi_ = 0;  // entry k-1 before this insertion
#pragma unroll
      for (int k = 0; k < KPT; ++k) {
        const unsigned long long ek =
            (static_cast<unsigned long long>(static_cast<unsigned>(sd[k])) << 32) | static_cast<unsigned>(si[k]);
        const bool lt = rec < ek;
        const int od = sd[k], oi = si[k];
        sd[k] = lt_prev ? pd_ : (lt ? rd : od);
        si[k] = lt_prev ? pi_ : (lt ? rid : oi);
        lt_prev = lt;
        pd_ = od;
        pi_ = oi;
      }
    }
    T = min(T, sd[KPT - 1]);  // "infinity" while the set is not full
    if (__any(T != T_seen))
      bounds_stale = true;  // folded into -c before the next tile
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };

  // bound exchange with the other slices (bf_i8_sets.hpp), between tiles only: rows equal to the bound
  // are kept, which is the test value <= T
  auto refresh = [&]() {
    if (__any(pc_w[lane] > 0))
      flush();
    if (gl_q && my_valid)
      T = min(T, i8_exchange_bound<KPT>(sd, gl_q, sl4, blockIdx.y, a.rank_mask));
    if (__any(T != T_seen))
      bounds_stale = true;
  };

  // ---- staging (bf_i8w_kernel): 32 rows x 512 bytes = 1024 pieces of 16 bytes, four per thread; threads
  // 0..31 carry the row records.  Every load is unconditional with a clamped address: rows past the end of
  // the slice repeat its last row and are excluded in the epilogue, columns past D repeat the last 16 and
  // meet zeros in the query operand (chunks past the row are not contracted at all)
  uint4 sv[4];
  int4 srec = make_int4(0, 0, 0, 0);
  auto stage_load = [&](uint32_t row0, uint32_t col0) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t p = tid + 256 * e, srow = p >> 5, scol = 16 * (p & 31);
      const uint32_t r = min(row0 + srow, end - 1), c = min(col0 + scol, a.D - 16u);
      sv[e] = *reinterpret_cast<const uint4*>(base + static_cast<size_t>(r) * a.D + c);
    }
    srec = a.brec[min(row0 + (tid & 31), end - 1)];
  };
  auto stage_store = [&](uint32_t buf) __attribute__((always_inline)) {
    uint8_t* t = lds_b + buf * kI8cStageBytes;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t p = tid + 256 * e, srow = p >> 5, scol = 16 * (p & 31);
      *reinterpret_cast<uint4*>(t + srow * kI8cRowStride + scol) =
          make_uint4(sv[e].x ^ kFlip, sv[e].y ^ kFlip, sv[e].z ^ kFlip, sv[e].w ^ kFlip);
    }
    if (tid < kBfTileRows)
      *reinterpret_cast<int4*>(t + tid * kI8cRowStride + kI8cStageCols) = srec;
  };

  // the query operand of chunk c: packed[32-query set][chunk][m][lane]
  const uint4* qp = a.query_packed + static_cast<size_t>(qw / 32) * nch * 256 + lane;
  auto query_load = [&](i32x4 (&dst)[2][4], uint32_t c) __attribute__((always_inline)) {
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const uint4 v = qp[(static_cast<size_t>(s2) * nch + c) * 256 + m * 64];
        dst[s2][m] = i32x4{static_cast<int>(v.x), static_cast<int>(v.y), static_cast<int>(v.z),
                           static_cast<int>(v.w)};
      }
  };

  // passing outputs of one tile-set in the matrix layout -> pending lists of the queries, as exact values
  auto scan_pass = [&](const i32x16& acc, const f32x16& nc, const int s2, const int4 rec, const bool row_ok,
                       int id, unsigned& redo, const bool first) __attribute__((always_inline)) {
    const float rinv = __int_as_float(rec.x), bnf = static_cast<float>(rec.y);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int dot = SIGNED ? acc[r] : acc[r] + rec.z;
      const bool hit = first ? (row_ok && fmaf(static_cast<float>(dot), rinv, nc[r]) >= 0.0f)
                             : ((redo >> r) & 1u);
      if (!__any(hit))
        continue;
      redo &= ~(1u << r);
      if (hit) {
        const int q = s2 * 32 + i8v2_qrow(r, h);
        const int slot = atomicAdd(pc_w + q, 1);
        if (slot < kI8v2Pend) {
          // finish_cos, operation by operation
          const float norm_sqr = qn_w[q] * bnf;
          const float v =
              (norm_sqr > 0.0f) ? fabsf(1.0f - static_cast<float>(dot) / sqrtf(norm_sqr)) : 1.0f;
          pd_w[slot * 64 + q] = __float_as_int(v);
          pi_w[slot * 64 + q] = id;
        }
        else
          redo |= 1u << r;
      }
    }
  };
  auto tile_set = [&](const i32x16& acc, const f32x16& nc, const int s2, const int4 rec, const bool row_ok,
                      int id) __attribute__((always_inline)) {
    unsigned redo = 0;
    scan_pass(acc, nc, s2, rec, row_ok, id, redo, true);
    while (__any(redo != 0u)) {
      flush();  // (resets the pending counts: the lists have room again)
      scan_pass(acc, nc, s2, rec, row_ok, id, redo, false);
    }
    if (__any(pc_w[lane] >= kI8v2Pend / 2))
      flush();
  };

  const uint32_t ntiles = end > begin ? (end - begin + kBfTileRows - 1) / kBfTileRows : 0;
  const uint32_t spt = (nch + kI8cStageChunks - 1) / kI8cStageChunks;  // stages per tile
  const uint32_t nsteps = ntiles * spt;
  i32x4 aqa[2][4];
  [[maybe_unused]] i32x4 aqb[2][4];
  if (nsteps) {
    stage_load(begin, 0);
    stage_store(0);
  }
  if constexpr (AHEAD)
    query_load(aqa, 0);
  refresh_bounds();
  __syncthreads();

  i32x16 acc[2];
  // one chunk: the next chunk's operand is requested first, then 8 MFMAs on this one
  // (!AHEAD: this chunk's, into the one set)
  auto chunk = [&](i32x4 (&cur)[2][4], i32x4 (&nxt)[2][4], const uint8_t* brow, uint32_t c, uint32_t nc)
                   __attribute__((always_inline)) {
    if constexpr (AHEAD)
      query_load(nxt, nc);
    else
      query_load(cur, c);
    i32x4 b[4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
      b[m] = *reinterpret_cast<const i32x4*>(brow + 32 * m + 16 * h);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(cur[0][m], b[m], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(cur[1][m], b[m], acc[1], 0, 0, 0);
    }
  };

  uint32_t t = 0, s = 0;  // tile of the slice, stage of the tile
  for (uint32_t p = 0; p < nsteps; ++p) {
    const bool last_s = s + 1 == spt;
    const uint32_t n_t = last_s ? t + 1 : t, n_s = last_s ? 0u : s + 1;
    const bool has_next = p + 1 < nsteps;
    const uint32_t row0 = begin + t * kBfTileRows;
    if (s == 0) {
      // (the exchange first: it waits with vmcnt(0), which must not have this stage's staging loads
      // in front of it)
      if (gl_q_any && i8_exchange_stage(t, a.refresh_every))
        refresh();
      if (bounds_stale)
        refresh_bounds();
      // (int8: a block of zeros, read like the uint8 terms -- as 32 register moves the KPT = 10 kernel
      // came out with a 96-byte private segment)
      acc[0] = i8_load_offsets(hq_w, 0, h);
      acc[1] = i8_load_offsets(hq_w, 1, h);
    }
    if (has_next)
      stage_load(begin + n_t * kBfTileRows, n_s * kI8cStageCols);
    const uint8_t* trow = lds_b + (p & 1) * kI8cStageBytes + j * kI8cRowStride;
#pragma unroll
    for (uint32_t cc = 0; cc < kI8cStageChunks; ++cc) {
      const uint32_t c = s * kI8cStageChunks + cc;
      if (c >= nch)
        break;  // uniform
      const uint32_t nc = c + 1 < nch ? c + 1 : 0u;  // (after the last chunk: the next tile's first)
      if (AHEAD && (cc & 1))
        chunk(aqb, aqa, trow + 128 * cc, c, nc);
      else
        chunk(aqa, aqb, trow + 128 * cc, c, nc);
    }
    // (the other buffer was last read before the barrier that ended the previous step; storing in front of
    // the epilogue frees the staging registers for it)
    if (has_next)
      stage_store((p + 1) & 1);
    if (last_s) {
      // every stage but the last has four chunks: the sets are out of step after a tile iff nch is odd
      if (AHEAD && (nch & 1u)) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int m = 0; m < 4; ++m)
            aqa[s2][m] = aqb[s2][m];
      }
      const int4 rec = *reinterpret_cast<const int4*>(trow + kI8cStageCols);
      const float rinv = __int_as_float(rec.x);
      const bool row_ok = row0 + j < end;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        // (-c in pieces of four: the fast path keeps no block of 16 alive; a hit reads it again)
        const f32x4* ncp = reinterpret_cast<const f32x4*>(nc_w + s2 * 32 + 16 * h);
        float mx = -inf_f();
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const f32x4 nc = ncp[g4];
          float f[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * g4 + e;
            f[e] = fmaf(static_cast<float>(SIGNED ? acc[s2][r] : acc[s2][r] + rec.z), rinv, nc[e]);
          }
          mx = fmaxf(fmaxf(fmaxf(mx, f[0]), f[1]), fmaxf(f[2], f[3]));
        }
        if (__any(row_ok && mx >= 0.0f))
          tile_set(acc[s2], load_bounds(s2), s2, rec, row_ok, static_cast<int>(row0) + j);
      }
    }
    __syncthreads();
    t = n_t;
    s = n_s;
  }

  flush();
  if (a.seeding && a.seed && my_valid)
    a.seed[my_q] = sd[KPT - 1];
  if (a.part_ids && my_valid) {
    const size_t o = (static_cast<size_t>(blockIdx.y) * a.Nq + my_q) * KPT;
#pragma unroll
    for (int k = 0; k < KPT; ++k) {
      const bool used = sd[k] != kI8cNone;
      a.part_ids[o + k] = used ? si[k] : kEmptyKey;
      a.part_dists[o + k] = used ? __int_as_float(sd[k]) : inf_f();
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------
static size_t bf_i8cos_lds_bytes()
{
  return 2 * kI8cStageBytes + (4 * 4 * 64 + 2 * 4 * kI8v2Pend * 64) * sizeof(int);
}

bool bf_i8_cos_supported(const BfLaunch& a)
{
  return (a.dtype == GGNN_U8 || a.dtype == GGNN_I8) && a.measure == GGNN_COSINE && a.D >= 16 &&
         a.D <= 4096 && a.D % 16 == 0 && a.k_query >= 1 && a.k_query <= 16 && !a.filter_bits &&
         !a.label_sets.labels && !a.label_ranges.labels && !a.label_masks.labels && a.Nq >= 256 &&
         a.N_base >= 4096 && hook(kHookBfNoI8) == 0 && bf_i8cos_lds_bytes() <= 160 * 1024;
}

// Hook BF_I8_COS: 1 never, 2 whenever the launch is supported, 0 auto -- the shape class measured
// against the float32-staged tiles: batches of at least 10000 queries over at least
// 1M rows.  Smaller launches keep the kernels they ran before.
bool bf_i8_cos_routes(const BfLaunch& a)
{
  const int64_t mode = hook(kHookBfI8Cos);
  if (mode == 1 || !bf_i8_cos_supported(a))
    return false;
  return mode == 2 || (a.Nq >= 10000 && a.N_base >= 1000000);
}

void launch_bf_i8_cos_records(const void* rows, uint32_t N, uint32_t D, bool is_signed, int4* rec,
                              uint32_t* norm_max, hipStream_t stream)
{
  const dim3 grid(std::max(1u, std::min((N + 15) / 16, 4096u)));
  const uint8_t* r = static_cast<const uint8_t*>(rows);
  if (is_signed)
    hipLaunchKernelGGL((bf_i8cos_records_kernel<true>), grid, dim3(256), 0, stream, r, N, D, rec, norm_max);
  else
    hipLaunchKernelGGL((bf_i8cos_records_kernel<false>), grid, dim3(256), 0, stream, r, N, D, rec, norm_max);
  GGNN_HIP_CHECK(hipGetLastError());
}

void launch_bf_i8_cos_uncertified(const int4* qrec, const uint32_t* norm_max, uint32_t Nq,
                                  uint32_t* rescan_list, uint32_t* rescan_count, hipStream_t stream)
{
  hipLaunchKernelGGL(bf_i8cos_uncertified_kernel, dim3((Nq + 255) / 256), dim3(256), 0, stream, qrec,
                     norm_max, Nq, rescan_list, rescan_count);
  GGNN_HIP_CHECK(hipGetLastError());
}

void launch_bf_i8_cos(const BfI8CosArgs& m, uint32_t KP, bool is_signed, uint32_t qblocks,
                      uint32_t seed_rows, hipStream_t stream)
{
  GGNN_REQUIRE(KP == 4 || KP == 10 || KP == 16, GGNN_INVALID_ARGUMENT, "unsupported list length");
#define GGNN_I8C(S_)                                                             \
  (KP == 4    ? reinterpret_cast<const void*>(&bf_i8cos_kernel<4, S_>)           \
   : KP == 10 ? reinterpret_cast<const void*>(&bf_i8cos_kernel<10, S_>)          \
              : reinterpret_cast<const void*>(&bf_i8cos_kernel<16, S_>))
  const void* kern = is_signed ? GGNN_I8C(true) : GGNN_I8C(false);
#undef GGNN_I8C
  const size_t lds = bf_i8cos_lds_bytes();
  GGNN_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(lds)));
  // seeding launch (hook BF_I8_SEED, as for bf_i8w_kernel): the first seed_rows rows, all queries, one
  // workgroup per query block, no lists written -- its K-th best value is every slice's first bound
  const uint32_t seed = std::min(m.N_base, seed_rows / kBfTileRows * kBfTileRows);
  const bool seeded = m.seed && seed >= static_cast<uint32_t>(kBfTileRows) && m.slices > 1;
  if (seeded) {
    BfI8CosArgs w = m;
    w.part_ids = nullptr;
    w.part_dists = nullptr;
    w.N_base = seed;
    w.rows_per_slice = seed;
    w.slices = 1;
    w.gthr = nullptr;
    w.rank_mask = 0;
    w.seeding = 1;
    void* wargs[] = {&w};
    GGNN_HIP_CHECK(hipLaunchKernel(kern, dim3(qblocks, 1), dim3(256), wargs, lds, stream));
  }
  BfI8CosArgs mm = m;
  mm.seeding = 0;
  if (!seeded)
    mm.seed = nullptr;
  void* kargs[] = {&mm};
  GGNN_HIP_CHECK(hipLaunchKernel(kern, dim3(qblocks, m.slices), dim3(256), kargs, lds, stream));
}

}  // namespace ggnn_amd
