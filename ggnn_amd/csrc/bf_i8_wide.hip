// bf_query, uint8 / int8 rows of 128 < D <= 4096 bytes under squared L2, K <= 16, no filter: the
// K-best search on v_mfma_i32_32x32x32_i8 with per-query sets in registers -- bf_i8v2_kernel's scheme
// (bf_i8.hip) with the row streamed in 128-byte column chunks.  Separate translation unit, compiled like
// bf_i8.hip with -mllvm -amdgpu-mfma-vgpr-form (Makefile): accumulators and their C operand in VGPRs.
//
// Arithmetic contract.  With b' = b ^ 0x80 for uint8 and b itself for int8 (squared L2 does not change
// under a common shift), as in bf_range_i8.hip:
//   * |q'.b'| <= 128^2 * 4096 = 2^26, the norms |q'|^2, |b'|^2 are <= 2^26 (int32:
//     bf_range_i8_norms_kernel; float norms stop being exact above 2^24), and
//     d = |q'|^2 + |b'|^2 - 2 q'.b' <= 2^28 fits int32.
//   * The kernel selects, per query and slice, the KPT (4 / 10 / 16) smallest rows by the integer pair
//     (d, id); bf_rerank_kernel (exact_arith = 1) then computes the scan's float32 values of the union
//     and orders it.
//   * The scan's value of a pair is (float)d exactly when d < 2^24, and >= 2^24 (rounded per row
//     layout; rounding is monotonic and 2^24 is representable) when d >= 2^24, which needs D > 258.
//     So a query whose K-th best integer distance is < 2^24 gets the scan's ids and bits: every row
//     left out has d >= d_K in (d, id) order, and its float value cannot tie below.
//   * A query whose K-th best distance is >= 2^24 is not certified: bf_i8w_uncertified_kernel reads
//     dists[n K + K - 1] >= 2^24 after the re-rank, appends the query to the rescan list, and
//     launch_bf_rescan answers it, as on the float path.  n_rescanned is the number of such queries,
//     0 whenever D <= 258.  No other certificate, no error model, no measured constant.
//
// The tile kernel.  256 threads; wave w owns 64 queries as two 32-query sets that share every B operand
// read from LDS.  The base is walked in 32-row tiles.  A STAGE is one tile x up to four 128-byte column
// chunks (512 columns), double buffered in LDS at a row stride of 528 bytes (33 slots of 16: odd, like
// kBfI8RowStride) with the row's int32 norm in the spare bytes.  One barrier per stage = up to 32 MFMAs
// of a wave (bf_range_i8's chunked kernel: one chunk, 8 MFMAs).  All chunks of a tile go into the same
// 2 x 16 i32 accumulators, which start at the -hq offset block (C operand of the tile's first MFMA).
//   Query operand: 2 sets x 4 x 16 bytes per lane and chunk -- at D = 1024 that is 256 registers for
// the row, so it is streamed instead, ONE CHUNK AHEAD, from a copy of the query set in operand order
// (bf_i8w_pack_kernel: flipped, zero past D and past Nq, so every load is unconditional and 1 KB
// coalesced per wave).  Two register sets alternate by chunk parity; after a tile with an odd
// number of chunks the set that is ahead is copied (32 moves per tile).  The 16-entry sets leave no
// room for the second operand set (256 registers and a 104-byte private segment with it): that kernel
// loads each chunk's operand right in front of its MFMAs and leans on the SIMD's other wave.
//   Epilogue: once per tile, after its last chunk -- bf_i8v2's, in its LEAN form (offsets read from
// LDS per tile: the two operand sets need the 32 registers): threshold folded into the accumulator
// (8 v_max3_i32 + one compare on the fast path), hit tiles transposed through LDS into lane = query
// pending lists, sorted K-best sets in registers, the slice-bound exchange through gthr[] on the
// doubling schedule (counted in tiles here), the optional seeding launch.  Per tile it is amortised
// over 4 ceil(D / 128) MFMAs per set instead of 4.
//   Why the query is re-read per tile and not held across several tiles: two tiles per operand load
// need 64 accumulator registers; with the 16-entry sets that does not leave two waves per SIMD.  The
// price is L2 traffic: every tile re-reads 64 D bytes per wave (DESIGN.md 4.6 has what that costs).
#include <algorithm>

#include "bf_i8_sets.hpp"
#include "hooks.hpp"

namespace ggnn_amd {

constexpr uint32_t kI8wStageChunks = 4;                       // 128-byte column chunks per stage
constexpr uint32_t kI8wStageCols = 128 * kI8wStageChunks;
constexpr uint32_t kI8wRowStride = kI8wStageCols + 16;        // + the row's norm; 33 slots of 16 bytes
constexpr uint32_t kI8wStageBytes = kBfTileRows * kI8wRowStride;
constexpr int kI8wPadNorm = 0x3fffffff;                       // rows past the end of a slice
constexpr uint32_t kI8wQueries = 256;                         // per workgroup

// the query set in operand order: [32-query set][chunk][m = 0..3][lane] x 16 bytes -- lane (j, h) of a
// wave holds columns 128 c + 32 m + 16 h .. + 16 of query 32 set + j
template <bool SIGNED>
__global__ void __launch_bounds__(256) bf_i8w_pack_kernel(const uint8_t* query, uint32_t Nq, uint32_t D,
                                                         uint32_t nch, uint64_t n16, uint4* out)
{
  constexpr uint32_t kFlip = SIGNED ? 0u : 0x80808080u;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; i < n16;
       i += static_cast<uint64_t>(gridDim.x) * 256) {
    const uint32_t lane = i & 63, m = (i >> 6) & 3;
    const uint64_t rest = i >> 8;
    const uint32_t c = static_cast<uint32_t>(rest % nch);
    const uint64_t q = rest / nch * 32 + (lane & 31);
    const uint32_t col = 128 * c + 32 * m + 16 * (lane >> 5);
    uint4 v = make_uint4(0, 0, 0, 0);
    if (q < Nq && col < D) {  // (D % 16 == 0: the 16 bytes are inside the row)
      v = *reinterpret_cast<const uint4*>(query + q * D + col);
      v = make_uint4(v.x ^ kFlip, v.y ^ kFlip, v.z ^ kFlip, v.w ^ kFlip);
    }
    out[i] = v;
  }
}

__global__ void __launch_bounds__(256) bf_i8w_uncertified_kernel(const float* dists, uint32_t Nq,
                                                                uint32_t K, uint32_t* rescan_list,
                                                                uint32_t* rescan_count)
{
  const uint32_t n = blockIdx.x * 256 + threadIdx.x;
  if (n < Nq && !(dists[static_cast<size_t>(n) * K + K - 1] < 16777216.f))
    rescan_list[atomicAdd(rescan_count, 1u)] = n;
}

template <int KPT, bool SIGNED>
__global__ void __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(2))) bf_i8w_kernel(const BfI8WideArgs a)
{
  constexpr uint32_t kFlip = SIGNED ? 0u : 0x80808080u;
  constexpr bool AHEAD = KPT < 16;  // the query operand is requested one chunk ahead (two register sets)
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_b[];
  int* hq_l = reinterpret_cast<int*>(lds_b + 2 * kI8wStageBytes);  // [4 waves][64] -hq, matrix order
  int* qn_l = hq_l + 4 * 64;                                        // [4 waves][64] |q'|^2
  int* te_l = qn_l + 4 * 64;                                        // [4 waves][64] thresholds (d < te)
  int* pc_l = te_l + 4 * 64;                                        // [4 waves][64] pending counts
  int* pd_l = pc_l + 4 * 64;                                        // [4 waves][kPend][64] pending dist
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
  int* qn_w = qn_l + wave * 64;
  int* te_w = te_l + wave * 64;
  int* pc_w = pc_l + wave * 64;
  int* pd_w = pd_l + wave * kI8v2Pend * 64;
  int* pi_w = pi_l + wave * kI8v2Pend * 64;

  // ---- lane = query state (bf_i8v2_kernel) ----
  const uint32_t my_q = qw + lane;
  const bool my_valid = my_q < a.Nq;
  const int qn_q = my_valid ? a.qnorm[my_q] : 0;
  int Te = my_valid ? kTeInf : -kTeInf;  // candidates need d < Te (d <= 2^28)
  const int sl4 = static_cast<int>((a.slices + 15) / 16 * 4);  // int4 groups per position
  int* gl_q = a.gthr ? reinterpret_cast<int*>(a.gthr) +
                           static_cast<size_t>(my_valid ? my_q : 0) * kI8MaxRanks * 4 * sl4
                     : nullptr;
  const bool gl_q_any = a.gthr != nullptr && a.rank_mask != 0;  // uniform: anything to exchange
  if (my_valid && a.seed && !a.seeding) {
    const int g = a.seed[my_q];
    if (g < 0x7fffffff)
      Te = min(Te, g + 1);
  }
  // the query's K-best set: sorted ascending by (distance, index), unused slots hold "infinity"
  int sd[KPT], si[KPT];
#pragma unroll
  for (int k = 0; k < KPT; ++k) {
    sd[k] = 0x7fffffff;
    si[k] = 0x7fffffff;
  }
  int Te_seen = 0x7fffffff;
  bool offsets_stale = false;  // wave-uniform
  qn_w[lane] = qn_q;
  te_w[lane] = Te;
  pc_w[lane] = 0;

  // ---- matrix layout state ----
  // query (lane & 31) of a set sits in accumulator register (q & 3) + 4 (q >> 3) of half (q >> 2) & 1
  const int my_slot = (lane & 32) + 16 * ((lane >> 2) & 1) + (lane & 3) + 4 * ((lane & 31) >> 3);
  // offsets change only here, and only between tiles: the accumulators of a tile and its epilogue
  // see the same block
  auto refresh_offsets = [&]() {
    hq_w[my_slot] = -((qn_q - Te) >> 1);
    Te_seen = Te;
    offsets_stale = false;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  auto load_offsets = [&](int s2) __attribute__((always_inline)) -> i32x16 {
    const i32x4* p = reinterpret_cast<const i32x4*>(hq_w + s2 * 32 + 16 * h);
    const i32x4 a0 = p[0], a1 = p[1], a2 = p[2], a3 = p[3];
    return i32x16{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3],
                  a2[0], a2[1], a2[2], a2[3], a3[0], a3[1], a3[2], a3[3]};
  };

  // applies the pending candidates of all 64 queries in lockstep (bf_i8v2_kernel)
  auto flush = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int cnt = min(pc_w[lane], kI8v2Pend);
    pc_w[lane] = 0;
    for (int i = 0; __any(i < cnt); ++i) {
      const bool have = i < cnt;
      const int rd = have ? qn_q - pd_w[i * 64 + lane] : 0x7fffffff;
      const int rid = have ? pi_w[i * 64 + lane] : 0x7fffffff;
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
    Te = min(Te, sd[KPT - 1]);  // "infinity" while the set is not full
    te_w[lane] = Te;
    if (__any(Te != Te_seen))
      offsets_stale = true;  // folded into the offsets before the next tile
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };

  // threshold exchange with the other slices (bf_i8_sets.hpp), between tiles only
  auto refresh = [&]() {
    if (__any(pc_w[lane] > 0))
      flush();
    if (gl_q && my_valid) {
      constexpr int NR = i8_ranks<KPT>();
      [&]<int... I>(std::integer_sequence<int, I...>) {
        ((((a.rank_mask >> I) & 1u)
              ? __hip_atomic_store(gl_q + I * 4 * sl4 + blockIdx.y, sd[i8_rank_pos<KPT>(I)],
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
              : (void)0),
         ...);
        int bound = 0x7fffffff;
        ((bound = ((a.rank_mask >> I) & 1u)
                      ? min(bound, i8_mth_smallest<(KPT + i8_rank_pos<KPT>(I)) / (i8_rank_pos<KPT>(I) + 1)>(
                                       gl_q + I * 4 * sl4, sl4))
                      : bound),
         ...);
        if (bound < 0x7fffffff)
          Te = min(Te, bound + 1);
      }(std::make_integer_sequence<int, NR>{});
      te_w[lane] = Te;
    }
    if (__any(Te != Te_seen))
      offsets_stale = true;
  };

  // ---- staging: a stage is 32 rows x 512 bytes = 1024 pieces of 16 bytes, four per thread (32
  // consecutive threads read 512 contiguous bytes of a row); threads 0..31 carry the row norms.  Every
  // load is unconditional with a clamped address (bf_i8v2_kernel says why): rows past the end of the
  // slice repeat its last row and get the padding norm, columns past D repeat the last 16 and meet
  // zeros in the query operand (chunks past the row are not contracted at all)
  uint4 sv[4];
  int sbn = 0;
  auto stage_load = [&](uint32_t row0, uint32_t col0) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t p = tid + 256 * e, srow = p >> 5, scol = 16 * (p & 31);
      const uint32_t r = min(row0 + srow, end - 1), c = min(col0 + scol, a.D - 16u);
      sv[e] = *reinterpret_cast<const uint4*>(base + static_cast<size_t>(r) * a.D + c);
    }
    sbn = a.bnorm[min(row0 + (tid & 31), end - 1)];
  };
  auto stage_store = [&](uint32_t buf, uint32_t row0) __attribute__((always_inline)) {
    uint8_t* t = lds_b + buf * kI8wStageBytes;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t p = tid + 256 * e, srow = p >> 5, scol = 16 * (p & 31);
      *reinterpret_cast<uint4*>(t + srow * kI8wRowStride + scol) =
          make_uint4(sv[e].x ^ kFlip, sv[e].y ^ kFlip, sv[e].z ^ kFlip, sv[e].w ^ kFlip);
    }
    if (tid < kBfTileRows)  // rows past the end never pass the accumulator test
      *reinterpret_cast<int*>(t + tid * kI8wRowStride + kI8wStageCols) =
          (row0 + tid < end) ? sbn : kI8wPadNorm;
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

  // hits of one tile-set in the matrix layout -> pending lists of the queries (bf_i8v2_kernel)
  auto scan_pass = [&](const i32x16& acc, const i32x16& off, const int s2, int bnv, int b0, int id,
                       unsigned& redo, const bool first) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool hit = first ? (acc[r] > b0) : ((redo >> r) & 1u);
      if (!__any(hit))
        continue;
      redo &= ~(1u << r);
      if (hit) {
        const int q = s2 * 32 + i8v2_qrow(r, h);
        const int slot = atomicAdd(pc_w + q, 1);
        if (slot < kI8v2Pend) {
          pd_w[slot * 64 + q] = 2 * (acc[r] - off[r]) - bnv;  // 2 q'.b' - |b'|^2
          pi_w[slot * 64 + q] = id;
        }
        else
          redo |= 1u << r;
      }
    }
  };
  auto tile_set = [&](const i32x16& acc, const int s2, int bnv, int b0, int id)
                      __attribute__((always_inline)) {
    const i32x16 off = load_offsets(s2);
    unsigned redo = 0;
    scan_pass(acc, off, s2, bnv, b0, id, redo, true);
    while (__any(redo != 0u)) {
      flush();  // (resets the pending counts: the lists have room again)
      scan_pass(acc, off, s2, bnv, b0, id, redo, false);
    }
    if (__any(pc_w[lane] >= kI8v2Pend / 2))
      flush();
  };

  const uint32_t ntiles = end > begin ? (end - begin + kBfTileRows - 1) / kBfTileRows : 0;
  const uint32_t spt = (nch + kI8wStageChunks - 1) / kI8wStageChunks;  // stages per tile
  const uint32_t nsteps = ntiles * spt;
  i32x4 aqa[2][4];
  [[maybe_unused]] i32x4 aqb[2][4];
  if (nsteps) {
    stage_load(begin, 0);
    stage_store(0, begin);
  }
  if constexpr (AHEAD)
    query_load(aqa, 0);
  refresh_offsets();
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
      if (offsets_stale)
        refresh_offsets();
      acc[0] = load_offsets(0);
      acc[1] = load_offsets(1);
    }
    if (has_next)
      stage_load(begin + n_t * kBfTileRows, n_s * kI8wStageCols);
    const uint8_t* trow = lds_b + (p & 1) * kI8wStageBytes + j * kI8wRowStride;
#pragma unroll
    for (uint32_t cc = 0; cc < kI8wStageChunks; ++cc) {
      const uint32_t c = s * kI8wStageChunks + cc;
      if (c >= nch)
        break;  // uniform
      const uint32_t nc = c + 1 < nch ? c + 1 : 0u;  // (after the last chunk: the next tile's first)
      if (AHEAD && (cc & 1))
        chunk(aqb, aqa, trow + 128 * cc, c, nc);
      else
        chunk(aqa, aqb, trow + 128 * cc, c, nc);
    }
    if (last_s) {
      // every stage but the last has four chunks: the sets are out of step after a tile iff nch is odd
      if (AHEAD && (nch & 1u)) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int m = 0; m < 4; ++m)
            aqa[s2][m] = aqb[s2][m];
      }
      const int bnv = *reinterpret_cast<const int*>(trow + kI8wStageCols);
      const int b0 = (bnv == kI8wPadNorm) ? 0x7fffffff : (bnv >> 1);
      int mx0 = acc[0][0], mx1 = acc[1][0];
#pragma unroll
      for (int r = 1; r < 16; r += 2) {
        mx0 = max(max(mx0, acc[0][r]), acc[0][(r + 1) & 15]);
        mx1 = max(max(mx1, acc[1][r]), acc[1][(r + 1) & 15]);
      }
      if (__any(mx0 > b0))
        tile_set(acc[0], 0, bnv, b0, static_cast<int>(row0) + j);
      if (__any(mx1 > b0))
        tile_set(acc[1], 1, bnv, b0, static_cast<int>(row0) + j);
    }
    if (has_next)
      stage_store((p + 1) & 1, begin + n_t * kBfTileRows);
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
      const bool used = sd[k] != 0x7fffffff;
      a.part_ids[o + k] = used ? si[k] : kEmptyKey;
      a.part_dists[o + k] = used ? static_cast<float>(sd[k]) : inf_f();
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------
static size_t bf_i8w_lds_bytes()
{
  return 2 * kI8wStageBytes + (4 * 4 * 64 + 2 * 4 * kI8v2Pend * 64) * sizeof(int);
}

bool bf_i8_wide_supported(const BfLaunch& a)
{
  return (a.dtype == GGNN_U8 || a.dtype == GGNN_I8) && a.measure == GGNN_EUCLIDEAN && a.D > 128 &&
         a.D <= 4096 && a.D % 16 == 0 && a.k_query >= 1 && a.k_query <= 16 && !a.filter_bits &&
         a.Nq >= 256 && a.N_base >= 4096 && hook(kHookBfNoI8) == 0 &&
         bf_i8w_lds_bytes() <= 160 * 1024;
}

// Hook BF_I8_WIDE: 1 never, 2 whenever the launch is supported, 0 auto -- the shape class measured
// against the float32-staged tiles: batches of at least 10000 queries over at least
// 1M rows.  Smaller launches keep the kernels they ran before.
bool bf_i8_wide_routes(const BfLaunch& a)
{
  const int64_t mode = hook(kHookBfI8Wide);
  if (mode == 1 || !bf_i8_wide_supported(a))
    return false;
  return mode == 2 || (a.Nq >= 10000 && a.N_base >= 1000000);
}

size_t bf_i8_wide_packed_words(uint32_t qblocks, uint32_t D)
{
  return static_cast<size_t>(qblocks) * kI8wQueries * ((D + 127) / 128) * 32;
}

void launch_bf_i8_wide_pack(const void* query, uint32_t Nq, uint32_t D, bool is_signed,
                            uint32_t qblocks, uint4* packed, hipStream_t stream)
{
  const uint32_t nch = (D + 127) / 128;
  const uint64_t n16 = bf_i8_wide_packed_words(qblocks, D) / 4;
  const dim3 grid(static_cast<uint32_t>(std::min<uint64_t>((n16 + 255) / 256, 8192)));
  const uint8_t* q = static_cast<const uint8_t*>(query);
  if (is_signed)
    hipLaunchKernelGGL((bf_i8w_pack_kernel<true>), grid, dim3(256), 0, stream, q, Nq, D, nch, n16, packed);
  else
    hipLaunchKernelGGL((bf_i8w_pack_kernel<false>), grid, dim3(256), 0, stream, q, Nq, D, nch, n16, packed);
  GGNN_HIP_CHECK(hipGetLastError());
}

void launch_bf_i8_wide_uncertified(const float* dists, uint32_t Nq, uint32_t K, uint32_t* rescan_list,
                                   uint32_t* rescan_count, hipStream_t stream)
{
  hipLaunchKernelGGL(bf_i8w_uncertified_kernel, dim3((Nq + 255) / 256), dim3(256), 0, stream, dists, Nq,
                     K, rescan_list, rescan_count);
  GGNN_HIP_CHECK(hipGetLastError());
}

void launch_bf_i8_wide(const BfI8WideArgs& m, uint32_t KP, bool is_signed, uint32_t qblocks,
                       uint32_t seed_rows, hipStream_t stream)
{
  GGNN_REQUIRE(KP == 4 || KP == 10 || KP == 16, GGNN_INVALID_ARGUMENT, "unsupported list length");
#define GGNN_I8W(S_)                                                           \
  (KP == 4    ? reinterpret_cast<const void*>(&bf_i8w_kernel<4, S_>)           \
   : KP == 10 ? reinterpret_cast<const void*>(&bf_i8w_kernel<10, S_>)          \
              : reinterpret_cast<const void*>(&bf_i8w_kernel<16, S_>))
  const void* kern = is_signed ? GGNN_I8W(true) : GGNN_I8W(false);
#undef GGNN_I8W
  const size_t lds = bf_i8w_lds_bytes();
  GGNN_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(lds)));
  // seeding launch (hook BF_I8_SEED, as for bf_i8v2_kernel): the first seed_rows rows, all queries, one
  // workgroup per query block, no lists written -- its K-th best distance is every slice's first bound
  const uint32_t seed = std::min(m.N_base, seed_rows / kBfTileRows * kBfTileRows);
  const bool seeded = m.seed && seed >= static_cast<uint32_t>(kBfTileRows) && m.slices > 1;
  if (seeded) {
    BfI8WideArgs w = m;
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
  BfI8WideArgs mm = m;
  mm.seeding = 0;
  if (!seeded)
    mm.seed = nullptr;
  void* kargs[] = {&mm};
  GGNN_HIP_CHECK(hipLaunchKernel(kern, dim3(qblocks, m.slices), dim3(256), kargs, lds, stream));
}

}  // namespace ggnn_amd
