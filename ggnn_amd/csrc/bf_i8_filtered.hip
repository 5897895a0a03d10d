// bf_query with a filter, uint8 / int8 rows under squared L2, K <= 16: the register-set integer kernels
// (bf_i8.hip for rows of up to 128 bytes, bf_i8_wide.hip for 128 < D <= 4096) in a filtered form.  The
// unfiltered kernels keep their code objects; this unit has kernels of its own, bf_i8f_kernel (the query
// operand resident in registers) and bf_i8fw_kernel (the operand streamed from the packed copy), and is
// compiled like those two with -mllvm -amdgpu-mfma-vgpr-form, once per filter mode (Makefile,
// GGNN_I8F_MODE): the per-call bitset (with the host side), the filter table, the labels.
//
// What is taken over unchanged: v_mfma_i32_32x32x32_i8 on bytes shifted to signed, 256 threads, a wave
// owns 64 queries as two 32-query sets that share every B operand; the threshold folded into the
// accumulator offsets, so that a tile without a hit costs 8 v_max3_i32 and one compare per set; hit tiles
// transposed through LDS into lane = query pending lists; sorted K-best sets of 4 / 10 / 16 entries in
// registers; the slice-bound exchange through gthr[] and the seeding launch (bf_i8_sets.hpp).  Norms are
// int32 in both regimes and the row type is a kernel argument (the xor constant 0x80808080 or 0), not a
// template parameter.  Both kernels read their offsets from LDS per tile (bf_i8.hip's LEAN form): the 32
// registers of an offset block are what the filter state and one operand set fit into at two waves per
// SIMD for every list length.  Rows of up to 64 bytes contract two 32-column blocks, longer ones four.
//
// Where the filter enters.  The contraction does not depend on it; only the path from "the accumulator
// passed" to "the candidate takes a pending slot" does.
//   * Per-call bitset: one bitset serves every query, so it is folded into the row constant.  The thread
//     that carries a row's norm through staging also carries that row's bitset word, loaded with the
//     stage's rows by the same unconditional, clamped loads, and stores the padding norm for a denied row
//     as for a row past the end of the slice.  Denied rows never pass the accumulator test; the epilogue
//     is the unfiltered one, instruction for instruction.
//   * Filter table: lane = query picks its row once (the table row, the all-ones row for -1, the all-zero
//     row for any other id: bf_thread_filter_row, an unsigned compare) and carries the words of the coming
//     stage -- one per 32-row tile -- through staging into a double-buffered LDS area of its wave.  Every
//     (query, row) bit is read once per call.  The verdict is taken on the hit path only: a lane whose
//     accumulator r passed tests bit j of the word of query (r, h) before the LDS atomic that takes the
//     slot.  A denied hit takes no slot.
//   * Labels: the row's int32 label is staged beside its norm, the 64 query labels of a wave sit beside
//     its query norms, and denied = (ql != -1) && (ql != row label) at the same point.
//   * A query that can admit nothing -- a filter id that is neither -1 nor a table row -- starts closed
//     (Te = -kTeInf, like a query past Nq): with its unbounded threshold every tile of its wave would be
//     a hit tile.
//
// Why the bounds stay valid.  A set receives admitted rows only.  The position argument of
// bf_i8_sets.hpp -- m slices each hold p + 1 rows at or below B_p, slices hold disjoint rows, so KPT >= K
// rows lie at or below B_p -- then speaks about admitted rows, which are the only rows the filtered top K
// is taken from; a position that a slice has not filled publishes 0x7fffffff and bounds nothing.  The
// seeding launch runs with the filter for the same reason, and seed[q] stays "nothing" when the head of the
// base admits fewer than KPT rows of the query.  A query with fewer than K admitted rows never sees a
// finite bound, so every admitted row is in the union of its sets: slots that never filled leave as
// kEmptyKey / +inf, the re-rank (exact_arith = 1, no filter needed) orders what there is and pads with
// -1 / +inf, as the filtered scan does.
//
// The 2^24 rule (bf_i8_wide.hip's header) holds as it stands for a query with a full set; a query whose
// K-th reported distance is finite and >= 2^24 goes to the filtered re-scan, one with +inf there is
// complete by construction and does not (bf_i8f_uncertified_kernel).
#include <algorithm>

#include "bf_i8_sets.hpp"
#include "bf_thread_filter.hpp"
#include "hooks.hpp"

#ifndef GGNN_I8F_MODE
#define GGNN_I8F_MODE 1
#endif

namespace ggnn_amd {

constexpr uint32_t kI8fStageRows = 128;                       // resident regime: four tiles per barrier
constexpr uint32_t kI8fwStageChunks = 4;                      // streamed regime: 128-byte chunks per stage
constexpr uint32_t kI8fwStageCols = 128 * kI8fwStageChunks;
constexpr uint32_t kI8fwRowStride = kI8fwStageCols + 16;      // + the row's norm and label
constexpr uint32_t kI8fwStageBytes = kBfTileRows * kI8fwRowStride;
constexpr int kI8fPadNorm = 0x3fffffff;                       // rows past the end of a slice, denied rows

// ints of a wave's bookkeeping area: -hq, |q'|^2, pending counts, pending (dist, id), then the filter
// state -- table: [2 buffers][tiles of a stage][64] verdict words; labels: [64] query labels
constexpr uint32_t i8f_wave_ints(int fm, uint32_t stage_tiles)
{
  return 3 * 64 + 2 * kI8v2Pend * 64 + (fm == kI8fTable ? 2 * stage_tiles * 64 : fm == kI8fLabels ? 64 : 0);
}

// the LDS of one wave, in the order above
struct I8fWaveLds {
  int *hq, *qn, *pc, *pd, *pi;
  uint32_t* filt;
  GGNN_DEV I8fWaveLds(int* area, int wave, int fm, uint32_t stage_tiles)
  {
    hq = area + wave * i8f_wave_ints(fm, stage_tiles);
    qn = hq + 64;
    pc = qn + 64;
    pd = pc + 64;
    pi = pd + kI8v2Pend * 64;
    filt = reinterpret_cast<uint32_t*>(pi + kI8v2Pend * 64);
  }
};

// lane = query: the start threshold.  Closed for a query past Nq and for one whose filter id names neither
// a table row nor "unfiltered"
template <int FM>
GGNN_DEV int i8f_start_threshold(const BfI8FilteredArgs& a, uint32_t my_q)
{
  if (my_q >= a.Nq)
    return -kTeInf;
  if constexpr (FM == kI8fTable) {
    const int32_t f = a.filter_table.ids[my_q];
    if (static_cast<uint32_t>(f) >= a.filter_table.num_filters && f != -1)
      return -kTeInf;
  }
  return kTeInf;
}

// the verdict of query q on row j of the tile.  vw: table -- the wave's verdict words of this tile;
// labels -- its query labels
template <int FM>
GGNN_DEV bool i8f_admits(const uint32_t* vw, int q, int j, int row_label)
{
  if constexpr (FM == kI8fTable)
    return (vw[q] >> j) & 1u;
  else if constexpr (FM == kI8fLabels) {
    const int ql = static_cast<int>(vw[q]);
    return ql == -1 || ql == row_label;
  }
  else
    return true;
}

// Hits of one tile-set, in the matrix layout (bf_i8v2_kernel's scan_pass and tile_set): a lane whose
// accumulator r passed the test and whose row the query admits appends (2 q'.b' - |b'|^2, row index) to the
// pending list of query (r, h).  A lane whose list is full remembers the register; the pending candidates
// are applied and the pass runs again for those.
template <int FM, class Flush>
GGNN_DEV void i8f_tile_set(const i32x16& acc, const i32x16& off, const int s2, const int j, const int h,
                           const int lane, const int bnv, const int b0, const int id,
                           const uint32_t* vw, const int row_label, const I8fWaveLds& w, Flush&& flush)
{
  unsigned redo = 0;
  auto pass = [&](const bool first) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool hit = first ? (acc[r] > b0) : ((redo >> r) & 1u);
      if (!__any(hit))
        continue;
      redo &= ~(1u << r);
      if (hit) {
        const int q = s2 * 32 + i8v2_qrow(r, h);
        if (i8f_admits<FM>(vw, q, j, row_label)) {  // a denied hit takes no slot
          const int slot = atomicAdd(w.pc + q, 1);
          if (slot < kI8v2Pend) {
            w.pd[slot * 64 + q] = 2 * (acc[r] - off[r]) - bnv;
            w.pi[slot * 64 + q] = id;
          }
          else
            redo |= 1u << r;
        }
      }
    }
  };
  pass(true);
  while (__any(redo != 0u)) {
    flush();  // (resets the pending counts: the lists have room again)
    pass(false);
  }
  if (__any(w.pc[lane] >= kI8v2Pend / 2))
    flush();
}

// ---- D <= 128: the query operand stays in registers, stages of 128 rows at kBfI8RowStride ---------------
template <int NM, int KPT, int FM>
__global__ void __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(2))) bf_i8f_kernel(const BfI8FilteredArgs a)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_b[];
  constexpr uint32_t SR = kI8fStageRows;
  constexpr uint32_t stage_bytes = SR * kBfI8RowStride;
  constexpr uint32_t TPS = SR / kBfTileRows;
  int* bns = reinterpret_cast<int*>(lds_b + 2 * stage_bytes);  // [2][SR] |b'|^2 or the padding norm
  int* bls = bns + 2 * SR;                                      // labels: [2][SR] row labels
  int* wave_area = bls + (FM == kI8fLabels ? 2 * SR : 0);

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int j = lane & 31, h = lane >> 5;  // matrix layout: base row j of the tile, half h
  // bookkeeping layout: lane = query (lane & 31) of set (lane >> 5)
  const I8fWaveLds w(wave_area, wave, FM, TPS);
  const uint8_t* base = static_cast<const uint8_t*>(a.base);
  const uint8_t* query = static_cast<const uint8_t*>(a.query);
  const uint32_t qw = (blockIdx.x * 4 + wave) * 64;
  const uint32_t begin = blockIdx.y * a.rows_per_slice;
  const uint32_t end = min(a.N_base, begin + a.rows_per_slice);
  const uint32_t flip = a.flip;

  // ---- lane = query state ----
  const uint32_t my_q = qw + lane;
  const bool my_valid = my_q < a.Nq;
  const int qn_q = my_valid ? a.qnorm[my_q] : 0;
  int Te = i8f_start_threshold<FM>(a, my_q);  // candidates need d < Te
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
  int sd[KPT], si[KPT];  // sorted ascending by (distance, index), unused slots hold "infinity"
#pragma unroll
  for (int k = 0; k < KPT; ++k) {
    sd[k] = 0x7fffffff;
    si[k] = 0x7fffffff;
  }
  int Te_seen = 0x7fffffff;
  bool offsets_stale = false;  // wave-uniform
  w.qn[lane] = qn_q;
  w.pc[lane] = 0;
  [[maybe_unused]] const uint32_t* frow = nullptr;  // table: this query's bitset row
  if constexpr (FM == kI8fTable)
    frow = bf_thread_filter_row(a.filter_bits, a.filter_table, my_q, a.Nq);
  if constexpr (FM == kI8fLabels)
    w.filt[lane] = static_cast<uint32_t>(my_valid ? a.filter_table.query_labels[my_q] : -1);

  // ---- matrix layout state ----
  i32x4 aq[2][NM];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    const uint32_t qi = qw + s2 * 32 + j;
    const bool qv = qi < a.Nq;
    const uint8_t* qrow = query + static_cast<size_t>(qv ? qi : 0) * a.D;
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      const uint32_t col = 32 * m + 16 * h;
      aq[s2][m] = i32x4{0, 0, 0, 0};
      if (qv && col < a.D) {
        const uint4 v = *reinterpret_cast<const uint4*>(qrow + col);
        aq[s2][m] = i32x4{static_cast<int>(v.x ^ flip), static_cast<int>(v.y ^ flip),
                          static_cast<int>(v.z ^ flip), static_cast<int>(v.w ^ flip)};
      }
    }
  }
  const int my_slot = i8_offset_slot(lane);
  auto refresh_offsets = [&]() {
    w.hq[my_slot] = -((qn_q - Te) >> 1);
    Te_seen = Te;
    offsets_stale = false;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  auto flush = [&]() {
    i8_apply_pending<KPT>(sd, si, qn_q, w.pc, w.pd, w.pi, lane);
    Te = min(Te, sd[KPT - 1]);  // "infinity" while the set is not full
    if (__any(Te != Te_seen))
      offsets_stale = true;  // folded into the offsets before the next tile
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  auto refresh = [&]() {
    if (__any(w.pc[lane] > 0))
      flush();
    if (gl_q && my_valid) {
      const int bound = i8_exchange_bound<KPT>(sd, gl_q, sl4, blockIdx.y, a.rank_mask);
      if (bound < 0x7fffffff)
        Te = min(Te, bound + 1);
    }
    if (__any(Te != Te_seen))
      refresh_offsets();
  };

  // Staging: a stage of 128 rows is 1024 pieces of 16 bytes, 4 per thread; threads 0..127 carry the row
  // constants -- the norm and, per mode, the row's bitset word or its label; table: every lane carries the
  // four words of its query.  One stage ahead, every load unconditional with a clamped address
  // (bf_i8v2_kernel says why).
  constexpr int PPT = SR / 32;
  uint4 sv[PPT];
  int sbn = 0;
  [[maybe_unused]] uint32_t sfw = 0;       // bitset: the word of this thread's row; labels: its label
  [[maybe_unused]] uint32_t sqw[TPS] = {};  // table: this query's words of the stage's tiles
  auto stage_load = [&](uint32_t row0) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < PPT; ++e) {
      const uint32_t p = tid + 256 * e, srow = p >> 3, scol = 16 * (p & 7);
      const uint32_t r = min(row0 + srow, end - 1), c = min(scol, a.D - 16u);
      sv[e] = *reinterpret_cast<const uint4*>(base + static_cast<size_t>(r) * a.D + c);
    }
    const uint32_t crow = min(row0 + (tid & (SR - 1)), end - 1);
    sbn = a.bnorm[crow];
    if constexpr (FM == kI8fBits)
      sfw = a.filter_bits[(crow + a.filter_bit_offset) >> 5];
    if constexpr (FM == kI8fLabels)
      sfw = filter_word_at(a.filter_bits + a.filter_bit_offset, crow << 2);
    if constexpr (FM == kI8fTable) {
#pragma unroll
      for (uint32_t t = 0; t < TPS; ++t)
        sqw[t] = frow[(min(row0 + t * kBfTileRows, end - 1) + a.filter_bit_offset) >> 5];
    }
  };
  auto stage_store = [&](uint32_t buf, uint32_t row0) __attribute__((always_inline)) {
    uint8_t* t = lds_b + buf * stage_bytes;
#pragma unroll
    for (int e = 0; e < PPT; ++e) {
      const uint32_t p = tid + 256 * e, srow = p >> 3, scol = 16 * (p & 7);
      *reinterpret_cast<uint4*>(t + srow * kBfI8RowStride + scol) =
          make_uint4(sv[e].x ^ flip, sv[e].y ^ flip, sv[e].z ^ flip, sv[e].w ^ flip);
    }
    if (tid < (int)SR) {  // rows past the end and denied rows never pass the accumulator test
      bool keep = row0 + tid < end;
      if constexpr (FM == kI8fBits)
        keep = keep && ((sfw >> ((row0 + tid + a.filter_bit_offset) & 31u)) & 1u);
      bns[buf * SR + tid] = keep ? sbn : kI8fPadNorm;
      if constexpr (FM == kI8fLabels)
        bls[buf * SR + tid] = static_cast<int>(sfw);
    }
    if constexpr (FM == kI8fTable) {
#pragma unroll
      for (uint32_t tt = 0; tt < TPS; ++tt)
        w.filt[(buf * TPS + tt) * 64 + lane] = sqw[tt];
    }
  };

  const uint32_t nstages = (end > begin) ? (end - begin + SR - 1) / SR : 0;
  if (nstages) {
    stage_load(begin);
    stage_store(0, begin);
  }
  refresh_offsets();
  __syncthreads();

  for (uint32_t st = 0; st < nstages; ++st) {
    const uint32_t row0 = begin + st * SR;
    const uint32_t buf = st & 1;
    const uint8_t* blk = lds_b + buf * stage_bytes;
    // (the exchange first: it waits with vmcnt(0), which must not have this stage's staging loads in
    // front of it)
    if (gl_q_any && i8_exchange_stage(st, a.refresh_every))
      refresh();
    if (st + 1 < nstages)
      stage_load(row0 + SR);  // written to the other buffer at the end of this stage
#pragma unroll
    for (int t = 0; t < (int)TPS; ++t) {
      if (row0 + t * kBfTileRows >= end)
        break;  // uniform
      if (offsets_stale)
        refresh_offsets();
      const uint8_t* trow = blk + (t * kBfTileRows + j) * kBfI8RowStride;
      i32x4 b[NM];
#pragma unroll
      for (int m = 0; m < NM; ++m)
        b[m] = *reinterpret_cast<const i32x4*>(trow + 32 * m + 16 * h);
      i32x16 acc[2];
      acc[0] = i8_load_offsets(w.hq, 0, h);
      acc[1] = i8_load_offsets(w.hq, 1, h);
#pragma unroll
      for (int m = 0; m < NM; ++m) {
        acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(aq[0][m], b[m], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(aq[1][m], b[m], acc[1], 0, 0, 0);
      }
      const int bnv = bns[buf * SR + t * kBfTileRows + j];
      const int b0 = (bnv == kI8fPadNorm) ? 0x7fffffff : (bnv >> 1);
      int mx0 = acc[0][0], mx1 = acc[1][0];
#pragma unroll
      for (int r = 1; r < 16; r += 2) {
        mx0 = max(max(mx0, acc[0][r]), acc[0][(r + 1) & 15]);
        mx1 = max(max(mx1, acc[1][r]), acc[1][(r + 1) & 15]);
      }
      const int id = static_cast<int>(row0 + t * kBfTileRows) + j;
      const uint32_t* vw = FM == kI8fTable ? w.filt + (buf * TPS + t) * 64 : w.filt;
      if (__any(mx0 > b0)) {
        const int rl = FM == kI8fLabels ? bls[buf * SR + t * kBfTileRows + j] : 0;
        i8f_tile_set<FM>(acc[0], i8_load_offsets(w.hq, 0, h), 0, j, h, lane, bnv, b0, id, vw, rl, w, flush);
      }
      if (__any(mx1 > b0)) {
        const int rl = FM == kI8fLabels ? bls[buf * SR + t * kBfTileRows + j] : 0;
        i8f_tile_set<FM>(acc[1], i8_load_offsets(w.hq, 1, h), 1, j, h, lane, bnv, b0, id, vw, rl, w, flush);
      }
    }
    if (st + 1 < nstages)
      stage_store((st + 1) & 1, row0 + SR);
    __syncthreads();
  }

  flush();
  if (a.seeding && a.seed && my_valid)
    a.seed[my_q] = sd[KPT - 1];
  if (a.part_ids && my_valid) {
    const size_t o = (static_cast<size_t>(blockIdx.y) * a.Nq + my_q) * KPT;
    i8_write_set<KPT>(sd, si, a.part_ids + o, a.part_dists + o);
  }
}

// ---- 128 < D <= 4096: the query operand streamed from the packed copy, stages of one tile x 512 columns --
template <int KPT, int FM>
__global__ void __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(2))) bf_i8fw_kernel(const BfI8FilteredArgs a)
{
  constexpr bool AHEAD = KPT < 16;  // the query operand is requested one chunk ahead (two register sets)
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_b[];
  int* wave_area = reinterpret_cast<int*>(lds_b + 2 * kI8fwStageBytes);

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int j = lane & 31, h = lane >> 5;  // matrix layout: base row j of the tile, half h
  const I8fWaveLds w(wave_area, wave, FM, 1);
  const uint8_t* base = static_cast<const uint8_t*>(a.base);
  const uint32_t qw = (blockIdx.x * 4 + wave) * 64;
  const uint32_t begin = blockIdx.y * a.rows_per_slice;
  const uint32_t end = min(a.N_base, begin + a.rows_per_slice);
  const uint32_t nch = a.nch;
  const uint32_t flip = a.flip;

  // ---- lane = query state (bf_i8f_kernel) ----
  const uint32_t my_q = qw + lane;
  const bool my_valid = my_q < a.Nq;
  const int qn_q = my_valid ? a.qnorm[my_q] : 0;
  int Te = i8f_start_threshold<FM>(a, my_q);  // candidates need d < Te (d <= 2^28)
  const int sl4 = static_cast<int>((a.slices + 15) / 16 * 4);
  int* gl_q = a.gthr ? reinterpret_cast<int*>(a.gthr) +
                           static_cast<size_t>(my_valid ? my_q : 0) * kI8MaxRanks * 4 * sl4
                     : nullptr;
  const bool gl_q_any = a.gthr != nullptr && a.rank_mask != 0;
  if (my_valid && a.seed && !a.seeding) {
    const int g = a.seed[my_q];
    if (g < 0x7fffffff)
      Te = min(Te, g + 1);
  }
  int sd[KPT], si[KPT];
#pragma unroll
  for (int k = 0; k < KPT; ++k) {
    sd[k] = 0x7fffffff;
    si[k] = 0x7fffffff;
  }
  int Te_seen = 0x7fffffff;
  bool offsets_stale = false;  // wave-uniform
  w.qn[lane] = qn_q;
  w.pc[lane] = 0;
  [[maybe_unused]] const uint32_t* frow = nullptr;  // table: this query's bitset row
  if constexpr (FM == kI8fTable)
    frow = bf_thread_filter_row(a.filter_bits, a.filter_table, my_q, a.Nq);
  if constexpr (FM == kI8fLabels)
    w.filt[lane] = static_cast<uint32_t>(my_valid ? a.filter_table.query_labels[my_q] : -1);

  const int my_slot = i8_offset_slot(lane);
  // offsets change only between tiles: the accumulators of a tile and its epilogue see the same block
  auto refresh_offsets = [&]() {
    w.hq[my_slot] = -((qn_q - Te) >> 1);
    Te_seen = Te;
    offsets_stale = false;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  auto flush = [&]() {
    i8_apply_pending<KPT>(sd, si, qn_q, w.pc, w.pd, w.pi, lane);
    Te = min(Te, sd[KPT - 1]);
    if (__any(Te != Te_seen))
      offsets_stale = true;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  auto refresh = [&]() {
    if (__any(w.pc[lane] > 0))
      flush();
    if (gl_q && my_valid) {
      const int bound = i8_exchange_bound<KPT>(sd, gl_q, sl4, blockIdx.y, a.rank_mask);
      if (bound < 0x7fffffff)
        Te = min(Te, bound + 1);
    }
    if (__any(Te != Te_seen))
      offsets_stale = true;
  };

  // ---- staging: a stage is 32 rows x 512 bytes = 1024 pieces of 16 bytes, four per thread; threads
  // 0..31 carry the row constants (norm; bitset word or label), table: every lane the word of its query for
  // the tile.  Every load unconditional with a clamped address.
  uint4 sv[4];
  int sbn = 0;
  [[maybe_unused]] uint32_t sfw = 0;  // bitset: the word of this thread's row; labels: its label
  [[maybe_unused]] uint32_t sqw = 0;  // table: this query's word of the tile
  auto stage_load = [&](uint32_t row0, uint32_t col0) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t p = tid + 256 * e, srow = p >> 5, scol = 16 * (p & 31);
      const uint32_t r = min(row0 + srow, end - 1), c = min(col0 + scol, a.D - 16u);
      sv[e] = *reinterpret_cast<const uint4*>(base + static_cast<size_t>(r) * a.D + c);
    }
    const uint32_t crow = min(row0 + (tid & 31), end - 1);
    sbn = a.bnorm[crow];
    if constexpr (FM == kI8fBits)
      sfw = a.filter_bits[(crow + a.filter_bit_offset) >> 5];
    if constexpr (FM == kI8fLabels)
      sfw = filter_word_at(a.filter_bits + a.filter_bit_offset, crow << 2);
    if constexpr (FM == kI8fTable)
      sqw = frow[(min(row0, end - 1) + a.filter_bit_offset) >> 5];
  };
  // tile: the tile of the slice that the stage belongs to
  auto stage_store = [&](uint32_t buf, uint32_t row0, uint32_t tile) __attribute__((always_inline)) {
    uint8_t* t = lds_b + buf * kI8fwStageBytes;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t p = tid + 256 * e, srow = p >> 5, scol = 16 * (p & 31);
      *reinterpret_cast<uint4*>(t + srow * kI8fwRowStride + scol) =
          make_uint4(sv[e].x ^ flip, sv[e].y ^ flip, sv[e].z ^ flip, sv[e].w ^ flip);
    }
    if (tid < kBfTileRows) {  // rows past the end and denied rows never pass the accumulator test
      bool keep = row0 + tid < end;
      if constexpr (FM == kI8fBits)
        keep = keep && ((sfw >> ((row0 + tid + a.filter_bit_offset) & 31u)) & 1u);
      int* rc = reinterpret_cast<int*>(t + tid * kI8fwRowStride + kI8fwStageCols);
      rc[0] = keep ? sbn : kI8fPadNorm;
      if constexpr (FM == kI8fLabels)
        rc[1] = static_cast<int>(sfw);
    }
    if constexpr (FM == kI8fTable)
      w.filt[(tile & 1u) * 64 + lane] = sqw;  // (every stage of a tile writes the same word)
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

  const uint32_t ntiles = end > begin ? (end - begin + kBfTileRows - 1) / kBfTileRows : 0;
  const uint32_t spt = (nch + kI8fwStageChunks - 1) / kI8fwStageChunks;  // stages per tile
  const uint32_t nsteps = ntiles * spt;
  i32x4 aqa[2][4];
  [[maybe_unused]] i32x4 aqb[2][4];
  if (nsteps) {
    stage_load(begin, 0);
    stage_store(0, begin, 0);
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
      if (gl_q_any && i8_exchange_stage(t, a.refresh_every))
        refresh();
      if (offsets_stale)
        refresh_offsets();
      acc[0] = i8_load_offsets(w.hq, 0, h);
      acc[1] = i8_load_offsets(w.hq, 1, h);
    }
    if (has_next)
      stage_load(begin + n_t * kBfTileRows, n_s * kI8fwStageCols);
    const uint8_t* trow = lds_b + (p & 1) * kI8fwStageBytes + j * kI8fwRowStride;
#pragma unroll
    for (uint32_t cc = 0; cc < kI8fwStageChunks; ++cc) {
      const uint32_t c = s * kI8fwStageChunks + cc;
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
      const int* rc = reinterpret_cast<const int*>(trow + kI8fwStageCols);
      const int bnv = rc[0];
      const int b0 = (bnv == kI8fPadNorm) ? 0x7fffffff : (bnv >> 1);
      int mx0 = acc[0][0], mx1 = acc[1][0];
#pragma unroll
      for (int r = 1; r < 16; r += 2) {
        mx0 = max(max(mx0, acc[0][r]), acc[0][(r + 1) & 15]);
        mx1 = max(max(mx1, acc[1][r]), acc[1][(r + 1) & 15]);
      }
      const int id = static_cast<int>(row0) + j;
      const uint32_t* vw = FM == kI8fTable ? w.filt + (t & 1u) * 64 : w.filt;
      if (__any(mx0 > b0))
        i8f_tile_set<FM>(acc[0], i8_load_offsets(w.hq, 0, h), 0, j, h, lane, bnv, b0, id, vw,
                         FM == kI8fLabels ? rc[1] : 0, w, flush);
      if (__any(mx1 > b0))
        i8f_tile_set<FM>(acc[1], i8_load_offsets(w.hq, 1, h), 1, j, h, lane, bnv, b0, id, vw,
                         FM == kI8fLabels ? rc[1] : 0, w, flush);
    }
    if (has_next)
      stage_store((p + 1) & 1, begin + n_t * kBfTileRows, n_t);
    __syncthreads();
    t = n_t;
    s = n_s;
  }

  flush();
  if (a.seeding && a.seed && my_valid)
    a.seed[my_q] = sd[KPT - 1];
  if (a.part_ids && my_valid) {
    const size_t o = (static_cast<size_t>(blockIdx.y) * a.Nq + my_q) * KPT;
    i8_write_set<KPT>(sd, si, a.part_ids + o, a.part_dists + o);
  }
}

// ---- the kernels of this object's filter mode ------------------------------------------------------------
#if GGNN_I8F_MODE == 1
#define GGNN_I8F_GETTER bf_i8f_bits_kernel
#elif GGNN_I8F_MODE == 2
#define GGNN_I8F_GETTER bf_i8f_table_kernel
#else
#define GGNN_I8F_GETTER bf_i8f_labels_kernel
#endif
const void* GGNN_I8F_GETTER(int nm, uint32_t KP)
{
  constexpr int FM = GGNN_I8F_MODE;
  GGNN_REQUIRE(KP == 4 || KP == 10 || KP == 16, GGNN_INVALID_ARGUMENT, "unsupported list length");
#define GGNN_I8F(NM_)                                                            \
  (KP == 4    ? reinterpret_cast<const void*>(&bf_i8f_kernel<NM_, 4, FM>)        \
   : KP == 10 ? reinterpret_cast<const void*>(&bf_i8f_kernel<NM_, 10, FM>)       \
              : reinterpret_cast<const void*>(&bf_i8f_kernel<NM_, 16, FM>))
  if (nm == 2)
    return GGNN_I8F(2);
  if (nm == 4)
    return GGNN_I8F(4);
#undef GGNN_I8F
  return KP == 4    ? reinterpret_cast<const void*>(&bf_i8fw_kernel<4, FM>)
         : KP == 10 ? reinterpret_cast<const void*>(&bf_i8fw_kernel<10, FM>)
                    : reinterpret_cast<const void*>(&bf_i8fw_kernel<16, FM>);
}
#undef GGNN_I8F_GETTER

// ---- host (in the bitset object) ---------------------------------------------------------------------------
#if GGNN_I8F_MODE == 1
__global__ void __launch_bounds__(256) bf_i8f_uncertified_kernel(const float* dists, uint32_t Nq, uint32_t K,
                                                                uint32_t* rescan_list,
                                                                uint32_t* rescan_count)
{
  const uint32_t n = blockIdx.x * 256 + threadIdx.x;
  if (n >= Nq)
    return;
  const float d = dists[static_cast<size_t>(n) * K + K - 1];
  if (d >= 16777216.f && d < inf_f())  // (+inf: fewer than K admitted rows, all of them reported)
    rescan_list[atomicAdd(rescan_count, 1u)] = n;
}

size_t bf_i8f_lds_bytes(int fm, bool wide)
{
  if (wide)
    return 2 * kI8fwStageBytes + 4 * i8f_wave_ints(fm, 1) * sizeof(int);
  return 2 * kI8fStageRows * kBfI8RowStride +
         ((fm == kI8fLabels ? 4 : 2) * kI8fStageRows + 4 * i8f_wave_ints(fm, kI8fStageRows / kBfTileRows)) *
             sizeof(int);
}

bool bf_i8_filtered_supported(const BfLaunch& a)
{
  if (!a.filter_bits || a.label_sets.labels || a.label_ranges.labels || a.label_masks.labels)
    return false;
  const bool bits = !a.filter_table.query_labels;
  return (a.dtype == GGNN_U8 || a.dtype == GGNN_I8) && a.measure == GGNN_EUCLIDEAN && a.D >= 16 &&
         a.D <= 4096 && a.D % 16 == 0 && a.k_query >= 1 && a.k_query <= 16 && a.Nq >= 256 &&
         a.N_base >= 4096 && a.N_base <= 0x7fffffffu && !(bits && a.filter_bit_offset % 32 != 0) &&
         static_cast<uint64_t>(a.filter_bit_offset) + a.N_base <= 0xffffffffull &&
         !(a.filter_table.query_labels && a.filter_table.ids) && hook(kHookBfNoI8) == 0;
}

// Hook BF_I8_FILTERED: 1 never (the routing without these kernels), 2 whenever the launch is supported,
// 0 auto -- the shape class measured against that routing (both types, both row regimes and
// all three filter modes were faster at every density): batches of at least 10000 queries over at least 1M
// rows.  Smaller launches keep the kernels they ran before.
bool bf_i8_filtered_routes(const BfLaunch& a)
{
  const int64_t mode = hook(kHookBfI8Filtered);
  if (mode == 1 || !bf_i8_filtered_supported(a))
    return false;
  return mode == 2 || (a.Nq >= 10000 && a.N_base >= 1000000);
}

void launch_bf_i8_filtered_uncertified(const float* dists, uint32_t Nq, uint32_t K, uint32_t* rescan_list,
                                       uint32_t* rescan_count, hipStream_t stream)
{
  hipLaunchKernelGGL(bf_i8f_uncertified_kernel, dim3((Nq + 255) / 256), dim3(256), 0, stream, dists, Nq,
                     K, rescan_list, rescan_count);
  GGNN_HIP_CHECK(hipGetLastError());
}

void launch_bf_i8_filtered(const BfI8FilteredArgs& m, int fm, uint32_t KP, uint32_t qblocks,
                           uint32_t seed_rows, hipStream_t stream)
{
  const bool wide = m.D > 128;
  const int nm = wide ? 0 : m.D <= 64 ? 2 : 4;
  const void* kern = fm == kI8fBits    ? bf_i8f_bits_kernel(nm, KP)
                     : fm == kI8fTable ? bf_i8f_table_kernel(nm, KP)
                                       : bf_i8f_labels_kernel(nm, KP);
  const size_t lds = bf_i8f_lds_bytes(fm, wide);
  GGNN_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(lds)));
  // seeding launch (hook BF_I8_SEED): the first seed_rows rows, all queries under their filters, one
  // workgroup per query block, no lists written -- its K-th best admitted distance is every slice's first
  // bound
  const uint32_t quant = wide ? static_cast<uint32_t>(kBfTileRows) : kI8fStageRows;
  const uint32_t seed = std::min(m.N_base, seed_rows / quant * quant);
  const bool seeded = m.seed && seed >= quant && m.slices > 1;
  if (seeded) {
    BfI8FilteredArgs s = m;
    s.part_ids = nullptr;
    s.part_dists = nullptr;
    s.N_base = seed;
    s.rows_per_slice = seed;
    s.slices = 1;
    s.gthr = nullptr;
    s.rank_mask = 0;
    s.seeding = 1;
    void* sargs[] = {&s};
    GGNN_HIP_CHECK(hipLaunchKernel(kern, dim3(qblocks, 1), dim3(256), sargs, lds, stream));
  }
  BfI8FilteredArgs mm = m;
  mm.seeding = 0;
  if (!seeded)
    mm.seed = nullptr;
  void* kargs[] = {&mm};
  GGNN_HIP_CHECK(hipLaunchKernel(kern, dim3(qblocks, m.slices), dim3(256), kargs, lds, stream));
}
#endif  // GGNN_I8F_MODE == 1

}  // namespace ggnn_amd
