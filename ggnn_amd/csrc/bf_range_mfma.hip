// bf_range on the matrix cores: the tile kernels pre-select, every hit is decided exactly.
//
// The scan of bf_range.hip reads the whole base once per query and pass.  Here the base is read once
// per block of 128 queries: Q x B^T on v_mfma_f32_32x32x2_f32 gives the expanded-form distance d_e of
// every pair, and a pair becomes a CANDIDATE iff the filter admits it and d_e does not exceed a
// threshold that no hit can exceed (below).  Candidates are then evaluated with the direct form
// (DistEngine, compute_distances: the scan's bits) and compared with the radius itself, so lims, ids
// and dists are bit for bit what the scan returns.  All device memory, nothing waits for the host,
// no atomic decides a position:
//   thr      bf_range_thr_kernel: one threshold per query (NaN: the query has no candidates)
//   count    bf_range_tile_kernel<FILL = false>: candidates per (query, part), a part being a
//            contiguous, tile-aligned row range; parts ascend with the rows
//   prefix   bf_range_prefix_kernel (bf_range.hip): candidate offsets and cand_lims[Nq]
//   budget   the candidate buffer was allocated before anything was known about the data; if
//            cand_lims[Nq] exceeds it a flag is set, the passes below leave at once and the scan
//            passes of bf_range.hip -- always enqueued behind this path, gated by the flag -- answer
//   fill     bf_range_tile_kernel<FILL = true>: the same predicate on the same bits; the lane that
//            owns a verdict writes the row id at offset + candidates before it: ascending ids
//   exact    bf_range_exact_kernel: one wave per (query, part) evaluates its candidates in blocks
//            of kKBlock, leaves the distance beside the id and counts d <= r
//   prefix   again: lims and the hit offsets
//   compact  bf_range_compact_kernel: if lims[Nq] <= capacity every (query, part) copies its hits
//            to ids / dists by ballot + popcount, ascending id preserved
//
// Why the pre-selection loses no hit (the model of bf_mfma.hip: u = 2^-24, a = fl(q - mu),
// b = fl(x - mu), any summation order)
//     |d_e - ||a-b||^2|  <= (2D+4) u (|a|^2+|b|^2)
//     | ||a-b||^2 - ||q-x||^2 | <= 4u (|a|^2+|b|^2)
//     d_dir >= ||q-x||^2 (1 - (D+3)u)
//   so d_dir <= r implies
//     d_e <= r / (1 - 1.01 (D+3) u) + 1.01 (2D+8) u (|a|^2+|b|^2) + (2D+8) 2^-125.
//   The kernel uses the norm of the row itself, which the tile carries anyway: with c >= 1.01 (2D+8) u
//     candidate  iff  !( fl(d_e - c |b|^2) > t ),   t >= r / (1 - 1.01 (D+3) u) + c |a|^2 + (2D+8) 2^-125
//   (rounding is monotonic: a real value <= the float t rounds to a float <= t; c and t are formed
//   with 1.02 in place of 1.01 and a few ulps on top, which covers their own roundings).  Cosine:
//   both forms are within (2D+8)u of the true value, t = r + 2.02 (2D+8) u.  The negated compare
//   makes a NaN d_e a candidate; rows past the end of a part and queries without candidates (NaN or
//   negative radius, padding) are masked out of the ballots, which are wave-uniform.
#include <algorithm>
#include <cstdlib>

#define GGNN_BF_SHARED_ONLY
#include "bf_mfma.hip"  // norms, TileStage, FilterStage, the query operand, mfma_chain, bf_expand

namespace ggnn_amd {

template <int FM>
struct BfRangeTileArgs : BfMfmaArgsOf<FM> {
  // (of the base struct: base, query, query_packed, mean, bnorm, qnorm, D, Nq, N_base, DM,
  // slices = parts per query, rows_per_slice = rows per part, and the filter)
  const float* thr;           // [Nq] thresholds (NaN: no candidates)
  float c;                    // squared L2: coefficient of |b|^2 in the compare
  uint32_t* counts;           // [Nq x parts], written by the count pass
  const uint64_t* offsets;    // [Nq x parts] exclusive, read by the fill pass
  const uint64_t* cand_lims;  // [Nq + 1]
  uint64_t budget;            // entries of cand_ids
  int32_t* cand_ids;
};

// one threshold per query (see the top of this file); qnorm: |a|^2 as the tile kernel sees it
template <int MODE>
__global__ void __launch_bounds__(256) bf_range_thr_kernel(const float* radii, const float* qnorm,
                                                          uint32_t Nq, float Df, float c, float* thr)
{
  const uint32_t n = blockIdx.x * 256 + threadIdx.x;
  if (n >= Nq)
    return;
  constexpr float u = 5.9604645e-8f;  // 2^-24
  const float r = radii[n];
  // (the constants 1.02, 2.04 and the 16 ulps, and c on the host, are restated by thresholds() of
  // tests/test_bf_range_threshold_math.py: change them together)
  float t;
  if (MODE == kL2) {
    t = r / (1.f - 1.02f * (Df + 3.f) * u);
    t = fmaf(c, qnorm[n], t);
    t += (2.f * Df + 8.f) * 2.3509887e-38f;
  }
  else
    t = r + 2.04f * (2.f * Df + 8.f) * u;
  t += 16.f * u * t;  // (t >= 0 here or unused; +inf stays +inf)
  thr[n] = (r >= 0.f) ? t : __uint_as_float(0x7fc00000u);
}

// Workgroup = 4 waves x 32 queries against base tiles of 32 rows, double buffered in LDS with the
// padded row stride of bf_mfma_kernel; one 32x32 accumulator tile per wave; LDS holds tiles, the
// shift vector and per-query words, no lists.
// CH = false: one chunk of 2*Dh = 8*NU columns (D <= 128), the query operand stays in registers.
// CH = true (NU = 16): rows stream through the stages in chunks of 128 columns into the same
//   accumulators, the query chunk of the next pair comes from the packed copy (QueryWindow) while
//   the chain of this one runs.
// Epilogue per tile: d_e, the filter verdict, the compare, one ballot per accumulator register --
// register r holds query rows qa = (r&3) + 8*(r>>2) (lanes 0..31) and qa + 4 (lanes 32..63), so a
// ballot is the 32 row verdicts of two queries.  Count: lane q of the wave keeps the count of its
// query q.  Fill: the lane that owns a set bit writes its row at offset + count so far + set bits
// below it.  Count and fill are one body with one `if constexpr`: they cannot disagree.
template <typename BaseT, int MODE, int FM, bool FILL, bool CH, int NU>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(CH ? 2 : 3)))
    bf_range_tile_kernel(const BfRangeTileArgs<FM> a)
{
  static_assert(!CH || NU == 16, "chunks are 128 columns");
  extern __shared__ __attribute__((aligned(16))) float lds_f[];
  constexpr uint32_t Dh = 4 * NU, CW = 2 * Dh, DP = CW + ((CW % 8 == 0) ? 4 : 8);
  constexpr uint32_t tile_floats = kBfTileRows * DP;
  float* mean_lds = lds_f + 2 * tile_floats;
  float* qn_lds = mean_lds + a.DM;
  float* thr_lds = qn_lds + kBfQueriesPerBlock;
  [[maybe_unused]] uint32_t* filt_lds = reinterpret_cast<uint32_t*>(thr_lds + kBfQueriesPerBlock);
  // (fill pass: the 128 candidate offsets of this (query block, part) behind the verdict area)
  [[maybe_unused]] uint64_t* off_lds =
      reinterpret_cast<uint64_t*>(filt_lds + bf_filter_lds_words(FM, 1));

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  if constexpr (FILL) {
    // the candidates do not fit their buffer: the scan answers the call (wave-uniform)
    if (a.cand_lims[a.Nq] > a.budget)
      return;
  }
  const BaseT* base = static_cast<const BaseT*>(a.base);
  const uint32_t qblock = blockIdx.x, part = blockIdx.y;
  const uint32_t begin = min(a.N_base, part * a.rows_per_slice);
  const uint32_t end = min(a.N_base, begin + a.rows_per_slice);
  const uint32_t qbase = (qblock * 4 + wave) * 32;
  const uint32_t nch = CH ? (a.D + CW - 1) / CW : 1u;

  for (uint32_t i = tid; i < a.DM; i += 256)
    mean_lds[i] = (a.mean && i < a.D) ? a.mean[i] : 0.f;
  uint32_t livebits;  // bit q: query q of this wave exists and has a threshold (wave-uniform)
  {
    const uint32_t qi = qbase + (lane & 31);
    const bool qok = qi < a.Nq;
    const float t = qok ? a.thr[qi] : __uint_as_float(0x7fc00000u);
    livebits = static_cast<uint32_t>(__ballot(lane < 32 && t == t));
    if (lane < 32) {  // this wave's entries only: nothing to order against the other waves
      qn_lds[wave * 32 + lane] = qok ? a.qnorm[qi] : 0.f;
      thr_lds[wave * 32 + lane] = t;
      if constexpr (FM == kBfLabels)
        reinterpret_cast<int32_t*>(filt_lds)[wave * 32 + lane] =
            qok ? a.filter_table.query_labels[qi] : -1;
      if constexpr (FILL)
        off_lds[wave * 32 + lane] =
            qok ? a.offsets[static_cast<size_t>(qi) * a.slices + part] : 0ull;
    }
  }
  TileStage<BaseT> stage;
  FilterStage<FM> fstage;
  fstage.open(a, qblock);
  __syncthreads();
  const uint32_t ntiles = (end - begin + kBfTileRows - 1) / kBfTileRows;
  // (rows past the end of the part get the norm 0: their verdicts are masked, and with +inf the
  // squared-L2 compare would see inf - inf)
  if (ntiles) {
    stage.load(base, a.D, begin, end, 0, CW, a.bnorm, 0.f);
    fstage.load(a, begin, end);
    stage.store_shifted(lds_f, DP, CW, mean_lds, 0);
    fstage.store_single(lds_f, DP, CW, filt_lds, 0);
  }
  __syncthreads();

  float aq[64];
  [[maybe_unused]] QueryWindow qw;
  if constexpr (CH) {
    qw.open(a.query_packed, nch, qblock, wave, lane);
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const float4 v = qw.piece(h * Dh, t);
      aq[4 * t + 0] = v.x;
      aq[4 * t + 1] = v.y;
      aq[4 * t + 2] = v.z;
      aq[4 * t + 3] = v.w;
    }
  }
  else {
    const bool qvalid = qbase + j < a.Nq;
    const BaseT* qrow = static_cast<const BaseT*>(a.query) + static_cast<size_t>(qvalid ? qbase + j : 0) * a.D;
    load_query_chunk(aq, qrow, qvalid, a.D, Dh, h * Dh);
    // (everything loaded so far has arrived before the loop: see bf_mfma_kernel)
    __builtin_amdgcn_s_waitcnt(0x0F70);
  }
  const float* qn_w = qn_lds + wave * 32;
  const float* thr_w = thr_lds + wave * 32;
  uint32_t cnt = 0;  // lane q < 32: candidates of query q of this wave so far
  uint32_t p = 0;    // (tile, chunk) pairs processed: buffer p & 1 holds the current pair
  for (uint32_t tt = 0; tt < ntiles; ++tt) {
    f32x16 acc = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (uint32_t c = 0; c < nch; ++c) {
      // the pair after this one: next chunk of the tile, else the first chunk of the next tile
      const bool next_chunk = c + 1 < nch;
      const bool has_next = next_chunk || tt + 1 < ntiles;
      const uint32_t n_row0 = begin + (next_chunk ? tt : tt + 1) * kBfTileRows;
      const uint32_t n_col0 = next_chunk ? (c + 1) * CW : 0u;
      if (has_next) {
        stage.load(base, a.D, n_row0, end, n_col0, CW, a.bnorm, 0.f);
        fstage.load(a, n_row0, end);
      }
      const uint32_t buf = p & 1;
      const float* bt = lds_f + buf * tile_floats + j * DP + h * Dh;
      if constexpr (CH)
        mfma_chain<NU, true>(acc, aq, bt, qw, n_col0 + h * Dh);
      else {
#pragma unroll
        for (int u = 0; u < NU; ++u) {
          const float4 bv = *reinterpret_cast<const float4*>(bt + 4 * u);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[4 * u + 0], bv.x, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[4 * u + 1], bv.y, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[4 * u + 2], bv.z, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[4 * u + 3], bv.w, acc, 0, 0, 0);
        }
      }
      if (!next_chunk) {
        // ---- epilogue of tile tt (norm, label and verdict words sit in buffer `buf`) -----------
        const uint32_t row0 = begin + tt * kBfTileRows;
        const uint32_t rows = min(static_cast<uint32_t>(kBfTileRows), end - row0);
        const uint32_t rm = rows >= 32u ? ~0u : (1u << rows) - 1u;
        const float bn = lds_f[buf * tile_floats + j * DP + CW];
        [[maybe_unused]] int32_t row_label = 0;
        if constexpr (FM == kBfLabels)
          row_label = reinterpret_cast<const int32_t*>(lds_f)[buf * tile_floats + j * DP + CW + 1];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4 qn4 = *reinterpret_cast<const float4*>(qn_w + 8 * g + 4 * h);
          const float4 th4 = *reinterpret_cast<const float4*>(thr_w + 8 * g + 4 * h);
          const float qn[4] = {qn4.x, qn4.y, qn4.z, qn4.w};
          const float th[4] = {th4.x, th4.y, th4.z, th4.w};
          [[maybe_unused]] uint32_t fw[4] = {0u, 0u, 0u, 0u};
          [[maybe_unused]] int32_t ql[4] = {0, 0, 0, 0};
          if constexpr (FM == kBfBits) {
            const uint4 fw4 = *reinterpret_cast<const uint4*>(
                filt_lds + buf * kBfQueriesPerBlock + wave * 32 + 8 * g + 4 * h);
            fw[0] = fw4.x, fw[1] = fw4.y, fw[2] = fw4.z, fw[3] = fw4.w;
          }
          if constexpr (FM == kBfLabels) {
            const int4 ql4 = *reinterpret_cast<const int4*>(
                reinterpret_cast<const int32_t*>(filt_lds) + wave * 32 + 8 * g + 4 * h);
            ql[0] = ql4.x, ql[1] = ql4.y, ql[2] = ql4.z, ql[3] = ql4.w;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int qa = e + 8 * g, qb = qa + 4;
            const float d = bf_expand<MODE>(acc[4 * g + e], qn[e], bn, true);
            const float x = (MODE == kL2) ? fmaf(-a.c, bn, d) : d;
            bool cand = !(x > th[e]);
            if constexpr (FM == kBfBits)
              cand = cand && ((fw[e] >> j) & 1u);
            if constexpr (FM == kBfLabels)
              cand = cand && !bf_label_denied(ql[e], row_label);
            // rows that exist, of queries that have a threshold (scalar masks)
            const uint32_t lo = static_cast<uint32_t>((livebits >> qa) & 1u ? rm : 0u);
            const uint32_t hi = static_cast<uint32_t>((livebits >> qb) & 1u ? rm : 0u);
            const unsigned long long m =
                __ballot(cand) & (static_cast<unsigned long long>(lo) |
                                  (static_cast<unsigned long long>(hi) << 32));
            const uint32_t m_lo = static_cast<uint32_t>(m), m_hi = static_cast<uint32_t>(m >> 32);
            if constexpr (FILL) {
              if (m) {  // (wave-uniform, and rare)
                const uint32_t run_a = __builtin_amdgcn_readlane(static_cast<int>(cnt), qa);
                const uint32_t run_b = __builtin_amdgcn_readlane(static_cast<int>(cnt), qb);
                const uint32_t half = h ? m_hi : m_lo;
                if ((half >> j) & 1u) {
                  const uint64_t pos = off_lds[wave * 32 + (h ? qb : qa)] + (h ? run_b : run_a) +
                                       __popc(half & ((1u << j) - 1u));
                  // (pos < cand_lims[Nq] <= budget whenever the inputs are those of the count pass)
                  if (pos < a.budget)
                    a.cand_ids[pos] = static_cast<int32_t>(row0 + j);
                }
              }
            }
            cnt += lane == qa ? __popc(m_lo) : lane == qb ? __popc(m_hi) : 0u;
          }
        }
      }
      if (has_next) {
        float* nt = lds_f + ((p + 1) & 1) * tile_floats;
        stage.store_shifted(nt, DP, CW, mean_lds, n_col0);
        fstage.store_single(nt, DP, CW, filt_lds, (p + 1) & 1);
      }
      __syncthreads();
      ++p;
    }
  }
  if constexpr (!FILL) {
    if (lane < 32 && qbase + lane < a.Nq)
      a.counts[static_cast<size_t>(qbase + lane) * a.slices + part] = cnt;
  }
}

// ---- budget, exact evaluation, compaction ---------------------------------------------------------
// flag = the candidates do not fit (the gate of the scan passes); fell_back: optional copy
__global__ void bf_range_budget_kernel(const uint64_t* cand_lims, uint32_t Nq, uint64_t budget,
                                       uint32_t* flag, uint32_t* fell_back)
{
  const uint32_t over = cand_lims[Nq] > budget ? 1u : 0u;
  *flag = over;
  if (fell_back)
    *fell_back = over;
}

// the scan passes wrote lims of their own: they become the call's if the scan answered
__global__ void __launch_bounds__(256) bf_range_take_lims_kernel(const uint32_t* flag,
                                                                const uint64_t* from, uint32_t n,
                                                                uint64_t* lims)
{
  if (*flag == 0)
    return;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
    lims[i] = from[i];
}

struct BfRangeExactArgs {
  const void* base;
  const void* query;
  const float* radii;
  const uint32_t* cand_counts;   // [Nq x parts]
  const uint64_t* cand_offsets;  // [Nq x parts]
  const uint64_t* cand_lims;     // [Nq + 1]
  const int32_t* cand_ids;
  float* cand_dists;             // direct-form distance of every candidate, beside its id
  uint32_t* hit_counts;          // [Nq x parts]
  uint64_t budget;
  uint32_t D, Nq, N_base, parts;
};

// One wave per (query, part): the direct form of the part's candidates in blocks of kKBlock, as
// bf_rerank_kernel evaluates its lists -- the scan's bits.
template <typename BaseT, int LPR, int NCH, int MODE>
__global__ void __launch_bounds__(kWave) bf_range_exact_kernel(const BfRangeExactArgs a)
{
  __shared__ __attribute__((aligned(16))) int lds_raw[WaveLds::extra_ints];
  const WaveLds lds(lds_raw, 0);
  const int lane = threadIdx.x;
  const uint32_t bid = block_linear_index();
  if (bid >= a.Nq * a.parts)
    return;
  if (a.cand_lims[a.Nq] > a.budget) {  // the scan answers: nothing was filled (wave-uniform)
    if (lane == 0)
      a.hit_counts[bid] = 0;
    return;
  }
  const uint32_t n = bid / a.parts;
  const float r = a.radii[n];
  const uint64_t off = a.cand_offsets[bid];
  const uint32_t total = a.cand_counts[bid];
  const BaseT* base = static_cast<const BaseT*>(a.base);
  DistEngine<BaseT, LPR, NCH> de;
  de.template load_query<MODE>(base, a.D, static_cast<const BaseT*>(a.query) + static_cast<size_t>(n) * a.D);
  uint32_t hits = 0;
  for (uint32_t c0 = 0; c0 < total; c0 += kKBlock) {
    const int nsurv = static_cast<int>(min(kKBlock, total - c0));
    __syncthreads();
    if (lane < nsurv)  // (ids are rows of the base; the clamp keeps a wrong one inside it)
      lds.ckeys[lane] = static_cast<int>(
          min(static_cast<uint32_t>(a.cand_ids[off + c0 + lane]), a.N_base - 1));
    __syncthreads();
    compute_distances<MODE>(de, lds, nsurv, nullptr);
    __syncthreads();
    bool hit = false;
    if (lane < nsurv) {
      const float d = lds.cd0[lane];
      a.cand_dists[off + c0 + lane] = d;
      hit = d <= r;  // NaN on either side is no hit, as in the scan
    }
    hits += __popcll(__ballot(hit));
  }
  if (lane == 0)
    a.hit_counts[bid] = hits;
}

// One wave per (query, part): its hits, in candidate order (ascending id), to ids / dists.
__global__ void __launch_bounds__(kWave) bf_range_compact_kernel(const BfRangeCompactArgs a)
{
  const int lane = threadIdx.x;
  const uint32_t bid = block_linear_index();
  if (bid >= a.Nq * a.parts)
    return;
  // the scan answers, or the total does not fit: nothing is written (wave-uniform)
  if (a.cand_lims[a.Nq] > a.budget || a.lims[a.Nq] > a.capacity)
    return;
  const float r = a.radii[bid / a.parts];
  const uint64_t off = a.cand_offsets[bid];
  const uint32_t total = a.cand_counts[bid];
  uint64_t out = a.hit_offsets[bid];
  for (uint32_t c0 = 0; c0 < total; c0 += kWave) {
    const bool valid = c0 + lane < total;
    const float d = valid ? a.cand_dists[off + c0 + lane] : 0.f;
    const int32_t id = valid ? a.cand_ids[off + c0 + lane] : 0;
    const bool hit = valid && d <= r;
    const unsigned long long m = __ballot(hit);
    const uint64_t pos = out + __popcll(m & ((1ull << lane) - 1ull));
    if (hit && pos < a.capacity) {
      a.ids[pos] = id;
      a.dists[pos] = d;
    }
    out += __popcll(m);
  }
}

// ---- host -----------------------------------------------------------------------------------------
void launch_bf_range_compact(const BfRangeCompactArgs& cp, hipStream_t stream)
{
  hipLaunchKernelGGL(bf_range_compact_kernel, grid_for(static_cast<uint64_t>(cp.Nq) * cp.parts),
                     dim3(kWave), 0, stream, cp);
  GGNN_HIP_CHECK(hipGetLastError());
}

void launch_bf_range_take_lims(const uint32_t* flag, const uint64_t* from, uint32_t n, uint64_t* lims,
                               hipStream_t stream)
{
  hipLaunchKernelGGL(bf_range_take_lims_kernel, dim3(std::min((n + 255) / 256, 1024u)), dim3(256), 0,
                     stream, flag, from, n, lims);
  GGNN_HIP_CHECK(hipGetLastError());
}

static int bf_range_filter_mode(const BfRangeLaunch& a)
{
  return !a.filter_bits ? kBfNoFilter : a.filter_table.query_labels ? kBfLabels : kBfBits;
}

bool bf_range_mfma_supported(const BfRangeLaunch& a)
{
  const int64_t path = hook(kHookBfRangePath);
  if (path == 1)
    return false;
  if (a.dtype != GGNN_F32 && a.dtype != GGNN_F16 && a.dtype != GGNN_BF16)
    return false;  // u8 / i8: exact integer sums, and the i8 tile kernels are a different design
  if (a.D % dtype_elems_per_chunk(a.dtype) != 0 || a.D > 4096)
    return false;
  if (bf_range_filter_mode(a) == kBfBits && a.filter_bit_offset % 32 != 0)
    return false;  // a tile's verdicts must be one word of the bitset
  if (path == 2)
    return true;
  // bf_mfma_supported's minima.  A count-only call is a dozen launches around one tile pass: measured
  // slower than the scan's single pass at 1024 x 4096 and 256 x 65536, faster from 1024 x 65536 on
  // (DESIGN.md 4.6), so it takes the tiles from there
  if (a.capacity == 0)
    return a.Nq >= 1024 && a.N_base >= 65536;
  return a.Nq >= 256 && a.N_base >= 4096;
}

// dynamic LDS of a tile workgroup: tiles, shift, query norms, thresholds, verdict words, and the
// fill pass's offsets
size_t bf_range_tile_lds_bytes(uint32_t D, int fm)
{
  const bool chunked = D > 128;
  const uint32_t CW = chunked ? 128u : D <= 64 ? 64u : 128u, DP = CW + 4;
  const uint32_t DM = chunked ? (D + 127) / 128 * 128 : CW;
  return (2 * kBfTileRows * DP + DM + 2 * kBfQueriesPerBlock + bf_filter_lds_words(fm, 1) +
          2 * kBfQueriesPerBlock) * sizeof(float);
}

template <typename BaseT, int MODE, int FM, bool FILL>
static const void* bf_range_tile_kernel_of(bool chunked, uint32_t Dh)
{
  if (chunked)
    return reinterpret_cast<const void*>(&bf_range_tile_kernel<BaseT, MODE, FM, FILL, true, 16>);
  if (Dh == 32)
    return reinterpret_cast<const void*>(&bf_range_tile_kernel<BaseT, MODE, FM, FILL, false, 8>);
  return reinterpret_cast<const void*>(&bf_range_tile_kernel<BaseT, MODE, FM, FILL, false, 16>);
}

template <typename BaseT, int MODE, int FM>
static void launch_bf_range_tiles(BfRangeTileArgs<FM>& t, bool fill, bool chunked, uint32_t Dh,
                                  uint32_t qblocks, size_t lds, hipStream_t stream)
{
  const void* kern = fill ? bf_range_tile_kernel_of<BaseT, MODE, FM, true>(chunked, Dh)
                          : bf_range_tile_kernel_of<BaseT, MODE, FM, false>(chunked, Dh);
  void* kargs[] = {&t};
  GGNN_HIP_CHECK(hipLaunchKernel(kern, dim3(qblocks, t.slices), dim3(256), kargs, lds, stream));
}

// Workgroups per CU of the tile kernels: three by registers (single chunk: 3 waves per SIMD) or two
// (chunked), and what their LDS allows of 160 KB
static uint32_t bf_range_groups_per_cu(bool chunked, size_t lds)
{
  return static_cast<uint32_t>(std::clamp<size_t>(160 * 1024 / lds, 1, chunked ? 2 : 3));
}

template <typename BaseT, int MODE>
static void launch_bf_range_mfma_t(const BfRangeLaunch& a, hipStream_t stream)
{
  const int fm = bf_range_filter_mode(a);
  const bool chunked = a.D > 128;
  const uint32_t Dh = chunked ? 64u : a.D <= 64 ? 32u : 64u;
  const uint32_t CW = 2 * Dh, DP = CW + 4;
  const uint32_t nch = chunked ? (a.D + 127) / 128 : 0u;
  const uint32_t DM = chunked ? nch * 128 : CW;
  const uint32_t qblocks = (a.Nq + kBfQueriesPerBlock - 1) / kBfQueriesPerBlock;
  const size_t lds = bf_range_tile_lds_bytes(a.D, fm);
  // parts per query: one round of resident workgroups; hook BF_RANGE_SLICES forces the count
  uint32_t parts = std::clamp(256u * bf_range_groups_per_cu(chunked, lds) / qblocks, 1u, 64u);
  if (const int64_t forced = hook(kHookBfRangeSlices); forced > 0)
    parts = static_cast<uint32_t>(std::min<int64_t>(forced, 64));
  uint32_t rows_per_part = (a.N_base + parts - 1) / parts;
  rows_per_part = (rows_per_part + kBfTileRows - 1) / kBfTileRows * kBfTileRows;
  parts = (a.N_base + rows_per_part - 1) / rows_per_part;
  const size_t pairs = static_cast<size_t>(a.Nq) * parts;

  // candidate budget: max(capacity, 32 Nq) plus one eighth, the (id, distance) buffer within 1 GiB
  uint64_t budget = std::max<uint64_t>(a.capacity, 32ull * a.Nq);
  budget = std::min<uint64_t>(budget + budget / 8, (1ull << 30) / 8);
  if (const int64_t forced = hook(kHookBfRangeCand); forced > 0)
    budget = static_cast<uint64_t>(forced);

  const bool center = std::is_same<BaseT, float>::value && MODE == kL2 && hook(kHookBfNoCenter) == 0;
  auto pad4 = [](size_t words) { return (words + 3) / 4 * 4; };
  const size_t n_norms = pad4(static_cast<size_t>(a.N_base) + a.Nq);
  const size_t n_mean = pad4(a.D);
  const size_t n_partial = center ? static_cast<size_t>(kBfMeanBlocks) * n_mean : 0;
  const size_t n_qshift = center ? pad4(static_cast<size_t>(a.Nq) * a.D) : 0;
  const size_t n_qpack = static_cast<size_t>(qblocks) * kBfQueriesPerBlock * nch * 128;
  const size_t n_thr = pad4(a.Nq);
  const size_t n_pairs = pad4(pairs), n_lims = pad4(2 * (static_cast<size_t>(a.Nq) + 1));
  const size_t n_cand = pad4(budget);
  // [norms][mean][partials][shifted queries][packed queries][thr][flag][cand / hit counts]
  // [cand / hit offsets (uint64)][cand_lims, scan lims (uint64)][cand ids][cand dists]
  const size_t words = n_norms + n_mean + n_partial + n_qshift + n_qpack + n_thr + 4 + 2 * n_pairs +
                       4 * n_pairs + 2 * n_lims + 2 * n_cand;
  ScratchGuard scratch{scratch_alloc(words * 4, stream), stream};
  float* bnorm = static_cast<float*>(scratch.p);
  float* qnorm = bnorm + a.N_base;
  float* mean = bnorm + n_norms;
  float* partial = mean + n_mean;
  float* q_shifted = partial + n_partial;
  float* q_packed = q_shifted + n_qshift;
  float* thr = q_packed + n_qpack;
  uint32_t* flag = reinterpret_cast<uint32_t*>(thr + n_thr);
  uint32_t* cand_counts = flag + 4;
  uint32_t* hit_counts = cand_counts + n_pairs;
  uint64_t* cand_offsets = reinterpret_cast<uint64_t*>(hit_counts + n_pairs);
  uint64_t* hit_offsets = cand_offsets + n_pairs;
  uint64_t* cand_lims = hit_offsets + n_pairs;
  uint64_t* scan_lims = cand_lims + n_lims / 2;
  int32_t* cand_ids = reinterpret_cast<int32_t*>(scan_lims + n_lims / 2);
  float* cand_dists = reinterpret_cast<float*>(cand_ids + n_cand);

  if (center)
    bf_center_rows(static_cast<const float*>(a.base), a.N_base, a.D,
                   static_cast<const float*>(a.query), a.Nq, mean, partial, q_shifted, stream);
  const float* d_mean = center ? mean : nullptr;
  const BaseT* tile_query =
      center ? reinterpret_cast<const BaseT*>(q_shifted) : static_cast<const BaseT*>(a.query);
  if (chunked) {
    const uint64_t n4 = n_qpack / 4;
    hipLaunchKernelGGL((pack_query_kernel<BaseT>),
                       dim3(static_cast<uint32_t>(std::min<uint64_t>((n4 + 255) / 256, 8192))),
                       dim3(256), 0, stream, tile_query, a.Nq, a.D, nch, n4,
                       reinterpret_cast<float4*>(q_packed));
  }
  hipLaunchKernelGGL((row_norms_kernel<BaseT>), dim3(norm_grid(a.N_base)), dim3(256), 0, stream,
                     static_cast<const BaseT*>(a.base), a.N_base, a.D, d_mean, bnorm,
                     static_cast<uint32_t*>(nullptr));
  hipLaunchKernelGGL((row_norms_kernel<BaseT>), dim3(norm_grid(a.Nq)), dim3(256), 0, stream,
                     tile_query, a.Nq, a.D, static_cast<const float*>(nullptr), qnorm,
                     static_cast<uint32_t*>(nullptr));
  constexpr float u = 5.9604645e-8f;
  const float Df = static_cast<float>(a.D);
  const float c = MODE == kL2 ? 1.02f * (2.f * Df + 8.f) * u : 0.f;
  hipLaunchKernelGGL((bf_range_thr_kernel<MODE>), dim3((a.Nq + 255) / 256), dim3(256), 0, stream,
                     a.radii, qnorm, a.Nq, Df, c, thr);
  GGNN_HIP_CHECK(hipGetLastError());

  auto tiles = [&](auto& t, bool fill) {
    constexpr int FM = std::is_same<std::decay_t<decltype(t)>, BfRangeTileArgs<kBfBits>>::value ? kBfBits
                       : std::is_same<std::decay_t<decltype(t)>, BfRangeTileArgs<kBfLabels>>::value
                           ? kBfLabels
                           : kBfNoFilter;
    t.base = a.base;
    t.query = tile_query;
    t.query_packed = q_packed;
    t.mean = d_mean;
    t.bnorm = bnorm;
    t.qnorm = qnorm;
    t.D = a.D;
    t.Dh = Dh;
    t.DP = DP;
    t.Nq = a.Nq;
    t.N_base = a.N_base;
    t.slices = parts;
    t.rows_per_slice = rows_per_part;
    t.DM = DM;
    t.thr = thr;
    t.c = c;
    t.counts = cand_counts;
    t.offsets = cand_offsets;
    t.cand_lims = cand_lims;
    t.budget = budget;
    t.cand_ids = cand_ids;
    if constexpr (FM != kBfNoFilter) {
      t.filter_bits = a.filter_bits;
      t.filter_bit_offset = a.filter_bit_offset;
      t.filter_table = a.filter_table;
    }
    launch_bf_range_tiles<BaseT, MODE, FM>(t, fill, chunked, Dh, qblocks, lds, stream);
  };
  auto tile_pass = [&](bool fill) {
    if (fm == kBfBits) {
      BfRangeTileArgs<kBfBits> t{};
      tiles(t, fill);
    }
    else if (fm == kBfLabels) {
      BfRangeTileArgs<kBfLabels> t{};
      tiles(t, fill);
    }
    else {
      BfRangeTileArgs<kBfNoFilter> t{};
      tiles(t, fill);
    }
  };

  tile_pass(false);
  launch_bf_range_prefix(cand_counts, a.Nq, parts, cand_offsets, cand_lims, stream);
  hipLaunchKernelGGL(bf_range_budget_kernel, dim3(1), dim3(1), 0, stream, cand_lims, a.Nq, budget,
                     flag, a.fell_back);
  tile_pass(true);

  BfRangeExactArgs ex{};
  ex.base = a.base;
  ex.query = a.query;
  ex.radii = a.radii;
  ex.cand_counts = cand_counts;
  ex.cand_offsets = cand_offsets;
  ex.cand_lims = cand_lims;
  ex.cand_ids = cand_ids;
  ex.cand_dists = cand_dists;
  ex.hit_counts = hit_counts;
  ex.budget = budget;
  ex.D = a.D;
  ex.Nq = a.Nq;
  ex.N_base = a.N_base;
  ex.parts = parts;
#define GGNN_BF_RANGE_EXACT(T, LPR, NCH)                                                            \
  do {                                                                                              \
    if constexpr (std::is_same<T, BaseT>::value)                                                    \
      hipLaunchKernelGGL((bf_range_exact_kernel<T, LPR, NCH, MODE>), grid_for(pairs), dim3(kWave), 0, \
                         stream, ex);                                                               \
  } while (0)
  GGNN_DISPATCH_DIST(a.dtype, a.D, GGNN_BF_RANGE_EXACT);
#undef GGNN_BF_RANGE_EXACT
  GGNN_HIP_CHECK(hipGetLastError());
  launch_bf_range_prefix(hit_counts, a.Nq, parts, hit_offsets, a.lims, stream);
  if (a.capacity != 0) {
    BfRangeCompactArgs cp{};
    cp.radii = a.radii;
    cp.cand_counts = cand_counts;
    cp.cand_offsets = cand_offsets;
    cp.cand_lims = cand_lims;
    cp.cand_ids = cand_ids;
    cp.cand_dists = cand_dists;
    cp.hit_offsets = hit_offsets;
    cp.lims = a.lims;
    cp.ids = a.ids;
    cp.dists = a.dists;
    cp.budget = budget;
    cp.capacity = a.capacity;
    cp.Nq = a.Nq;
    cp.parts = parts;
    launch_bf_range_compact(cp, stream);
  }

  // the scan passes, gated by the flag: they answer the call iff the candidates did not fit
  BfRangeLaunch fb = a;
  fb.lims = scan_lims;
  launch_bf_range_scan(fb, flag, stream);
  launch_bf_range_take_lims(flag, scan_lims, a.Nq + 1, a.lims, stream);
}

void launch_bf_range_query_mfma(const BfRangeLaunch& a, hipStream_t stream)
{
  const bool l2 = a.measure == GGNN_EUCLIDEAN;
  switch (a.dtype) {
    case GGNN_F32:
      return l2 ? launch_bf_range_mfma_t<float, kL2>(a, stream)
                : launch_bf_range_mfma_t<float, kCos>(a, stream);
    case GGNN_F16:
      return l2 ? launch_bf_range_mfma_t<f16_t, kL2>(a, stream)
                : launch_bf_range_mfma_t<f16_t, kCos>(a, stream);
    case GGNN_BF16:
      return l2 ? launch_bf_range_mfma_t<bf16_t, kL2>(a, stream)
                : launch_bf_range_mfma_t<bf16_t, kCos>(a, stream);
    default:
      throw Error(GGNN_UNSUPPORTED, "range search: no tile kernels for this dtype");
  }
}

}  // namespace ggnn_amd
