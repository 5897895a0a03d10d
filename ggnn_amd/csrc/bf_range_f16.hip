// bf_range for float16 / bfloat16 rows under squared L2: the tile pre-selection runs on the 16-bit
// matrix cores (v_mfma_f32_32x32x16_f16 / _bf16, 16 columns per instruction, f32 accumulate) on tiles
// staged RAW in 16 bits; every hit is decided exactly.  bf_range_mfma.hip widens such rows to float32 in
// LDS and contracts them two columns per instruction; it keeps cosine and BF_RANGE_F16 = 1.
//
// The passes are those of bf_range_mfma.hip, the operand layout and the instruction model those of
// bf_f16.hip.  One stream, all device memory, nothing waits for the host, no atomic decides a position:
//   norms    row_norms_kernel<T16> (bf_mfma.hip): float32 |x|^2 of every base row and query
//   flag     bf_f16_flag_kernel (bf_f16.hip): an element that is subnormal in its 16-bit type or
//            non-finite, or a non-finite norm.  Under the flag the tile passes leave at once and the
//            gated scan passes answer the whole call (fell_back = 1)
//   pack     bf_f16_pack_kernel<2> (D > 128): the query set in operand order, in 16 bits
//   thr      bf_range_f16_thr_kernel: one threshold per query (NaN: the query has no candidates)
//   count    bf_range_f16_kernel<FILL = false>: candidates per (query, part), a part being a
//            contiguous, tile-aligned row range; parts ascend with the rows
//   prefix   bf_range_prefix_kernel (bf_range.hip): candidate offsets and cand_lims[Nq]
//   budget   bf_range_f16_budget_kernel: the eligibility flag, or candidates that do not fit their
//            buffer, raise the gate of the scan passes.  Under the eligibility flag the counts are the
//            zeros the launcher cleared them to (every offset is defined: empty parts); the kernel then
//            sets cand_lims[Nq] = 2^64 - 1, the one word every later pass tests against the budget
//            before it touches a candidate
//   fill     bf_range_f16_kernel<FILL = true>: the same predicate on the same bits; the lane that owns
//            a verdict writes the row id, and d_e beside it, at offset + candidates before it
//   exact    bf_range_f16_exact_kernel: one wave per (query, part), the direct form (DistEngine,
//            compute_distances: the scan's bits) of its candidates, d <= r counted; and the MODEL
//            GUARD below on every candidate, which has both values here
//   guard    bf_range_f16_guard_kernel: a violation raises the gate (fell_back = 1) and closes the
//            compaction the same way the budget kernel closes the passes before it
//   prefix, compact, gated scan, take lims: bf_range_mfma.hip's and bf_range.hip's
//
// The tile kernel.  256 threads, 256 queries per workgroup: wave w owns two sets of 32 queries that
// share every B operand read from LDS (there are no lists, so two sets fit at every D).  Queries are
// the M side: accumulator register r of half h holds query row (r & 3) + 8 (r >> 2) + 4 h of its set,
// lanes are base rows.  Lane (j, h) contributes columns 16 m + 8 h .. + 7 of query row j (A) and of base
// row j (B) to instruction m: one ds_read_b128 per B operand.  LDS rows are 32 NM bytes of raw halves
// plus 16 spare bytes -- the row's float32 norm and, under label filters, its label -- an odd number of
// 16-byte slots: conflict-free b128 reads.  Columns past D are zero in the tile and the query operand.
//   * D <= 128: one chunk of 16 NM columns, NM in {2, 4, 8}; the query operand lives in registers; a
//     stage is 16 / NM tiles (32 instructions of a wave per barrier at every NM).
//   * D > 128 (CH): chunks of 128 columns into the same accumulators, a stage is two tiles x one chunk,
//     the query operand of the next chunk comes from the packed copy behind this chunk's instructions.
//   Stages are double buffered; every global load is unconditional with a clamped address; rows past
//   the end of a part get the norm +inf and are masked out of the ballots.
//   Epilogue per (tile, set): d_e = fmaf(-2, dot, |q|^2 + |b|^2), the filter verdict from the staged words
//   (thread t stages the bitset word of query t per tile of the stage; labels ride in the tile rows),
//   the negated compare against the per-query threshold in LDS (a NaN d_e is a candidate), one ballot
//   per accumulator register = the 32 row verdicts of two queries.  Lane q of a wave keeps the count of
//   the wave's query q.  Fill: the lane owning a set bit writes at offset + count so far + set bits
//   below it, so ids ascend without a sort.  Count and fill are one body with one `if constexpr`.
//   No pre-test on accumulators seeded through the C operand: bf_f16.hip's header says why.
//
// Why the pre-selection loses no hit.  No centring: a = q, b = x.  u = 2^-24.  bf_f16.hip's model of the
// instruction (constant c_m = kBfF16Cm, measured) gives, with G(D) = 2.0625 D + 24 and the float32 norms,
//     |d_e - ||q-x||^2| <= B(q, x) = 1.02 c_m G(D) u (|q|^2 + |x|^2) + (2D + 8) 2^-125
//     d_dir >= ||q-x||^2 (1 - (D+3) u)
//   so d_dir <= r implies  d_e <= r / (1 - 1.01 (D+3) u) + 1.02 c_m G(D) u (|q|^2 + |x|^2) + (2D+8) 2^-125.
//   The kernel uses the norm of the row itself, which the tile carries anyway: with c >= 1.02 c_m G(D) u
//     candidate  iff  !( fl(d_e - c |x|^2) > t ),   t >= r / (1 - 1.01 (D+3) u) + c |q|^2 + (2D+8) 2^-125
//   (rounding is monotonic; c is formed with 1.03, t with 1.02 (D+3) u and 16 ulps on top, which covers
//   their own roundings -- the discipline of bf_range_mfma.hip one step up, because 1.02 is the model's).
// The model guard.  c_m is measured, not derived, so the exact pass checks on every candidate
//     |d_e - d_dir| <= B(q, x) + 1.01 (D+3) u d_dir
//   -- bf_f16_rerank_kernel's test.  Candidates thereby check the model on every call; left-out rows
//   rest on it.  One violation sends the whole call to the scan.
#include <algorithm>

#define GGNN_BF_F16_SHARED_ONLY
#include "bf_f16.hip"  // Half16, kBfF16Cm, the flag and pack kernels; bf_mfma.hip's shared device code
#include "bf_thread_filter.hpp"

namespace ggnn_amd {

constexpr int kRangeF16Queries = 256;  // per workgroup: 4 waves x 2 sets x 32

struct BfRangeF16Args {
  const void* base;
  const void* query;
  const uint4* query_packed;  // CH only
  const float* bnorm;
  const float* qnorm;
  const float* thr;           // [Nq] thresholds (NaN: no candidates)
  const uint32_t* flag;       // eligibility: != 0, the scan answers the call
  float c;                    // coefficient of |x|^2 in the compare
  uint32_t D, Nq, N_base, nch, parts, rows_per_part;
  uint32_t* counts;           // [Nq x parts], written by the count pass
  const uint64_t* offsets;    // [Nq x parts] exclusive, read by the fill pass
  const uint64_t* cand_lims;  // [Nq + 1]
  uint64_t budget;            // entries of cand_ids / cand_de
  int32_t* cand_ids;
  float* cand_de;             // d_e of every candidate, beside its id (the guard's input)
};
struct BfRangeF16FilteredArgs : BfRangeF16Args {
  const uint32_t* filter_bits;  // bitset / filter table / label column (BfRangeLaunch)
  uint32_t filter_bit_offset;   // kBfBits: a multiple of 32
  FilterTable filter_table;
};
template <int FM>
using BfRangeF16ArgsOf = std::conditional_t<FM != kBfNoFilter, BfRangeF16FilteredArgs, BfRangeF16Args>;

constexpr int bf_range_f16_nm(uint32_t D)
{
  return D > 64 ? 8 : D > 32 ? 4 : 2;
}
// LDS words of the filter area: kBfBits [2 buffers][tiles per stage][256] verdict words, kBfLabels [256]
// query labels (the row labels sit beside the norms in the tile rows)
constexpr uint32_t bf_range_f16_filter_words(int fm, uint32_t tiles_per_stage)
{
  return fm == kBfBits ? 2u * tiles_per_stage * kRangeF16Queries : fm == kBfLabels ? kRangeF16Queries : 0u;
}

// one threshold per query (see the top of this file).  tests/test_bf_range_f16.py restates the constants
// 1.02, 1.03 (c, on the host) and the 16 ulps: change them together
__global__ void __launch_bounds__(256) bf_range_f16_thr_kernel(const float* radii, const float* qnorm,
                                                              uint32_t Nq, float Df, float c, float* thr)
{
  const uint32_t n = blockIdx.x * 256 + threadIdx.x;
  if (n >= Nq)
    return;
  constexpr float u = 5.9604645e-8f;  // 2^-24
  const float r = radii[n];
  float t = r / (1.f - 1.02f * (Df + 3.f) * u);
  t = fmaf(c, qnorm[n], t);
  t += (2.f * Df + 8.f) * 2.3509887e-38f;
  t += 16.f * u * t;  // (t >= 0 here or unused; +inf stays +inf)
  thr[n] = (r >= 0.f) ? t : __uint_as_float(0x7fc00000u);
}

template <typename T16, int FM, bool FILL, int NM, bool CH>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
    bf_range_f16_kernel(const BfRangeF16ArgsOf<FM> a)
{
  static_assert(!CH || NM == 8, "chunks are 128 columns");
  constexpr int TPS = bf_f16_stage_tiles(NM, CH);
  constexpr uint32_t SR = TPS * kBfTileRows;          // rows of a stage
  constexpr uint32_t CB = NM * 32, RS = CB + 16;      // bytes of a chunk row, LDS row stride
  constexpr uint32_t stage_bytes = SR * RS;
  constexpr uint32_t PPR = 2 * NM;                    // 16-byte pieces per chunk row
  constexpr int PPT = static_cast<int>(SR * PPR / 256);  // pieces per thread and stage
  static_assert(PPT == 4 && SR <= 256, "stage geometry");
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_b[];
  float* qn_l = reinterpret_cast<float*>(lds_b + 2 * stage_bytes);  // [256] |q|^2
  float* thr_l = qn_l + kRangeF16Queries;                           // [256]
  // (fill pass: the 256 candidate offsets of this (query block, part))
  uint64_t* off_l = reinterpret_cast<uint64_t*>(thr_l + kRangeF16Queries);
  [[maybe_unused]] uint32_t* filt_l = reinterpret_cast<uint32_t*>(off_l + kRangeF16Queries);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  if (*a.flag != 0u)  // subnormal or non-finite input: the scan answers the call (uniform)
    return;
  if constexpr (FILL) {
    if (a.cand_lims[a.Nq] > a.budget)  // the candidates do not fit: the scan answers (uniform)
      return;
  }
  const uint16_t* base = static_cast<const uint16_t*>(a.base);
  const uint16_t* query = static_cast<const uint16_t*>(a.query);
  const uint32_t qblock = blockIdx.x, part = blockIdx.y;
  const uint32_t begin = min(a.N_base, part * a.rows_per_part);
  const uint32_t end = min(a.N_base, begin + a.rows_per_part);
  const uint32_t qw = (qblock * 4 + wave) * 64;  // first query of this wave
  const uint32_t nch = CH ? a.nch : 1u;
  const uint32_t nstages = (end - begin + SR - 1) / SR;
  const uint32_t nsteps = nstages * nch;

  // ---- lane = query state: entry tid of the per-query arrays is query qw + lane ----
  const uint32_t my_q = qw + lane;
  const bool my_valid = my_q < a.Nq;
  {
    // (NaN: the query does not exist or has no threshold -- the epilogue masks it by t == t)
    const float t = my_valid ? a.thr[my_q] : __uint_as_float(0x7fc00000u);
    qn_l[tid] = my_valid ? a.qnorm[my_q] : 0.f;
    thr_l[tid] = t;
    if constexpr (FILL)
      off_l[tid] = my_valid ? a.offsets[static_cast<size_t>(my_q) * a.parts + part] : 0ull;
    if constexpr (FM == kBfLabels)
      filt_l[tid] = static_cast<uint32_t>(my_valid ? a.filter_table.query_labels[my_q] : -1);
  }
  // kBfBits: the bitset row of this thread's query (padding queries are masked anyway)
  [[maybe_unused]] const uint32_t* frow = nullptr;
  if constexpr (FM == kBfBits)
    frow = bf_thread_filter_row(a.filter_bits, a.filter_table, my_q, a.Nq);

  // ---- staging: PPT pieces of 16 bytes per thread, threads 0 .. SR - 1 carry the row constants ----
  u32x4 sv[PPT];
  float sbn = 0.f;
  [[maybe_unused]] uint32_t slab = 0u;
  [[maybe_unused]] uint32_t sfw[TPS];
  auto stage_load = [&](uint32_t row0, uint32_t col0) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < PPT; ++e) {
      const uint32_t p = tid + 256 * e, srow = p / PPR, col = col0 + 8 * (p % PPR);
      const uint32_t r = min(row0 + srow, end - 1), c = min(col, a.D - 8u);
      sv[e] = *reinterpret_cast<const u32x4*>(base + static_cast<size_t>(r) * a.D + c);
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
  // (the row constants and filter words are written with every chunk: the epilogue reads them from the
  // buffer of the stage's last chunk)
  auto stage_store = [&](uint32_t buf, uint32_t row0, uint32_t col0) __attribute__((always_inline)) {
    uint8_t* t = lds_b + buf * stage_bytes;
#pragma unroll
    for (int e = 0; e < PPT; ++e) {
      const uint32_t p = tid + 256 * e, srow = p / PPR, sc = p % PPR;
      *reinterpret_cast<u32x4*>(t + srow * RS + 16 * sc) =
          col0 + 8 * sc < a.D ? sv[e] : u32x4{0u, 0u, 0u, 0u};
    }
    if (tid < static_cast<int>(SR)) {
      float* rc = reinterpret_cast<float*>(t + tid * RS + CB);
      rc[0] = (row0 + tid < end) ? sbn : inf_f();
      if constexpr (FM == kBfLabels)
        rc[1] = __uint_as_float(slab);
    }
    if constexpr (FM == kBfBits) {
#pragma unroll
      for (int tl = 0; tl < TPS; ++tl)
        filt_l[(buf * TPS + tl) * kRangeF16Queries + tid] = sfw[tl];
    }
  };

  // ---- the query operand: aq[s][m] = columns col0 + 16 m + 8 h .. + 7 of query row j of set s ----
  u32x4 aq[2][NM];
  auto query_load = [&](uint32_t c) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int m = 0; m < NM; ++m) {
        if constexpr (CH) {
          const size_t o = ((((static_cast<size_t>(qblock) * 4 + wave) * a.nch + c) * 2 + s) * 8 + m) * 64;
          const uint4 v = a.query_packed[o + lane];
          aq[s][m] = u32x4{v.x, v.y, v.z, v.w};
        }
        else {
          const uint32_t qi = qw + s * 32 + j, col = 16 * m + 8 * h;
          u32x4 v = u32x4{0u, 0u, 0u, 0u};
          if (qi < a.Nq && col < a.D)
            v = *reinterpret_cast<const u32x4*>(query + static_cast<size_t>(qi) * a.D + col);
          aq[s][m] = v;
        }
      }
  };

  uint32_t cnt = 0;  // candidates of query qw + lane so far
  // verdicts of one (tile, set); wave-uniform control flow throughout
  auto epilogue = [&](const f32x16& acc, const int s, const uint8_t* trow, const uint32_t buf, const int t,
                      const uint32_t row0) __attribute__((always_inline)) {
    // (the per-query words are re-read from LDS for every tile: hoisted out of the tile loop they would
    // hold 64 registers beside the query operand, and the fill kernels of NM = 8 would not fit 256)
    asm volatile("" ::: "memory");
    const float bn = *reinterpret_cast<const float*>(trow + CB);
    [[maybe_unused]] int32_t row_label = 0;
    if constexpr (FM == kBfLabels)
      row_label = *reinterpret_cast<const int32_t*>(trow + CB + 4);
    const uint32_t rows = min(static_cast<uint32_t>(kBfTileRows), end - row0);
    const uint32_t rm = rows >= 32u ? ~0u : (1u << rows) - 1u;
    // rows that exist, in both halves of the wave: one scalar pair per tile
    const unsigned long long rowmask = static_cast<unsigned long long>(rm) * 0x100000001ull;
    const int ql0 = wave * 64 + s * 32;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 qn4 = *reinterpret_cast<const float4*>(qn_l + ql0 + 8 * g + 4 * h);
      const float4 th4 = *reinterpret_cast<const float4*>(thr_l + ql0 + 8 * g + 4 * h);
      const float qn[4] = {qn4.x, qn4.y, qn4.z, qn4.w};
      const float th[4] = {th4.x, th4.y, th4.z, th4.w};
      [[maybe_unused]] i32x4 f4 = i32x4{0, 0, 0, 0};  // verdict words / labels of four queries
      if constexpr (FM == kBfBits)
        f4 = *reinterpret_cast<const i32x4*>(filt_l + (buf * TPS + t) * kRangeF16Queries + ql0 + 8 * g +
                                             4 * h);
      if constexpr (FM == kBfLabels)
        f4 = *reinterpret_cast<const i32x4*>(filt_l + ql0 + 8 * g + 4 * h);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int qa = s * 32 + e + 8 * g, qb = qa + 4;  // queries of the wave in lanes 0..31 / 32..63
        const float d = bf_expand<kL2>(acc[4 * g + e], qn[e], bn, true);
        const float x = fmaf(-a.c, bn, d);
        // (a query without a threshold carries NaN: masked here, in vector form -- per-register scalar
        // masks cost some 200 SGPRs spilled into VGPR lanes)
        bool cand = !(x > th[e]) && th[e] == th[e];
        if constexpr (FM == kBfBits)
          cand = cand && ((static_cast<uint32_t>(f4[e]) >> j) & 1u);
        if constexpr (FM == kBfLabels)
          cand = cand && !bf_label_denied(f4[e], row_label);
        const unsigned long long m = __ballot(cand) & rowmask;
        const uint32_t m_lo = static_cast<uint32_t>(m), m_hi = static_cast<uint32_t>(m >> 32);
        if constexpr (FILL) {
          if (m) {  // (wave-uniform)
            const uint32_t run_a = __builtin_amdgcn_readlane(static_cast<int>(cnt), qa);
            const uint32_t run_b = __builtin_amdgcn_readlane(static_cast<int>(cnt), qb);
            const uint32_t half = h ? m_hi : m_lo;
            if ((half >> j) & 1u) {
              const uint64_t pos = off_l[wave * 64 + (h ? qb : qa)] + (h ? run_b : run_a) +
                                   __popc(half & ((1u << j) - 1u));
              // (pos < cand_lims[Nq] <= budget whenever the inputs are those of the count pass)
              if (pos < a.budget) {
                a.cand_ids[pos] = static_cast<int32_t>(row0 + j);
                a.cand_de[pos] = d;
              }
            }
          }
        }
        cnt += lane == qa ? __popc(m_lo) : lane == qb ? __popc(m_hi) : 0u;
      }
    }
  };

  if (nsteps) {
    stage_load(begin, 0);
    stage_store(0, begin, 0);
  }
  query_load(0);
  __syncthreads();

  constexpr int NT = CH ? TPS : 1;  // accumulator tiles alive across steps
  f32x16 acc[NT][2];
  uint32_t st = 0, c = 0;
  for (uint32_t p = 0; p < nsteps; ++p) {
    // the step after this one: the next chunk of the stage, else the first chunk of the next stage
    const bool last_c = c + 1 == nch;
    const uint32_t n_st = last_c ? st + 1 : st, n_c = last_c ? 0u : c + 1;
    const bool has_next = p + 1 < nsteps;
    const uint32_t row0 = begin + st * SR;
    if (has_next)
      stage_load(begin + n_st * SR, n_c * 128);
    const uint32_t buf = p & 1;
    const uint8_t* blk = lds_b + buf * stage_bytes;
#pragma unroll
    for (int t = 0; t < TPS; ++t) {
      if (row0 + t * kBfTileRows >= end)
        break;  // uniform
      const uint8_t* trow = blk + (t * kBfTileRows + j) * RS;
      u32x4 b[NM];
#pragma unroll
      for (int m = 0; m < NM; ++m)
        b[m] = *reinterpret_cast<const u32x4*>(trow + 32 * m + 16 * h);
      const int ti = CH ? t : 0;  // (a constant after unrolling)
      if (!CH || c == 0) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
          acc[ti][s] = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int s = 0; s < 2; ++s)
          acc[ti][s] = Half16<T16>::mfma(aq[s][m], b[m], acc[ti][s]);
      if (!CH || last_c) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
          epilogue(acc[ti][s], s, trow, buf, t, row0 + t * kBfTileRows);
      }
    }
    if constexpr (CH) {
      if (has_next)
        query_load(n_c);
    }
    if (has_next)
      stage_store((p + 1) & 1, begin + n_st * SR, n_c * 128);
    __syncthreads();
    st = n_st;
    c = n_c;
  }
  if constexpr (!FILL) {
    if (my_valid)
      a.counts[static_cast<size_t>(my_q) * a.parts + part] = cnt;
  }
}

// ---- budget, exact evaluation with the model guard ------------------------------------------------
// gate = the scan passes answer: the inputs are not eligible, or the candidates do not fit
__global__ void bf_range_f16_budget_kernel(uint64_t* cand_lims, uint32_t Nq, uint64_t budget,
                                           const uint32_t* eligibility, uint32_t* gate, uint32_t* fell_back)
{
  const bool flagged = *eligibility != 0u;
  if (flagged)  // (the counts were never written: close every pass that tests this word)
    cand_lims[Nq] = ~0ull;
  const uint32_t over = (flagged || cand_lims[Nq] > budget) ? 1u : 0u;
  *gate = over;
  if (fell_back)
    *fell_back = over;
}

// a candidate outside the model's bound: the scan answers, the compaction finds its gate closed
__global__ void bf_range_f16_guard_kernel(const uint32_t* violated, uint64_t* cand_lims, uint32_t Nq,
                                          uint32_t* gate, uint32_t* fell_back)
{
  if (*violated == 0u)
    return;
  cand_lims[Nq] = ~0ull;
  *gate = 1u;
  if (fell_back)
    *fell_back = 1u;
}

struct BfRangeF16ExactArgs {
  const void* base;
  const void* query;
  const float* radii;
  const float* bnorm;
  const float* qnorm;
  const uint32_t* cand_counts;   // [Nq x parts]
  const uint64_t* cand_offsets;  // [Nq x parts]
  const uint64_t* cand_lims;     // [Nq + 1]
  const int32_t* cand_ids;
  float* cand_dists;             // in: d_e of every candidate; out: its direct-form distance
  uint32_t* hit_counts;          // [Nq x parts]
  uint32_t* violated;            // the model guard's flag
  uint64_t budget;
  uint32_t D, Nq, N_base, parts;
};

// bf_range_exact_kernel (bf_range_mfma.hip) with the model guard: one wave per (query, part), the
// direct form of the part's candidates in blocks of kKBlock -- the scan's bits
template <typename T16, int LPR, int NCH>
__global__ void __launch_bounds__(kWave) bf_range_f16_exact_kernel(const BfRangeF16ExactArgs a)
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
  const T16* base = static_cast<const T16*>(a.base);
  DistEngine<T16, LPR, NCH> de;
  de.template load_query<kL2>(base, a.D, static_cast<const T16*>(a.query) + static_cast<size_t>(n) * a.D);
  constexpr float u = 5.9604645e-8f;  // 2^-24
  const float Df = static_cast<float>(a.D);
  const float qn = a.qnorm[n];
  const float cB = 1.02f * kBfF16Cm * (2.0625f * Df + 24.f) * u;
  const float absB = (2.f * Df + 8.f) * 2.3509887e-38f;
  bool model_ok = true;
  uint32_t hits = 0;
  for (uint32_t c0 = 0; c0 < total; c0 += kKBlock) {
    const int nsurv = static_cast<int>(min(kKBlock, total - c0));
    __syncthreads();
    if (lane < nsurv)  // (ids are rows of the base; the clamp keeps a wrong one inside it)
      lds.ckeys[lane] = static_cast<int>(
          min(static_cast<uint32_t>(a.cand_ids[off + c0 + lane]), a.N_base - 1));
    __syncthreads();
    compute_distances<kL2>(de, lds, nsurv, nullptr);
    __syncthreads();
    bool hit = false;
    if (lane < nsurv) {
      const float d = lds.cd0[lane];
      const float d_e = a.cand_dists[off + c0 + lane];
      const float norms = qn + a.bnorm[lds.ckeys[lane]];
      // (a NaN on either side fails the compare: the scan answers)
      model_ok = model_ok && fabsf(d_e - d) <= cB * norms + absB + 1.01f * (Df + 3.f) * u * d;
      a.cand_dists[off + c0 + lane] = d;
      hit = d <= r;  // NaN on either side is no hit, as in the scan
    }
    hits += __popcll(__ballot(hit));
  }
  if (lane == 0)
    a.hit_counts[bid] = hits;
  if (!__all(model_ok) && lane == 0)
    atomicOr(a.violated, 1u);
}

// ---- host -----------------------------------------------------------------------------------------
static int bf_range_f16_filter_mode(const BfRangeLaunch& a)
{
  return !a.filter_bits ? kBfNoFilter : a.filter_table.query_labels ? kBfLabels : kBfBits;
}

// dynamic LDS of a tile workgroup: two stages, norms / thresholds / offsets of 256 queries, filter area
size_t bf_range_f16_lds_bytes(uint32_t D, int fm)
{
  const bool ch = D > 128;
  const int nm = bf_range_f16_nm(D);
  const uint32_t tps = bf_f16_stage_tiles(nm, ch);
  return 2ull * tps * kBfTileRows * (nm * 32 + 16) +
         kRangeF16Queries * (2 * sizeof(float) + sizeof(uint64_t)) +
         bf_range_f16_filter_words(fm, tps) * sizeof(uint32_t);
}

bool bf_range_f16_supported(const BfRangeLaunch& a)
{
  const int64_t mode = hook(kHookBfRangeF16);
  if (hook(kHookBfRangePath) == 1 || mode == 1)
    return false;
  if (a.dtype != GGNN_F16 && a.dtype != GGNN_BF16)
    return false;
  if (a.measure != GGNN_EUCLIDEAN)
    return false;  // cosine keeps the float32-staged tiles
  if (a.D == 0 || a.D % 8 != 0 || a.D > 4096)
    return false;
  const int fm = bf_range_f16_filter_mode(a);
  if (fm == kBfBits && a.filter_bit_offset % 32 != 0)
    return false;  // a tile's verdicts must be one word of the bitset
  if (2 * bf_range_f16_lds_bytes(a.D, fm) > 160 * 1024)
    return false;  // (two workgroups per CU; holds at every D and filter today)
  if (mode == 2)
    return true;
  // auto: bf_f16.hip's policy -- bfloat16 from 10k x 1M on, where the full call measured 3.4x (D = 128)
  // and 6x (D = 960) ahead of the float32-staged tiles; of the four shapes {256, 1024} x {4096, 65536}
  // only 1024 x 65536 won.  float16 is hook only: N(0,1) rows rounded to float16 hold
  // subnormals and a flagged call pays for both paths
  return a.dtype == GGNN_BF16 && a.Nq >= 10000 && a.N_base >= 1000000;
}

template <typename T16, int FM, bool FILL>
static const void* bf_range_f16_kernel_of(uint32_t D)
{
  if (D > 128)
    return reinterpret_cast<const void*>(&bf_range_f16_kernel<T16, FM, FILL, 8, true>);
  if (D > 64)
    return reinterpret_cast<const void*>(&bf_range_f16_kernel<T16, FM, FILL, 8, false>);
  if (D > 32)
    return reinterpret_cast<const void*>(&bf_range_f16_kernel<T16, FM, FILL, 4, false>);
  return reinterpret_cast<const void*>(&bf_range_f16_kernel<T16, FM, FILL, 2, false>);
}

template <typename T16, int FM>
static void launch_bf_range_f16_tiles(const BfRangeLaunch& a, BfRangeF16ArgsOf<FM> t, bool fill,
                                      uint32_t qblocks, hipStream_t stream)
{
  if constexpr (FM != kBfNoFilter) {
    t.filter_bits = a.filter_bits;
    t.filter_bit_offset = a.filter_bit_offset;
    t.filter_table = a.filter_table;
  }
  const void* kern = fill ? bf_range_f16_kernel_of<T16, FM, true>(a.D)
                          : bf_range_f16_kernel_of<T16, FM, false>(a.D);
  void* kargs[] = {&t};
  GGNN_HIP_CHECK(hipLaunchKernel(kern, dim3(qblocks, t.parts), dim3(256), kargs,
                                 bf_range_f16_lds_bytes(a.D, FM), stream));
}

template <typename T16>
static void launch_bf_range_f16_t(const BfRangeLaunch& a, hipStream_t stream)
{
  const int fm = bf_range_f16_filter_mode(a);
  const bool ch = a.D > 128;
  const uint32_t nch = ch ? (a.D + 127) / 128 : 1;
  const uint32_t qblocks = (a.Nq + kRangeF16Queries - 1) / kRangeF16Queries;
  // parts per query: one round of resident workgroups (two per CU); hook BF_RANGE_SLICES forces the count
  uint32_t parts = std::clamp(256u * 2u / qblocks, 1u, 64u);
  if (const int64_t forced = hook(kHookBfRangeSlices); forced > 0)
    parts = static_cast<uint32_t>(std::min<int64_t>(forced, 64));
  uint32_t rows_per_part = (a.N_base + parts - 1) / parts;
  rows_per_part = (rows_per_part + kBfTileRows - 1) / kBfTileRows * kBfTileRows;
  parts = (a.N_base + rows_per_part - 1) / rows_per_part;
  const size_t pairs = static_cast<size_t>(a.Nq) * parts;

  // candidate budget: bf_range_mfma.hip's rule
  uint64_t budget = std::max<uint64_t>(a.capacity, 32ull * a.Nq);
  budget = std::min<uint64_t>(budget + budget / 8, (1ull << 30) / 8);
  if (const int64_t forced = hook(kHookBfRangeCand); forced > 0)
    budget = static_cast<uint64_t>(forced);

  auto pad4 = [](size_t words) { return (words + 3) / 4 * 4; };
  const size_t n_norms = pad4(static_cast<size_t>(a.N_base) + a.Nq), n_thr = pad4(a.Nq);
  const uint64_t n16 = ch ? static_cast<uint64_t>(qblocks) * 4 * nch * 2 * 8 * 64 : 0;
  const size_t n_pairs = pad4(pairs), n_lims = pad4(2 * (static_cast<size_t>(a.Nq) + 1));
  const size_t n_cand = pad4(budget);
  // [norms][packed queries][thr][gate, eligibility, violated, -][cand / hit counts]
  // [cand / hit offsets (uint64)][cand_lims, scan lims (uint64)][cand ids][cand d_e -> dists]
  const size_t words = n_norms + 4 * n16 + n_thr + 4 + 2 * n_pairs + 4 * n_pairs + 2 * n_lims + 2 * n_cand;
  ScratchGuard scratch{scratch_alloc(words * 4, stream), stream};
  float* bnorm = static_cast<float*>(scratch.p);
  float* qnorm = bnorm + a.N_base;
  uint4* q_packed = reinterpret_cast<uint4*>(bnorm + n_norms);
  float* thr = reinterpret_cast<float*>(q_packed + n16);
  uint32_t* flags = reinterpret_cast<uint32_t*>(thr + n_thr);  // [0] gate [1] eligibility [2] violated
  uint32_t* cand_counts = flags + 4;
  uint32_t* hit_counts = cand_counts + n_pairs;
  uint64_t* cand_offsets = reinterpret_cast<uint64_t*>(hit_counts + n_pairs);
  uint64_t* hit_offsets = cand_offsets + n_pairs;
  uint64_t* cand_lims = hit_offsets + n_pairs;
  uint64_t* scan_lims = cand_lims + n_lims / 2;
  int32_t* cand_ids = reinterpret_cast<int32_t*>(scan_lims + n_lims / 2);
  float* cand_dists = reinterpret_cast<float*>(cand_ids + n_cand);
  // the flags, and the candidate counts behind them: under the eligibility flag the count pass writes
  // none, and the prefix pass must still see defined (empty) parts
  GGNN_HIP_CHECK(hipMemsetAsync(flags, 0, (4 + n_pairs) * sizeof(uint32_t), stream));

  const T16* base = static_cast<const T16*>(a.base);
  const T16* query = static_cast<const T16*>(a.query);
  hipLaunchKernelGGL((row_norms_kernel<T16>), dim3(norm_grid(a.N_base)), dim3(256), 0, stream, base,
                     a.N_base, a.D, static_cast<const float*>(nullptr), bnorm,
                     static_cast<uint32_t*>(nullptr));
  hipLaunchKernelGGL((row_norms_kernel<T16>), dim3(norm_grid(a.Nq)), dim3(256), 0, stream, query, a.Nq,
                     a.D, static_cast<const float*>(nullptr), qnorm, static_cast<uint32_t*>(nullptr));
  const uint64_t nb = static_cast<uint64_t>(a.N_base) * a.D / 8, nq = static_cast<uint64_t>(a.Nq) * a.D / 8;
  hipLaunchKernelGGL((bf_f16_flag_kernel<T16>),
                     dim3(static_cast<uint32_t>(std::clamp<uint64_t>((nb + nq + 1023) / 1024, 1, 2048))),
                     dim3(256), 0, stream, static_cast<const uint4*>(a.base), nb,
                     static_cast<const uint4*>(a.query), nq, bnorm,
                     static_cast<uint64_t>(a.N_base) + a.Nq, flags + 1);
  if (ch)
    hipLaunchKernelGGL((bf_f16_pack_kernel<2>),
                       dim3(static_cast<uint32_t>(std::min<uint64_t>((n16 + 255) / 256, 8192))), dim3(256),
                       0, stream, static_cast<const uint16_t*>(a.query), a.Nq, a.D, nch, n16, q_packed);
  constexpr float u = 5.9604645e-8f;
  const float Df = static_cast<float>(a.D);
  const float c = 1.03f * kBfF16Cm * (2.0625f * Df + 24.f) * u;
  hipLaunchKernelGGL(bf_range_f16_thr_kernel, dim3((a.Nq + 255) / 256), dim3(256), 0, stream, a.radii,
                     qnorm, a.Nq, Df, c, thr);
  GGNN_HIP_CHECK(hipGetLastError());

  BfRangeF16FilteredArgs t{};
  t.base = a.base;
  t.query = a.query;
  t.query_packed = q_packed;
  t.bnorm = bnorm;
  t.qnorm = qnorm;
  t.thr = thr;
  t.flag = flags + 1;
  t.c = c;
  t.D = a.D;
  t.Nq = a.Nq;
  t.N_base = a.N_base;
  t.nch = nch;
  t.parts = parts;
  t.rows_per_part = rows_per_part;
  t.counts = cand_counts;
  t.offsets = cand_offsets;
  t.cand_lims = cand_lims;
  t.budget = budget;
  t.cand_ids = cand_ids;
  t.cand_de = cand_dists;
  auto tile_pass = [&](bool fill) {
    if (fm == kBfBits)
      launch_bf_range_f16_tiles<T16, kBfBits>(a, t, fill, qblocks, stream);
    else if (fm == kBfLabels)
      launch_bf_range_f16_tiles<T16, kBfLabels>(a, t, fill, qblocks, stream);
    else
      launch_bf_range_f16_tiles<T16, kBfNoFilter>(a, static_cast<const BfRangeF16Args&>(t), fill, qblocks,
                                                  stream);
  };
  tile_pass(false);
  launch_bf_range_prefix(cand_counts, a.Nq, parts, cand_offsets, cand_lims, stream);
  hipLaunchKernelGGL(bf_range_f16_budget_kernel, dim3(1), dim3(1), 0, stream, cand_lims, a.Nq, budget,
                     flags + 1, flags, a.fell_back);
  tile_pass(true);

  BfRangeF16ExactArgs ex{};
  ex.base = a.base;
  ex.query = a.query;
  ex.radii = a.radii;
  ex.bnorm = bnorm;
  ex.qnorm = qnorm;
  ex.cand_counts = cand_counts;
  ex.cand_offsets = cand_offsets;
  ex.cand_lims = cand_lims;
  ex.cand_ids = cand_ids;
  ex.cand_dists = cand_dists;
  ex.hit_counts = hit_counts;
  ex.violated = flags + 2;
  ex.budget = budget;
  ex.D = a.D;
  ex.Nq = a.Nq;
  ex.N_base = a.N_base;
  ex.parts = parts;
#define GGNN_BF_RANGE_F16_EXACT(T, LPR, NCH)                                                           \
  do {                                                                                                 \
    if constexpr (std::is_same<T, T16>::value)                                                         \
      hipLaunchKernelGGL((bf_range_f16_exact_kernel<T, LPR, NCH>), grid_for(pairs), dim3(kWave), 0,    \
                         stream, ex);                                                                  \
  } while (0)
  GGNN_DISPATCH_DIST_16(a.dtype, a.D, GGNN_BF_RANGE_F16_EXACT);
#undef GGNN_BF_RANGE_F16_EXACT
  hipLaunchKernelGGL(bf_range_f16_guard_kernel, dim3(1), dim3(1), 0, stream, flags + 2, cand_lims, a.Nq,
                     flags, a.fell_back);
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

  // the scan passes, gated: they answer the call iff the gate was raised
  BfRangeLaunch fb = a;
  fb.lims = scan_lims;
  launch_bf_range_scan(fb, flags, stream);
  launch_bf_range_take_lims(flags, scan_lims, a.Nq + 1, a.lims, stream);
}

void launch_bf_range_query_f16(const BfRangeLaunch& a, hipStream_t stream)
{
  if (a.dtype == GGNN_F16)
    launch_bf_range_f16_t<f16_t>(a, stream);
  else if (a.dtype == GGNN_BF16)
    launch_bf_range_f16_t<bf16_t>(a, stream);
  else
    throw Error(GGNN_UNSUPPORTED, "range search: the 16-bit tile kernels take float16 / bfloat16 rows");
}

}  // namespace ggnn_amd
