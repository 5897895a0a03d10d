// bf_query for float16 / bfloat16 rows under squared L2, unfiltered: the contraction runs on the 16-bit
// matrix cores (v_mfma_f32_32x32x16_f16 / _bf16: 16 columns per instruction, f32 accumulate), tiles
// are staged RAW in 16 bits.  bf_mfma.hip widens such rows to float32 and contracts them two columns
// per instruction; it keeps cosine, every filtered call and BF_F16 = 1.
//
// Passes, one stream, nothing waits for the host:
//   norms    row_norms_kernel<T16> (bf_mfma.hip): float32 |x|^2 of every base row and query from the
//            widened values, fmaf chains and a tree; the running maximum of the base norms
//   flag     bf_f16_flag_kernel: raised if any base or query element is subnormal in its 16-bit type or
//            non-finite, or if a norm is non-finite.  Whether the 16-bit matrix instructions flush
//            subnormal inputs is not established for this part, so the certificate does not rest on
//            it: under the flag the tile pass leaves at once, the re-rank puts EVERY query onto the
//            rescan list and launch_bf_rescan answers the call with the scan's bits (n_rescanned = Nq)
//   pack     bf_f16_pack_kernel (D > 128): the query set in operand order, in 16 bits
//   tiles    bf_f16_kernel: candidate lists of KP = K + 8 (d_e, id) per (query, part)
//   re-rank  bf_f16_rerank_kernel: direct form (DistEngine, the scan's bits) of all candidates, ranked by
//            (distance, id); the certificate and the run-time guard below; uncertified -> rescan list
//   rescan   launch_bf_rescan (bf_query.hip)
//
// The tile kernel.  256 threads; a wave owns NS sets of 32 queries (NS = 2 while the lists of 256 queries
// fit beside the tiles with two workgroups per CU, else 1) that share every B operand read from LDS.
// Queries are the M side of the instruction: accumulator register r of half h holds query row
// (r & 3) + 8 (r >> 2) + 4 h of its set, lanes are base rows -- the row norm is one value per lane, and
// bf_insert_hits (bf_mfma.hip) takes the accumulators as they are.  Lane (j, h) contributes columns
// 16 m + 8 h .. + 7 of query row j (A) and of base row j (B) to instruction m: one ds_read_b128 per B
// operand.  LDS rows are CB = 32 NM bytes of raw halves plus 16 spare bytes that hold the row's float32
// norm: an odd number of 16-byte slots, conflict-free b128 reads.  Columns past D are zero in the
// tile and in the query operand.
//   * D <= 128: one chunk of 16 NM columns, NM in {2, 4, 8} (D <= 32 / 64 / 128; D = 96 runs NM = 8);
//     the query operand lives in registers (4 VGPRs per instruction and set); a stage is 16 / NM tiles,
//     so a wave with two sets sees one barrier per 32 instructions at every NM.
//   * D > 128 (CH): chunks of 128 columns, a stage is two tiles x one chunk (32 instructions per
//     barrier), all chunks of a stage go into the same f32 accumulators, the query operand of the next
//     chunk is requested from the packed copy (one contiguous kilobyte per load instruction) right
//     behind the instructions of this one and arrives under the stage store and the barrier.
//   Stages are double buffered; every global load is unconditional with a clamped address (rows past
//   the end of a range repeat its last row and get the norm +inf when stored: d_e = +inf, never below
//   a threshold).
//   Epilogue per (tile, set): d_e = fmaf(-2, dot, |q|^2 + |b|^2) for the lane's 16 query rows against the
//   per-query thresholds (worst list entries, in LDS), one ballot; only a set whose ballot is non-zero
//   enters bf_insert_hits (stable insertion: equal d_e keep the lower id first).
//   Not built: a max3 pre-test on accumulators that start from a per-query constant in the C operand.
//   It would decide "no hit" from a value whose rounding inside the instruction is exactly what is not
//   known (below), and a miss there is silent; the epilogue stays the exact expanded form.
//   Work split: (query block, stage-sized unit) pairs in one sequence cut into one round of resident
//   workgroups, as bf_mfma_kernel's equal ranges; parts and the part_ids / part_dists layout likewise.
//
// Why the pre-selection cannot lose a neighbour.  No centring (a 16-bit shift is not representable):
// a = q, b = x exactly.  u = 2^-24.  Products of two f16 (22 significant bits) or two bf16 values (16)
// are exact in float32.  How one instruction sums its 16 products and C is NOT known, so it is modelled:
//     C' = C + sum_k a_k b_k   with error at most   c_m 17 u (|C| + sum_k |a_k b_k|)
//   A chain of n = ceil(D / 16) instructions from C = 0 then has, with A = sum |a_k b_k| <= (|a|^2+|b|^2)/2,
//     |dot - a.b| <= n 17 c_m u A (1 + 17 c_m u)^n <= 1.02 c_m (1.0625 D + 17) u (|a|^2 + |b|^2) / 2
//   (n <= 256 and c_m <= 64).  The norms are within 1.01 (D + 4) u of |a|^2, |b|^2, the sum of the norms and
//   the final fmaf add two roundings of at most u (|a|^2 + |b|^2) each.  With G(D) = 2.0625 D + 24, c_m >= 1:
//     |d_e - ||q-x||^2| <= B(q, x) = 1.02 c_m G(D) u (|q|^2 + |x|^2) + (2D + 8) 2^-125
//   (the absolute term: products and sums in the float32 denormal range, as in bf_mfma.hip), and
//     d_dir >= ||q-x||^2 (1 - (D+3) u)                                          (direct form, as today)
//   A row left out of the list of part s has d_e >= w_s.  With w = min_s w_s and
//     E = 1.02 c_m G(D) u (|q|^2 + max_rows |x|^2) + 4 u w + (2D + 8) 2^-125
//   (4 u w: the roundings of E and of the compare itself) every left-out row has
//   d_dir >= (w - E)(1 - 1.01 (D+3) u); if that exceeds the K-th re-ranked distance the query is certified.
//   c_m is MEASURED, not derived (kBfF16Cm; DESIGN.md 4.6 has the figures).  Because the model is
//   empirical the re-rank also checks it on every candidate it holds, which has both values:
//     |d_e - d_dir| <= B(q, x) + 1.01 (D+3) u d_dir
//   A query with a candidate outside this is not certified and goes to the rescan.  Kept rows thereby
//   check the model on every call; left-out rows rest on it.
#include <algorithm>

#define GGNN_BF_SHARED_ONLY
#include "bf_mfma.hip"  // row_norms_kernel, norm_grid, bf_expand, bf_test_and_insert

namespace ggnn_amd {

// the model constant c_m of the header: measured by scripts/bf_f16_cm.py on adversarial
// inputs (DESIGN.md 4.6 has the figures), the next power of two at or above four times the observed
// value, never below 1.  tests/test_bf_f16.py restates the bound with c_m as a parameter.
constexpr float kBfF16Cm = 1.0f;

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

template <typename T16>
struct Half16;
template <>
struct Half16<f16_t> {
  static constexpr uint32_t kExp = 0x7c00u, kMant = 0x03ffu;
  static GGNN_DEV f32x16 mfma(const u32x4& a, const u32x4& b, const f32x16& c)
  {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a),
                                                  __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
};
template <>
struct Half16<bf16_t> {
  static constexpr uint32_t kExp = 0x7f80u, kMant = 0x007fu;
  static GGNN_DEV f32x16 mfma(const u32x4& a, const u32x4& b, const f32x16& c)
  {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a),
                                                   __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};

// ---- eligibility flag -------------------------------------------------------------------------------
// nb / nq: 16-byte chunks of the base and of the query set; norms: the nn = N + Nq float32 norms
template <typename T16>
__global__ void __launch_bounds__(256) bf_f16_flag_kernel(const uint4* base, uint64_t nb,
                                                         const uint4* query, uint64_t nq,
                                                         const float* norms, uint64_t nn, uint32_t* flag)
{
  constexpr uint32_t E = Half16<T16>::kExp, M = Half16<T16>::kMant;
  auto bad_half = [](uint32_t x) { return (x & E) == E || ((x & E) == 0u && (x & M) != 0u); };
  auto bad_word = [&](uint32_t w) { return bad_half(w) || bad_half(w >> 16); };
  bool bad = false;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
  const uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  for (uint64_t i = i0; i < nb + nq; i += stride) {
    const uint4 v = i < nb ? base[i] : query[i - nb];
    bad = bad || bad_word(v.x) || bad_word(v.y) || bad_word(v.z) || bad_word(v.w);
  }
  for (uint64_t i = i0; i < nn; i += stride)
    bad = bad || !(norms[i] < inf_f());  // +inf or NaN
  if (__any(bad) && (threadIdx.x & 63) == 0)
    atomicOr(flag, 1u);
}

// ---- packed query copy (D > 128) ----------------------------------------------------------------------
// [query block][wave][chunk][set][instruction m][lane] 16 bytes: columns 128 c + 16 m + 8 h .. + 7 of
// query row j of the set -- what lane (j, h) feeds instruction m of chunk c, so one load instruction of
// a wave is one contiguous kilobyte.  Padding queries and columns past D are zero.
template <int NS>
__global__ void __launch_bounds__(256) bf_f16_pack_kernel(const uint16_t* query, uint32_t Nq, uint32_t D,
                                                         uint32_t nch, uint64_t n16, uint4* out)
{
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; i < n16;
       i += static_cast<uint64_t>(gridDim.x) * 256) {
    const uint32_t lane = static_cast<uint32_t>(i & 63);
    uint64_t r = i >> 6;
    const uint32_t m = static_cast<uint32_t>(r & 7);
    r >>= 3;
    const uint32_t s = static_cast<uint32_t>(r % NS);
    r /= NS;
    const uint32_t c = static_cast<uint32_t>(r % nch);
    r /= nch;  // = query block * 4 + wave
    const uint64_t q = r * (32 * NS) + s * 32 + (lane & 31);
    const uint32_t col = c * 128 + 16 * m + 8 * (lane >> 5);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (q < Nq && col < D)  // (D is a multiple of 8: all eight columns exist)
      v = *reinterpret_cast<const uint4*>(query + q * D + col);
    out[i] = v;
  }
}

constexpr int bf_f16_stage_tiles(int NM, bool CH)
{
  return CH ? 2 : 16 / NM;
}

// (bf_range_f16.hip takes the shared device code above only: GGNN_BF_F16_SHARED_ONLY)
#ifndef GGNN_BF_F16_SHARED_ONLY
// ---- tile kernel ------------------------------------------------------------------------------------
struct BfF16Args {
  const void* base;
  const void* query;
  const uint4* query_packed;  // CH only
  const float* bnorm;
  const float* qnorm;
  const uint32_t* flag;  // != 0: the scan answers the call
  int32_t* part_ids;     // [parts][Nq][KP]
  float* part_dists;
  uint32_t D, Nq, N_base, KP, nch;
  uint32_t units_per_q;      // stage-sized units per query block
  uint32_t units_per_block;  // range of one workgroup
  uint64_t total_units;      // query blocks * units_per_q
};

// dynamic LDS of a tile workgroup: two stages, norms and thresholds of its queries, the lists, and 128
// words that bf_insert_hits may read (never use) past the last list
constexpr size_t bf_f16_lds_bytes(int NM, int NS, bool CH, uint32_t KP)
{
  return 2ull * bf_f16_stage_tiles(NM, CH) * kBfTileRows * (NM * 32 + 16) +
         (2ull * 128 * NS + 2ull * 128 * NS * KP + 128) * sizeof(float);
}

template <typename T16, int NM, int NS, bool CH>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
    bf_f16_kernel(const BfF16Args a)
{
  static_assert(!CH || NM == 8, "chunks are 128 columns");
  constexpr int TPS = bf_f16_stage_tiles(NM, CH);
  constexpr uint32_t SR = TPS * kBfTileRows;          // rows of a stage
  constexpr uint32_t CB = NM * 32, RS = CB + 16;      // bytes of a chunk row, LDS row stride
  constexpr uint32_t stage_bytes = SR * RS;
  constexpr uint32_t PPR = 2 * NM;                    // 16-byte pieces per chunk row
  constexpr int PPT = static_cast<int>(SR * PPR / 256);  // pieces per thread and stage
  static_assert(PPT == 4 && SR <= 256, "stage geometry");
  constexpr uint32_t QW = 32 * NS;                    // queries of a wave
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_b[];
  float* qn_l = reinterpret_cast<float*>(lds_b + 2 * stage_bytes);  // [4 QW] |q|^2
  float* thr_l = qn_l + 4 * QW;                                     // [4 QW] worst list entries
  float* list_d = thr_l + 4 * QW;
  const uint32_t KP = a.KP;
  int* list_id = reinterpret_cast<int*>(list_d + 4 * QW * KP);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  if (*a.flag != 0u)  // subnormal or non-finite input: the scan answers the call (uniform)
    return;
  const uint16_t* base = static_cast<const uint16_t*>(a.base);
  const uint16_t* query = static_cast<const uint16_t*>(a.query);
  float* wave_d = list_d + wave * QW * KP;
  int* wave_id = list_id + wave * QW * KP;
  float* qn_w = qn_l + wave * QW;
  float* thr_w = thr_l + wave * QW;

  uint64_t work = static_cast<uint64_t>(blockIdx.x) * a.units_per_block;
  const uint64_t work_end = min(a.total_units, work + a.units_per_block);
  while (work < work_end) {
    // a segment: the part of this workgroup's range that lies in one query block
    const uint32_t qblock = static_cast<uint32_t>(work / a.units_per_q);
    const uint64_t q_first = static_cast<uint64_t>(qblock) * a.units_per_q;
    const uint32_t u0 = static_cast<uint32_t>(work - q_first);
    const uint32_t cnt =
        static_cast<uint32_t>(min(static_cast<uint64_t>(a.units_per_q - u0), work_end - work));
    const uint32_t begin = u0 * SR;
    const uint32_t end = min(a.N_base, (u0 + cnt) * SR);
    // parts of a query block are numbered from the first workgroup that touches it
    const uint32_t part = blockIdx.x - static_cast<uint32_t>(q_first / a.units_per_block);
    work += cnt;
    const uint32_t qw = (qblock * 4 + wave) * QW;  // first query of this wave

    // this wave's lists, norms and thresholds; padding queries get -inf: nothing beats it
    for (uint32_t i = lane; i < QW * KP; i += 64) {
      wave_d[i] = (qw + i / KP < a.Nq) ? inf_f() : -inf_f();
      wave_id[i] = kEmptyKey;
    }
    if (lane < static_cast<int>(QW)) {
      const uint32_t qi = qw + lane;
      qn_w[lane] = qi < a.Nq ? a.qnorm[qi] : 0.f;
      thr_w[lane] = qi < a.Nq ? inf_f() : -inf_f();
    }

    // ---- staging: PPT pieces of 16 bytes per thread, threads 0 .. SR - 1 carry the row norms ----
    u32x4 sv[PPT];
    float sbn = 0.f;
    auto stage_load = [&](uint32_t row0, uint32_t col0) __attribute__((always_inline)) {
#pragma unroll
      for (int e = 0; e < PPT; ++e) {
        const uint32_t p = tid + 256 * e, srow = p / PPR, col = col0 + 8 * (p % PPR);
        const uint32_t r = min(row0 + srow, end - 1), c = min(col, a.D - 8u);
        sv[e] = *reinterpret_cast<const u32x4*>(base + static_cast<size_t>(r) * a.D + c);
      }
      sbn = a.bnorm[min(row0 + (tid & (SR - 1)), end - 1)];
    };
    auto stage_store = [&](uint32_t buf, uint32_t row0, uint32_t col0) __attribute__((always_inline)) {
      uint8_t* t = lds_b + buf * stage_bytes;
#pragma unroll
      for (int e = 0; e < PPT; ++e) {
        const uint32_t p = tid + 256 * e, srow = p / PPR, sc = p % PPR;
        *reinterpret_cast<u32x4*>(t + srow * RS + 16 * sc) =
            col0 + 8 * sc < a.D ? sv[e] : u32x4{0u, 0u, 0u, 0u};
      }
      if (tid < static_cast<int>(SR))
        *reinterpret_cast<float*>(t + tid * RS + CB) = (row0 + tid < end) ? sbn : inf_f();
    };

    // ---- the query operand: aq[s][m] = columns col0 + 16 m + 8 h .. + 7 of query row j of set s ----
    u32x4 aq[NS][NM];
    auto query_load = [&](uint32_t c) __attribute__((always_inline)) {
#pragma unroll
      for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          if constexpr (CH) {
            const size_t o = ((((static_cast<size_t>(qblock) * 4 + wave) * a.nch + c) * NS + s) * 8 + m) * 64;
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

    // distances of one (tile, set) against the thresholds; insertion only when a lane beats one
    auto epilogue = [&](const f32x16& acc, const int s, const float bn, const uint32_t row0)
                        __attribute__((always_inline)) {
      float dd[16];
      unsigned long long any = 0;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 qn4 = *reinterpret_cast<const float4*>(qn_w + s * 32 + 8 * g + 4 * h);
        const float4 th4 = *reinterpret_cast<const float4*>(thr_w + s * 32 + 8 * g + 4 * h);
        dd[4 * g + 0] = bf_expand<kL2>(acc[4 * g + 0], qn4.x, bn, true);
        dd[4 * g + 1] = bf_expand<kL2>(acc[4 * g + 1], qn4.y, bn, true);
        dd[4 * g + 2] = bf_expand<kL2>(acc[4 * g + 2], qn4.z, bn, true);
        dd[4 * g + 3] = bf_expand<kL2>(acc[4 * g + 3], qn4.w, bn, true);
        any |= __ballot(dd[4 * g + 0] < th4.x) | __ballot(dd[4 * g + 1] < th4.y) |
               __ballot(dd[4 * g + 2] < th4.z) | __ballot(dd[4 * g + 3] < th4.w);
      }
      if (any)
        bf_test_and_insert(dd, thr_w + s * 32, row0, wave_d + s * 32 * KP, wave_id + s * 32 * KP, KP, h);
    };

    const uint32_t nstages = (end - begin + SR - 1) / SR;  // >= 1
    const uint32_t nch = CH ? a.nch : 1u;
    const uint32_t nsteps = nstages * nch;
    stage_load(begin, 0);
    stage_store(0, begin, 0);
    query_load(0);
    __syncthreads();

    constexpr int NT = CH ? TPS : 1;  // accumulator tiles alive across steps
    f32x16 acc[NT][NS];
    uint32_t st = 0, c = 0;
    for (uint32_t p = 0; p < nsteps; ++p) {
      const bool last_c = c + 1 == nch;
      const uint32_t n_st = last_c ? st + 1 : st, n_c = last_c ? 0u : c + 1;
      const bool has_next = p + 1 < nsteps;
      const uint32_t row0 = begin + st * SR;
      if (has_next)
        stage_load(begin + n_st * SR, n_c * 128);
      const uint8_t* blk = lds_b + (p & 1) * stage_bytes;
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
          for (int s = 0; s < NS; ++s)
            acc[ti][s] =
                f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int m = 0; m < NM; ++m)
#pragma unroll
          for (int s = 0; s < NS; ++s)
            acc[ti][s] = Half16<T16>::mfma(aq[s][m], b[m], acc[ti][s]);
        if (!CH || last_c) {
          const float bn = *reinterpret_cast<const float*>(trow + CB);
#pragma unroll
          for (int s = 0; s < NS; ++s)
            epilogue(acc[ti][s], s, bn, row0 + t * kBfTileRows);
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

    // the lists of this segment: part `part` of the wave's queries
    for (uint32_t i = lane; i < QW * KP; i += 64) {
      const uint32_t qi = qw + i / KP;
      if (qi < a.Nq) {
        const size_t o = (static_cast<size_t>(part) * a.Nq + qi) * KP + i % KP;
        a.part_ids[o] = wave_id[i];
        a.part_dists[o] = wave_d[i];
      }
    }
  }
}

// ---- exact re-rank, certificate, run-time guard -----------------------------------------------------
struct BfF16RerankArgs {
  const void* base;
  const void* query;
  const int32_t* part_ids;
  const float* part_dists;
  const float* bnorm;
  const float* qnorm;
  const uint32_t* bnorm_max;  // float bits of the largest base-row norm
  const uint32_t* flag;
  uint32_t* rescan_count;
  uint32_t* rescan_list;
  uint32_t* ratio_sink;  // tests / scripts: float bits of max |d_e - d_dir| / ((2D+8) u (|q|^2+|x|^2)), or null
  int32_t* ids;
  float* dists;
  uint32_t D, Nq, K, KP, parts, cap;
};

template <typename T16, int LPR, int NCH>
__global__ void __launch_bounds__(kWave) bf_f16_rerank_kernel(const BfF16RerankArgs a)
{
  extern __shared__ __attribute__((aligned(16))) int lds_raw[];
  const WaveLds lds(lds_raw, 2 * a.cap);
  float* all_d = reinterpret_cast<float*>(lds.known);
  int* all_id = lds.known + a.cap;
  const int lane = threadIdx.x;
  const uint32_t n = block_linear_index();
  if (n >= a.Nq)
    return;
  if (*a.flag != 0u) {  // every query is answered by the scan
    if (lane == 0)
      a.rescan_list[atomicAdd(a.rescan_count, 1u)] = n;
    return;
  }
  const T16* base = static_cast<const T16*>(a.base);
  DistEngine<T16, LPR, NCH> de;
  de.template load_query<kL2>(base, a.D, static_cast<const T16*>(a.query) + static_cast<size_t>(n) * a.D);

  constexpr float u = 5.9604645e-8f;  // 2^-24
  const float Df = static_cast<float>(a.D);
  const float qn = a.qnorm[n];
  const float cB = 1.02f * kBfF16Cm * (2.0625f * Df + 24.f) * u;
  const float absB = (2.f * Df + 8.f) * 2.3509887e-38f;
  bool model_ok = true;
  float ratio = 0.f;

  const uint32_t total = a.parts * a.KP;
  uint32_t count = 0;
  for (uint32_t c0 = 0; c0 < total; c0 += kKBlock) {
    const uint32_t c = c0 + lane;
    int cand = kEmptyKey;
    float d_e = 0.f;
    if (lane < (int)kKBlock && c < total) {
      const size_t o = (static_cast<size_t>(c / a.KP) * a.Nq + n) * a.KP + c % a.KP;
      cand = a.part_ids[o];
      d_e = a.part_dists[o];
    }
    const unsigned long long surv = __ballot(cand != kEmptyKey);
    const int nsurv = __popcll(surv);
    if (!nsurv)
      continue;
    const int pos = __popcll(surv & ((1ull << lane) - 1ull));
    __syncthreads();
    if (cand != kEmptyKey)
      lds.ckeys[pos] = cand;
    __syncthreads();
    compute_distances<kL2>(de, lds, nsurv, nullptr);
    __syncthreads();
    if (cand != kEmptyKey) {
      // the guard: the model's two-sided bound between the two forms of this candidate
      const float d_dir = lds.cd0[pos];
      const float norms = qn + a.bnorm[cand];
      const float diff = fabsf(d_e - d_dir);
      model_ok = model_ok && diff <= cB * norms + absB + 1.01f * (Df + 3.f) * u * d_dir;
      if (a.ratio_sink)
        ratio = fmaxf(ratio, diff / ((2.f * Df + 8.f) * u * norms));  // (NaN for 0 / 0: fmaxf drops it)
    }
    if (lane < nsurv) {
      all_d[count + lane] = lds.cd0[lane];
      all_id[count + lane] = lds.ckeys[lane];
    }
    count += nsurv;
  }
  __syncthreads();
  int32_t* out_i = a.ids + static_cast<size_t>(n) * a.K;
  float* out_d = a.dists + static_cast<size_t>(n) * a.K;
  for (uint32_t i = lane; i < count; i += kWave) {
    const float d = all_d[i];
    const int id = all_id[i];
    uint32_t rank = 0;
    for (uint32_t jj = 0; jj < count; ++jj) {
      const float dj = all_d[jj];
      rank += (dj < d) || (dj == d && all_id[jj] < id);
    }
    if (rank < a.K) {
      out_i[rank] = id;
      out_d[rank] = d;
    }
    if (rank + 1 == a.K)
      lds.cd0[0] = d;  // K-th distance, for the certificate below
  }
  for (uint32_t k = count + lane; k < a.K; k += kWave) {
    out_i[k] = kEmptyKey;
    out_d[k] = inf_f();
  }
  if (a.ratio_sink) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
      ratio = fmaxf(ratio, __shfl_xor(ratio, o));
    if (lane == 0)
      atomicMax(a.ratio_sink, __float_as_uint(ratio));
  }

  // ---- certificate (see the top of this file) -------------------------------------------------
  bool ok = __all(model_ok);
  if (ok && count >= a.K) {  // (count < K: every row of the base is a candidate)
    float w = inf_f();
    for (uint32_t s = lane; s < a.parts; s += kWave)
      w = fminf(w, a.part_dists[(static_cast<size_t>(s) * a.Nq + n) * a.KP + a.KP - 1]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
      w = fminf(w, __shfl_xor(w, o));
    __syncthreads();  // the K-th distance was left in LDS by the lane that ranked it
    const float d_k = lds.cd0[0];
    const float E = cB * (qn + __uint_as_float(*a.bnorm_max)) + 4.f * u * w + absB;
    ok = (w - E) * (1.f - 1.01f * (Df + 3.f) * u) > d_k;
    if (!(w < inf_f()))
      ok = true;  // no list is full: nothing was left out
  }
  if (!ok && lane == 0)
    a.rescan_list[atomicAdd(a.rescan_count, 1u)] = n;
}

// ---- host -----------------------------------------------------------------------------------------
size_t bf_rescan_tmp_entries(const BfLaunch& a, uint32_t* slices_out);
void launch_bf_rescan(const BfLaunch& a, const uint32_t* qlist, const uint32_t* qcount,
                      int32_t* tmp_ids, float* tmp_dists, hipStream_t stream);

static uint32_t* g_bf_f16_ratio_sink = nullptr;
void bf_f16_set_ratio_sink(uint32_t* device_word)
{
  g_bf_f16_ratio_sink = device_word;
}

// the tile kernel's shape for (D, KP): instructions per set and tile, chunked or not, and sets per wave --
// two while two workgroups per CU hold their lists beside the tiles
struct BfF16Shape {
  int nm, ns;
  bool ch;
  size_t lds;
};
static BfF16Shape bf_f16_shape(uint32_t D, uint32_t KP)
{
  BfF16Shape s{};
  s.ch = D > 128;
  s.nm = s.ch ? 8 : D <= 32 ? 2 : D <= 64 ? 4 : 8;
  s.ns = 2 * bf_f16_lds_bytes(s.nm, 2, s.ch, KP) <= 160 * 1024 ? 2 : 1;
  s.lds = bf_f16_lds_bytes(s.nm, s.ns, s.ch, KP);
  return s;
}

bool bf_f16_supported(const BfLaunch& a)
{
  const int64_t mode = hook(kHookBfF16);
  if (mode == 1)
    return false;
  if (a.dtype != GGNN_F16 && a.dtype != GGNN_BF16)
    return false;
  if (a.measure != GGNN_EUCLIDEAN)
    return false;
  if (a.filter_bits || a.filter_table.ids || a.filter_table.query_labels || a.label_sets.labels ||
      a.label_ranges.labels || a.label_masks.labels)
    return false;
  if (a.D == 0 || a.D % 8 != 0 || a.D > 4096 || a.k_query == 0 || a.k_query + 8 > kBfMaxKP)
    return false;
  if (a.N_base == 0 || a.N_base > 0x7fffffffu)
    return false;
  // the lists of one workgroup beside its stages: at D <= 32 the widest stages leave room for KP <= 118
  // only, and k = 111 / 112 stay with the float32-staged tiles
  const BfF16Shape sh = bf_f16_shape(a.D, a.k_query + 8);
  if (sh.lds > 160 * 1024)
    return false;
  if (mode == 2)
    return true;
  // auto, from the sweep of DESIGN.md 4.6: bfloat16 won at 10k x 1M (D = 128 and 960) and lost at all
  // four shapes of {256, 1024} x {4096, 65536}; nothing in between was measured, so the old path stays
  // there.  float16 is hook only: N(0,1) rows rounded to float16 hold subnormals at that scale, the flag
  // sends the whole call to the scan (308 ms against 23.8).  Both wins were on the two-set kernels of
  // 128-column chunks (NM = 8): narrower rows and lists too long for two sets were not measured
  return a.dtype == GGNN_BF16 && a.Nq >= 10000 && a.N_base >= 1000000 && sh.nm == 8 && sh.ns == 2;
}

template <typename T16>
static const void* bf_f16_kernel_of(uint32_t D, int ns)
{
#define GGNN_F16_K(NM_, CH_)                                                          \
  (ns == 2 ? reinterpret_cast<const void*>(&bf_f16_kernel<T16, NM_, 2, CH_>)           \
           : reinterpret_cast<const void*>(&bf_f16_kernel<T16, NM_, 1, CH_>))
  if (D > 128)
    return GGNN_F16_K(8, true);
  return D <= 32 ? GGNN_F16_K(2, false) : D <= 64 ? GGNN_F16_K(4, false) : GGNN_F16_K(8, false);
#undef GGNN_F16_K
}

template <typename T16>
static void launch_bf_f16_t(const BfLaunch& a, hipStream_t stream)
{
  check_vector_layout(a.base, a.D, a.dtype);
  check_vector_layout(a.query, a.D, a.dtype);
  const uint32_t KP = a.k_query + 8;
  const BfF16Shape sh = bf_f16_shape(a.D, KP);
  const bool ch = sh.ch;
  const int nm = sh.nm, ns = sh.ns;
  const size_t lds = sh.lds;
  GGNN_REQUIRE(lds <= 160 * 1024, GGNN_UNSUPPORTED, "k too large for the 16-bit tile kernels");
  const uint32_t qpb = 128u * ns;
  const uint32_t qblocks = (a.Nq + qpb - 1) / qpb;
  const uint32_t nch = ch ? (a.D + 127) / 128 : 1;
  // one round of resident workgroups: as many per CU as their LDS allows, two at the most
  const uint32_t resident = 256u * static_cast<uint32_t>(std::clamp<size_t>(160 * 1024 / lds, 1, 2));
  const uint32_t unit_rows = bf_f16_stage_tiles(nm, ch) * kBfTileRows;
  const uint32_t units_per_q = (a.N_base + unit_rows - 1) / unit_rows;
  const uint64_t total_units = static_cast<uint64_t>(qblocks) * units_per_q;
  // ranges of at least 1/32 of a query block (lists start empty in every part); BF_SLICES forces them
  uint64_t per = (total_units + resident - 1) / resident;
  per = std::max<uint64_t>(per, (units_per_q + 31) / 32);
  if (const int64_t hs = hook(kHookBfSlices); hs > 0)
    per = (units_per_q + static_cast<uint32_t>(std::clamp<int64_t>(hs, 1, 64)) - 1) /
          static_cast<uint32_t>(std::clamp<int64_t>(hs, 1, 64));
  per = std::clamp<uint64_t>(per, 1, 0xffffffffu);
  const uint32_t units_per_block = static_cast<uint32_t>(per);
  const uint32_t nblocks = static_cast<uint32_t>((total_units + per - 1) / per);
  const uint32_t parts = (units_per_q + units_per_block - 1) / units_per_block + 1;

  // one scratch block: [norms N + Nq][bn_max, rescan count, flag, -][rescan list Nq][part ids]
  // [part dists][re-scan slices ids][re-scan slices dists][packed queries]
  auto pad4 = [](size_t words) { return (words + 3) / 4 * 4; };
  const size_t n_parts = pad4(static_cast<size_t>(parts) * a.Nq * KP);
  uint32_t rescan_slices = 0;
  const size_t n_rescan = pad4(bf_rescan_tmp_entries(a, &rescan_slices));
  const size_t n_norms = pad4(static_cast<size_t>(a.N_base) + a.Nq), n_list = pad4(a.Nq);
  const uint64_t n16 = ch ? static_cast<uint64_t>(qblocks) * 4 * nch * ns * 8 * 64 : 0;
  const size_t words = n_norms + 4 + n_list + 2 * n_parts + 2 * n_rescan + 4 * n16;
  ScratchGuard scratch{scratch_alloc(words * 4, stream), stream};
  float* bnorm = static_cast<float*>(scratch.p);
  float* qnorm = bnorm + a.N_base;
  uint32_t* flags = reinterpret_cast<uint32_t*>(bnorm + n_norms);  // [0] bn_max [1] count [2] flag
  uint32_t* rescan_list = flags + 4;
  int32_t* part_ids = reinterpret_cast<int32_t*>(rescan_list + n_list);
  float* part_dists = reinterpret_cast<float*>(part_ids + n_parts);
  int32_t* rescan_ids = reinterpret_cast<int32_t*>(part_dists + n_parts);
  float* rescan_dists = reinterpret_cast<float*>(rescan_ids + n_rescan);
  uint4* q_packed = reinterpret_cast<uint4*>(rescan_dists + n_rescan);
  GGNN_HIP_CHECK(hipMemsetAsync(flags, 0, 4 * sizeof(uint32_t), stream));
  // not every query block has all parts: the others read as empty lists
  GGNN_HIP_CHECK(hipMemsetAsync(part_ids, 0xff, n_parts * sizeof(int32_t), stream));
  GGNN_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(part_dists), 0x7f800000, n_parts,
                                   stream));

  const T16* base = static_cast<const T16*>(a.base);
  const T16* query = static_cast<const T16*>(a.query);
  hipLaunchKernelGGL((row_norms_kernel<T16>), dim3(norm_grid(a.N_base)), dim3(256), 0, stream, base,
                     a.N_base, a.D, static_cast<const float*>(nullptr), bnorm, flags);
  hipLaunchKernelGGL((row_norms_kernel<T16>), dim3(norm_grid(a.Nq)), dim3(256), 0, stream, query, a.Nq,
                     a.D, static_cast<const float*>(nullptr), qnorm, static_cast<uint32_t*>(nullptr));
  const uint64_t nb = static_cast<uint64_t>(a.N_base) * a.D / 8, nq = static_cast<uint64_t>(a.Nq) * a.D / 8;
  hipLaunchKernelGGL((bf_f16_flag_kernel<T16>),
                     dim3(static_cast<uint32_t>(std::clamp<uint64_t>((nb + nq + 1023) / 1024, 1, 2048))),
                     dim3(256), 0, stream, static_cast<const uint4*>(a.base), nb,
                     static_cast<const uint4*>(a.query), nq, bnorm,
                     static_cast<uint64_t>(a.N_base) + a.Nq, flags + 2);
  if (ch) {
    const dim3 grid(static_cast<uint32_t>(std::min<uint64_t>((n16 + 255) / 256, 8192)));
    const uint16_t* q16 = static_cast<const uint16_t*>(a.query);
    if (ns == 2)
      hipLaunchKernelGGL((bf_f16_pack_kernel<2>), grid, dim3(256), 0, stream, q16, a.Nq, a.D, nch, n16,
                         q_packed);
    else
      hipLaunchKernelGGL((bf_f16_pack_kernel<1>), grid, dim3(256), 0, stream, q16, a.Nq, a.D, nch, n16,
                         q_packed);
  }
  GGNN_HIP_CHECK(hipGetLastError());

  BfF16Args t{};
  t.base = a.base;
  t.query = a.query;
  t.query_packed = q_packed;
  t.bnorm = bnorm;
  t.qnorm = qnorm;
  t.flag = flags + 2;
  t.part_ids = part_ids;
  t.part_dists = part_dists;
  t.D = a.D;
  t.Nq = a.Nq;
  t.N_base = a.N_base;
  t.KP = KP;
  t.nch = nch;
  t.units_per_q = units_per_q;
  t.units_per_block = units_per_block;
  t.total_units = total_units;
  const void* kern = bf_f16_kernel_of<T16>(a.D, ns);
  if (lds > 64 * 1024)
    GGNN_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(lds)));
  void* kargs[] = {&t};
  GGNN_HIP_CHECK(hipLaunchKernel(kern, dim3(nblocks), dim3(256), kargs, lds, stream));

  BfF16RerankArgs rr{};
  rr.base = a.base;
  rr.query = a.query;
  rr.part_ids = part_ids;
  rr.part_dists = part_dists;
  rr.bnorm = bnorm;
  rr.qnorm = qnorm;
  rr.bnorm_max = flags;
  rr.flag = flags + 2;
  rr.rescan_count = flags + 1;
  rr.rescan_list = rescan_list;
  rr.ratio_sink = g_bf_f16_ratio_sink;
  rr.ids = a.ids;
  rr.dists = a.dists;
  rr.D = a.D;
  rr.Nq = a.Nq;
  rr.K = a.k_query;
  rr.KP = KP;
  rr.parts = parts;
  rr.cap = (parts * KP + 3) / 4 * 4;
  const size_t rr_lds = wave_lds_bytes(2 * rr.cap);
#define GGNN_F16_RERANK(T, LPR, NCH)                                                              \
  do {                                                                                            \
    if constexpr (std::is_same<T, T16>::value) {                                                  \
      const void* rk = reinterpret_cast<const void*>(&bf_f16_rerank_kernel<T16, LPR, NCH>);       \
      if (rr_lds > 64 * 1024)                                                                     \
        GGNN_HIP_CHECK(hipFuncSetAttribute(rk, hipFuncAttributeMaxDynamicSharedMemorySize,        \
                                           static_cast<int>(rr_lds)));                            \
      void* rargs[] = {&rr};                                                                      \
      GGNN_HIP_CHECK(hipLaunchKernel(rk, grid_for(a.Nq), dim3(kWave), rargs, rr_lds, stream));    \
    }                                                                                             \
  } while (0)
  GGNN_DISPATCH_DIST_16(a.dtype, a.D, GGNN_F16_RERANK);
#undef GGNN_F16_RERANK
  GGNN_HIP_CHECK(hipGetLastError());
  launch_bf_rescan(a, rescan_list, flags + 1, rescan_ids, rescan_dists, stream);
  if (a.n_rescanned)
    GGNN_HIP_CHECK(hipMemcpyAsync(a.n_rescanned, flags + 1, sizeof(uint32_t), hipMemcpyDeviceToDevice,
                                  stream));
}

void launch_bf_query_f16(const BfLaunch& a, hipStream_t stream)
{
  if (a.dtype == GGNN_F16)
    launch_bf_f16_t<f16_t>(a, stream);
  else if (a.dtype == GGNN_BF16)
    launch_bf_f16_t<bf16_t>(a, stream);
  else
    throw Error(GGNN_UNSUPPORTED, "the 16-bit tile kernels take float16 / bfloat16 rows");
}
#endif  // GGNN_BF_F16_SHARED_ONLY

}  // namespace ggnn_amd
