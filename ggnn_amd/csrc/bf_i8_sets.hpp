// Device helpers shared by the register-set integer kernels of bf_query: bf_i8.hip (rows of up to 128
// bytes) and bf_i8_wide.hip (wider rows).  Pending-list size, the "no threshold yet" constant, the
// accumulator-register / query-row map, and the bound exchange between the slices of a query.
#pragma once
#include <utility>

#include "bf_common.hpp"

namespace ggnn_amd {

#ifndef GGNN_I8_PEND
#define GGNN_I8_PEND 8
#endif
constexpr int kI8v2Pend = GGNN_I8_PEND;         // pending candidates per query before a batch update
// (stages between bound exchanges once past the doubling phase: BfMfmaArgs::refresh_every, hook
//  BF_I8_REFRESH, default 64.  With the single shared bound of rounds 3-4: every 2 stages 3.82 ms,
//  4: 3.54, 8-16: 3.42, 64: 3.50.)
constexpr int kTeInf = 1 << 30;

// ---- bound exchange between the slices of a query (round 5) ---------------------------------------
// Round 3-4: every slice published the last entry of its K-best set and took the minimum over the
// slices as an extra bound.  That bound is the best "K-th of ONE slice", i.e. about the 65th best
// row seen by all 12 slices together, when the 10th would do -- and each slice starts cold.  Now a
// slice publishes several POSITIONS p of its sorted set, and every slice derives, per position,
//     B_p = the m-th smallest of the published entries [p] over the slices,  m = ceil(KPT / (p+1)):
// m slices each hold p+1 rows at or below B_p, slices hold disjoint rows, so at least KPT >= K rows
// lie at or below B_p and no row above it can be among the K best (rows EQUAL to it are kept).
// Every position is valid on its own with one value per slice, read whenever (entries only ever
// decrease; a stale value is a looser bound), so there is nothing to tear.  For 12 slices and
// KPT = 10: p = 1 (the 5th smallest second-best) sits near the 17th best row overall, p = 0 near
// the 21st, p = 9 (the old bound) near the 65th.  Exchanges follow a doubling schedule (stages 1,
// 2, 4, ... 64, then every 64): the lists move fastest at the start.
// Layout: gl[query][rank][slices padded to 16] ints, 0x7fffffff = nothing published.
constexpr int kI8MaxRanks = 5;
template <int KPT>
__host__ __device__ constexpr int i8_rank_pos(int i)
{
  return KPT == 4    ? (i == 0 ? 0 : i == 1 ? 1 : 3)
         : KPT == 10 ? (i == 0 ? 0 : i == 1 ? 1 : i == 2 ? 2 : i == 3 ? 4 : 9)
                     : (i == 0 ? 0 : i == 1 ? 1 : i == 2 ? 3 : i == 3 ? 7 : 15);
}
template <int KPT>
GGNN_DEV constexpr int i8_ranks()
{
  return KPT == 4 ? 3 : 5;
}
// the M-th smallest of `n4` x 4 published values (unused slots hold 0x7fffffff)
template <int M>
GGNN_DEV int i8_mth_smallest(const int* col, int n4)
{
  int t[M];
#pragma unroll
  for (int k = 0; k < M; ++k)
    t[k] = 0x7fffffff;
  // up to 32 slices in two rounds of 16 (16 registers, not 32: the kernel has none to spare).
  // The four 16-byte loads of a round are issued back to back and waited for ONCE, device-
  // coherent (sc1: the values come from other XCDs).  As sixteen relaxed agent-scope atomic loads
  // -- the first version -- the compiler waited for each one separately: ~17 us per exchange, 12 %
  // of the kernel (stats build), where one round trip is ~1-2 us.  Slots past the slices were
  // initialised to 0x7fffffff by the host (the area is padded to 16 per position).
  for (int b0 = 0; b0 < n4; b0 += 4) {
    i32x4 w0, w1, w2, w3;
    const int* p = col + b0 * 4;
    asm volatile(
        "global_load_dwordx4 %0, %4, off sc1\n\t"
        "global_load_dwordx4 %1, %4, off offset:16 sc1\n\t"
        "global_load_dwordx4 %2, %4, off offset:32 sc1\n\t"
        "global_load_dwordx4 %3, %4, off offset:48 sc1\n\t"
        "s_waitcnt vmcnt(0)"
        : "=&v"(w0), "=&v"(w1), "=&v"(w2), "=&v"(w3)
        : "v"(p)
        : "memory");
    const int v[16] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3],
                       w2[0], w2[1], w2[2], w2[3], w3[0], w3[1], w3[2], w3[3]};
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      int x = v[e];
#pragma unroll
      for (int k = 0; k < M; ++k) {
        const int lo = min(t[k], x);
        x = max(t[k], x);
        t[k] = lo;
      }
    }
  }
  return t[M - 1];
}

// stages at which a slice exchanges: 1, 2, 4, ... while the lists still move fast, then every
// kI8v2Refresh-th (an exchange is five dependent-free batches of device-coherent loads, ~1.5 stages)
GGNN_DEV bool i8_exchange_stage(uint32_t st, uint32_t every)
{
  if (st == 0)
    return false;
  return st < every ? (st & (st - 1)) == 0 : st % every == 0;
}

GGNN_DEV int i8v2_qrow(int r, int h)
{
  return (r & 3) + 8 * (r >> 2) + 4 * h;  // query row of accumulator register r in half-wave h
}

// ---- the lane = query bookkeeping as functions (bf_i8_filtered.hip: both of its kernels) ------------
// bf_i8v2_kernel and bf_i8w_kernel carry the same steps as lambdas; these are their bodies, word for word.
// slot of query (lane & 31) of set (lane >> 5) in the offset block, which is kept in matrix order
GGNN_DEV int i8_offset_slot(int lane)
{
  return (lane & 32) + 16 * ((lane >> 2) & 1) + (lane & 3) + 4 * ((lane & 31) >> 3);
}
// offsets of set s2 as the accumulators of half-wave h want them
GGNN_DEV i32x16 i8_load_offsets(const int* hq_w, int s2, int h)
{
  const i32x4* p = reinterpret_cast<const i32x4*>(hq_w + s2 * 32 + 16 * h);
  const i32x4 a0 = p[0], a1 = p[1], a2 = p[2], a3 = p[3];
  return i32x16{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3],
                a2[0], a2[1], a2[2], a2[3], a3[0], a3[1], a3[2], a3[3]};
}
// applies the pending candidates of all 64 queries in lockstep: one sorted insertion per query and
// iteration, all in registers; the pending counts are reset
template <int KPT>
GGNN_DEV void i8_apply_pending(int (&sd)[KPT], int (&si)[KPT], int qn_q, int* pc_w, const int* pd_w,
                               const int* pi_w, int lane)
{
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int cnt = min(pc_w[lane], kI8v2Pend);
  pc_w[lane] = 0;
  for (int i = 0; __any(i < cnt); ++i) {
    const bool have = i < cnt;
    // (an absent record is "infinity": it changes nothing)
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
}
// publishes this slice's entries at the positions of rank_mask (single writer per word) and derives the
// bound of the query from what all slices published: 0x7fffffff = none yet
template <int KPT>
GGNN_DEV int i8_exchange_bound(const int (&sd)[KPT], int* gl_q, int sl4, uint32_t slice, uint32_t rank_mask)
{
  constexpr int NR = i8_ranks<KPT>();
  int bound = 0x7fffffff;
  [&]<int... I>(std::integer_sequence<int, I...>) {
    ((((rank_mask >> I) & 1u) ? __hip_atomic_store(gl_q + I * 4 * sl4 + slice, sd[i8_rank_pos<KPT>(I)],
                                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                              : (void)0),
     ...);
    ((bound = ((rank_mask >> I) & 1u)
                  ? min(bound, i8_mth_smallest<(KPT + i8_rank_pos<KPT>(I)) / (i8_rank_pos<KPT>(I) + 1)>(
                                   gl_q + I * 4 * sl4, sl4))
                  : bound),
     ...);
  }(std::make_integer_sequence<int, NR>{});
  return bound;
}
// a slice's set of one query leaves: unused slots as kEmptyKey / +inf
template <int KPT>
GGNN_DEV void i8_write_set(const int (&sd)[KPT], const int (&si)[KPT], int32_t* ids, float* dists)
{
#pragma unroll
  for (int k = 0; k < KPT; ++k) {
    const bool used = sd[k] != 0x7fffffff;
    ids[k] = used ? si[k] : kEmptyKey;
    dists[k] = used ? static_cast<float>(sd[k]) : inf_f();
  }
}

}  // namespace ggnn_amd
