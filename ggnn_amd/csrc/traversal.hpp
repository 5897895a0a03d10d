// Wave64 device primitives of the GGNN traversal (query / merge / sym kernels), gfx950.
//
// Design: ONE WAVE PER SEARCH.  The reference keeps a per-block cache in shared
// memory and pays >= 3 block barriers plus a SORTED-wide LDS scan per accepted candidate
// (include/ggnn/cuda_utils/simple_knn_cache.cuh:126-213).  Here the sorted part of that cache
// (best list + priority-queue ring) lives in registers, one entry per lane in LOGICAL order, so
// push/pop are a ballot + one cross-lane shift; only the visited ring stays in LDS.  The state
// evolution is identical to the reference's (including the ring-wrap quirk Q1 and the tie
// rules Q2); this is validated on the CPU by oracle/wave_model.hpp against the literal
// emulation, and on the GPU against the oracle.
//
// Distances are computed for all surviving candidates of a fetch at once (LPR lanes per base
// row, 64/LPR rows per wave-wide 16-byte load instruction, i.e. fully coalesced 16 B/lane
// gathers), then the accept/push sequence is replayed in candidate order, which is what the
// reference does one candidate at a time (simple_knn_cache.cuh:268-286).  The replay is the part of
// a pop that no memory request hides, so it is written without exec-mask regions: a push is selects
// (push_step), and for one-register lists the criteria and duplicate tests are part of its masks
// (push_if, replay_push) -- one basic block per candidate.
#pragma once
#include <cstdlib>
#include <type_traits>

#include "common.hpp"
#include "hooks.hpp"

namespace ggnn_amd {

#define GGNN_DEV __device__ __forceinline__

// Stats build (-DGGNN_PHASE_CYCLES, scripts/phase_cycles.py): shader cycles per phase of a pop,
// accumulated by lane 0 in LDS behind the first 16 KB of the workgroup's allocation and added to
// g_phase_acc when the wave ends.  Every tick drains the memory counters first, so phases are
// separated (and the kernel is slower than the product build).
#ifdef GGNN_PHASE_CYCLES
static __device__ unsigned long long g_phase_acc[16];
GGNN_DEV void phase_tick(int i)
{
  extern __shared__ __attribute__((aligned(16))) int ph_lds[];
  unsigned long long* p = reinterpret_cast<unsigned long long*>(ph_lds + 4096);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  const unsigned long long t = __builtin_amdgcn_s_memtime();
  if (threadIdx.x == 0) {
    if (i >= 0)
      p[1 + i] += t - p[0];
    p[0] = t;
  }
}
GGNN_DEV void phase_begin()
{
  extern __shared__ __attribute__((aligned(16))) int ph_lds[];
  unsigned long long* p = reinterpret_cast<unsigned long long*>(ph_lds + 4096);
  if (threadIdx.x < 17)
    p[threadIdx.x] = 0;
  phase_tick(-1);
}
GGNN_DEV void phase_end()
{
  extern __shared__ __attribute__((aligned(16))) int ph_lds[];
  unsigned long long* p = reinterpret_cast<unsigned long long*>(ph_lds + 4096);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  if (threadIdx.x < 16)
    atomicAdd(&g_phase_acc[threadIdx.x], p[1 + threadIdx.x]);
}
#define GGNN_TICK(i) phase_tick(i)
#else
#define GGNN_TICK(i) ((void)0)
#endif

GGNN_DEV int rdlane(int v, int l)
{
  return __builtin_amdgcn_readlane(v, l);
}
GGNN_DEV float rdlanef(float v, int l)
{
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
GGNN_DEV int uni(int v)
{
  return __builtin_amdgcn_readfirstlane(v);
}
GGNN_DEV float inf_f()
{
  return __builtin_huge_valf();
}

template <int CTRL>
GGNN_DEV float dpp_f(float v)
{
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}

// whole-wave shifts by one lane as single DPP moves (gfx9 wave_shr / wave_shl); the boundary
// lane keeps its own value, like __shfl_up / __shfl_down
GGNN_DEV int lane_up1(int v)    // lane i <- lane i-1
{
  return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false);
}
GGNN_DEV int lane_down1(int v)  // lane i <- lane i+1
{
  return __builtin_amdgcn_update_dpp(v, v, 0x130, 0xf, 0xf, false);
}
GGNN_DEV float lane_up1(float v)
{
  return __int_as_float(lane_up1(__float_as_int(v)));
}
GGNN_DEV float lane_down1(float v)
{
  return __int_as_float(lane_down1(__float_as_int(v)));
}

// Cross-half exchange as ONE VALU instruction (gfx950 v_permlane32_swap) instead of an LDS
// crossbar round trip (ds_bpermute): lower[i] / upper[i] = the value lanes i and i+32 hold, both
// delivered to lanes i and i+32.
GGNN_DEV void halves(int v, int& lower, int& upper)
{
  const auto r = __builtin_amdgcn_permlane32_swap(static_cast<unsigned>(v),
                                                  static_cast<unsigned>(v), false, false);
  lower = static_cast<int>(r[0]);
  upper = static_cast<int>(r[1]);
}
// lanes j and j+32 <- the value of lane j (j < 32)
GGNN_DEV int lower_half_to_both(int v)
{
  int lo, up;
  halves(v, lo, up);
  return lo;
}
// min over the two half-waves, lane by lane
GGNN_DEV unsigned min_over_halves(unsigned v)
{
  int lo, up;
  halves(static_cast<int>(v), lo, up);
  return min(static_cast<unsigned>(lo), static_cast<unsigned>(up));
}

// sum over groups of LPR consecutive lanes; every lane of a group receives the group total
template <int LPR>
GGNN_DEV float group_sum(float v)
{
  v += dpp_f<0xB1>(v);  // quad_perm:[1,0,3,2]
  v += dpp_f<0x4E>(v);  // quad_perm:[2,3,0,1]
  if (LPR >= 8)
    v += dpp_f<0x141>(v);  // row_half_mirror
  if (LPR >= 16)
    v += dpp_f<0x140>(v);  // row_mirror
  // rows of 16 / half-waves exchanged by v_permlane16_swap / v_permlane32_swap: one VALU
  // instruction each instead of a ds_bpermute round trip (a + b in either order: same bits)
  if (LPR >= 32) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false,
                                                    false);
    v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
  if (LPR >= 64) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false,
                                                    false);
    v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
  return v;
}

// LDS layout of one wave (ints): known[CACHE] | ckeys[32] | cd0[32] | cd1[32] | [hashed visited set]
//   known[0,SORTED)        copy of the sorted keys, refreshed at every filtered fetch
//   known[SORTED,CACHE)    visited ring (reference: s_cache[SORTED_SIZE..CACHE_SIZE))
//   buckets[64*HB][8] | stash[32]   only for SortedList<R, HB> with HB > 0 (see there)
struct WaveLds {
  int* known;
  int* ckeys;
  float* cd0;
  float* cd1;
  GGNN_DEV WaveLds(int* base, int cache)
      : known(base), ckeys(base + cache), cd0(reinterpret_cast<float*>(base + cache + 32)),
        cd1(reinterpret_cast<float*>(base + cache + 64))
  {
  }
  static constexpr size_t extra_ints = 96;
};
constexpr int kVisSlots = 8;    // keys per bucket of the hashed visited set
constexpr int kVisStash = 32;   // overflow entries before the filter falls back to the ring scan
// ints of one wave's regions (device and host); hash_regs < 0 (tag set) is sized separately
__host__ __device__ inline size_t wave_lds_ints(uint32_t cache, int hash_regs = 0)
{
  const size_t hash_ints = hash_regs > 0 ? hash_regs * 64 * kVisSlots + kVisStash : 0;
  return cache + WaveLds::extra_ints + hash_ints;
}
inline size_t wave_lds_bytes(uint32_t cache, uint32_t hash_regs = 0)
{
  return wave_lds_ints(cache, static_cast<int>(hash_regs)) * sizeof(int);
}
// bucket registers of the hashed visited set for a visited ring of `vis` entries: ~3 keys per
// bucket on average when the ring is full; 0 = rings too long for it (see the tag set below)
inline uint32_t vis_hash_regs(uint32_t vis)
{
  return vis <= 192 ? 1u : vis <= 480 ? 2u : 0u;
}

// ---- long rings (992 / 2016 keys: searches of 1000-2000 iterations) -----------------------------
// SortedList<1, -nb_bits>.  A scan of the ring costs ~0.75 VALU instructions per key and candidate
// group (768 per fetch on a full 992-key ring, twice the rest of a pop) and 32-bit buckets for such
// a ring cost 8-25 KB of LDS per wave, i.e. the occupancy a search this long lives on.  Here
//   * the ring itself is in GLOBAL memory (one store per pop, never read unless the ring wraps or
//     the set overflows -- both rare), and
//   * the set keeps 16-bit TAGS: with M = nb_bits + 16 >= bits(N_base - 1), k -> (k * C) mod 2^M
//     (C odd) is a bijection on the keys, so (bucket = its top nb_bits, tag = its low 16 bits)
//     identifies the key EXACTLY -- no false positives, 2 bytes per key: 256 buckets x 16 bytes =
//     4 KB for a 992-key ring.  A bucket is SEVEN tags + the number of tags in use in its eighth
//     halfword (round 6; rounds 4-5 kept eight tags and a count byte elsewhere): one 16-byte read
//     brings both, buckets fill from slot 0 (tags are never removed), the probe masks the others.
//     With the candidate scratch cut to what the query kernels use this is 5.0 KB of LDS per wave
//     incl. the float query row -- 5.4 KB were 26 waves per CU, one less than the registers allow.
// A full bucket sends the key to the stash as before; a stash overflow, or the first wrap of the
// ring, switches to the scan of the global ring for the rest of the search (exact in every case).
// HB = -nb_bits selects the tag set with 2^nb_bits buckets (a compile-time constant: the table
// offsets and the hash mask fold into immediates instead of living in scalar registers)
constexpr bool is_tag_set(int hb)
{
  return hb < 0;
}
constexpr uint32_t kTagMul = 0x9E3779B1u;
constexpr int kTagSlots = 7;          // tags per 16-byte bucket (the eighth halfword counts them)
constexpr int kTagScratchInts = 64;   // candidate scratch of the tag-set kernels: ckeys[32] | cd0[32]
// buckets (log2) for a ring of `vis` keys: load factor <= 0.57 with 7 tags per bucket (256 buckets
// for 992 keys, 512 for 2016)
inline uint32_t tag_set_bucket_bits(uint32_t vis)
{
  uint32_t b = 5;
  while ((static_cast<uint32_t>(kTagSlots) << b) * 4 < 7 * vis)
    ++b;
  return b;
}
// usable when every key of the shard fits into nb_bits + 16 bits
inline bool tag_set_usable(uint32_t vis, uint32_t n_base)
{
  if (vis < 481 || vis > 2016)
    return false;
  const uint32_t m = tag_set_bucket_bits(vis) + 16;
  return m >= 32 || (static_cast<uint64_t>(n_base) <= (1ull << m));
}
// LDS of one wave: known[sorted] | ckeys[32] | cd0[32] | buckets (16 bytes each) | stash
__host__ __device__ inline size_t tag_set_lds_ints(uint32_t sorted, uint32_t nb_bits)
{
  const size_t nb = size_t{1} << nb_bits;
  return sorted + kTagScratchInts + kVisStash + nb * 4;
}
inline size_t tag_set_lds_bytes(uint32_t sorted, uint32_t vis)
{
  return tag_set_lds_ints(sorted, tag_set_bucket_bits(vis)) * sizeof(int);
}

// ---------------------------------------------------------------------------------------------
// Sorted part of the cache: logical entry i = r*64 + lane.
//   [0,BEST) best list, [BEST,SORTED) priority queue in logical order (head first).
// Reference: SimpleKNNCache, simple_knn_cache.cuh:58-352.  push() follows the cache's tie rule
// (Q2: a new equal distance goes first), push_best_stable() the KBestList's (k_best_list.cuh:
// 92-103: equal distances keep insertion order).
// ---------------------------------------------------------------------------------------------
// HB > 0: the visited ring is mirrored in an exact hash set so that the membership test of a fetch
// (simple_knn_cache.cuh:246-261 scans the whole cache for every candidate) is one bucket read
// per candidate instead of a scan of up to CACHE entries:
//   * 64*HB buckets of kVisSlots keys in LDS; lane b of hcnt[b >> 6] counts bucket b, so an
//     insert (one per pop, the key is wave-uniform) needs no LDS read;
//   * a key whose bucket is full goes to a small stash that every probe scans (normally empty);
//   * if the stash overflows too, scan_mode switches the filter back to the ring scan for the rest
//     of the search -- the ring is always maintained, so the answer is exact in every case;
//   * when the ring wraps (more pops than ring entries) the overwritten key is removed again.
// The set of keys reported as known is exactly the reference's: sorted part + visited ring.
// GR (with HB > 0): NO visited ring at all -- for searches that cannot wrap it (max_iterations <=
// ring length, the launcher's condition) the ring's only job is to say which keys are known, and
// the buckets + stash hold exactly those keys (nothing is ever removed without a wrap).  A wave's
// LDS then holds only the sorted keys, the scratch and the buckets: for kernels whose occupancy
// the 2 KB ring of a 512-key cache limits.  A key that fits neither its bucket nor the stash goes
// to an overflow list in global memory (`ring_g`, normally empty; every probe scans it when it is
// not).  (First version: the ring itself in global memory, one store per pop -- slower than the
// LDS ring at higher occupancy, 3.69 vs 3.38 ms on the 12.5M x 96 shard: with a store in flight
// the compiler can no longer wait for "all but the newest n" loads -- loads and stores retire out
// of order with respect to each other -- so every wait for the requested code rows became
// vmcnt(0) and also waited for the speculative graph row issued after them.)
// SEL: push() written with selects, and for R == 1 the one-block replay (push_if).  false keeps the
// nested `if` and the branches in front of it, for the kernels (named where they are defined) whose
// register allocation the select form pushes into scratch memory.
template <int R, int HB = 0, bool GR = false, bool SEL = true>
struct SortedList {
  static_assert(!GR || HB != 0, "ring-less: only with a hashed set or a tag set");
  static constexpr int kHashRegs = HB;
  // (the tag set of long rings keeps its ring in global memory unless the search cannot wrap it:
  // then it is ring-less as well, GR, with the same overflow list)
  static constexpr bool kGlobalRing = is_tag_set(HB) && !GR;
  int ovf_n;                  // GR: keys in the overflow list (global memory)
  static constexpr int NB = 64 * HB;
  int key[R];
  float dist[R];
  int BEST, SORTED, P, VIS;
  int head_in;    // r_prioQ_head - BEST
  int vis_head;   // r0_visited_head - SORTED
  int vis_count;  // valid entries of the visited ring
  float xi;
  int hcnt[HB > 0 ? HB : 1];  // lane b: number of keys in bucket b (+64 per register)
  int stash_n;
  int scan_mode;
  int slots;                  // usable keys per bucket (kVisSlots; tests shrink it)
  int* hbuckets;
  int* hstash;
  // tag set (HB < 0) only
  static constexpr bool kTag = is_tag_set(HB);
  static constexpr int nb_bits = kTag ? -HB : 0;
  int* ring_g;                // [VIS] visited ring of this search in global memory

  GGNN_DEV void init(int best, int sorted, int cache, float xi_, int* known,
                     int usable_slots = kVisSlots)
  {
    BEST = best;
    SORTED = sorted;
    P = sorted - best;
    VIS = cache - sorted;
    xi = xi_;
    slots = usable_slots;
    hbuckets = known + cache + static_cast<int>(WaveLds::extra_ints);
    hstash = hbuckets + NB * kVisSlots;
    reset(known);
  }
  // ring-less form of the hashed set: only known[0, sorted) lives in LDS (WaveLds(base, sorted));
  // ring: this search's overflow list, (cache - sorted) ints of global memory
  GGNN_DEV void init_global_ring(int best, int sorted, int cache, float xi_, int* known,
                                 int usable_slots, int* ring)
  {
    BEST = best;
    SORTED = sorted;
    P = sorted - best;
    VIS = cache - sorted;
    xi = xi_;
    slots = usable_slots;
    ring_g = ring;
    hbuckets = known + sorted + static_cast<int>(WaveLds::extra_ints);
    hstash = hbuckets + NB * kVisSlots;
    reset(known);
  }
  // tag-set form: only known[0, sorted) lives in LDS (WaveLds(base, sorted)); the ring is ring
  GGNN_DEV void init_tagged(int best, int sorted, int cache, float xi_, int* known, int usable_slots,
                            int* ring)
  {
    BEST = best;
    SORTED = sorted;
    P = sorted - best;
    VIS = cache - sorted;
    xi = xi_;
    slots = usable_slots < kTagSlots ? usable_slots : kTagSlots;
    ring_g = ring;
    hbuckets = known + sorted + kTagScratchInts;  // 4 ints per bucket: 7 tags + their number
    hstash = hbuckets + (4 << nb_bits);
    reset(known);
  }
  // visited ring (and its hashed mirror) empty, simple_knn_cache.cuh:73-87
  GGNN_DEV void clear_visited(int* known)
  {
    vis_head = 0;
    vis_count = 0;
    ovf_n = 0;
    if constexpr (kTag) {
      // counts (the upper half of a bucket's last word) to zero; tags need no clearing (masked
      // by the counts), the global ring is only ever read below vis_count
      for (int i = threadIdx.x; i < (1 << nb_bits); i += kWave)
        hbuckets[i * 4 + 3] = 0;
      stash_n = 0;
      scan_mode = 0;
      return;
    }
    if constexpr (!GR) {
      for (int i = SORTED + threadIdx.x; i < SORTED + VIS; i += kWave)
        known[i] = kEmptyKey;
    }
    if constexpr (HB > 0) {
      int4* hb = reinterpret_cast<int4*>(hbuckets);
      for (int i = threadIdx.x; i < NB * kVisSlots / 4; i += kWave)
        hb[i] = make_int4(kEmptyKey, kEmptyKey, kEmptyKey, kEmptyKey);
#pragma unroll
      for (int r = 0; r < (HB > 0 ? HB : 1); ++r)
        hcnt[r] = 0;
      stash_n = 0;
      scan_mode = 0;
    }
  }
  GGNN_DEV void reset(int* known)
  {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      key[r] = kEmptyKey;
      dist[r] = inf_f();
    }
    head_in = 0;
    clear_visited(known);
  }

  // bucket of a key: 24-bit multiplicative hash (v_mul_u32_u24 is full rate), top bits
  static GGNN_DEV uint32_t vis_hash(uint32_t k)
  {
    k ^= k >> 20;
    const uint32_t h = __umul24(k, 0x9E3779u);
    return HB == 2 ? (h >> 25) : (h >> 26);
  }
  GGNN_DEV int bucket_count(uint32_t b) const
  {
    if constexpr (HB == 2)
      return (b >> 6) ? rdlane(hcnt[1], b & 63) : rdlane(hcnt[0], b & 63);
    return rdlane(hcnt[0], b & 63);
  }
  GGNN_DEV void bucket_add(uint32_t b, int delta)
  {
    const int lane = threadIdx.x;
#pragma unroll
    for (int r = 0; r < (HB > 0 ? HB : 1); ++r)
      if (lane + 64 * r == static_cast<int>(b))
        hcnt[r] += delta;
  }
  // k: wave-uniform key that has just entered the visited ring
  GGNN_DEV void vis_insert(int k)
  {
    const uint32_t b = vis_hash(static_cast<uint32_t>(k));
    const int c = bucket_count(b);
    if (c < slots) {
      if (threadIdx.x == 0)
        hbuckets[b * kVisSlots + c] = k;
      bucket_add(b, 1);
    }
    else if (stash_n < kVisStash) {
      if (threadIdx.x == 0)
        hstash[stash_n] = k;
      ++stash_n;
    }
    else if constexpr (GR) {
      if (threadIdx.x == 0)
        ring_g[ovf_n] = k;  // (at most one entry per pop, pops <= ring length)
      ++ovf_n;
    }
    else
      scan_mode = 1;  // the ring scan takes over; the set is no longer maintained
  }
  // k: wave-uniform key that the ring is about to overwrite (it is in the set exactly once)
  GGNN_DEV void vis_remove(int k)
  {
    const int lane = threadIdx.x;
    const uint32_t b = vis_hash(static_cast<uint32_t>(k));
    const int c = bucket_count(b);
    __syncthreads();
    const int v = (lane < c) ? hbuckets[b * kVisSlots + lane] : -2;
    const unsigned long long hit = __ballot(v == k);
    if (hit) {
      const int p = __ffsll(static_cast<long long>(hit)) - 1;
      const int last = hbuckets[b * kVisSlots + c - 1];
      __syncthreads();
      if (lane == 0) {
        hbuckets[b * kVisSlots + p] = last;
        hbuckets[b * kVisSlots + c - 1] = kEmptyKey;
      }
      bucket_add(b, -1);
    }
    else {
      const int sv = (lane < stash_n) ? hstash[lane] : -2;
      const unsigned long long shit = __ballot(sv == k);
      if (shit) {
        const int p = __ffsll(static_cast<long long>(shit)) - 1;
        const int last = hstash[stash_n - 1];
        __syncthreads();
        if (lane == 0)
          hstash[p] = last;
        --stash_n;
      }
    }
    __syncthreads();
  }

  // tag set: bucket / tag of a key (see "long rings" above)
  GGNN_DEV uint32_t tag_hash(uint32_t k) const
  {
    const uint32_t h = k * kTagMul;
    return nb_bits + 16 >= 32 ? h : (h & ((1u << (nb_bits + 16)) - 1u));
  }
  // k: wave-uniform key that has just entered the visited ring
  GGNN_DEV void tag_insert(int k)
  {
    const uint32_t h = tag_hash(static_cast<uint32_t>(k));
    const uint32_t b = h >> 16;
    // lane l reads halfword (l & 7) of the bucket: lanes 0-6 a tag, lane 7 the number of tags
    const int lane = threadIdx.x;
    unsigned short* bucket = reinterpret_cast<unsigned short*>(hbuckets) + b * 8;
    const int mine = bucket[lane & 7];
    const int c = rdlane(mine, 7);
    // A key can be popped more than once (quirk Q1 duplicates a queue entry when the ring of the
    // priority queue has wrapped): the set keeps it once, or its copies would fill their bucket
    if (__any(lane < c && mine == static_cast<int>(h & 0xffffu)))
      return;
    if (c < slots) {
      if (threadIdx.x == 0) {
        bucket[c] = static_cast<unsigned short>(h & 0xffffu);
        bucket[7] = static_cast<unsigned short>(c + 1);
      }
    }
    else if (stash_n < kVisStash) {
      if (threadIdx.x == 0)
        hstash[stash_n] = k;
      ++stash_n;
    }
    else if constexpr (GR) {
      if (threadIdx.x == 0)
        ring_g[ovf_n] = k;  // overflow list (at most one entry per pop, pops <= ring length)
      ++ovf_n;
    }
    else
      scan_mode = 1;
  }

  GGNN_DEV float dist_at(int i) const
  {
    if constexpr (R == 1)
      return rdlanef(dist[0], i);
    float v = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r)
      if ((i >> 6) == r)
        v = rdlanef(dist[r], i & 63);
    return v;
  }
  GGNN_DEV int key_at(int i) const
  {
    if constexpr (R == 1)
      return rdlane(key[0], i);
    int v = 0;
#pragma unroll
    for (int r = 0; r < R; ++r)
      if ((i >> 6) == r)
        v = rdlane(key[r], i & 63);
    return v;
  }
  // simple_knn_cache.cuh:121-124
  GGNN_DEV float criteria() const
  {
    return dist_at(BEST - 1) + xi;
  }

  // simple_knn_cache.cuh:126-213 in lane form (oracle/wave_model.hpp::push)
  // denied (wave-uniform, filtered search): the key may be queued but never enters the best list
  GGNN_DEV void push(int k, float d, const bool denied = false)
  {
    bool dup = false;
#pragma unroll
    for (int r = 0; r < R; ++r)
      dup |= (key[r] == k);
    if (__any(dup))
      return;
    // logical index of the entry in physical slot BEST; Q1: nothing shifts into it
    const int qlane = head_in ? BEST + (P - head_in) : -1;
    if constexpr (R >= 16) {
      // long lists: the registers are walked in groups of four with two wave-uniform skips --
      // groups beyond SORTED hold nothing (R comes in steps of 16), and once the lowest
      // register of a best-list group had nothing to shift, nothing below shifts either (the
      // list is sorted).  One branch per FOUR registers: a branch per register serialises the
      // DPP / readlane chains of neighbouring registers and costs more than it skips
      // (K = 1000: 118 ms against 108 without any skip), a `break` sends the arrays to scratch.
      bool settled = false;
#pragma unroll
      for (int g = R / 4 - 1; g >= 0; --g) {
        if (g * 4 * kWave >= SORTED || settled)
          continue;
        bool low_active = false;
#pragma unroll
        for (int r = g * 4 + 3; r >= g * 4; --r)
          low_active = push_step(r, k, d, qlane, denied);
        if ((g * 4 + 1) * kWave <= BEST && !__any(low_active))
          settled = true;
      }
    }
    else {
#pragma unroll
      for (int r = R - 1; r >= 0; --r)
        push_step(r, k, d, qlane, denied);
    }
  }

  // one register of push(): entry i takes (k, d) at the insertion point, its lower neighbour above
  GGNN_DEV bool push_step(const int r, const int k, const float d, const int qlane,
                          const bool denied = false)
  {
    const int lane = threadIdx.x;
    const int i = r * kWave + lane;
    int pk = lane_up1(key[r]);
    float pd = lane_up1(dist[r]);
    if (r > 0) {
      const int bk = rdlane(key[r - 1], 63);
      const float bd = rdlanef(dist[r - 1], 63);
      if (lane == 0) {
        pk = bk;
        pd = bd;
      }
    }
    const bool first = (i == 0) || (i == BEST);
    const bool active = (dist[r] >= d) && (i < SORTED) && !(denied && i < BEST);
    const bool prev_active = !first && (pd >= d);
    if constexpr (SEL) {
      // two selects per value instead of a nested `if`: the nested form compiles to three nested
      // exec-mask regions (ten basic blocks and 16 phi copies per pushed candidate)
      const bool take_new = active && (first || !prev_active);
      const bool take_prev = active && !take_new && i != qlane && pk != kEmptyKey;
      key[r] = take_new ? k : take_prev ? pk : key[r];
      dist[r] = take_new ? d : take_prev ? pd : dist[r];
    }
    else if (active) {
      if (first || !prev_active) {
        key[r] = k;
        dist[r] = d;
      }
      else if (i != qlane && pk != kEmptyKey) {
        key[r] = pk;
        dist[r] = pd;
      }
    }
    return active;
  }

  // One-register lists: the replay of a fetch pushes through push_if(), one basic block per
  // candidate (longer lists keep the wave-uniform tests as branches in front of push())
  static constexpr bool kReplayOneBlock = (R == 1) && SEL;

  // push(k, d, denied) if `go` (wave-uniform), for R == 1: no branch, no exec-mask region.  Every
  // lane-dependent condition of push_step() is a ballot, and what a lane needs to know about its
  // lower neighbour -- "is it active", "is it empty" -- is that ballot shifted by one, so the
  // conditions combine in scalar registers, off the vector pipe:
  //   ge        lanes whose distance is >= d                      (the reference's `active`, Q2)
  //   active  = ge & [0, SORTED) & not [0, BEST) if denied, or nothing at all if the push is off
  //             (!go, or k is in the list already: the early returns of push())
  //   new     = active & (first | ~(ge << 1))                     the insertion points
  //   prev    = active & ~new & ~qlane & (nonempty << 1)          lanes taking their lower neighbour
  // and come back to the lanes as the masks of four selects.  A push that is off leaves the list
  // untouched, as the early returns do.
  GGNN_DEV void push_if(const int k, const float d, const bool go, const bool denied = false)
  {
    static_assert(R == 1 && SEL, "push_if: one list register per lane");
    using u64 = unsigned long long;
    const u64 ge = __ballot(dist[0] >= d);
    const u64 dup = __ballot(key[0] == k);
    const u64 nonempty = __ballot(key[0] != kEmptyKey);
    const u64 below_best = (2ull << (BEST - 1)) - 1ull;  // [0, BEST), 1 <= BEST <= 64
    const u64 in_sorted = ~0ull >> (kWave - SORTED);     // [0, SORTED), 1 <= SORTED <= 64
    const u64 first = 1ull | (below_best + 1ull);        // lanes 0 and BEST
    const u64 q1 = head_in ? 1ull << (BEST + (P - head_in)) : 0ull;  // Q1: nothing shifts into it
    u64 active = ge & in_sorted;
    if (denied)
      active &= ~below_best;
    if (!go || dup)
      active = 0ull;
    const u64 take_new = active & (first | ~(ge << 1));
    const u64 take_prev = active & ~take_new & ~q1 & (nonempty << 1);
    // (lane 0 never takes its neighbour: the shift may leave anything there, which saves the copy
    // that keeps the boundary lane's own value)
    const int pk = __builtin_amdgcn_update_dpp(0, key[0], 0x138, 0xf, 0xf, true);
    const float pd = dpp_f<0x138>(dist[0]);
    const bool tn = __builtin_amdgcn_inverse_ballot_w64(take_new);
    const bool tp = __builtin_amdgcn_inverse_ballot_w64(take_prev);
    key[0] = tn ? k : tp ? pk : key[0];
    dist[0] = tn ? d : tp ? pd : dist[0];
  }

  // KBestList::add_unique, k_best_list.cuh:77-109 (stable insert after equal distances, no
  // duplicate check); only the best list is used (BEST == SORTED).
  GGNN_DEV void push_best_stable(int k, float d)
  {
    const int lane = threadIdx.x;
#pragma unroll
    for (int r = R - 1; r >= 0; --r) {
      const int i = r * kWave + lane;
      int pk = lane_up1(key[r]);
      float pd = lane_up1(dist[r]);
      if (r > 0) {
        const int bk = rdlane(key[r - 1], 63);
        const float bd = rdlanef(dist[r - 1], 63);
        if (lane == 0) {
          pk = bk;
          pd = bd;
        }
      }
      const bool active = (d < dist[r]) && (i < BEST);
      const bool prev_active = (i != 0) && (d < pd);
      if (active) {
        if (!prev_active) {
          key[r] = k;
          dist[r] = d;
        }
        else {
          key[r] = pk;
          dist[r] = pd;
        }
      }
    }
  }

  // simple_knn_cache.cuh:215-239 ; crit is criteria() (or criteria_sym() for the sym cache)
  GGNN_DEV int pop(float crit, int* known)
  {
    const int k0 = peek(crit);
    if (k0 != kEmptyKey)
      pop_commit(k0, known);
    return k0;
  }
  // the two halves of pop(): the decision (which key would be popped, simple_knn_cache.cuh:218-224)
  // and the bookkeeping (:225-238).  Kernels that request the rows of the popped key's neighbours
  // between the two hide the bookkeeping under that memory latency.
  GGNN_DEV int peek(float crit) const
  {
    const int k0 = key_at(BEST);
    const float d0 = dist_at(BEST);
    return (k0 == kEmptyKey || d0 >= crit) ? kEmptyKey : k0;
  }
  GGNN_DEV void pop_commit(const int k0, int* known)
  {
    if constexpr (HB > 0 && !GR) {
      if (!scan_mode) {
        if (vis_count == VIS)  // the ring wraps: its oldest key is forgotten
          vis_remove(uni(known[SORTED + vis_head]));
        vis_insert(k0);
      }
    }
    if constexpr (GR && !kTag)
      vis_insert(k0);  // (no wrap: pops <= max_iterations <= ring length)
    if constexpr (GR && kTag)
      tag_insert(k0);
    if constexpr (kTag && !GR) {
      if (vis_count == VIS)
        scan_mode = 1;  // the ring wraps (tags are never removed): the ring scan takes over
      if (!scan_mode)
        tag_insert(k0);
    }
    if constexpr (kGlobalRing) {
      if (threadIdx.x == 0)
        ring_g[vis_head] = k0;
    }
    else if constexpr (!GR) {
      if (threadIdx.x == 0)
        known[SORTED + vis_head] = k0;
    }
    vis_head = (vis_head + 1 >= VIS) ? 0 : vis_head + 1;
    vis_count = (vis_count + 1 > VIS) ? VIS : vis_count + 1;
    const int lane = threadIdx.x;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = r * kWave + lane;
      int nk = lane_down1(key[r]);
      float nd = lane_down1(dist[r]);
      if (r + 1 < R) {
        const int bk = rdlane(key[r + 1], 0);
        const float bd = rdlanef(dist[r + 1], 0);
        if (lane == 63) {
          nk = bk;
          nd = bd;
        }
      }
      if (i >= BEST && i < SORTED) {
        const bool last = (i == SORTED - 1);
        key[r] = last ? kEmptyKey : nk;
        dist[r] = last ? inf_f() : nd;
      }
    }
    head_in = (head_in + 1 >= P) ? 0 : head_in + 1;
  }

  // Second half of the membership test of simple_knn_cache.cuh:246-261 for kernels that skipped
  // the scan of the sorted part (filter<.., false>): clears the bits of `m` whose candidate (lane
  // j holds its key in k_of) sits in the best list or the priority queue.  Must run before the
  // first push of the fetch -- the reference tests every candidate against the cache as it is when
  // the fetch starts -- and costs one compare per candidate that is still in the race (the ~5
  // that passed the pre-screen, or the ~4 whose distance beats the criteria) instead of a scan
  // of 32 / 64 keys for all 24.
  GGNN_DEV unsigned long long drop_sorted(unsigned long long m, const int k_of) const
  {
    unsigned long long out = m;
    while (m) {
      const int j = __ffsll(static_cast<long long>(m)) - 1;
      m &= m - 1;
      const int k = rdlane(k_of, j);
      bool hit = false;
#pragma unroll
      for (int r = 0; r < R; ++r)
        hit |= (key[r] == k);
      if (__any(hit))
        out &= ~(1ull << j);
    }
    return out;
  }

  // simple_knn_cache.cuh:297-333 ; goes through LDS (known[0,SORTED)), called once per layer
  GGNN_DEV void transform(const int32_t* selection, int* known, float* scratch_d)
  {
    const int lane = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = r * kWave + lane;
      if (i < BEST) {
        int k = key[r];
        if (k != kEmptyKey)
          k = selection[k];
        key[r] = k;
        known[i] = k;
        scratch_d[i] = dist[r];
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = r * kWave + lane;
      if (i >= BEST) {
        const bool copy = (i < 2 * BEST) && (i < SORTED);
        key[r] = copy ? known[i - BEST] : kEmptyKey;
        dist[r] = copy ? scratch_d[i - BEST] : inf_f();
      }
    }
    __syncthreads();
    head_in = 0;
    clear_visited(known);
  }

  // filter part of fetch(): simple_knn_cache.cuh:246-261 / simple_knn_sym_cache.cuh:408-419.
  // cand: lanes j and j+32 hold candidate j (or EMPTY).  Returns cand with known keys blanked.
  // rare: the ring in global memory is scanned, 16 bytes per lane and step, both half-waves.
  // The keys were stored by lane 0 of this wave and another lane's store does not update the
  // vector L1: it is invalidated first (agent-scope acquire)
  // count: valid entries at the head of ring_g
  GGNN_DEV unsigned scan_global_ring(unsigned acc, const unsigned c, const int h, const int count) const
  {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const int4* rp = reinterpret_cast<const int4*>(ring_g);
    const int steps = (count + 3) >> 2;  // the ring length is a multiple of four
    // (one step in flight: more would cost the whole kernel registers for a path that runs
    // for the last few pops of a search, if at all)
    for (int t = h; t < steps; t += 2) {
      int4 e = rp[t];
      if (t * 4 + 1 >= count)
        e.y = kEmptyKey;
      if (t * 4 + 2 >= count)
        e.z = kEmptyKey;
      if (t * 4 + 3 >= count)
        e.w = kEmptyKey;
      acc = min(min(acc, static_cast<unsigned>(e.x) ^ c), static_cast<unsigned>(e.y) ^ c);
      acc = min(min(acc, static_cast<unsigned>(e.z) ^ c), static_cast<unsigned>(e.w) ^ c);
    }
    return acc;
  }

  // AHEAD: the reads of the next pair of 16-byte groups are issued before the current pair is
  // folded (a lone wave otherwise pays one LDS latency per pair).  The early-rows order runs the
  // test under the latency of the candidates' row loads and prefers the 8 registers.
  // SCAN_SORTED = false (kernels that do not count evaluations, fetch_early<.., COUNT = false>):
  // only the VISITED keys are tested here -- the hashed / tag set, stash and overflow list -- and
  // the sorted part is tested later, for the few candidates that would go on to the float rows
  // (drop_sorted below).  Only while the set is in use: once a search has fallen back to the ring
  // scan (scan_mode) the full test runs as before.
  template <bool AHEAD = true, bool SCAN_SORTED = true>
  GGNN_DEV int filter(int cand, int* known) const
  {
    const int lane = threadIdx.x;
    // with the hashed set only the sorted part is scanned; the visited ring is one bucket read
    const bool hashed = (HB != 0) && !scan_mode;
    const bool scan = SCAN_SORTED || !hashed;
    if (scan) {
      __syncthreads();
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int i = r * kWave + lane;
        if (i < SORTED)
          known[i] = key[r];
      }
      __syncthreads();
    }
    const int E = (hashed || kGlobalRing || GR) ? SORTED : SORTED + vis_count;
    const int h = lane >> 5;
    const int4* kp = reinterpret_cast<const int4*>(known);
    // min over (entry XOR cand) is 0 iff some entry equals cand.  Pure VALU on purpose: the
    // v_cmp + s_or form needs fewer VALU instructions but measured slower (scalar dependency
    // chain per entry).
    const unsigned c = static_cast<unsigned>(cand);
    auto fold = [c](unsigned acc, const int4& e) {
      acc = min(min(acc, static_cast<unsigned>(e.x) ^ c), static_cast<unsigned>(e.y) ^ c);
      return min(min(acc, static_cast<unsigned>(e.z) ^ c), static_cast<unsigned>(e.w) ^ c);
    };
    unsigned acc0 = 0xffffffffu, acc1 = 0xffffffffu;
    if constexpr (kTag) {
      if (hashed) {
        // lower half-wave: candidate j probes its bucket (one 16-byte read: 7 tags and, in the
        // last halfword, how many of them are in use); upper half-wave: the stash
        const uint32_t hh = tag_hash(c);
        const uint32_t b = hh >> 16;
        const uint32_t tt = (hh & 0xffffu) * 0x10001u;
        if (h == 0) {
          const int4 w = *reinterpret_cast<const int4*>(hbuckets + b * 4);
          const int v = static_cast<int>(static_cast<unsigned>(w.w) >> 16);
          auto pair = [tt, v](unsigned a, int wv, int slot) {
            const unsigned x = static_cast<unsigned>(wv) ^ tt;
            const unsigned lo = slot < v ? (x & 0xffffu) : 1u;
            const unsigned hi = slot + 1 < v ? (x >> 16) : 1u;
            return min(a, min(lo, hi));
          };
          acc1 = pair(pair(pair(acc1, w.x, 0), w.y, 2), w.z, 4);
          acc1 = min(acc1, 6 < v ? ((static_cast<unsigned>(w.w) ^ tt) & 0xffffu) : 1u);
        }
        else {
          for (int t = 0; t < stash_n; ++t)
            acc1 = min(acc1, static_cast<unsigned>(hstash[t]) ^ c);
        }
      }
      else if constexpr (!GR)
        acc1 = scan_global_ring(acc1, c, h, vis_count);
    }
    if constexpr (GR) {
      // overflow list (normally empty): one key at a time -- this rare path must not add to the
      // register peak of the test, which the requested code rows of the early-rows order share.
      // The keys were stored by lane 0: the vector L1 is invalidated first.
      if (ovf_n) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        for (int t = 0; t < ovf_n; ++t)
          acc1 = min(acc1, static_cast<unsigned>(ring_g[t]) ^ c);
      }
    }
    if constexpr (HB > 0) {
      if (hashed) {
        // lanes j and j+32 hold candidate j: each reads one half of its bucket
        const uint32_t b = vis_hash(c);
        acc1 = fold(acc1, *reinterpret_cast<const int4*>(hbuckets + b * kVisSlots + 4 * h));
        for (int t = 0; t < stash_n; ++t)
          acc1 = min(acc1, static_cast<unsigned>(hstash[t]) ^ c);
      }
    }
    const int4* p = kp + h;
    const int T = (E + 7) >> 3;  // >= 4: SORTED >= 32
    if (!scan) {
      // (visited keys only: nothing of known[] is read)
    }
    // the reads of the next pair are issued before the current pair is folded: a lone wave
    // (small batches, tail of a launch) otherwise pays one LDS latency per pair
    else if constexpr (AHEAD) {
      int4 e0 = p[0], e1 = p[2];
      int t = 0;
      for (; t + 4 <= T; t += 2) {
        const int4 n0 = p[2 * t + 4], n1 = p[2 * t + 6];
        acc0 = fold(acc0, e0);
        acc1 = fold(acc1, e1);
        e0 = n0;
        e1 = n1;
      }
      acc0 = fold(acc0, e0);
      acc1 = fold(acc1, e1);
      t += 2;
      if (t < T)
        acc0 = fold(acc0, p[2 * t]);
    }
    else if (R == 1 && E == 32) {
      // one list register per lane: the sorted part has 32 or 64 keys, i.e. 4 or 8 groups of
      // eight -- straight-line code instead of a loop with a run-time trip count (the loop's
      // unrolled body, its remainder loops and their scalar bookkeeping cost more than the scan)
#pragma unroll
      for (int t = 0; t < 4; t += 2) {
        acc0 = fold(acc0, p[2 * t]);
        acc1 = fold(acc1, p[2 * t + 2]);
      }
    }
    else if (R == 1 && E == 64) {
#pragma unroll
      for (int t = 0; t < 8; t += 2) {
        acc0 = fold(acc0, p[2 * t]);
        acc1 = fold(acc1, p[2 * t + 2]);
      }
    }
    else {
      int t = 0;
      for (; t + 2 <= T; t += 2) {
        const int4 e0 = p[2 * t], e1 = p[2 * t + 2];
        acc0 = fold(acc0, e0);
        acc1 = fold(acc1, e1);
      }
      if (t < T)
        acc0 = fold(acc0, p[2 * t]);
    }
    return (min_over_halves(min(acc0, acc1)) == 0u) ? kEmptyKey : cand;
  }
};

// ---------------------------------------------------------------------------------------------
// LDS-resident form of the same cache for SORTED > 256 (KQuery up to 6000): a wave64 port of the
// reference's physical layout and chunked shift-insert (simple_knn_cache.cuh:58-352, emulated
// literally by oracle/ggnn_oracle.cpp::Cache with BLOCK = 64; the result does not depend on the
// chunk width).  Slow path: every push walks the sorted region through LDS.
// ---------------------------------------------------------------------------------------------
struct LdsList {
  static constexpr bool kReplayOneBlock = false;  // (every push walks LDS: see replay_push())
  int* key;     // [CACHE] physical layout: best | priority-queue ring | visited ring
  float* dist;  // [SORTED]
  int BEST, SORTED, CACHE;
  int pq_head, vis_head, vis_count;
  float xi;

  GGNN_DEV void init(int best, int sorted, int cache, float xi_, int* key_, float* dist_)
  {
    key = key_;
    dist = dist_;
    BEST = best;
    SORTED = sorted;
    CACHE = cache;
    xi = xi_;
    for (int i = threadIdx.x; i < CACHE; i += kWave) {
      key[i] = kEmptyKey;
      if (i < SORTED)
        dist[i] = inf_f();
    }
    pq_head = BEST;
    vis_head = SORTED;
    vis_count = 0;
    __syncthreads();
  }
  GGNN_DEV float dist_at(int i) const { return dist[i]; }
  GGNN_DEV int key_at(int i) const { return key[i]; }
  GGNN_DEV float criteria() const { return dist[BEST - 1] + xi; }

  // simple_knn_cache.cuh:126-213, one chunk of 64 logical entries at a time from the top.  The
  // reference separates "shift", "read the left neighbour", "insert" by barriers (four per chunk);
  // here a chunk is ONE read phase (entry, and the left neighbour's distance) and ONE write phase:
  //  * the left neighbour's distance is read before anything in or below this chunk is written,
  //    and that is the value the reference's later read decides on as well: a slot left of an
  //    insertion point is not active, so nothing shifts into it;
  //  * an inserting lane and the lane left of it never write the same slot for the same reason;
  //  * writes of a chunk touch the chunk itself and the first slot of the chunk above, which was
  //    read an iteration earlier.
  // denied (wave-uniform, filtered search): logical entries below BEST are never active
  GGNN_DEV void push(int k, float d, const bool denied = false)
  {
    const int lane = threadIdx.x;
    __syncthreads();
    bool dup = false;
    for (int i = lane; i < SORTED; i += kWave)
      dup |= (key[i] == k);
    if (__any(dup))
      return;
    const int head = pq_head;
    const int head_in = head - BEST;
    for (int block_start = (SORTED + kWave - 1) / kWave * kWave - kWave; block_start >= 0;
         block_start -= kWave) {
      const int li = block_start + lane;
      bool active = li < SORTED && !(denied && li < BEST);
      int idx = 0, r_key = kEmptyKey;
      float r_dist = 0.f, p_dist = -inf_f();
      if (active) {
        idx = li;
        if (li >= BEST)
          idx = (li + head_in < SORTED) ? li + head_in : li + head_in - SORTED + BEST;
        r_key = key[idx];
        r_dist = dist[idx];
        const bool has_prev = idx != 0 && idx != head;
        const int idx_prev = idx != BEST ? idx - 1 : SORTED - 1;
        if (has_prev)
          p_dist = dist[idx_prev];
        active = r_dist >= d;  // Q2
      }
      __syncthreads();  // every read of the chunk before its writes
      if (active) {
        if (p_dist < d) {
          key[idx] = k;
          dist[idx] = d;
        }
        if (r_key != kEmptyKey) {
          const int idx_next = (idx + 1 == SORTED) ? BEST : idx + 1;
          if (idx_next != BEST && idx_next != head) {  // Q1
            key[idx_next] = r_key;
            dist[idx_next] = r_dist;
          }
        }
      }
      // a chunk of the best list in which nothing shifts: neither does anything below it (the
      // list is sorted) -- on average this halves the walk
      if (block_start + kWave <= BEST && !__any(active))
        break;
      __syncthreads();
    }
    __syncthreads();
  }

  GGNN_DEV int pop(float crit)
  {
    __syncthreads();
    const int k0 = key[pq_head];
    const float d0 = dist[pq_head];
    if (k0 == kEmptyKey || d0 >= crit)
      return kEmptyKey;
    __syncthreads();
    if (threadIdx.x == 0) {
      key[vis_head] = k0;
      key[pq_head] = kEmptyKey;
      dist[pq_head] = inf_f();
    }
    vis_head = (vis_head + 1 >= CACHE) ? SORTED : vis_head + 1;
    vis_count = (vis_count + 1 > CACHE - SORTED) ? CACHE - SORTED : vis_count + 1;
    pq_head = (pq_head + 1 >= SORTED) ? BEST : pq_head + 1;
    __syncthreads();
    return k0;
  }

  GGNN_DEV int filter(int cand, int* /*unused*/) const
  {
    const int lane = threadIdx.x;
    __syncthreads();
    const int E = SORTED + vis_count;  // the visited ring fills contiguously until it wraps
    const int h = lane >> 5;
    const int4* kp = reinterpret_cast<const int4*>(key);
    unsigned acc = 0xffffffffu;
    const unsigned c = static_cast<unsigned>(cand);
    for (int t = 0; t * 8 < E; ++t) {
      const int4 e = kp[t * 2 + h];
      const unsigned a = min(static_cast<unsigned>(e.x) ^ c, static_cast<unsigned>(e.y) ^ c);
      const unsigned b = min(static_cast<unsigned>(e.z) ^ c, static_cast<unsigned>(e.w) ^ c);
      acc = min(acc, min(a, b));
    }
    return (min_over_halves(acc) == 0u) ? kEmptyKey : cand;
  }
};

// ---------------------------------------------------------------------------------------------
// Distance engine.  Reference: Distance, include/ggnn/cuda_utils/distance.cuh:34-164 (squared
// L2 / |1-cos|) and the two-point variant of simple_knn_sym_cache.cuh:143-283.
// LPR lanes cooperate on one base row, each lane owns NCH chunks of 16 bytes.
// ---------------------------------------------------------------------------------------------
template <typename BaseT>
struct ChunkOf;
template <>
struct ChunkOf<float> {
  using type = float4;
  static constexpr int EPC = 4;
  static GGNN_DEV float get(const float4& v, int e)
  {
    return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w;
  }
  static GGNN_DEV float4 zero()
  {
    return make_float4(0.f, 0.f, 0.f, 0.f);
  }
};
template <>
struct ChunkOf<uint8_t> {
  using type = uint4;
  static constexpr int EPC = 16;
  static GGNN_DEV float get(const uint4& v, int e)
  {
    const uint32_t w = (e >> 2) == 0 ? v.x : (e >> 2) == 1 ? v.y : (e >> 2) == 2 ? v.z : v.w;
    return static_cast<float>((w >> (8 * (e & 3))) & 0xffu);
  }
  static GGNN_DEV uint4 zero()
  {
    return make_uint4(0u, 0u, 0u, 0u);
  }
};

// signed bytes (GGNN_I8): the chunk of uint8 rows, get() sign-extends (one v_cvt_f32_i32 with an
// SDWA sext(byte) operand)
template <>
struct ChunkOf<int8_t> {
  using type = uint4;
  static constexpr int EPC = 16;
  static GGNN_DEV float get(const uint4& v, int e)
  {
    const uint32_t w = (e >> 2) == 0 ? v.x : (e >> 2) == 1 ? v.y : (e >> 2) == 2 ? v.z : v.w;
    return static_cast<float>(static_cast<int32_t>(w << (24 - 8 * (e & 3))) >> 24);
  }
  static GGNN_DEV uint4 zero()
  {
    return make_uint4(0u, 0u, 0u, 0u);
  }
};
// 8-bit rows, unsigned or signed: packed integer arithmetic in DistEngine, no pre-screen copy, and
// the register carve-outs of the kernels that read 16 elements per chunk
template <typename BaseT>
inline constexpr bool is_byte_row = std::is_same<BaseT, uint8_t>::value || std::is_same<BaseT, int8_t>::value;
// sum of the four byte products of two words on top of acc: v_dot4_u32_u8 for uint8 rows,
// v_dot4c_i32_i8 for int8 rows (the sum modulo 2^32 as uint32_t: a sum of squares is its own value,
// a signed dot product its two's complement)
template <typename BaseT>
GGNN_DEV uint32_t byte_dot4(uint32_t a, uint32_t b, uint32_t acc)
{
  if constexpr (std::is_same<BaseT, int8_t>::value)
    return static_cast<uint32_t>(__builtin_amdgcn_sdot4(static_cast<int>(a), static_cast<int>(b),
                                                        static_cast<int>(acc), false));
  else
    return __builtin_amdgcn_udot4(a, b, acc, false);
}

// 16-bit rows (GGNN_F16 / GGNN_BF16): element types of their own, 2 bytes of storage each; a
// chunk is 8 elements in one uint4.  get() widens one element to float32 exactly where it is
// used (no chunk is widened up front: 8 floats per chunk would double the registers of the rows
// in flight); everything after it is the float32 arithmetic of the generic path.
struct f16_t {
  uint16_t bits;
};
struct bf16_t {
  uint16_t bits;
};
template <>
struct ChunkOf<f16_t> {
  using type = uint4;
  static constexpr int EPC = 8;
  static GGNN_DEV float get(const uint4& v, int e)
  {
    const uint32_t w = (e >> 1) == 0 ? v.x : (e >> 1) == 1 ? v.y : (e >> 1) == 2 ? v.z : v.w;
    // v_cvt_f32_f16 (the high half through SDWA): exact
    return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>((e & 1) ? w >> 16 : w)));
  }
  static GGNN_DEV uint4 zero()
  {
    return make_uint4(0u, 0u, 0u, 0u);
  }
};
template <>
struct ChunkOf<bf16_t> {
  using type = uint4;
  static constexpr int EPC = 8;
  static GGNN_DEV float get(const uint4& v, int e)
  {
    const uint32_t w = (e >> 1) == 0 ? v.x : (e >> 1) == 1 ? v.y : (e >> 1) == 2 ? v.z : v.w;
    // bfloat16 is the high half of a float32: a shift or a mask, exact
    return __uint_as_float((e & 1) ? (w & 0xffff0000u) : (w << 16));
  }
  static GGNN_DEV uint4 zero()
  {
    return make_uint4(0u, 0u, 0u, 0u);
  }
};

enum DistMode { kL2 = 0, kCos = 1 };

// QL: the query chunks live in LDS (q_lds[c * LPR + g], LPR * NCH chunks = one padded row per
// wave) instead of NCH x 4 registers per lane, and are read where a distance is summed.  For
// kernels whose register peak lies elsewhere (early rows: the requested code rows are live across
// the membership test, the float rows are only needed for the ~4 candidates that pass).
template <typename BaseT, int LPR_, int NCH_, bool QL = false>
struct DistEngine {
  using Base = BaseT;
  using Chunk = typename ChunkOf<BaseT>::type;
  static constexpr int EPC = ChunkOf<BaseT>::EPC;
  static constexpr int LPR = LPR_;
  static constexpr int NCH = NCH_;
  static constexpr int ROWS = kWave / LPR;
  static constexpr bool kQueryInLds = QL;
  static constexpr size_t kQueryLdsBytes = QL ? sizeof(Chunk) * LPR_ * NCH_ : 0;

  const BaseT* base;
  uint32_t D;
  int g;  // lane within the row group
  bool all_chunks;  // wave-uniform: the row fills every chunk of every lane (e.g. D = 128 f32)
  Chunk q[QL ? 1 : NCH];
  Chunk* q_lds;    // QL only
  float q_norm;    // cosine: |q|^2
  uint32_t qq_u8;  // 8-bit rows: sum of squares of this lane's query elements

  GGNN_DEV Chunk qchunk(int c) const
  {
    if constexpr (QL)
      return q_lds[c * LPR + g];
    else
      return q[c];
  }

  GGNN_DEV bool chunk_valid(int c) const
  {
    return static_cast<uint32_t>((c * LPR + g) * EPC) < D;
  }
  GGNN_DEV Chunk load_chunk(const BaseT* row, int c) const
  {
    return *reinterpret_cast<const Chunk*>(row + (c * LPR + g) * EPC);
  }
  GGNN_DEV const BaseT* row_ptr(int m) const
  {
    return base + static_cast<size_t>(static_cast<uint32_t>(m)) * D;  // 64-bit addressing
  }

  // distance.cuh:104-117
  // q_lds_: the wave's LPR * NCH chunks of LDS (QL only)
  template <int MODE>
  GGNN_DEV void load_query(const BaseT* base_, uint32_t D_, const BaseT* qrow, void* q_lds_ = nullptr)
  {
    base = base_;
    D = D_;
    g = threadIdx.x % LPR;
    all_chunks = D_ == static_cast<uint32_t>(LPR * NCH * EPC);
    q_lds = static_cast<Chunk*>(q_lds_);
    float nrm = 0.f;
    qq_u8 = 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const Chunk qc = chunk_valid(c) ? load_chunk(qrow, c) : ChunkOf<BaseT>::zero();
      if constexpr (QL)
        q_lds[c * LPR + g] = qc;  // (every row group writes the same values)
      else
        q[c] = qc;
      if (MODE == kCos) {
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
          const float v = ChunkOf<BaseT>::get(qc, e);
          nrm = fmaf(v, v, nrm);
        }
      }
      if constexpr (is_byte_row<BaseT>) {
        qq_u8 = byte_dot4<BaseT>(qc.x, qc.x, qq_u8);
        qq_u8 = byte_dot4<BaseT>(qc.y, qc.y, qq_u8);
        qq_u8 = byte_dot4<BaseT>(qc.z, qc.z, qq_u8);
        qq_u8 = byte_dot4<BaseT>(qc.w, qc.w, qq_u8);
      }
    }
    q_norm = 0.f;
    if (MODE == kCos)
      q_norm = group_sum<LPR>(nrm);
    if constexpr (QL)
      __syncthreads();
  }

  // per-lane partial sums over the lane's chunks of one row
  template <int MODE>
  GGNN_DEV void partial(const Chunk (&v)[NCH], float& a, float& b) const
  {
    if constexpr (is_byte_row<BaseT>) {
      // packed integer arithmetic (v_dot4_u32_u8 / v_dot4c_i32_i8), exact: sum (o-q)^2 = sum o^2 +
      // sum q^2 - 2 sum oq.  Equals the reference's float accumulation whenever that is exact
      // (D <= 258).  int8 rows: ab is the signed dot product modulo 2^32, so the squared L2 sum below
      // is the same uint32_t as for the rows x ^ 0x80 read as uint8
      uint32_t ab = 0, bb = 0;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const Chunk qc = qchunk(c);
        ab = byte_dot4<BaseT>(v[c].x, qc.x, ab);
        ab = byte_dot4<BaseT>(v[c].y, qc.y, ab);
        ab = byte_dot4<BaseT>(v[c].z, qc.z, ab);
        ab = byte_dot4<BaseT>(v[c].w, qc.w, ab);
        bb = byte_dot4<BaseT>(v[c].x, v[c].x, bb);
        bb = byte_dot4<BaseT>(v[c].y, v[c].y, bb);
        bb = byte_dot4<BaseT>(v[c].z, v[c].z, bb);
        bb = byte_dot4<BaseT>(v[c].w, v[c].w, bb);
      }
      if (MODE == kL2) {
        a = static_cast<float>((qq_u8 + bb) - 2u * ab);
        b = 0.f;
      }
      else {
        if constexpr (std::is_same<BaseT, int8_t>::value)
          a = static_cast<float>(static_cast<int32_t>(ab));
        else
          a = static_cast<float>(ab);
        b = static_cast<float>(bb);
      }
      return;
    }
    a = 0.f;
    b = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      Chunk qc = qchunk(c);
      if constexpr (EPC == 8) {
        // 16-bit rows: the query chunk is widened again for every row.  Without the opaque copy
        // the compiler widens it once and keeps the 8 floats per chunk live across all rows in
        // flight: twice the registers of the packed chunk, and the two-chunk kernels spill.
        asm volatile("" : "+v"(qc.x), "+v"(qc.y), "+v"(qc.z), "+v"(qc.w));
      }
#pragma unroll
      for (int e = 0; e < EPC; ++e) {
        const float o = ChunkOf<BaseT>::get(v[c], e);
        const float qq = ChunkOf<BaseT>::get(qc, e);
        if (MODE == kL2) {
          const float diff = o - qq;
          a = fmaf(diff, diff, a);
        }
        else {
          a = fmaf(o, qq, a);
          b = fmaf(o, o, b);
        }
      }
    }
  }
  // distance.cuh:153-158
  GGNN_DEV float finish_cos(float dot, float nrm) const
  {
    const float norm_sqr = q_norm * nrm;
    return (norm_sqr > 0.0f) ? fabsf(1.0f - dot / sqrtf(norm_sqr)) : 1.0f;
  }
};

// rows in flight per distance pass (register budget: STEPS*NCH chunks of 4 VGPRs)
template <int LPR, int NCH>
struct StepsOf {
  static constexpr int value = (NCH <= 2) ? 4 : (NCH <= 4) ? 2 : 1;
};

// Computes the distances of the nsurv compacted candidates in lds.ckeys[0,nsurv) and leaves
// them in lds.cd0[0,nsurv).  Out-of-range chunks are neither loaded nor accumulated.
template <int MODE, class DE, int STEPS = StepsOf<DE::LPR, DE::NCH>::value>
GGNN_DEV void compute_distances(const DE& de, const WaveLds& lds, int nsurv,
                                const int32_t* translation)
{
  constexpr int ROWS = DE::ROWS;
  using Chunk = typename DE::Chunk;
  const int lane = threadIdx.x;
  const int grp = lane / DE::LPR;
  for (int s0 = 0; s0 < nsurv; s0 += ROWS * STEPS) {
    Chunk v[STEPS][DE::NCH];
    int rr[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      if (s > 0 && s0 + s * ROWS >= nsurv)
        break;  // wave-uniform: no rows left for this and the following steps
      const int r = s0 + s * ROWS + grp;
      const bool valid = r < nsurv;
      rr[s] = valid ? r : -1;
      // slots past the end read the row of the first candidate (cached, result never stored):
      // no branch and no zero-fill around the loads
      int m = lds.ckeys[valid ? r : s0];
      if (translation)
        m = translation[m];
      const auto* row = de.row_ptr(m);
#pragma unroll
      for (int c = 0; c < DE::NCH; ++c) {
        if (de.all_chunks || de.chunk_valid(c))
          v[s][c] = de.load_chunk(row, c);
        else
          v[s][c] = ChunkOf<typename DE::Base>::zero();
      }
    }
    GGNN_TICK(6);  // float rows arrived (issue + wait)
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      if (s0 + s * ROWS >= nsurv)
        break;  // wave-uniform: no rows left for this and the following steps
      if (s > 0)
        asm volatile("" ::: "memory");  // keep the branch: the later steps are usually empty
      float a, b;
      de.template partial<MODE>(v[s], a, b);
      a = group_sum<DE::LPR>(a);
      if (MODE == kCos)
        b = group_sum<DE::LPR>(b);
      if (rr[s] >= 0 && de.g == 0)
        lds.cd0[rr[s]] = (MODE == kCos) ? de.finish_cos(a, b) : a;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Exact pre-screen of candidates on a compact copy of the rows (float32 rows).
//
// ~85 % of the distance evaluations of a traversal end in "d >= criteria(): not pushed"
// (simple_knn_cache.cuh:283-285) -- for those the value of d is irrelevant.  Every row x is
// therefore also kept as 8-bit codes c with x^ = o + s*c (per-dimension offset o, one
// scale s, prescreen.hip) and   e_max >= max_rows ||x - x^||.   By the triangle
// inequality  ||q - x|| >= ||q - x^|| - e_max,  so a candidate whose bound already reaches the
// criteria at the start of the fetch can be dropped WITHOUT reading its float row: the reference
// would evaluate it and drop it as well (criteria() only tightens during a fetch).  Survivors of
// the test are evaluated exactly as before, so ids, distances and counters are unchanged; only
// HBM traffic shrinks (D bytes instead of 4D for a rejected candidate).
//
// The query is coded the same way (q^ = o + s*cq, cq clamped to [0,255]) and pays for it with its
// own coding error e_q = ||q - q^||:   ||q - x|| >= ||q^ - x^|| - e_q - e_max,   where
// ||q^ - x^||^2 = s^2 * sum (cq_d - c_d)^2 is exact integer arithmetic on v_dot4_u32_u8.
//
// Rounding: with u = 2^-24, q' = fl(fl(q-o) * fl(1/s)) has ||s q' - (q-o)|| <= 3u(||q|| + ||o||),
// e_q is a float sum of non-negative terms (relative
// error <= (Dc+8)u), and the float distance of the exact phase is >= exact*(1 - (D+8)u).  All of
// these are covered by the relative margin m = 4(Dc+32)u and the absolute slack
// e_q(1+m) + 8u(||q|| + ||o||) + e_max used in threshold().
// ---------------------------------------------------------------------------------------------
//
// Distances from lossless codes (query kernels, squared L2).  prescreen.hip publishes params[5] = 1
// for a copy coded WITHOUT loss on a power-of-two grid: every row is x_d = o_d + s*c_d exactly, with
// o_d = k_d*s, |k_d| <= 2^23.  A query with q_d = o_d + s*cq_d, cq_d an integer in [0, 255], in every
// dimension -- tested in float32 without rounding: s*cq_d is exact (8 bits times a power of two) and
// so is the sum, (k_d + cq_d)*s with |k_d + cq_d| < 2^24, hence `o_d + s*cq_d == q_d` compares the
// real numbers -- lies on the same grid.  Then x_d - q_d = s*(c_d - cq_d) is representable, and so
// is every partial sum of its squares, s^2 times an integer <= Dc * 255^2 < 2^24 (Dc <= 128: early
// rows): the float phase (diff = o - q, fmaf(diff, diff, a), group_sum; traversal order, FMA or not)
// rounds nowhere and returns s^2 * S, S = sum (cq_d - c_d)^2 -- the integer the verdicts already
// hold.  fetch_early<.., EXACT> takes the distance from there: no threshold, no compaction, no float
// rows.  The certificate is wave-uniform (Prescreen::s2 != 0); any other base or query (fractional,
// clamped, off the grid) keeps the float phase.  tests/test_lossless_math.py re-derives all of this.
constexpr int kPsHeader = 8;  // params: [0] s  [1] 1/s  [2] e_max  [3] ||o||  [4] valid
                              //         [5] lossless grid  [8..] o_d
struct NoPrescreen {
  static constexpr bool enabled = false;
};

// Cosine (MODE = kCos): rows and queries are coded after normalisation to unit length; for unit
// vectors |1 - cos| = ||q^ - x^||^2 / 2, so the same bound applies to 2 * criteria.  The float
// evaluation |1 - dot / sqrt(|q|^2 |x|^2)| (distance.cuh:153-158) is within (D+8)u of that in
// ABSOLUTE terms, covered by adding m to the criteria.  A query of zero norm (distance 1 to
// everything in the reference) switches the pre-screen off.
template <int LPR_, int NCH_, int MODE_ = kL2>
struct Prescreen {
  static constexpr bool enabled = true;
  static constexpr int LPR = LPR_;
  static constexpr int NCH = NCH_;
  static constexpr int ROWS = kWave / LPR;
  using Chunk = uint4;

  const uint8_t* codes;
  uint32_t Dc;  // code row length (multiple of 16)
  int g;
  uint4 qc[NCH];  // codes of the query for this lane's dimensions
  uint32_t qq;    // sum of their squares
  float inv_s, slack, m;
  bool usable;
  bool all_chunks;  // wave-uniform: the code row fills every chunk of every lane
  float s2;         // wave-uniform: s * s when base and query lie on the lossless grid, else 0
                    // (load<true> only; ONE scalar register for flag and factor)

  GGNN_DEV bool chunk_valid(int c) const
  {
    return static_cast<uint32_t>((c * LPR + g) * 16) < Dc;
  }
  GGNN_DEV const uint8_t* row_ptr(int k) const
  {
    return codes + static_cast<size_t>(static_cast<uint32_t>(k)) * Dc;
  }
  GGNN_DEV uint4 load_chunk(const uint8_t* row, int c) const
  {
    return *reinterpret_cast<const uint4*>(row + (c * LPR + g) * 16);
  }

  // D: float row length of the query (multiple of 4, <= Dc)
  // EXACT (the kernels of PrescreenExact): also derive the certificate of "Distances from lossless
  // codes" above
  template <bool EXACT = false>
  GGNN_DEV void load(const uint8_t* codes_, const float* params, uint32_t Dc_, const float* qrow,
                     uint32_t D)
  {
    constexpr bool kCert = EXACT && MODE_ == kL2;
    [[maybe_unused]] float s_grid = 0.f;
    [[maybe_unused]] bool on_grid = true;
    if constexpr (kCert)
      s_grid = params[0];
    codes = codes_;
    Dc = Dc_;
    g = threadIdx.x % LPR;
    all_chunks = Dc_ == static_cast<uint32_t>(LPR * NCH * 16);
    inv_s = params[1];
    const float* offs = params + kPsHeader;
    constexpr float u = 5.9604645e-8f;  // 2^-24
    m = 4.f * static_cast<float>(Dc + 32) * u;

    // cosine: the norm is needed before coding; the row is read twice (it is in cache) instead
    // of being held in registers
    float qs = 0.f;
    if (MODE_ == kCos) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const uint32_t d0 = static_cast<uint32_t>((c * LPR + g) * 16);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (d0 + 4 * j < D) {
            const float4 v = *reinterpret_cast<const float4*>(qrow + d0 + 4 * j);
            qs = fmaf(v.x, v.x, qs);
            qs = fmaf(v.y, v.y, qs);
            qs = fmaf(v.z, v.z, qs);
            qs = fmaf(v.w, v.w, qs);
          }
        }
      }
    }
    float q_scale = 1.f;
    usable = true;
    if (MODE_ == kCos) {
      const float q_norm = sqrtf(group_sum<LPR>(qs));
      usable = q_norm > 0.f && q_norm < inf_f();
      q_scale = usable ? 1.f / q_norm : 0.f;
      qs = 0.f;
    }

    float eq = 0.f;
    qq = 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const uint32_t d0 = static_cast<uint32_t>((c * LPR + g) * 16);
      uint32_t w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float4 qv = make_float4(0.f, 0.f, 0.f, 0.f), ov = qv;
        if (d0 + 4 * j < D) {
          qv = *reinterpret_cast<const float4*>(qrow + d0 + 4 * j);
          ov = *reinterpret_cast<const float4*>(offs + d0 + 4 * j);
        }
        const float qe[4] = {qv.x, qv.y, qv.z, qv.w};
        const float oe[4] = {ov.x, ov.y, ov.z, ov.w};
        w[j] = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float t = (qe[e] * q_scale - oe[e]) * inv_s;
          const float code = fminf(fmaxf(rintf(t), 0.f), 255.f);
          const float diff = t - code;
          eq = fmaf(diff, diff, eq);
          qs = fmaf(qe[e], qe[e], qs);
          w[j] |= static_cast<uint32_t>(code) << (8 * e);
          if constexpr (kCert)
            on_grid &= (oe[e] + s_grid * code == qe[e]);  // exact on a lossless-grid base (see above)
        }
        qq = __builtin_amdgcn_udot4(w[j], w[j], qq, false);
      }
      qc[c] = make_uint4(w[0], w[1], w[2], w[3]);
      // one chunk at a time: without this barrier the loads of all chunks are hoisted and the
      // kernel's register allocation is set by this prologue (184 instead of ~110 VGPRs at D=960)
      if (NCH > 2)
        asm volatile("" ::: "memory");
    }
    // norm of the vector that was coded (unit length for the cosine measure)
    const float q_norm = (MODE_ == kCos) ? 1.f : sqrtf(group_sum<LPR>(qs));
    const float e_q = params[0] * sqrtf(group_sum<LPR>(eq)) * (1.f + m);
    slack = e_q + 8.f * u * (q_norm + params[3]) + params[2];
    s2 = 0.f;
    if constexpr (kCert) {
      if (params[5] != 0.f && __all(on_grid))
        s2 = s_grid * s_grid;  // (>= 2^-80: never 0 on a certified base)
    }
  }

  // sum (cq - c)^2 over this lane's chunks of one code row (exact)
  GGNN_DEV float partial(const uint4 (&v)[NCH]) const
  {
    uint32_t ab = 0, bb = qq;  // (|cq|^2 is the accumulator's start: no add of its own)
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      ab = __builtin_amdgcn_udot4(v[c].x, qc[c].x, ab, false);
      ab = __builtin_amdgcn_udot4(v[c].y, qc[c].y, ab, false);
      ab = __builtin_amdgcn_udot4(v[c].z, qc[c].z, ab, false);
      ab = __builtin_amdgcn_udot4(v[c].w, qc[c].w, ab, false);
      bb = __builtin_amdgcn_udot4(v[c].x, v[c].x, bb, false);
      bb = __builtin_amdgcn_udot4(v[c].y, v[c].y, bb, false);
      bb = __builtin_amdgcn_udot4(v[c].z, v[c].z, bb, false);
      bb = __builtin_amdgcn_udot4(v[c].w, v[c].w, bb, false);
    }
    return static_cast<float>(bb - 2u * ab);
  }

  // a candidate with group-summed S >= threshold(crit) has a float distance >= crit
  GGNN_DEV float threshold(float crit) const
  {
    if (!(crit < inf_f()) || !usable)
      return inf_f();
    if (MODE_ == kCos)
      crit = 2.f * (crit + m) * (1.f + m);
    // v_sqrt_f32 (1 ulp) instead of the correctly rounded sequence: m >= 32 * 4 * 2^-24 covers it
    float t = __builtin_amdgcn_sqrtf(crit) * (1.f + m) + slack;
    t = t * inv_s * (1.f + m);
    return t * t * (1.f + m);
  }
};

// The pre-screen of the kernel VARIANTS that hold both phases (query kernels, early rows, squared
// L2): the same reader under a name of its own, so that they are code objects of their own next to
// the kernels of Prescreen<8, 1, kL2>, which stay what they were.  A launch takes them when the
// caller knows the base's lossless-grid flag (QueryLaunch::ps_lossless); a wave whose query is off
// the grid falls back to the float phase inside them.
template <int LPR_, int NCH_, int MODE_ = kL2>
struct PrescreenExact : Prescreen<LPR_, NCH_, MODE_> {
};
template <class PS>
struct PsExact {
  static constexpr bool value = false;
};
template <int LPR, int NCH, int MODE>
struct PsExact<PrescreenExact<LPR, NCH, MODE>> {
  static constexpr bool value = true;
};
// the two-phase counterpart of a pre-screen type (itself where there is none)
template <class PS>
struct ExactOf {
  using type = PS;
};
template <>
struct ExactOf<Prescreen<8, 1, kL2>> {
  using type = PrescreenExact<8, 1, kL2>;
};

// code-row layout used next to a float-row layout <LPR, NCH> (a code row has a quarter of the
// 16-byte chunks of the float row)
template <int LPR, int NCH, int MODE>
struct PsFor {
  using type = Prescreen<8, 1, MODE>;
};
template <int MODE>
struct PsFor<16, 4, MODE> {
  using type = Prescreen<16, 1, MODE>;
};
template <int MODE>
struct PsFor<64, 4, MODE> {
  using type = Prescreen<32, 2, MODE>;  // fewer registers than <16, 4> (2 instead of 4 chunks/lane)
};
template <int MODE>
struct PsFor<64, 16, MODE> {
  using type = Prescreen<64, 4, MODE>;
};

// lanes per row / chunks per lane of a pre-screen type (0 for NoPrescreen)
template <class PS>
struct PsLayout {
  static constexpr int lpr = PS::LPR, nch = PS::NCH;
};

template <>
struct PsLayout<NoPrescreen> {
  static constexpr int lpr = 0, nch = 0;
};

// Drops the candidates of lds.ckeys[0,nsurv) whose lower bound reaches the criteria; the others
// are compacted in place (order kept).  Returns their number.  translation: optional map from
// candidate keys to base rows (upper graph layers).
template <class PS>
GGNN_DEV int prescreen_pass(const PS& ps, const WaveLds& lds, int nsurv, float s_thr,
                            const int32_t* translation)
{
  // one-chunk layouts keep the usual KBuild = 24 neighbours of a graph row in flight in one round
  constexpr int STEPS = (PS::NCH == 1 && PS::ROWS <= 8) ? 24 / PS::ROWS
                                                        : StepsOf<PS::LPR, PS::NCH>::value;
  constexpr int ROWS = PS::ROWS;
  const int lane = threadIdx.x;
  const int grp = lane / PS::LPR;
  int npass = 0;
  for (int s0 = 0; s0 < nsurv; s0 += ROWS * STEPS) {
    uint4 v[STEPS][PS::NCH];
    int kk[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      const int r = s0 + s * ROWS + grp;
      const bool valid = r < nsurv;
      // slots past the end read the code row of the first candidate (cached, verdict ignored)
      int m = lds.ckeys[valid ? r : s0];
      kk[s] = valid ? m : kEmptyKey;
      if (translation)
        m = translation[m];
      const uint8_t* row = ps.row_ptr(m);
#pragma unroll
      for (int c = 0; c < PS::NCH; ++c) {
        if (ps.all_chunks || ps.chunk_valid(c))
          v[s][c] = ps.load_chunk(row, c);
        else
          v[s][c] = make_uint4(0u, 0u, 0u, 0u);
      }
    }
    __syncthreads();  // all keys of this round are in registers before the in-place compaction
    GGNN_TICK(4);     // code rows arrived (issue + wait)
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      if (s0 + s * ROWS >= nsurv)
        break;
      const float S = group_sum<PS::LPR>(ps.partial(v[s]));
      const bool pass = (kk[s] != kEmptyKey) && (ps.g == 0) && !(S >= s_thr);
      const unsigned long long pm = __ballot(pass);
      if (pass)
        lds.ckeys[npass + __popcll(pm & ((1ull << lane) - 1ull))] = kk[s];
      npass += __popcll(pm);
    }
  }
  return npass;
}

// fetch(): simple_knn_cache.cuh:241-289.  cand: lane j (<32) holds candidate key j or EMPTY.
// Returns the number of distance evaluations (of the reference: pre-screened candidates count);
// rows.x / rows.y are advanced by the numbers of float / code rows actually read.
// after_filter(): hook called once the candidate keys have been consumed by the filter -- the
// place for a caller's own prefetch: a load issued BEFORE fetch() is waited for together with the
// candidates' graph row (the compiler merges the waits to vmcnt(0)), i.e. not overlapped at all.
struct NoHook {
  GGNN_DEV void operator()() const {}
};

// Allowed-id bitset of a filtered search (query_filtered.hip): id i is allowed iff bit
// (i + offset) & 31 of word (i + offset) >> 5 is set (offset: first global id of the shard).
// request(): every lane asks for the word of the candidate it holds -- one dword gather, issued
// in front of the candidates' first-read rows, so that it travels with them and the wait for the
// rows covers it (loads return in order).  The verdict is taken at the replay: denied(dl, k) says
// whether candidate k of the last request is denied, a compare and a ballot per pushed candidate.
struct NoIdFilter {
  static constexpr bool enabled = false;
};
struct IdFilter {
  static constexpr bool enabled = true;
  const uint32_t* bits;
  uint32_t offset;
  int key;        // the candidate this lane asked for (or EMPTY)
  uint32_t word;  // its word of the bitset
  GGNN_DEV void request(const int cand)
  {
    key = cand;
    // EMPTY slots read the word of the shard's first id (verdict ignored)
    word = bits[(static_cast<uint32_t>(max(cand, 0)) + offset) >> 5];
  }
  // lanes whose candidate is denied
  GGNN_DEV unsigned long long denied_lanes() const
  {
    const uint32_t b = static_cast<uint32_t>(key) + offset;
    return __ballot(key != kEmptyKey && !((word >> (b & 31u)) & 1u));
  }
  GGNN_DEV bool denied(const unsigned long long dl, const int k) const
  {
    return (__ballot(key == k) & dl) != 0ull;
  }
};

// Filter table (per-query filters): [num_filters x words] bitsets of the format above, one int32
// id per query.  The wave picks its bitset ONCE, before its loop; everything here is scalar (the
// query number is wave-uniform), so IdFilter sees one more wave-uniform pointer and nothing else.
//   ids == nullptr         the per-call form: one row, shared by every query
//   id in [0, num_filters) that row of the table
//   id == -1               unfiltered: the constant all-ones row consts[0, words)
//   anything else          empty result: the constant all-zero row consts[words, 2 * words)
// No id value leads outside table / consts.  (FilterTable: common.hpp)
GGNN_DEV const uint32_t* wave_filter_bits(const uint32_t* table, const FilterTable& t,
                                          const uint32_t n)
{
  if (!t.ids)
    return table;
  const int32_t f = __builtin_amdgcn_readfirstlane(t.ids[n]);
  if (static_cast<uint32_t>(f) < t.num_filters)
    return table + static_cast<size_t>(static_cast<uint32_t>(f)) * t.words;
  return t.consts + (f == -1 ? 0u : t.words);
}

// Label filters: one int32 label per base vector, one per query; a candidate is denied iff its
// label differs from the query's (FilterTable, common.hpp).  The class has the interface of IdFilter
// -- the same one-dword gather per lane in front of the first-read rows, the verdict at the replay
// -- and is a class of its own, instantiated in translation units of their own (query_labeled.hip,
// query_labeled_16.hip), because a filter read parametrised over both forms costs registers in the
// bitset kernels: those stay instruction for instruction what they were.
//   word   = labels[id + offset]
//   denied = (word & vmask) != want        label L: vmask ~0u, want L;  label -1: vmask 0, want 0
// The shard offset is folded into the wave-uniform pointer and the word is addressed as a 32-bit
// BYTE offset from it (scalar base + lane offset, the form of the bitset gather; a 64-bit index
// would cost an address register pair per lane): a shard holds at most 2^30 vectors under labels
// (kMaxLabeledShardRows, checked by the launchers).  Label -1 still reads its in-bounds word.
constexpr uint32_t kMaxLabeledShardRows = 1u << 30;
GGNN_DEV uint32_t filter_word_at(const void* words, const uint32_t byte_offset)
{
  return *reinterpret_cast<const uint32_t*>(static_cast<const char*>(words) + byte_offset);
}
struct LabelFilter {
  static constexpr bool enabled = true;
  const int32_t* labels;  // the column at the shard's first global id
  uint32_t vmask, want;
  int key;        // the candidate this lane asked for (or EMPTY)
  uint32_t word;  // its label
  // the filter of the wave of query n (scalar: the query number is wave-uniform)
  GGNN_DEV LabelFilter(const uint32_t* column, const uint32_t offset, const FilterTable& t,
                       const uint32_t n)
      : labels(reinterpret_cast<const int32_t*>(column) + offset), key(kEmptyKey), word(0u)
  {
    const int32_t L = __builtin_amdgcn_readfirstlane(t.query_labels[n]);
    vmask = (L == -1) ? 0u : ~0u;
    want = static_cast<uint32_t>(L) & vmask;
  }
  GGNN_DEV void request(const int cand)
  {
    key = cand;
    // EMPTY slots read the label of the shard's first id (verdict ignored)
    word = filter_word_at(labels, static_cast<uint32_t>(max(cand, 0)) << 2);
  }
  // lanes whose candidate is denied
  GGNN_DEV unsigned long long denied_lanes() const
  {
    return __ballot(key != kEmptyKey && (word & vmask) != want);
  }
  GGNN_DEV bool denied(const unsigned long long dl, const int k) const
  {
    return (__ballot(key == k) & dl) != 0ull;
  }
};

// Label-set filters: query n carries up to kMaxLabelSet labels and, optionally, a filter id into a
// filter table; a candidate is denied iff its label is in none of the set's entries (an entry -1
// admits every label), or its bit of the query's table row is clear (LabelSetSpec, common.hpp).  The
// interface is IdFilter's; request() issues TWO gathers per lane in front of the first-read rows --
// the label dword as in LabelFilter, then the bitset word as in IdFilter -- and the verdict is taken
// once per fetch at the replay:
//   denied = ((label & vmask) != want[j] for all eight j)  ||  bit (id + offset) of `bits` is clear
// The wave constructor pads a narrower set to eight entries by repeating its first one, so there is
// one compare chain whatever the width; want[], vmask, both pointers and the offsets are
// wave-uniform, read once before the loop.  ONE class for calls with and without a bitset: a wave
// that has none (no filter ids, or id -1) points `bits` at a constant all-ones word and ANDs the
// byte offset of its gather with 0 (imask), so it indexes nothing it was not given; an id outside
// the table points at the all-zero word next to it in the same way (an empty result).
constexpr uint32_t kMaxLabelSet = 8;  // GGNN_MAX_LABEL_SET
// {all ones, all zeros}: emitted only into the code objects whose kernels name it
template <class T = void>
__device__ const uint32_t kFilterConstWords[2] = {~0u, 0u};
struct LabelSetFilter {
  static constexpr bool enabled = true;
  const int32_t* labels;  // the column at the shard's first global id
  const uint32_t* bits;   // the query's row of the table, or one of the constant words
  uint32_t offset;        // first global id of the shard (bit offset)
  uint32_t imask;         // ~3u: `bits` is a row;  0: it is one word
  uint32_t vmask, want[kMaxLabelSet];
  int key;               // the candidate this lane asked for (or EMPTY)
  uint32_t word, bword;  // its label, its word of the bitset
  // the filter of the wave of query n (scalar: the query number is wave-uniform)
  GGNN_DEV LabelSetFilter(const uint32_t* table, const uint32_t shard_offset, const FilterTable& t,
                          const LabelSetSpec& s, const uint32_t n)
      : labels(s.labels + shard_offset), bits(kFilterConstWords<>), offset(shard_offset), imask(0u),
        key(kEmptyKey), word(0u), bword(0u)
  {
    const int32_t* set = s.sets + static_cast<size_t>(n) * s.width;
    bool wildcard = false;
#pragma unroll
    for (uint32_t j = 0; j < kMaxLabelSet; ++j) {
      const int32_t L = __builtin_amdgcn_readfirstlane(set[j < s.width ? j : 0u]);
      wildcard = wildcard || L == -1;
      want[j] = static_cast<uint32_t>(L);
    }
    vmask = wildcard ? 0u : ~0u;
#pragma unroll
    for (uint32_t j = 0; j < kMaxLabelSet; ++j)
      want[j] &= vmask;
    if (t.ids) {
      const int32_t f = __builtin_amdgcn_readfirstlane(t.ids[n]);
      if (static_cast<uint32_t>(f) < t.num_filters) {
        bits = table + static_cast<size_t>(static_cast<uint32_t>(f)) * t.words;
        imask = ~3u;
      }
      else if (f != -1)
        bits = kFilterConstWords<> + 1;
    }
  }
  GGNN_DEV void request(const int cand)
  {
    key = cand;
    // EMPTY slots read the label and the bitset word of the shard's first id (verdict ignored)
    const uint32_t c = static_cast<uint32_t>(max(cand, 0));
    word = filter_word_at(labels, c << 2);
    bword = filter_word_at(bits, ((c + offset) >> 3) & imask);
  }
  // lanes whose candidate is denied
  GGNN_DEV unsigned long long denied_lanes() const
  {
    const uint32_t w = word & vmask;
    bool none = true;
#pragma unroll
    for (uint32_t j = 0; j < kMaxLabelSet; ++j)
      none = none && w != want[j];
    const uint32_t b = static_cast<uint32_t>(key) + offset;
    return __ballot(key != kEmptyKey && (none || !((bword >> (b & 31u)) & 1u)));
  }
  GGNN_DEV bool denied(const unsigned long long dl, const int k) const
  {
    return (__ballot(key == k) & dl) != 0ull;
  }
};

// Label-range filters: query n carries up to kMaxLabelRanges closed intervals (lo, hi) of signed
// int32 labels and, optionally, a filter id into a filter table; a candidate is denied iff its label
// lies in none of the intervals, or its bit of the query's table row is clear (LabelRangeSpec,
// common.hpp).  There is no wildcard value: -1 is a label like any other.  request() is
// LabelSetFilter's -- the label dword, then the bitset word, in front of the first-read rows -- and
// the verdict is taken once per fetch at the replay:
//   denied = (uint32(label - lo[j]) > span[j] for all four j)  ||  bit (id + offset) of `bits` is clear
// with span = uint32(hi - lo): one subtract and one unsigned compare per interval, exact for every
// signed lo <= hi, (INT32_MIN, INT32_MAX) included (span ~0u).  The form is WRONG for an empty
// interval (lo > hi: (1, 0) has span ~0u and would admit everything), so the wave constructor, which
// is scalar and runs before the loop, normalises: an empty interval becomes a copy of the query's
// first non-empty one, a list shorter than four is padded in the same way, and a query whose
// intervals are all empty points `bits` at the constant all-zero word with imask 0, as an
// out-of-table id does.  lo[], span[], both pointers and the offsets are wave-uniform: the same
// eight scalar registers as LabelSetFilter's want[8].
constexpr uint32_t kMaxLabelRanges = 4;  // GGNN_MAX_LABEL_RANGES
struct LabelRangeFilter {
  static constexpr bool enabled = true;
  const int32_t* labels;  // the column at the shard's first global id
  const uint32_t* bits;   // the query's row of the table, or one of the constant words
  uint32_t offset;        // first global id of the shard (bit offset)
  uint32_t imask;         // ~3u: `bits` is a row;  0: it is one word
  uint32_t lo[kMaxLabelRanges], span[kMaxLabelRanges];
  int key;               // the candidate this lane asked for (or EMPTY)
  uint32_t word, bword;  // its label, its word of the bitset
  // the filter of the wave of query n (scalar: the query number is wave-uniform)
  GGNN_DEV LabelRangeFilter(const uint32_t* table, const uint32_t shard_offset, const FilterTable& t,
                            const LabelRangeSpec& s, const uint32_t n)
      : labels(s.labels + shard_offset), bits(kFilterConstWords<>), offset(shard_offset), imask(0u),
        key(kEmptyKey), word(0u), bword(0u)
  {
    const int32_t* r = s.ranges + static_cast<size_t>(n) * s.n_ranges * 2;
    bool valid[kMaxLabelRanges];
    bool any = false;
    uint32_t lo0 = 0u, span0 = 0u;  // the first non-empty interval
#pragma unroll
    for (uint32_t j = 0; j < kMaxLabelRanges; ++j) {
      const uint32_t jj = j < s.n_ranges ? j : 0u;
      const int32_t l = __builtin_amdgcn_readfirstlane(r[2 * jj]);
      const int32_t h = __builtin_amdgcn_readfirstlane(r[2 * jj + 1]);
      valid[j] = l <= h;
      lo[j] = static_cast<uint32_t>(l);
      span[j] = static_cast<uint32_t>(h) - static_cast<uint32_t>(l);
      if (valid[j] && !any) {
        lo0 = lo[j];
        span0 = span[j];
        any = true;
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < kMaxLabelRanges; ++j) {
      lo[j] = valid[j] ? lo[j] : lo0;
      span[j] = valid[j] ? span[j] : span0;
    }
    if (t.ids) {
      const int32_t f = __builtin_amdgcn_readfirstlane(t.ids[n]);
      if (static_cast<uint32_t>(f) < t.num_filters) {
        bits = table + static_cast<size_t>(static_cast<uint32_t>(f)) * t.words;
        imask = ~3u;
      }
      else if (f != -1)
        bits = kFilterConstWords<> + 1;
    }
    if (!any) {
      // every interval is empty: the all-zero word, whatever the id said
      bits = kFilterConstWords<> + 1;
      imask = 0u;
    }
  }
  GGNN_DEV void request(const int cand)
  {
    key = cand;
    // EMPTY slots read the label and the bitset word of the shard's first id (verdict ignored)
    const uint32_t c = static_cast<uint32_t>(max(cand, 0));
    word = filter_word_at(labels, c << 2);
    bword = filter_word_at(bits, ((c + offset) >> 3) & imask);
  }
  // lanes whose candidate is denied
  GGNN_DEV unsigned long long denied_lanes() const
  {
    bool none = true;
#pragma unroll
    for (uint32_t j = 0; j < kMaxLabelRanges; ++j)
      none = none && (word - lo[j]) > span[j];
    const uint32_t b = static_cast<uint32_t>(key) + offset;
    return __ballot(key != kEmptyKey && (none || !((bword >> (b & 31u)) & 1u)));
  }
  GGNN_DEV bool denied(const unsigned long long dl, const int k) const
  {
    return (__ballot(key == k) & dl) != 0ull;
  }
};

// Label-mask filters: the label of a base row read as 32 tag bits.  Query n carries up to
// kMaxLabelMasks clauses (mask, value, any) and, optionally, a filter id into a filter table; a
// candidate is denied iff it passes none of the clauses, or its bit of the query's table row is
// clear (LabelMaskSpec, common.hpp).  A row passes a clause iff
//   (label & mask) == value  &&  (any == 0 || (label & any) != 0)
// `value` is compared as it was given, never pre-masked: a value with a bit outside its mask admits
// nothing, by definition.  There is no wildcard value, no invalid clause and nothing to normalise:
// (0, 0, 0) admits every row and bit 31 is a bit like any other.  request() is LabelRangeFilter's --
// the label dword, then the bitset word, in front of the first-read rows -- and the verdict is taken
// once per fetch at the replay, without a branch (| and & on the lane masks, not || and &&).  The
// wave constructor, scalar and in front of the loop, pads a one-clause query by repeating that
// clause.  mask[], value[] and any[] are wave-uniform: six scalar registers where LabelRangeFilter
// has the eight of lo[4] and span[4].  `any == 0` is a scalar compare at the verdict, not a stored
// word free = (any == 0) for ((label & any) | free) != 0: with every scalar register of these kernels
// taken, the compiler keeps two such words in VECTOR registers for the whole loop, and the headline
// kernels then need 77 / 79 registers where they need 75 / 77 like their label-range siblings
// without (read from the code object).
constexpr uint32_t kMaxLabelMasks = 2;  // GGNN_MAX_LABEL_MASKS
struct LabelMaskFilter {
  static constexpr bool enabled = true;
  const int32_t* labels;  // the column at the shard's first global id
  const uint32_t* bits;   // the query's row of the table, or one of the constant words
  uint32_t offset;        // first global id of the shard (bit offset)
  uint32_t imask;         // ~3u: `bits` is a row;  0: it is one word
  uint32_t mask[kMaxLabelMasks], value[kMaxLabelMasks], any[kMaxLabelMasks];
  int key;               // the candidate this lane asked for (or EMPTY)
  uint32_t word, bword;  // its label, its word of the bitset
  // the filter of the wave of query n (scalar: the query number is wave-uniform)
  GGNN_DEV LabelMaskFilter(const uint32_t* table, const uint32_t shard_offset, const FilterTable& t,
                           const LabelMaskSpec& s, const uint32_t n)
      : labels(s.labels + shard_offset), bits(kFilterConstWords<>), offset(shard_offset), imask(0u),
        key(kEmptyKey), word(0u), bword(0u)
  {
    const int32_t* c = s.masks + static_cast<size_t>(n) * s.n_masks * 3;
#pragma unroll
    for (uint32_t j = 0; j < kMaxLabelMasks; ++j) {
      const uint32_t jj = j < s.n_masks ? j : 0u;
      mask[j] = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(c[3 * jj]));
      value[j] = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(c[3 * jj + 1]));
      any[j] = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(c[3 * jj + 2]));
    }
    if (t.ids) {
      const int32_t f = __builtin_amdgcn_readfirstlane(t.ids[n]);
      if (static_cast<uint32_t>(f) < t.num_filters) {
        bits = table + static_cast<size_t>(static_cast<uint32_t>(f)) * t.words;
        imask = ~3u;
      }
      else if (f != -1)
        bits = kFilterConstWords<> + 1;
    }
  }
  GGNN_DEV void request(const int cand)
  {
    key = cand;
    // EMPTY slots read the label and the bitset word of the shard's first id (verdict ignored)
    const uint32_t c = static_cast<uint32_t>(max(cand, 0));
    word = filter_word_at(labels, c << 2);
    bword = filter_word_at(bits, ((c + offset) >> 3) & imask);
  }
  // does a row with label w pass one of the clauses
  GGNN_DEV bool passes(const uint32_t w) const
  {
    bool one = false;
#pragma unroll
    for (uint32_t j = 0; j < kMaxLabelMasks; ++j)
      one = one | (((w & mask[j]) == value[j]) & (((w & any[j]) != 0u) | (any[j] == 0u)));
    return one;
  }
  // lanes whose candidate is denied
  GGNN_DEV unsigned long long denied_lanes() const
  {
    const uint32_t b = static_cast<uint32_t>(key) + offset;
    return __ballot(key != kEmptyKey && (!passes(word) || !((bword >> (b & 31u)) & 1u)));
  }
  GGNN_DEV bool denied(const unsigned long long dl, const int k) const
  {
    return (__ballot(key == k) & dl) != 0ull;
  }
};

// One candidate of a replay (simple_knn_cache.cuh:283-285): pushed if it still beats the criteria,
// which the pushes before it may have tightened.  One-register lists take the test, and the
// duplicate test of push(), into the masks of push_if(): the loop around this is then ONE basic block
// per candidate.  Longer lists (and the list in LDS) keep the wave-uniform branch in front of push().
// (The criteria test as a scalar early-out in front of the one-block body, so that a candidate that
// fails the tightened criteria skips the body, was built and measured against this form: a tie --
// ten alternating headline runs each, 0.810-0.826 ms both, DESIGN.md 4.7 -- so the form without the
// branch stays.)
template <class SL>
GGNN_DEV void replay_push(SL& sl, const int k, const float d, const bool denied = false)
{
  if constexpr (SL::kReplayOneBlock)
    sl.push_if(k, d, d < sl.criteria(), denied);
  else if (d < sl.criteria())
    sl.push(k, d, denied);
}

// the replay of a fetch (simple_knn_cache.cuh:268-286) under a filter: as replay_lanes() below,
// a denied candidate is pushed with the flag
template <class SL, class IDF>
GGNN_DEV void replay_lanes_filtered(SL& sl, unsigned long long m, const int k_of, const float d_of,
                                    const IDF& filt)
{
  const unsigned long long dl = filt.denied_lanes();
  while (m) {
    const int j = __ffsll(static_cast<long long>(m)) - 1;
    m &= m - 1;
    const float d = rdlanef(d_of, j);
    const int k = rdlane(k_of, j);
    if constexpr (SL::kReplayOneBlock)
      replay_push(sl, k, d, filt.denied(dl, k));  // (no skip of the compare for dl == 0: a branch)
    else if (d < sl.criteria())
      sl.push(k, d, dl != 0ull && filt.denied(dl, k));
  }
}

template <int MODE, bool FILTER, class SL, class DE, class PS, class HOOK = NoHook,
          class FILT = NoIdFilter>
GGNN_DEV int fetch(SL& sl, const DE& de, const WaveLds& lds, int cand,
                   const int32_t* translation, const PS& ps, uint2& rows,
                   HOOK&& after_filter = NoHook{}, FILT&& filt = FILT{})
{
  constexpr bool kFiltered = std::remove_reference_t<FILT>::enabled;
  const int lane = threadIdx.x;
  cand = lower_half_to_both(cand);
  if constexpr (kFiltered)
    filt.request(cand);
  GGNN_TICK(1);  // graph row arrived
  if (FILTER)
    cand = sl.filter(cand, lds.known);
  const unsigned long long surv = __ballot(lane < 32 && cand != kEmptyKey);
  const int nsurv = __popcll(surv);
  GGNN_TICK(2);  // filter
  after_filter();
  if (nsurv == 0)
    return 0;
  __syncthreads();
  if (lane < 32 && cand != kEmptyKey)
    lds.ckeys[__popcll(surv & ((1ull << lane) - 1ull))] = cand;
  __syncthreads();
  int neval = nsurv;
  GGNN_TICK(3);  // compaction
  if constexpr (PS::enabled) {
    const float s_thr = ps.threshold(sl.criteria());
    if (s_thr < inf_f()) {
      neval = prescreen_pass(ps, lds, nsurv, s_thr, translation);
      rows.y += nsurv;
      GGNN_TICK(5);  // pre-screen verdicts + compaction
      if (neval == 0)
        return nsurv;
      __syncthreads();
    }
  }
  // after the pre-screen only a handful of candidates are left: fewer rows in flight, fewer VGPRs
  // (three chunks per lane, 8 rows per load instruction: one step already has 8 rows in flight)
  constexpr int kSteps = StepsOf<DE::LPR, DE::NCH>::value;
  constexpr int kExactSteps = !PS::enabled ? kSteps : (DE::NCH == 3 && DE::ROWS >= 8) ? 1
                              : (kSteps > 2)                                         ? 2
                                                                                     : kSteps;
  compute_distances<MODE, DE, kExactSteps>(de, lds, neval, translation);
  rows.x += neval;
  __syncthreads();
  GGNN_TICK(7);  // exact distances
  const float cd = lane < neval ? lds.cd0[lane] : inf_f();
  const int ck = lane < neval ? lds.ckeys[lane] : kEmptyKey;
  // criteria() never increases during a fetch, so candidates failing it now fail it later
  unsigned long long m = __ballot(cd < sl.criteria());
  if constexpr (kFiltered) {
    replay_lanes_filtered(sl, m, ck, cd, filt);
    return nsurv;
  }
  while (m) {
    const int j = __ffsll(static_cast<long long>(m)) - 1;
    m &= m - 1;
    const float d = rdlanef(cd, j);
    const int k = rdlane(ck, j);
    replay_push(sl, k, d);
  }
  GGNN_TICK(8);  // accept / push replay
  return nsurv;
}
template <int MODE, bool FILTER, class SL, class DE>
GGNN_DEV int fetch(SL& sl, const DE& de, const WaveLds& lds, int cand,
                   const int32_t* translation)
{
  uint2 rows = make_uint2(0u, 0u);
  return fetch<MODE, FILTER>(sl, de, lds, cand, translation, NoPrescreen{}, rows);
}

// ---------------------------------------------------------------------------------------------
// Early rows (round 5).  A pop of fetch() above is a chain of DEPENDENT steps: pop bookkeeping ->
// graph row -> membership test -> compaction -> code rows (or the rows themselves) -> verdicts ->
// float rows -> replay, i.e. every memory round trip starts only after the instruction chain in
// front of it has run.  For graph rows of at most 24 neighbours (KBuild <= 24, every BASELINE
// configuration) whose FIRST row read is 128 bytes wide -- 8 lanes x 16 bytes: the pre-screen codes
// of a float base (Prescreen<8,1>) or the rows of a base with <= 128-byte rows (uint8 D <= 128,
// DistEngine<.,8,1> without pre-screen) -- the order becomes
//     decide the pop (peek) -> graph row (speculated: usually there) -> REQUEST the first-read
//     rows of all <= 24 neighbours -> pop bookkeeping + membership test (under that latency) ->
//     verdicts with the membership verdict applied as a mask -> [float rows -> distances] -> replay.
// Candidate s*8 + grp goes to the eight lanes of group grp in step s (ds_bpermute), so there is no
// compaction in front of the loads; known candidates are read too (21.4 of 24 survive the test
// anyway) and are masked out afterwards.  Decisions, counters and results are those of fetch():
// the set of evaluated candidates, their order and the criteria they meet are unchanged (the row
// counters keep counting what the algorithm needs, not the extra rows of known candidates).
// ---------------------------------------------------------------------------------------------
constexpr int kEarlySteps = 3;  // 24 candidates
// Candidate c = 3 * grp + s goes to the eight lanes of row group grp in step s, and its verdict is
// taken in lane 8 * grp + s: ascending lanes are ascending candidates, so ONE ballot over the three
// steps lists the candidates that pass in the order the replay needs (simple_knn_cache.cuh:268-286
// evaluates them one after the other).
template <class RD>  // RD: the reader of the first rows (Prescreen<8,1,.> or DistEngine<.,8,1>)
struct EarlyRows {
  static_assert(RD::LPR == 8 && RD::NCH == 1, "early rows: 8 lanes x one 16-byte chunk per row");
  int kk[kEarlySteps];                       // candidate key of this lane's row group, per step
  typename RD::Chunk v[kEarlySteps][1];
  // cand: lane j (< 24) holds candidate j or EMPTY; translation: optional map from candidate keys
  // to base rows (upper graph layers of the merge kernel)
  GGNN_DEV void issue(const RD& rd, const int cand, const int32_t* translation = nullptr)
  {
    const int grp = threadIdx.x >> 3;
    // the three crossbar reads first (one wait for all of them, not one round trip per step)
#pragma unroll
    for (int s = 0; s < kEarlySteps; ++s)
      kk[s] = __builtin_amdgcn_ds_bpermute((grp * kEarlySteps + s) << 2, cand);
    int m[kEarlySteps];
#pragma unroll
    for (int s = 0; s < kEarlySteps; ++s) {
      // EMPTY slots read row 0 (verdict ignored): no branch and no zero-fill around the loads
      m[s] = max(kk[s], 0);
      if (translation)
        m[s] = translation[m[s]];
    }
    // ONE wave-uniform branch for "every lane's chunk lies inside the row" (the common shapes)
    // instead of an exec-mask region and a zero-fill around each of the three loads
    if (rd.all_chunks) {
#pragma unroll
      for (int s = 0; s < kEarlySteps; ++s)
        v[s][0] = rd.load_chunk(rd.row_ptr(m[s]), 0);
    }
    else {
#pragma unroll
      for (int s = 0; s < kEarlySteps; ++s) {
        if (rd.chunk_valid(0))
          v[s][0] = rd.load_chunk(rd.row_ptr(m[s]), 0);
        else
          v[s][0] = typename RD::Chunk{};
      }
      // (keeps the two paths apart: the optimiser otherwise sinks the third load of both into one
      // exec-mask region behind the branch, and the path above pays that region and its zero-fill)
      asm volatile("");
    }
  }
  // the value of step (lane & 7) in lanes whose (lane & 7) < 3 (their candidate's lane).  The three
  // values are taken BY VALUE: with a reference to the array the conditional operator reads the
  // element inside each branch, the optimiser sinks the three reads into one read of a selected
  // address, and the array (kk[] of every pop) goes to scratch memory -- three scratch stores and
  // a scratch load (vmcnt(0)) per pop, measured as +19 % memory traffic and +17 % kernel time.
  template <typename T>
  static GGNN_DEV T of_my_step(const T x0, const T x1, const T x2)
  {
    const int w = threadIdx.x & 7;
    T r = x2;
    r = (w == 1) ? x1 : r;
    r = (w == 0) ? x0 : r;
    return r;
  }
};

// Pushes, in ascending lane order, the candidates of `m` (lane j: key k_of, distance d_of) that
// still beat the criteria -- the replay of simple_knn_cache.cuh:268-286 (criteria() never increases
// during a fetch, so a candidate that fails it once fails it later too)
template <class SL>
GGNN_DEV void replay_lanes(SL& sl, unsigned long long m, const int k_of, const float d_of)
{
  while (m) {
    const int j = __ffsll(static_cast<long long>(m)) - 1;
    m &= m - 1;
    const float d = rdlanef(d_of, j);
    const int k = rdlane(k_of, j);
    replay_push(sl, k, d);
  }
}

// second half of a pop in the early-rows order: membership test, verdicts, exact phase, replay.
// cand: lane j (< 24) holds candidate j or EMPTY (the value issue() was given).
// COUNT = false (launches that do not collect work counters: every production call): the scan of
// the sorted part moves behind the verdicts (SortedList::drop_sorted) -- same candidates on the
// float rows, same pushes, same results; the return value and `rows` then count the survivors of
// the VISITED test only and are not used.
// filt (filtered search): the caller has requested the bit words of `cand` (IdFilter::request)
// in front of er.issue()
// EXACT (the kernels of PrescreenExact, squared L2; "Distances from lossless codes"): a wave whose
// certificate holds (ps.s2 != 0) takes the distances from the code sums, as the branch for rows read
// directly does.
template <int MODE, bool COUNT = true, bool EXACT = false, class SL, class DE, class PS, class ER,
          class HOOK, class FILT = NoIdFilter>
GGNN_DEV int fetch_early(SL& sl, const DE& de, const WaveLds& lds, int cand, const ER& er,
                         const PS& ps, uint2& rows, HOOK&& after_filter,
                         const int32_t* translation = nullptr, FILT&& filt = FILT{})
{
  constexpr bool kFiltered = std::remove_reference_t<FILT>::enabled;
  const int lane = threadIdx.x;
  const int grp = lane >> 3, w = lane & 7;
  cand = sl.template filter<false, COUNT>(lower_half_to_both(cand), lds.known);
  const unsigned surv = static_cast<unsigned>(__ballot(lane < 32 && cand != kEmptyKey));
  const int nsurv = __popc(surv);
  after_filter();
  // this lane's candidate (w < 3) survived the membership test
  const bool alive = w < kEarlySteps && ((surv >> (grp * kEarlySteps + w)) & 1u);
  // rows.x / rows.y count the rows the ALGORITHM needs, as fetch() does (code rows of the
  // survivors of the membership test while the pre-screen is active, float rows of those that pass
  // it): the roofline's algorithmic bytes do not grow because this order also requests the rows of
  // the ~11 % known candidates (measured fabric traffic shows those)
  if constexpr (PS::enabled) {
    if (nsurv == 0)
      return 0;
    // lossless codes (EXACT kernels): the code sum IS the distance, times s^2 -- no threshold, no
    // compaction, no float rows; the lane of the verdict keeps key and distance for the replay, as
    // in the branch for rows read directly below.  Wave-uniform; constant false without EXACT.
    constexpr bool kExact = EXACT && MODE == kL2;
    if constexpr (kExact) {
      static_assert(PS::LPR == 8 && PS::NCH == 1, "lossless codes: sums of at most 128 dimensions");
      static_assert(PS::LPR * PS::NCH * 16 * 255 * 255 < (1 << 24), "s^2 * S must be exact");
    }
    bool exact = false;
    if constexpr (kExact)
      exact = ps.s2 != 0.f;
    // +inf (list not full yet, pre-screen unusable): nothing is dropped, every survivor is evaluated
    const float crit = sl.criteria();
    const float s_thr = exact ? crit : ps.threshold(crit);  // (exact: only "is it finite" is used)
    if (s_thr < inf_f())
      rows.y += nsurv;
    float S[kEarlySteps];
#pragma unroll
    for (int s = 0; s < kEarlySteps; ++s)
      S[s] = group_sum<8>(ps.partial(er.v[s]));  // (every lane of the group holds the sum)
    const float smine = ER::of_my_step(S[0], S[1], S[2]);
    // this lane's candidate key.  The two-phase kernels select it here, for both phases (selected
    // inside each branch it costs them 2-4 registers: scratch); the others after the ballot, where
    // it always was -- their code is instruction for instruction what it was.
    int mykey = kEmptyKey;
    if constexpr (kExact)
      mykey = ER::of_my_step(er.kk[0], er.kk[1], er.kk[2]);
    float d_of;
    int k_of;
    unsigned long long m;
    if (exact) {
      d_of = ps.s2 * smine;
      k_of = mykey;
      m = __ballot(alive && d_of < crit);
      if constexpr (!COUNT)
        m = sl.drop_sorted(m, mykey);
    }
    else {
      bool pass = alive && !(smine >= s_thr);
      unsigned long long pm = __ballot(pass);   // ascending lanes = ascending candidates
      if constexpr (!kExact)
        mykey = ER::of_my_step(er.kk[0], er.kk[1], er.kk[2]);
      if constexpr (!COUNT) {
        pm = sl.drop_sorted(pm, mykey);
        pass = (pm >> lane) & 1ull;
      }
      const int neval = __popcll(pm);
      if (neval == 0)
        return nsurv;
      rows.x += neval;
      constexpr int kSteps = StepsOf<DE::LPR, DE::NCH>::value;
      constexpr int kExactSteps = (DE::NCH == 3 && DE::ROWS >= 8) ? 1 : (kSteps > 2) ? 2 : kSteps;
      // keys of the candidates that pass -> LDS in candidate order (one write: the ballot is already
      // in that order), float rows, distances -> LDS, replay.  (Routing the ~3 keys through scalar
      // registers to the row groups and keeping the distances in their lanes -- no LDS between the
      // verdicts and the replay -- was measured: identical results, 10k-query batch unchanged, 100k
      // batch and build -2 %; not worth a second code path.  DESIGN.md Appendix B.)
      // (EXACT kernels count the lanes below with v_mbcnt: the lane mask of the other form is loop
      // invariant, two registers the kernel holding both phases does not have -- it went to scratch)
      int slot;
      if constexpr (kExact)
        slot = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(pm >> 32),
                                         __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(pm), 0u));
      else
        slot = __popcll(pm & ((1ull << lane) - 1ull));
      if (pass)
        lds.ckeys[slot] = mykey;
      __syncthreads();
      compute_distances<MODE, DE, kExactSteps>(de, lds, neval, translation);
      __syncthreads();
      d_of = lane < neval ? lds.cd0[lane] : inf_f();
      k_of = lane < neval ? lds.ckeys[lane] : kEmptyKey;
      m = __ballot(d_of < sl.criteria());
    }
    if constexpr (kFiltered)
      replay_lanes_filtered(sl, m, k_of, d_of, filt);
    else
      replay_lanes(sl, m, k_of, d_of);
    return nsurv;
  }
  else {
    // the requested rows ARE the base rows: distances stay in the lanes that summed them (every
    // lane of a group holds the sum), the replay reads lane 8 * grp + s for candidate 3 * grp + s
    rows.x += nsurv;
    if (nsurv == 0)
      return 0;
    float dd[kEarlySteps];
#pragma unroll
    for (int s = 0; s < kEarlySteps; ++s) {
      float a, b;
      de.template partial<MODE>(er.v[s], a, b);
      a = group_sum<8>(a);
      if (MODE == kCos)
        b = group_sum<8>(b);
      dd[s] = (MODE == kCos) ? de.finish_cos(a, b) : a;
    }
    const float dmine = ER::of_my_step(dd[0], dd[1], dd[2]);
    const int mykey = ER::of_my_step(er.kk[0], er.kk[1], er.kk[2]);
    unsigned long long m = __ballot(alive && dmine < sl.criteria());
    if constexpr (!COUNT)
      m = sl.drop_sorted(m, mykey);
    if constexpr (kFiltered)
      replay_lanes_filtered(sl, m, mykey, dmine, filt);
    else
      replay_lanes(sl, m, mykey, dmine);
    return nsurv;
  }
}

// hook VIS_SLOTS = <1..8>: test hook that shrinks the buckets of the hashed visited set so that the
// stash, its overflow into the ring scan and the removal paths are exercised by ordinary searches
inline uint32_t vis_slots_hook()
{
  const int64_t v = hook(kHookVisSlots);
  return (v >= 1 && v <= kVisSlots) ? static_cast<uint32_t>(v) : static_cast<uint32_t>(kVisSlots);
}

// block-size / chunk configuration by dimension and element type (host side)
struct DistConfig {
  int lpr, nch;
};
inline DistConfig pick_dist_config(uint32_t D, ggnn_dtype dtype)
{
  const uint32_t epc = dtype_elems_per_chunk(dtype);
  const uint32_t chunks = (D + epc - 1) / epc;
  if (chunks <= 8)
    return {8, 1};
  if (chunks <= 16)
    return {8, 2};
  // 17..24 chunks (D = 96 float32, the DEEP shape): 8 lanes x 3 chunks cover the row exactly; the
  // {16, 2} layout would leave 8 of its 32 chunk slots -- a quarter of every load instruction --
  // on dead lanes
  if (chunks <= 24)
    return {8, 3};
  if (chunks <= 32)
    return {16, 2};
  if (chunks <= 64)
    return {16, 4};
  if (chunks <= 256)
    return {64, 4};
  return {64, 16};
}

// dispatch a functor templated on <BaseT, LPR, NCH> over the seven layouts of one element type
#define GGNN_DISPATCH_LAYOUT(T, _dc, F)                                            \
  do {                                                                            \
    if ((_dc).lpr == 8 && (_dc).nch == 1) { F(T, 8, 1); }                         \
    else if ((_dc).lpr == 8 && (_dc).nch == 2) { F(T, 8, 2); }                    \
    else if ((_dc).lpr == 8 && (_dc).nch == 3) { F(T, 8, 3); }                    \
    else if ((_dc).lpr == 16 && (_dc).nch == 2) { F(T, 16, 2); }                  \
    else if ((_dc).lpr == 16 && (_dc).nch == 4) { F(T, 16, 4); }                  \
    else if ((_dc).lpr == 64 && (_dc).nch == 4) { F(T, 64, 4); }                  \
    else { F(T, 64, 16); }                                                        \
  } while (0)

// int8 rows: the six layouts that rows of at most 4096 bytes reach ({64, 16} starts at 4097 bytes,
// so no kernel of it is instantiated for the type)
#define GGNN_DISPATCH_LAYOUT_I8(_dc, F)                                            \
  do {                                                                            \
    if ((_dc).lpr == 8 && (_dc).nch == 1) { F(int8_t, 8, 1); }                    \
    else if ((_dc).lpr == 8 && (_dc).nch == 2) { F(int8_t, 8, 2); }               \
    else if ((_dc).lpr == 8 && (_dc).nch == 3) { F(int8_t, 8, 3); }               \
    else if ((_dc).lpr == 16 && (_dc).nch == 2) { F(int8_t, 16, 2); }             \
    else if ((_dc).lpr == 16 && (_dc).nch == 4) { F(int8_t, 16, 4); }             \
    else if ((_dc).lpr == 64 && (_dc).nch == 4) { F(int8_t, 64, 4); }             \
    else                                                                          \
      throw ::ggnn_amd::Error(GGNN_INVALID_ARGUMENT, "D must be in [1, 4096]");   \
  } while (0)

// dispatch a functor templated on <BaseT, LPR, NCH>
#define GGNN_DISPATCH_DIST(dtype, D, F)                                           \
  do {                                                                            \
    const ::ggnn_amd::DistConfig _dc = ::ggnn_amd::pick_dist_config((D), (dtype)); \
    if ((dtype) == GGNN_F32)                                                      \
      GGNN_DISPATCH_LAYOUT(float, _dc, F);                                        \
    else if ((dtype) == GGNN_F16)                                                 \
      GGNN_DISPATCH_LAYOUT(::ggnn_amd::f16_t, _dc, F);                            \
    else if ((dtype) == GGNN_BF16)                                                \
      GGNN_DISPATCH_LAYOUT(::ggnn_amd::bf16_t, _dc, F);                           \
    else if ((dtype) == GGNN_I8)                                                  \
      GGNN_DISPATCH_LAYOUT_I8(_dc, F);                                            \
    else                                                                          \
      GGNN_DISPATCH_LAYOUT(uint8_t, _dc, F);                                      \
  } while (0)

// the same for float32 and uint8 rows only: query / merge / sym compile their 16-bit kernels in
// translation units of their own (query_16.hip, merge_16.hip, sym_16.hip), built in parallel
#define GGNN_DISPATCH_DIST_32_8(dtype, D, F)                                      \
  do {                                                                            \
    const ::ggnn_amd::DistConfig _dc = ::ggnn_amd::pick_dist_config((D), (dtype)); \
    if ((dtype) == GGNN_F32)                                                      \
      GGNN_DISPATCH_LAYOUT(float, _dc, F);                                        \
    else                                                                          \
      GGNN_DISPATCH_LAYOUT(uint8_t, _dc, F);                                      \
  } while (0)
#define GGNN_DISPATCH_DIST_16(dtype, D, F)                                        \
  do {                                                                            \
    const ::ggnn_amd::DistConfig _dc = ::ggnn_amd::pick_dist_config((D), (dtype)); \
    if ((dtype) == GGNN_F16)                                                      \
      GGNN_DISPATCH_LAYOUT(::ggnn_amd::f16_t, _dc, F);                            \
    else                                                                          \
      GGNN_DISPATCH_LAYOUT(::ggnn_amd::bf16_t, _dc, F);                           \
  } while (0)
// int8 rows: units of their own as well (query_i8.hip, merge_i8.hip, sym_i8.hip, ...)
#define GGNN_DISPATCH_DIST_I8(dtype, D, F)                                        \
  do {                                                                            \
    const ::ggnn_amd::DistConfig _dc = ::ggnn_amd::pick_dist_config((D), (dtype)); \
    GGNN_DISPATCH_LAYOUT_I8(_dc, F);                                              \
  } while (0)
// a unit that holds the kernels of further element types only (GGNN_ROWS_16_TU, GGNN_ROWS_I8_TU):
// the host code of the float32 / uint8 unit is left out of it
#if defined(GGNN_ROWS_16_TU) || defined(GGNN_ROWS_I8_TU)
#define GGNN_ROWS_EXTRA_TU
#endif

inline void check_vector_layout(const void* base, uint32_t D, ggnn_dtype dtype)
{
  const uint32_t epc = dtype_elems_per_chunk(dtype);
  GGNN_REQUIRE(D >= 1 && D <= 4096, GGNN_INVALID_ARGUMENT, "D must be in [1, 4096]");
  GGNN_REQUIRE(D % epc == 0, GGNN_UNSUPPORTED,
               "this build needs D to be a multiple of 16 bytes per row "
               "(4 for float32, 8 for float16 / bfloat16, 16 for uint8 / int8)");
  GGNN_REQUIRE((reinterpret_cast<uintptr_t>(base) & 15u) == 0, GGNN_INVALID_ARGUMENT,
               "base/query pointers must be 16-byte aligned");
}

}  // namespace ggnn_amd
