// Label spans: label sets and label ranges answered exactly through a label index (label_index.hip;
// DESIGN.md 4.9, "Label index").
//
// rows[] of the index is sorted by (label, id), so the rows of ONE label are one contiguous run of
// positions, and so are the rows of a closed label interval [lo, hi].  A set of up to eight labels or up
// to four intervals is therefore at most eight spans [begin, end) of positions:
//
//   label_spans_resolve_kernel   one thread per query: sets / ranges -> spans[Nq][8][2], totals[Nq], in
//                                normal form (sorted, disjoint, not touching, non-empty, (0, 0) tail):
//                                a duplicate set entry or two overlapping intervals must not make a row
//                                reachable twice
//   label_spans_scan_kernel      label_index_scan_kernel walking the VIRTUAL positions [0, total) of a
//   label_spans_scan_lds_kernel  query's spans laid end to end: one wave per (query, slice), the 16 span
//                                words wave-uniform, a lane maps its virtual position to a position in
//                                rows[] with seven compare/selects, and a batch may straddle spans
//   label_spans_merge_kernel     one wave per query re-inserts the slices' partial lists
//   label_spans_merge_lds_kernel
//   label_spans_flags_kernel     classify by totals; label_index_compact_kernel makes the lists
//
// Tie order.  The scan of the whole base (bf_query_labelset.hip, bf_query_labelrange.hip) visits rows in
// ascending id and inserts stably: among equal distances the lower id wins.  Positions ascend with the
// id inside ONE label only; across the labels of a set or a range they do not.  The K-best list here is
// therefore ordered by the pair (distance, id): a candidate goes in front of the first entry e with
// d < e.dist, or d == e.dist and id < e.key (e not empty).  The K smallest pairs under that order are
// exactly what the ascending-id stable scan keeps, whatever the visiting order, and a row's distance
// does not depend on the visiting order either -- so the result equals the scan's bit for bit.  Slices
// are not in id order for the same reason: launch_merge_results_subset ("lower part first on ties")
// would be wrong, the merge kernels insert by (distance, id) again.
//
// Filter table (optional): the bit of a row is fetched one batch ahead like its id, and a denied row
// becomes "no row" before any row load: it costs its id and its bitset word, not a base row.
#include <algorithm>
#include <cstdlib>

#include "hooks.hpp"
#include "label_index.hpp"

namespace ggnn_amd {

// ---- resolve ----------------------------------------------------------------------------------------------
constexpr uint32_t kDeadSpan = 0xffffffffu;  // sorts behind every position (an index has <= 2^30)

// first position of keys that is >= L (upper == false) or > L (upper == true)
GGNN_DEV uint32_t label_spans_bound(const int32_t* keys, const uint32_t n_keys, const int32_t L,
                                    const bool upper)
{
  uint32_t lo = 0, hi = n_keys;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    const int32_t key = keys[mid];
    if (upper ? key <= L : key < L)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// eight spans ascending by begin (dead spans last): the 19-comparator network.  Constant indices
// only, so that the spans stay in registers.
GGNN_DEV void label_spans_sort8(uint32_t (&b)[kMaxLabelSpans], uint32_t (&e)[kMaxLabelSpans])
{
#define GGNN_CX(i, j)                  \
  do {                                 \
    const bool sw = b[i] > b[j];       \
    const uint32_t bi = b[i], ei = e[i]; \
    b[i] = sw ? b[j] : bi;             \
    e[i] = sw ? e[j] : ei;             \
    b[j] = sw ? bi : b[j];             \
    e[j] = sw ? ei : e[j];             \
  } while (0)
  GGNN_CX(0, 1); GGNN_CX(2, 3); GGNN_CX(4, 5); GGNN_CX(6, 7);
  GGNN_CX(0, 2); GGNN_CX(1, 3); GGNN_CX(4, 6); GGNN_CX(5, 7);
  GGNN_CX(1, 2); GGNN_CX(5, 6); GGNN_CX(0, 4); GGNN_CX(3, 7);
  GGNN_CX(1, 5); GGNN_CX(2, 6);
  GGNN_CX(1, 4); GGNN_CX(3, 6);
  GGNN_CX(2, 4); GGNN_CX(3, 5);
  GGNN_CX(3, 4);
#undef GGNN_CX
}

__global__ void __launch_bounds__(kWave)
    label_spans_resolve_kernel(const int32_t* keys, const uint32_t n_keys, const uint32_t* offsets,
                               const int mode, const int32_t* sel, const uint32_t n_sel,
                               const uint32_t Nq, uint32_t* spans, uint32_t* totals)
{
  const uint32_t n = block_linear_index() * kWave + threadIdx.x;
  if (n >= Nq)
    return;
  uint32_t b[kMaxLabelSpans], e[kMaxLabelSpans];
#pragma unroll
  for (uint32_t j = 0; j < kMaxLabelSpans; ++j) {
    uint32_t sb = 0, se = 0;
    if (j < n_sel) {
      if (mode == kLabelSpanSets) {
        const int32_t L = sel[static_cast<size_t>(n) * n_sel + j];
        if (L == -1) {
          se = offsets[n_keys];  // the wildcard of *_labeled_in: the whole index
        }
        else {
          const uint32_t i = label_index_find(keys, n_keys, L);
          if (i < n_keys) {
            sb = offsets[i];
            se = offsets[i + 1];
          }
        }
      }
      else {
        const int32_t lo = sel[(static_cast<size_t>(n) * n_sel + j) * 2];
        const int32_t hi = sel[(static_cast<size_t>(n) * n_sel + j) * 2 + 1];
        if (lo <= hi) {
          sb = offsets[label_spans_bound(keys, n_keys, lo, false)];
          se = offsets[label_spans_bound(keys, n_keys, hi, true)];
        }
      }
    }
    const bool live = sb < se;
    b[j] = live ? sb : kDeadSpan;
    e[j] = live ? se : kDeadSpan;
  }
  label_spans_sort8(b, e);
  // a span that overlaps or touches its predecessor absorbs it (live spans are in front, ascending)
#pragma unroll
  for (uint32_t j = 1; j < kMaxLabelSpans; ++j) {
    const bool join = b[j] != kDeadSpan && b[j] <= e[j - 1];
    e[j] = join ? max(e[j], e[j - 1]) : e[j];
    b[j] = join ? b[j - 1] : b[j];
    b[j - 1] = join ? kDeadSpan : b[j - 1];
    e[j - 1] = join ? kDeadSpan : e[j - 1];
  }
  label_spans_sort8(b, e);
  uint32_t total = 0;
  uint32_t* out = spans + static_cast<size_t>(n) * kMaxLabelSpans * 2;
#pragma unroll
  for (uint32_t j = 0; j < kMaxLabelSpans; ++j) {
    const bool live = b[j] != kDeadSpan;
    out[2 * j] = live ? b[j] : 0u;
    out[2 * j + 1] = live ? e[j] : 0u;
    total += live ? e[j] - b[j] : 0u;
  }
  totals[n] = total;
}

void launch_label_spans_resolve(const int32_t* keys, uint32_t n_keys, const uint32_t* offsets,
                                int mode, const int32_t* sel, uint32_t n_sel, uint32_t Nq,
                                uint32_t* spans, uint32_t* totals, hipStream_t stream)
{
  GGNN_REQUIRE(mode == kLabelSpanSets || mode == kLabelSpanRanges, GGNN_INVALID_ARGUMENT,
               "label_spans_resolve: mode is 0 (label sets) or 1 (label ranges)");
  if (mode == kLabelSpanSets)
    GGNN_REQUIRE(n_sel >= 1 && n_sel <= GGNN_MAX_LABEL_SET, GGNN_INVALID_ARGUMENT,
                 "set_width must be in [1, 8]");
  else
    GGNN_REQUIRE(n_sel >= 1 && n_sel <= GGNN_MAX_LABEL_RANGES, GGNN_INVALID_ARGUMENT,
                 "n_ranges must be in [1, 4]");
  if (Nq == 0)
    return;
  GGNN_REQUIRE(keys && offsets && sel && spans && totals, GGNN_INVALID_ARGUMENT,
               "label_spans_resolve: null pointer");
  GGNN_REQUIRE(n_keys >= 1, GGNN_INVALID_ARGUMENT, "a label index has at least one key");
  hipLaunchKernelGGL(label_spans_resolve_kernel, grid_for((Nq + kWave - 1) / kWave), dim3(kWave), 0,
                     stream, keys, n_keys, offsets, mode, sel, n_sel, Nq, spans, totals);
  GGNN_HIP_CHECK(hipGetLastError());
}

// ---- the (distance, id) order ------------------------------------------------------------------------------
// does the candidate (d, id) go in front of the entry (ed, ek)?  Ids are compared as signed values
// (kEmptyKey is -1); an empty entry is displaced by a smaller distance only, never by +inf.
GGNN_DEV bool label_spans_before(const float d, const int id, const float ed, const int ek)
{
  return d < ed || (d == ed && ek != kEmptyKey && id < ek);
}

// SortedList::push_best_stable under the (distance, id) order; only the best list is used
template <int R>
GGNN_DEV void push_best_by_id(SortedList<R>& l, const int k, const float d)
{
  const int lane = threadIdx.x;
#pragma unroll
  for (int r = R - 1; r >= 0; --r) {
    const int i = r * kWave + lane;
    int pk = lane_up1(l.key[r]);
    float pd = lane_up1(l.dist[r]);
    if (r > 0) {
      const int bk = rdlane(l.key[r - 1], 63);
      const float bd = rdlanef(l.dist[r - 1], 63);
      if (lane == 0) {
        pk = bk;
        pd = bd;
      }
    }
    const bool active = label_spans_before(d, k, l.dist[r], l.key[r]) && (i < l.BEST);
    const bool prev_active = (i != 0) && label_spans_before(d, k, pd, pk);
    if (active) {
      if (!prev_active) {
        l.key[r] = k;
        l.dist[r] = d;
      }
      else {
        l.key[r] = pk;
        l.dist[r] = pd;
      }
    }
  }
}

// the candidates (idv, cd) of the wave's lanes into the register list: one ballot on cd <= worst, the
// same test again per candidate against the list as it is by then, and the exact decision (accepted
// iff its place is below K) in the insert
template <int R>
GGNN_DEV void label_spans_rank(SortedList<R>& best, const uint32_t K, const int idv, const float cd)
{
  unsigned long long m = __ballot(idv >= 0 && cd <= best.dist_at(K - 1));
  while (m) {
    const int j = __ffsll(static_cast<long long>(m)) - 1;
    m &= m - 1;
    const float d = rdlanef(cd, j);
    const int id = rdlane(idv, j);
    // (the exact decision is the insert's own: no entry below K in front of which it goes, no change)
    if (d <= best.dist_at(K - 1))
      push_best_by_id(best, id, d);
  }
}

// the same into a list in LDS (dists [K] | ids [K]): the chunked insert of label_index_scan_lds_kernel
// under the (distance, id) order -- chunks from the right so that every entry is read before it is
// overwritten.  Called by the whole wave with the same candidates.
GGNN_DEV void label_spans_rank_lds(float* best_d, int* best_i, const uint32_t K, const int idv,
                                   const float cd)
{
  const int lane = threadIdx.x;
  unsigned long long m = __ballot(idv >= 0 && cd <= best_d[K - 1]);
  while (m) {
    const int j = __ffsll(static_cast<long long>(m)) - 1;
    m &= m - 1;
    const float d = rdlanef(cd, j);
    const int id = rdlane(idv, j);
    if (!label_spans_before(d, id, best_d[K - 1], best_i[K - 1]))
      continue;
    for (int c0 = (static_cast<int>(K) - 1) / kWave * kWave; c0 >= 0; c0 -= kWave) {
      const int k = c0 + lane;
      const bool own = k < static_cast<int>(K);
      const float cur = own ? best_d[k] : inf_f();
      const int curi = own ? best_i[k] : kEmptyKey;
      const float prev = (own && k > 0) ? best_d[k - 1] : -inf_f();
      const int previ = (own && k > 0) ? best_i[k - 1] : kEmptyKey;
      __syncthreads();
      if (own && label_spans_before(d, id, cur, curi)) {
        const bool first = !label_spans_before(d, id, prev, previ);
        best_d[k] = first ? d : prev;
        best_i[k] = first ? id : previ;
      }
      __syncthreads();
    }
  }
}

// the two as what label_spans_walk calls per batch (inlined: the register list stays in registers)
template <int R>
struct LabelSpansRank {
  SortedList<R>& best;
  uint32_t K;
  GGNN_DEV void operator()(const int idv, const float cd) const { label_spans_rank(best, K, idv, cd); }
};
struct LabelSpansRankLds {
  float* best_d;
  int* best_i;
  uint32_t K;
  GGNN_DEV void operator()(const int idv, const float cd) const
  {
    label_spans_rank_lds(best_d, best_i, K, idv, cd);
  }
};

// ---- the scan through spans ----------------------------------------------------------------------------------
struct LabelSpansArgs {
  const void* base;
  const void* query;
  int32_t* ids;  // [slices x Nq x K] partial results (or final when slices == 1)
  float* dists;
  uint32_t D, Nq, N_base, K, slices;
  const int32_t* rows;
  const uint32_t* spans;         // [Nq x 8 x 2]
  const uint32_t* filter_table;  // [num_filters x words] or null
  uint32_t num_filters, words;
  const int32_t* filter_ids;  // [Nq] or null
};

// one (query, slice) wave: its virtual positions [vbeg, vend) of the query's spans laid end to end and
// the query's filter row.  Everything here is wave-uniform (scalar).
struct LabelSpansWave {
  // lane j: the virtual position at which span j starts, and what a lane at or behind it adds to reach
  // rows[] -- the gap between the spans j - 1 and j (mod 2^32; span 0: its begin).  Wave-uniform values, computed in
  // scalar registers and then parked in the lanes of two vector registers: fourteen more scalar
  // registers across the loop are more than the {64, 16} layouts have (their sixteen chunk masks take
  // sixty), and the kernels must not spill.  id_at() reads them back with constant-lane reads.
  uint32_t start_of, step_of;
  uint32_t vbeg, vend;
  const int32_t* rows;
  uint32_t N_base;
  const uint32_t* bits;  // the query's row of the table, or the constant all-ones word
  uint32_t imask;        // ~3u: `bits` is a row;  0: it is one word

  GGNN_DEV LabelSpansWave(const LabelSpansArgs& a, const uint32_t n, const uint32_t slice)
      : rows(a.rows), N_base(a.N_base), bits(kFilterConstWords<>), imask(0u)
  {
    const uint32_t* sp = a.spans + static_cast<size_t>(n) * kMaxLabelSpans * 2;
    uint32_t total = 0, delta = 0;
    start_of = step_of = 0u;
#pragma unroll
    for (uint32_t j = 0; j < kMaxLabelSpans; ++j) {
      uint32_t b = __builtin_amdgcn_readfirstlane(sp[2 * j]);
      uint32_t e = __builtin_amdgcn_readfirstlane(sp[2 * j + 1]);
      // (an index is at most N_base positions long: never read rows[] behind it.  Spans in normal
      // form are disjoint, so together they are no longer than that either; any others are cut there,
      // which keeps every sum below 2^32 and every position inside its span)
      e = min(e, a.N_base);
      b = min(b, e);
      e = min(e, b + (a.N_base - total));
      start_of = threadIdx.x == j ? total : start_of;
      step_of = threadIdx.x == j ? (b - total) - delta : step_of;
      delta = b - total;
      total += e - b;
    }
    // the slice: multiples of 64 virtual positions = of ROWS * STEPS for every configuration
    uint32_t per = (total + a.slices - 1) / a.slices;
    per = (per + 63u) & ~63u;
    vbeg = min(total, slice * per);
    vend = min(total, vbeg + per);
    if (a.filter_ids) {
      const int32_t f = __builtin_amdgcn_readfirstlane(a.filter_ids[n]);
      if (static_cast<uint32_t>(f) < a.num_filters) {
        bits = a.filter_table + static_cast<size_t>(static_cast<uint32_t>(f)) * a.words;
        imask = ~3u;
      }
      else if (f != -1)
        vend = vbeg;  // admits nothing: the empty result, and no row is read
    }
  }
  // this lane's row id for virtual position v0 + lane of a batch of B: one coalesced dword per span the
  // batch touches.  -1: no row (behind the slice, or an id outside the base: never addressed)
  template <int B>
  GGNN_DEV int id_at(const uint32_t v0)
  {
    // (the two registers count as changed here, so that their fourteen reads stay where they are used
    // instead of being hoisted in front of the loop, back into scalar registers)
    asm volatile("" : "+v"(start_of), "+v"(step_of));
    const uint32_t v = v0 + threadIdx.x;
    // a sum of selects, not a select of the span's offset: the compiler turns the latter into a table in
    // private memory.  Span 0 starts at 0 and its step is its begin, so v + d is exact mod 2^32.  (The
    // cross-lane reads come first, with every lane active.)
    uint32_t d = __builtin_amdgcn_readlane(step_of, 0);
#pragma unroll
    for (int j = 1; j < static_cast<int>(kMaxLabelSpans); ++j) {
      const uint32_t start = __builtin_amdgcn_readlane(start_of, j);
      const uint32_t step = __builtin_amdgcn_readlane(step_of, j);
      d += v >= start ? step : 0u;  // (an unused span starts at `total`: never reached)
    }
    int id = -1;
    if (static_cast<int>(threadIdx.x) < B && v < vend)
      id = rows[v + d];
    return static_cast<uint32_t>(id) < N_base ? id : -1;
  }
  // the word of the filter row that holds the bit of row id (no row: the first word, verdict ignored)
  GGNN_DEV uint32_t word_of(const int id) const
  {
    return filter_word_at(bits, (static_cast<uint32_t>(max(id, 0)) >> 3) & imask);
  }
  // id, or -1 if its bit is clear
  GGNN_DEV int admit(const int id, const uint32_t word) const
  {
    return (id >= 0 && ((word >> (static_cast<uint32_t>(id) & 31u)) & 1u)) ? id : -1;
  }
};

// The loop of both scan kernels.  Three batches are in flight: the rows of batch b, the bitset words
// of batch b + 1 (its ids arrived under batch b - 1) and the ids of batch b + 2 -- both requests are
// issued in front of the rows of batch b, so that the dependent chain id -> bit -> row is exposed once
// per wave.  rank(idv, cd) takes the batch's candidates.
template <typename BaseT, int LPR, int NCH, int MODE, class DE, class RANK>
GGNN_DEV void label_spans_walk(LabelSpansWave& w, const DE& de, float* s_d, const RANK rank)
{
  constexpr int B = (kWave / LPR) * StepsOf<LPR, NCH>::value;
  const int lane = threadIdx.x;
  const int first = w.template id_at<B>(w.vbeg);
  int cur = w.admit(first, w.word_of(first));
  int nxt = w.template id_at<B>(w.vbeg + B);
  for (uint32_t v0 = w.vbeg; v0 < w.vend; v0 += B) {
    const uint32_t word = w.word_of(nxt);
    const int after = w.template id_at<B>(v0 + 2 * B);
    label_index_batch<BaseT, LPR, NCH, MODE>(de, cur, s_d);
    const float cd = (lane < B && cur >= 0) ? s_d[lane] : inf_f();
    rank(cur, cd);
    cur = w.admit(nxt, word);
    nxt = after;
  }
}

template <typename BaseT, int LPR, int NCH, int R, int MODE>
__global__ void __launch_bounds__(kWave) label_spans_scan_kernel(const LabelSpansArgs a)
{
  constexpr int B = (kWave / LPR) * StepsOf<LPR, NCH>::value;
  using DE = DistEngine<BaseT, LPR, NCH>;
  __shared__ float s_d[B];

  const int lane = threadIdx.x;
  const uint32_t bid = block_linear_index();
  if (bid >= a.Nq * a.slices)
    return;
  const uint32_t n = bid / a.slices;
  const uint32_t slice = bid % a.slices;
  // the row of [slices, Nq] this wave writes, as ONE value across the loop (bid < Nq * slices < 2^32)
  const uint32_t part = slice * a.Nq + n;
  const BaseT* base = static_cast<const BaseT*>(a.base);
  const BaseT* query = static_cast<const BaseT*>(a.query);

  DE de;
  de.template load_query<MODE>(base, a.D, query + static_cast<size_t>(n) * a.D);

  SortedList<R> best;  // only key/dist/BEST are used
  best.BEST = a.K;
  best.SORTED = a.K;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    best.key[r] = kEmptyKey;
    best.dist[r] = inf_f();
  }

  LabelSpansWave w(a, n, slice);
  label_spans_walk<BaseT, LPR, NCH, MODE>(w, de, s_d, LabelSpansRank<R>{best, a.K});

  const size_t out = static_cast<size_t>(part) * a.K;  // [slices, Nq, K]
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t i = r * kWave + lane;
    if (i < a.K) {
      a.ids[out + i] = best.key[r];
      a.dists[out + i] = best.dist[r];
    }
  }
}

// k > 256: the K-best list lives in LDS (dists [K] | ids [K]), as in label_index_scan_lds_kernel
template <typename BaseT, int LPR, int NCH, int MODE>
__global__ void __launch_bounds__(kWave) label_spans_scan_lds_kernel(const LabelSpansArgs a)
{
  using DE = DistEngine<BaseT, LPR, NCH>;
  extern __shared__ __attribute__((aligned(16))) int lds_raw[];
  float* best_d = reinterpret_cast<float*>(lds_raw);
  int* best_i = lds_raw + a.K;
  float* s_d = reinterpret_cast<float*>(lds_raw + 2 * a.K);

  const int lane = threadIdx.x;
  const uint32_t bid = block_linear_index();
  if (bid >= a.Nq * a.slices)
    return;
  const uint32_t n = bid / a.slices;
  const uint32_t slice = bid % a.slices;
  const BaseT* base = static_cast<const BaseT*>(a.base);
  DE de;
  de.template load_query<MODE>(base, a.D,
                               static_cast<const BaseT*>(a.query) + static_cast<size_t>(n) * a.D);
  for (uint32_t i = lane; i < a.K; i += kWave) {
    best_d[i] = inf_f();
    best_i[i] = kEmptyKey;
  }
  __syncthreads();

  LabelSpansWave w(a, n, slice);
  label_spans_walk<BaseT, LPR, NCH, MODE>(w, de, s_d, LabelSpansRankLds{best_d, best_i, a.K});
  __syncthreads();
  const size_t out = (static_cast<size_t>(slice) * a.Nq + n) * a.K;
  for (uint32_t i = lane; i < a.K; i += kWave) {
    a.ids[out + i] = best_i[i];
    a.dists[out + i] = best_d[i];
  }
}

// ---- the merge of the slices' lists ----------------------------------------------------------------------------
// one wave per query: the slices x K candidates of [slices, Nq, K] re-inserted by (distance, id)
template <int R>
__global__ void __launch_bounds__(kWave)
    label_spans_merge_kernel(const int32_t* part_ids, const float* part_dists, const uint32_t Nq,
                             const uint32_t K, const uint32_t slices, int32_t* ids, float* dists)
{
  const int lane = threadIdx.x;
  const uint32_t n = block_linear_index();
  if (n >= Nq)
    return;
  SortedList<R> best;  // only key/dist/BEST are used
  best.BEST = K;
  best.SORTED = K;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    best.key[r] = kEmptyKey;
    best.dist[r] = inf_f();
  }
  for (uint32_t s = 0; s < slices; ++s) {
    const size_t in = (static_cast<size_t>(s) * Nq + n) * K;
    for (uint32_t c0 = 0; c0 < K; c0 += kWave) {
      const bool own = c0 + lane < K;
      const int idv = own ? part_ids[in + c0 + lane] : kEmptyKey;
      const float cd = own ? part_dists[in + c0 + lane] : inf_f();
      label_spans_rank(best, K, idv, cd);
    }
  }
  const size_t out = static_cast<size_t>(n) * K;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t i = r * kWave + lane;
    if (i < K) {
      ids[out + i] = best.key[r];
      dists[out + i] = best.dist[r];
    }
  }
}

__global__ void __launch_bounds__(kWave)
    label_spans_merge_lds_kernel(const int32_t* part_ids, const float* part_dists, const uint32_t Nq,
                                 const uint32_t K, const uint32_t slices, int32_t* ids, float* dists)
{
  extern __shared__ __attribute__((aligned(16))) int lds_raw[];
  float* best_d = reinterpret_cast<float*>(lds_raw);
  int* best_i = lds_raw + K;
  const int lane = threadIdx.x;
  const uint32_t n = block_linear_index();
  if (n >= Nq)
    return;
  for (uint32_t i = lane; i < K; i += kWave) {
    best_d[i] = inf_f();
    best_i[i] = kEmptyKey;
  }
  __syncthreads();
  for (uint32_t s = 0; s < slices; ++s) {
    const size_t in = (static_cast<size_t>(s) * Nq + n) * K;
    for (uint32_t c0 = 0; c0 < K; c0 += kWave) {
      const bool own = c0 + lane < K;
      const int idv = own ? part_ids[in + c0 + lane] : kEmptyKey;
      const float cd = own ? part_dists[in + c0 + lane] : inf_f();
      label_spans_rank_lds(best_d, best_i, K, idv, cd);
    }
  }
  __syncthreads();
  const size_t out = static_cast<size_t>(n) * K;
  for (uint32_t i = lane; i < K; i += kWave) {
    ids[out + i] = best_i[i];
    dists[out + i] = best_d[i];
  }
}

template <typename BaseT, int LPR, int NCH, int MODE>
static void launch_label_spans_r(const LabelSpansArgs& args, hipStream_t stream)
{
  const dim3 grid = grid_for(static_cast<uint64_t>(args.Nq) * args.slices);
  if (args.K <= 64)
    hipLaunchKernelGGL((label_spans_scan_kernel<BaseT, LPR, NCH, 1, MODE>), grid, dim3(kWave), 0,
                       stream, args);
  else if (args.K <= 128)
    hipLaunchKernelGGL((label_spans_scan_kernel<BaseT, LPR, NCH, 2, MODE>), grid, dim3(kWave), 0,
                       stream, args);
  else if (args.K <= 256)
    hipLaunchKernelGGL((label_spans_scan_kernel<BaseT, LPR, NCH, 4, MODE>), grid, dim3(kWave), 0,
                       stream, args);
  else
    hipLaunchKernelGGL((label_spans_scan_lds_kernel<BaseT, LPR, NCH, MODE>), grid, dim3(kWave),
                       (2 * args.K + 64) * sizeof(int), stream, args);
}

void launch_label_spans_scan(const LabelSpansLaunch& a, hipStream_t stream)
{
  GGNN_REQUIRE(a.k_query >= 1 && a.k_query <= 6000, GGNN_INVALID_ARGUMENT,
               "KQuery must be in [1, 6000]");
  GGNN_REQUIRE(a.N_base <= kMaxLabeledShardRows, GGNN_UNSUPPORTED,
               "label filters need at most 2^30 base vectors per scan");
  GGNN_REQUIRE((a.filter_table != nullptr) == (a.num_filters > 0), GGNN_INVALID_ARGUMENT,
               "filter_table and num_filters go together");
  GGNN_REQUIRE(!a.filter_table || static_cast<uint64_t>(a.words) * 32 >= a.N_base,
               GGNN_INVALID_ARGUMENT, "a filter needs N_base bits");
  if (a.Nq == 0)
    return;
  GGNN_REQUIRE(a.base != nullptr && a.query != nullptr, GGNN_INVALID_ARGUMENT,
               "base or query pointer is null");
  GGNN_REQUIRE(a.rows != nullptr && a.spans != nullptr, GGNN_INVALID_ARGUMENT,
               "the label index rows or the spans are missing");
  GGNN_REQUIRE(a.ids != nullptr && a.dists != nullptr, GGNN_INVALID_ARGUMENT,
               "result pointers are null");
  check_vector_layout(a.base, a.D, a.dtype);
  check_vector_layout(a.query, a.D, a.dtype);

  // enough waves to fill the chip, as launch_label_index_scan: the longest run of positions a query of
  // this call is expected to have is the cutoff it was classified with (the host cannot see totals[]
  // without a sync); hook LABEL_INDEX_SLICES forces a count
  const uint32_t longest = a.span_limit ? std::min(a.span_limit, a.N_base) : a.N_base;
  uint32_t slices = 1;
  const uint32_t target_waves = 256 * 16;
  if (a.Nq < target_waves)
    slices = std::min((target_waves + a.Nq - 1) / a.Nq, std::max(1u, longest / 4096u));
  const int64_t forced = hook(kHookLabelIndexSlices);
  if (forced > 0)
    slices = static_cast<uint32_t>(std::min<int64_t>(forced, 64));
  slices = std::max(1u, std::min(slices, 64u));

  int32_t* tmp_ids = nullptr;
  float* tmp_dists = nullptr;
  if (slices > 1) {
    const size_t part = static_cast<size_t>(a.Nq) * slices * a.k_query;
    GGNN_HIP_CHECK(
        hipMallocAsync(reinterpret_cast<void**>(&tmp_ids), 2 * part * sizeof(int32_t), stream));
    tmp_dists = reinterpret_cast<float*>(tmp_ids + part);
  }

  LabelSpansArgs args{};
  args.base = a.base;
  args.query = a.query;
  args.D = a.D;
  args.Nq = a.Nq;
  args.N_base = a.N_base;
  args.K = a.k_query;
  args.slices = slices;
  args.rows = a.rows;
  args.spans = a.spans;
  args.filter_table = a.filter_table;
  args.num_filters = a.num_filters;
  args.words = a.words;
  args.filter_ids = a.filter_ids;
  args.ids = slices > 1 ? tmp_ids : a.ids;
  args.dists = slices > 1 ? tmp_dists : a.dists;

#define GGNN_LAUNCH_LS(T, LPR, NCH)                          \
  do {                                                       \
    if (a.measure == GGNN_EUCLIDEAN)                         \
      launch_label_spans_r<T, LPR, NCH, kL2>(args, stream);  \
    else                                                     \
      launch_label_spans_r<T, LPR, NCH, kCos>(args, stream); \
  } while (0)
  GGNN_DISPATCH_DIST(a.dtype, a.D, GGNN_LAUNCH_LS);
#undef GGNN_LAUNCH_LS
  GGNN_HIP_CHECK(hipGetLastError());
  if (slices > 1) {
    // slices are NOT in id order: the lists are merged by (distance, id), not "lower part first"
    if (a.k_query <= 256)
      hipLaunchKernelGGL(label_spans_merge_kernel<4>, grid_for(a.Nq), dim3(kWave), 0, stream,
                         tmp_ids, tmp_dists, a.Nq, a.k_query, slices, a.ids, a.dists);
    else
      hipLaunchKernelGGL(label_spans_merge_lds_kernel, grid_for(a.Nq), dim3(kWave),
                         2 * a.k_query * sizeof(int), stream, tmp_ids, tmp_dists, a.Nq, a.k_query,
                         slices, a.ids, a.dists);
    GGNN_HIP_CHECK(hipGetLastError());
    GGNN_HIP_CHECK(hipFreeAsync(tmp_ids, stream));
  }
}

// ---- classify by totals ---------------------------------------------------------------------------------------
// routed iff totals[n] <= cutoff: a flag word per 64 queries (one ballot), then label_index_compact_kernel.
// No atomics, so the lists are the same for the same input.
__global__ void __launch_bounds__(kWave)
    label_spans_flags_kernel(const uint32_t* totals, const uint32_t Nq, const uint32_t cutoff,
                             unsigned long long* flags)
{
  const uint32_t w = block_linear_index();
  const uint32_t n = w * kWave + threadIdx.x;
  const bool routed = n < Nq && totals[n] <= cutoff;
  const unsigned long long m = __ballot(routed);
  if (threadIdx.x == 0 && w * kWave < Nq)
    flags[w] = m;
}

void launch_label_spans_classify(const uint32_t* totals, uint32_t Nq, uint32_t cutoff,
                                 uint32_t* routed_list, uint32_t* rest_list, uint32_t* counts,
                                 hipStream_t stream)
{
  GGNN_REQUIRE(counts != nullptr, GGNN_INVALID_ARGUMENT, "label_spans_classify: null pointer");
  if (!Nq) {
    GGNN_HIP_CHECK(hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), stream));
    return;
  }
  GGNN_REQUIRE(totals && routed_list && rest_list, GGNN_INVALID_ARGUMENT,
               "label_spans_classify: null pointer");
  const uint32_t words = (Nq + kWave - 1) / kWave;
  ScratchGuard flags{scratch_alloc(words * sizeof(unsigned long long), stream), stream};
  hipLaunchKernelGGL(label_spans_flags_kernel, grid_for(words), dim3(kWave), 0, stream, totals, Nq,
                     cutoff, static_cast<unsigned long long*>(flags.p));
  GGNN_HIP_CHECK(hipGetLastError());
  launch_label_index_compact(static_cast<const unsigned long long*>(flags.p), Nq, routed_list,
                             rest_list, counts, stream);
}

}  // namespace ggnn_amd
