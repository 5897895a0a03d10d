// Filtered query kernels: the traversal of query.hip restricted to an allowed-id bitset.
//
// One rule is added to the search: the push of a DENIED key never touches
// the best list [0, BEST) -- it is queued, popped and expanded like any other point, so the graph
// stays connected under every filter, but it is never reported.  criteria() = dist[BEST-1] + xi
// then only tightens on ALLOWED points and the search widens by itself under a selective filter.
//
// The filter bit of a candidate is requested together with the candidate's first-read row (one
// dword per lane, IdFilter in traversal.hpp) and consumed at the replay, after the rows.
//
// Variants (hooks never change a result, so the dispatch is narrower than launch_query_r):
//   * R = 1, early rows with the hashed visited set in LDS (one or two bucket registers): the
//     headline and shard shapes (KBuild <= 24, up to 480 ring entries);
//   * R = 1, 2, 4, 8, 16, 32 register lists and the LDS list in the round-1..4 order with the ring
//     scan: everything else (KBuild > 24, long rings, wide rows, hook QUERY_EARLY = 0).
// There is no ring-less / tag-set form: QUERY_GLOBAL_RING and VIS_TAG_SET do nothing here.
// The float16 / bfloat16 kernels are instantiated by query_filtered_16.hip.
//
// Label filters (GGNN_LABELS_TU: query_labeled.hip, query_labeled_16.hip): this file once more with
// LabelFilter in place of IdFilter, under kernel and launcher names of their own.  The bitset
// kernels above are not touched by it.
#include <algorithm>

#include "traversal.hpp"
#include "query_args.hpp"

#ifdef GGNN_LABELS_TU
#define query_filtered_kernel query_labeled_kernel
#define query_filtered_kernel_lds query_labeled_kernel_lds
#define launch_query_filtered_16 launch_query_labeled_16
#endif

namespace ggnn_amd {

// the filter of the wave of query n
namespace {
#ifdef GGNN_LABELS_TU
using WaveIdFilter = LabelFilter;
GGNN_DEV WaveIdFilter wave_id_filter(const FilteredQueryArgs& a, const uint32_t n)
{
  return LabelFilter(a.filter_bits, a.filter_bit_offset, a.filter_table, n);
}
#else
using WaveIdFilter = IdFilter;
// this wave's bitset: the call's, or the row of the table its query's filter id names
GGNN_DEV WaveIdFilter wave_id_filter(const FilteredQueryArgs& a, const uint32_t n)
{
  return IdFilter{wave_filter_bits(a.filter_bits, a.filter_table, n), a.filter_bit_offset, kEmptyKey,
                  0u};
}
#endif
}  // namespace

template <class PSC, typename BaseT>
GGNN_DEV void load_prescreen_filtered(PSC& ps, const QueryArgs& a, const BaseT* qrow)
{
  if constexpr (PSC::enabled)
    ps.load(a.ps_codes, a.ps_params, a.ps_Dc, reinterpret_cast<const float*>(qrow), a.D);
}

// Occupancy target as in query.hip (7 waves per SIMD = 72 registers).  The candidate key and the
// bit word of IdFilter are live from the request to the replay: the pre-screened early-rows kernels
// of two-chunk float rows (the headline shape) and of the cosine measure then spill 2-10 registers
// at 72 -- scratch traffic inside the pop loop -- so these get 80 registers (6 waves).
template <int NCH, int MODE, class PSC, bool EARLY>
constexpr int filtered_waves()
{
  return (EARLY && PSC::enabled && (NCH == 2 || MODE == kCos)) ? 6 : 7;
}

template <typename BaseT, int LPR, int NCH, int R, int MODE, class PSC, int HB = 0, bool EARLY = false>
__global__ void __launch_bounds__(kWave) __attribute__((
    amdgpu_waves_per_eu((R == 1 && NCH <= 3) ? filtered_waves<NCH, MODE, PSC, EARLY>() : 1)))
query_filtered_kernel(const FilteredQueryArgs a)
{
  static_assert(HB >= 0, "the filtered kernels keep their visited ring in LDS");
  extern __shared__ __attribute__((aligned(16))) int lds_raw[];
  const WaveLds lds(lds_raw, a.cache);
  const int lane = threadIdx.x;
  const uint32_t n = block_linear_index();
  if (n >= a.Nq)
    return;

  const BaseT* base = static_cast<const BaseT*>(a.base);
  const BaseT* query = static_cast<const BaseT*>(a.query);

  // query_layer.cu:48-50 (xi from the MAX nn1 distance, quirk Q4)
  const float nn1 = a.nn1_stats[1];
  const float xi = (MODE == kL2) ? (nn1 * nn1) * a.tau * a.tau : nn1 * a.tau;

  using DE = DistEngine<BaseT, LPR, NCH, EARLY && PSC::enabled>;
  DE de;
  de.template load_query<MODE>(base, a.D, query + static_cast<size_t>(n) * a.D,
                               lds_raw + wave_lds_ints(a.cache, HB));
  PSC ps;
  load_prescreen_filtered(ps, a, query + static_cast<size_t>(n) * a.D);

  SortedList<R, HB> sl;
  sl.init(a.KQuery, a.sorted, a.cache, xi, lds.known, static_cast<int>(a.vis_slots));
  WaveIdFilter idf = wave_id_filter(a, n);

  uint32_t cnt_dist = 0, cnt_pop = 0;
  uint2 cnt_rows = make_uint2(0u, 0u);

  // the start points are fetched like any candidate: a denied one is queued, not reported
  for (uint32_t i = 0; i < a.num_start; i += kKBlock) {
    const int cand = (lane < (int)kKBlock && i + lane < a.num_start) ? a.start[i + lane]
                                                                      : kEmptyKey;
    cnt_dist += fetch<MODE, false>(sl, de, lds, cand, nullptr, ps, cnt_rows, NoHook{}, idf);
  }

  // (speculative graph row of the queue head: see query.hip)
  int spec_key = kEmptyKey, spec_row = kEmptyKey;
  for (uint32_t ite = 0; ite < a.max_iters; ++ite) {
    // dist[0] is the best ALLOWED distance (+inf until one is found)
    const float d0 = sl.dist_at(0);
    sl.xi = (MODE == kL2) ? fminf(xi, d0 * a.tau * a.tau) : fminf(xi, d0 * a.tau);
    if constexpr (EARLY) {
      const int anchor = sl.peek(sl.criteria());
      if (anchor == kEmptyKey)
        break;
      ++cnt_pop;
      const bool in_row = lane < static_cast<int>(a.KBuild);  // KBuild <= 24 (host)
      int cand;
      if (anchor == spec_key)
        cand = in_row ? spec_row : kEmptyKey;
      else
        cand = in_row ? a.graph0[static_cast<size_t>(static_cast<uint32_t>(anchor)) * a.KBuild + lane]
                      : kEmptyKey;
      auto prefetch_head_row = [&]() {
        spec_key = sl.key_at(sl.BEST);
        spec_row = a.graph0[static_cast<size_t>(static_cast<uint32_t>(max(spec_key, 0))) * a.KBuild +
                            min(lane, static_cast<int>(a.KBuild) - 1)];
        __builtin_amdgcn_s_setprio(1);
      };
      // the bit words go out in front of the first-read rows: loads return in order, so the wait
      // for the rows covers them and the replay finds them there
      idf.request(cand);
      if constexpr (PSC::enabled) {
        EarlyRows<PSC> er;
        er.issue(ps, cand);
        __builtin_amdgcn_s_setprio(0);
        sl.pop_commit(anchor, lds.known);
        cnt_dist += fetch_early<MODE>(sl, de, lds, cand, er, ps, cnt_rows, prefetch_head_row,
                                      nullptr, idf);
      }
      else {
        EarlyRows<DE> er;
        er.issue(de, cand);
        __builtin_amdgcn_s_setprio(0);
        sl.pop_commit(anchor, lds.known);
        cnt_dist += fetch_early<MODE>(sl, de, lds, cand, er, ps, cnt_rows, prefetch_head_row,
                                      nullptr, idf);
      }
      continue;
    }
    const int anchor = sl.pop(sl.criteria(), lds.known);
    if (anchor == kEmptyKey)
      break;
    ++cnt_pop;
    const int32_t* row = a.graph0 + static_cast<size_t>(static_cast<uint32_t>(anchor)) * a.KBuild;
    for (uint32_t i = 0; i < a.KBuild; i += kKBlock) {
      const bool in_row = lane < (int)kKBlock && i + lane < a.KBuild;
      int cand;
      if (i == 0 && anchor == spec_key)
        cand = spec_row;
      else
        cand = in_row ? row[i + lane] : kEmptyKey;
      auto prefetch_head_row = [&]() {
        if (i == 0) {
          spec_key = sl.key_at(sl.BEST);
          if (spec_key != kEmptyKey)
            spec_row = in_row ? a.graph0[static_cast<size_t>(static_cast<uint32_t>(spec_key)) *
                                             a.KBuild + lane]
                              : kEmptyKey;
        }
      };
      cnt_dist += fetch<MODE, true>(sl, de, lds, cand, nullptr, ps, cnt_rows, prefetch_head_row, idf);
    }
  }

  // unfilled slots keep (EMPTY, +inf), written as -1 + offset like the unfiltered kernel's
  const size_t out_row = (static_cast<size_t>(n) * a.shards_per_gpu + a.on_gpu_shard) * a.KQuery;
  const int32_t id_offset = static_cast<int32_t>(a.on_gpu_shard * a.N_base);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t i = r * kWave + lane;
    if (i < a.KQuery) {
      a.ids[out_row + i] = sl.key[r] + id_offset;
      a.dists[out_row + i] = sl.dist[r];
    }
  }
  if (lane == 0) {
    if (a.n_dist)
      a.n_dist[n] = cnt_dist;
    if (a.n_pop)
      a.n_pop[n] = cnt_pop;
    if (a.n_rows)
      a.n_rows[n] = cnt_rows;
  }
}

// the LDS-resident list (SORTED > 2048, or > 512 with the pre-screen)
template <typename BaseT, int LPR, int NCH, int MODE, class PSC>
__global__ void __launch_bounds__(kWave) query_filtered_kernel_lds(const FilteredQueryArgs a)
{
  extern __shared__ __attribute__((aligned(16))) int lds_raw[];
  int* keys = lds_raw;
  float* dists = reinterpret_cast<float*>(lds_raw + a.cache);
  const WaveLds lds(lds_raw + a.cache + a.sorted, 0);
  const int lane = threadIdx.x;
  const uint32_t n = block_linear_index();
  if (n >= a.Nq)
    return;
  const BaseT* base = static_cast<const BaseT*>(a.base);
  const BaseT* query = static_cast<const BaseT*>(a.query);
  const float nn1 = a.nn1_stats[1];
  const float xi = (MODE == kL2) ? (nn1 * nn1) * a.tau * a.tau : nn1 * a.tau;
  DistEngine<BaseT, LPR, NCH> de;
  de.template load_query<MODE>(base, a.D, query + static_cast<size_t>(n) * a.D);
  PSC ps;
  load_prescreen_filtered(ps, a, query + static_cast<size_t>(n) * a.D);
  LdsList sl;
  sl.init(a.KQuery, a.sorted, a.cache, xi, keys, dists);
  WaveIdFilter idf = wave_id_filter(a, n);
  uint32_t cnt_dist = 0, cnt_pop = 0;
  uint2 cnt_rows = make_uint2(0u, 0u);
  for (uint32_t i = 0; i < a.num_start; i += kKBlock) {
    const int cand = (lane < (int)kKBlock && i + lane < a.num_start) ? a.start[i + lane]
                                                                      : kEmptyKey;
    cnt_dist += fetch<MODE, false>(sl, de, lds, cand, nullptr, ps, cnt_rows, NoHook{}, idf);
  }
  for (uint32_t ite = 0; ite < a.max_iters; ++ite) {
    __syncthreads();
    const float d0 = sl.dist_at(0);
    sl.xi = (MODE == kL2) ? fminf(xi, d0 * a.tau * a.tau) : fminf(xi, d0 * a.tau);
    const int anchor = sl.pop(sl.criteria());
    if (anchor == kEmptyKey)
      break;
    ++cnt_pop;
    const int32_t* row = a.graph0 + static_cast<size_t>(static_cast<uint32_t>(anchor)) * a.KBuild;
    for (uint32_t i = 0; i < a.KBuild; i += kKBlock) {
      const int cand = (lane < (int)kKBlock && i + lane < a.KBuild) ? row[i + lane] : kEmptyKey;
      cnt_dist += fetch<MODE, true>(sl, de, lds, cand, nullptr, ps, cnt_rows, NoHook{}, idf);
    }
  }
  __syncthreads();
  const size_t out_row = (static_cast<size_t>(n) * a.shards_per_gpu + a.on_gpu_shard) * a.KQuery;
  const int32_t id_offset = static_cast<int32_t>(a.on_gpu_shard * a.N_base);
  for (uint32_t i = lane; i < a.KQuery; i += kWave) {
    a.ids[out_row + i] = keys[i] + id_offset;
    a.dists[out_row + i] = dists[i];
  }
  if (lane == 0) {
    if (a.n_dist)
      a.n_dist[n] = cnt_dist;
    if (a.n_pop)
      a.n_pop[n] = cnt_pop;
    if (a.n_rows)
      a.n_rows[n] = cnt_rows;
  }
}

template <int LPR, int NCH, class PSC>
constexpr bool filtered_early_layout()
{
  return PSC::enabled ? (PsLayout<PSC>::lpr == 8 && PsLayout<PSC>::nch == 1) : (LPR == 8 && NCH == 1);
}

template <typename BaseT, int LPR, int NCH, int MODE, class PSC>
static void launch_query_filtered_r(const FilteredQueryArgs& args, hipStream_t stream)
{
  const uint32_t sorted = args.sorted;
  const size_t lds = wave_lds_bytes(args.cache);
  const dim3 grid = grid_for(args.Nq);
#define GGNN_QF(R_, HB_, EARLY_, LDS_)                                                            \
  hipLaunchKernelGGL((query_filtered_kernel<BaseT, LPR, NCH, R_, MODE, PSC, HB_, EARLY_>), grid, \
                     dim3(kWave), LDS_, stream, args)
  if constexpr (filtered_early_layout<LPR, NCH, PSC>()) {
    // early rows + hashed visited set (hook QUERY_EARLY = 0: the plain order below, A/B and tests)
    const uint32_t hb = sorted <= 64 ? vis_hash_regs(args.cache - sorted) : 0;
    if (hb != 0 && args.KBuild <= 8 * kEarlySteps && hook(kHookQueryEarly) != 0) {
      const size_t qrow = DistEngine<BaseT, LPR, NCH, PSC::enabled>::kQueryLdsBytes;
      if (hb == 1)
        GGNN_QF(1, 1, true, wave_lds_bytes(args.cache, 1) + qrow);
      else
        GGNN_QF(1, 2, true, wave_lds_bytes(args.cache, 2) + qrow);
      return;
    }
  }
  auto launch_lds = [&] {
    const size_t lds_big = (args.cache + sorted + WaveLds::extra_ints) * sizeof(int);
    GGNN_REQUIRE(lds_big <= 64 * 1024, GGNN_UNSUPPORTED, "cache too large for one workgroup");
    hipLaunchKernelGGL((query_filtered_kernel_lds<BaseT, LPR, NCH, MODE, PSC>), grid, dim3(kWave),
                       lds_big, stream, args);
  };
  if (sorted <= 64)
    GGNN_QF(1, 0, false, lds);
  else if (sorted <= 128)
    GGNN_QF(2, 0, false, lds);
  else if (sorted <= 256)
    GGNN_QF(4, 0, false, lds);
  else if (sorted <= 512)
    GGNN_QF(8, 0, false, lds);
  else if constexpr (!PSC::enabled) {
    if (sorted <= 1024)
      GGNN_QF(16, 0, false, lds);
    else if (sorted <= 2048)
      GGNN_QF(32, 0, false, lds);
    else
      launch_lds();
  }
  else
    launch_lds();
#undef GGNN_QF
}

template <typename BaseT, int LPR, int NCH>
static void launch_query_filtered_cfg(const FilteredQueryArgs& args, bool use_ps, ggnn_measure measure,
                                      hipStream_t stream)
{
  if constexpr (std::is_same<BaseT, float>::value) {
    if (use_ps && args.sorted <= 512) {
      if (measure == GGNN_EUCLIDEAN)
        launch_query_filtered_r<BaseT, LPR, NCH, kL2, typename PsFor<LPR, NCH, kL2>::type>(args, stream);
      else
        launch_query_filtered_r<BaseT, LPR, NCH, kCos, typename PsFor<LPR, NCH, kCos>::type>(args, stream);
      return;
    }
  }
  if (measure == GGNN_EUCLIDEAN)
    launch_query_filtered_r<BaseT, LPR, NCH, kL2, NoPrescreen>(args, stream);
  else
    launch_query_filtered_r<BaseT, LPR, NCH, kCos, NoPrescreen>(args, stream);
}

#ifndef GGNN_ROWS_16_TU
void launch_query_filtered_16(const FilteredQueryArgs& args, ggnn_measure measure, ggnn_dtype dtype,
                              hipStream_t stream);

#ifdef GGNN_LABELS_TU
// base: filled by launch_query (query.hip), filter_bits = the label column; table: query_labels set
void launch_query_labeled(const QueryArgs& base, const FilterTable& table, bool use_ps,
                          ggnn_measure measure, ggnn_dtype dtype, hipStream_t stream)
{
  GGNN_REQUIRE(table.query_labels != nullptr && !table.ids, GGNN_INVALID_ARGUMENT,
               "query labels are missing, or given together with filter ids");
  GGNN_REQUIRE(base.N_base <= kMaxLabeledShardRows, GGNN_UNSUPPORTED,
               "label filters need shards of at most 2^30 base vectors");
  FilteredQueryArgs args{};
  static_cast<QueryArgs&>(args) = base;
  args.filter_table = table;
  if (dtype_is_16bit(dtype)) {
    launch_query_filtered_16(args, measure, dtype, stream);
    return;
  }
#define GGNN_LAUNCH_QF(T, LPR, NCH) launch_query_filtered_cfg<T, LPR, NCH>(args, use_ps, measure, stream)
  GGNN_DISPATCH_DIST_32_8(dtype, args.D, GGNN_LAUNCH_QF);
#undef GGNN_LAUNCH_QF
}
#else
void launch_query_labeled(const QueryArgs& base, const FilterTable& table, bool use_ps,
                          ggnn_measure measure, ggnn_dtype dtype, hipStream_t stream);

// the all-ones / all-zero rows of a launch with filter ids that brings none (operator seam; the
// engine keeps them behind its resident table)
uint32_t* filter_consts_scratch(const FilterTable& t, hipStream_t stream)
{
  if (!t.ids || t.consts)
    return nullptr;
  const size_t row = static_cast<size_t>(t.words) * sizeof(uint32_t);
  uint8_t* p = static_cast<uint8_t*>(scratch_alloc(2 * row, stream));
  GGNN_HIP_CHECK(hipMemsetAsync(p, 0xff, row, stream));
  GGNN_HIP_CHECK(hipMemsetAsync(p + row, 0, row, stream));
  return reinterpret_cast<uint32_t*>(p);
}

// base: filled by launch_query (query.hip), filter_bits set; table: the launch's per-query filters
void launch_query_filtered(const QueryArgs& base, const FilterTable& table, bool use_ps,
                           ggnn_measure measure, ggnn_dtype dtype, hipStream_t stream)
{
  FilteredQueryArgs args{};
  static_cast<QueryArgs&>(args) = base;
  args.filter_table = table;
  if (table.ids)
    GGNN_REQUIRE(table.words != 0 && table.num_filters != 0, GGNN_INVALID_ARGUMENT,
                 "filter ids need a filter table");
  if (table.query_labels) {  // label filters: kernels of their own (query_labeled.hip)
    launch_query_labeled(base, table, use_ps, measure, dtype, stream);
    return;
  }
  struct ConstGuard {
    void* p;
    hipStream_t s;
    ~ConstGuard()
    {
      if (p)
        scratch_free(p, s);
    }
  } guard{filter_consts_scratch(table, stream), stream};
  if (guard.p)
    args.filter_table.consts = static_cast<const uint32_t*>(guard.p);
  if (dtype_is_16bit(dtype)) {
    launch_query_filtered_16(args, measure, dtype, stream);
    return;
  }
#define GGNN_LAUNCH_QF(T, LPR, NCH) launch_query_filtered_cfg<T, LPR, NCH>(args, use_ps, measure, stream)
  GGNN_DISPATCH_DIST_32_8(dtype, args.D, GGNN_LAUNCH_QF);
#undef GGNN_LAUNCH_QF
}
#endif
#else
void launch_query_filtered_16(const FilteredQueryArgs& args, ggnn_measure measure, ggnn_dtype dtype,
                              hipStream_t stream)
{
#define GGNN_LAUNCH_QF(T, LPR, NCH) launch_query_filtered_cfg<T, LPR, NCH>(args, false, measure, stream)
  GGNN_DISPATCH_DIST_16(dtype, args.D, GGNN_LAUNCH_QF);
#undef GGNN_LAUNCH_QF
}
#endif

}  // namespace ggnn_amd
