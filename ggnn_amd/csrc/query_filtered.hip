// Filtered query kernels: the traversal of query.hip restricted to an allowed-id bitset, or to the
// base vectors that carry the query's label.
//
// One rule is added to the search: the push of a DENIED key never touches
// the best list [0, BEST) -- it is queued, popped and expanded like any other point, so the graph
// stays connected under every filter, but it is never reported.  criteria() = dist[BEST-1] + xi
// then only tightens on ALLOWED points and the search widens by itself under a selective filter.
//
// The filter bit of a candidate is requested together with the candidate's first-read row (one
// dword per lane, IdFilter in traversal.hpp) and consumed at the replay, after the rows.
//
// Variants (hooks never change a result, so the dispatch is narrower than QueryLadder's):
//   * R = 1, early rows with the hashed visited set in LDS (one or two bucket registers): the
//     headline and shard shapes (KBuild <= 24, up to 480 ring entries);
//   * R = 1, 2, 4, 8, 16, 32 register lists and the LDS list in the round-1..4 order with the ring
//     scan: everything else (KBuild > 24, long rings, wide rows, hook QUERY_EARLY = 0).
// There is no ring-less / tag-set form: QUERY_GLOBAL_RING and VIS_TAG_SET do nothing here.
// The float16 / bfloat16 kernels are instantiated by query_filtered_16.hip.
//
// Label filters: the same wave program (query_wave_body.inc, shared with query.hip) with LabelFilter
// in place of IdFilter, in kernel templates of their own (query_labeled_kernel*).  Launchers and
// ladder are templates over the filter class; a translation unit instantiates them for ONE class
// (TuFilter: LabelFilter under GGNN_LABELS_TU -- query_labeled.hip, query_labeled_16.hip -- else
// IdFilter), so the bitset kernels are not touched by the label ones and the build compiles both
// in parallel.
//
// Label sets (any of up to 8 labels per query, with an optional filter id: LabelSetFilter): once more
// the same wave program in kernel templates of its own (query_labelset_kernel*), instantiated under
// GGNN_LABELSET_TU -- query_labelset.hip, query_labelset_16.hip.  Their argument block is
// LabelSetQueryArgs; there is no int8 unit and no PrescreenExact variant (a lossless base takes the
// ordinary pre-screened kernel: the same results by construction).
//
// Label ranges (the label in one of up to 4 closed intervals per query, with an optional filter id:
// LabelRangeFilter): the same once more, query_labelrange_kernel* under GGNN_LABELRANGE_TU --
// query_labelrange.hip, query_labelrange_16.hip -- with LabelRangeQueryArgs; no int8 unit and no
// PrescreenExact variant either.
//
// Label masks (the label's tag bits under one of up to 2 (mask, value, any) clauses per query, with an
// optional filter id: LabelMaskFilter): and once more, query_labelmask_kernel* under GGNN_LABELMASK_TU
// -- query_labelmask.hip, query_labelmask_16.hip -- with LabelMaskQueryArgs; no int8 unit and no
// PrescreenExact variant.
#include <algorithm>

#include "query_wave.hpp"

namespace ggnn_amd {

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
  using FILT = IdFilter;
  constexpr bool GR = false;
#include "query_wave_body.inc"
}

// the LDS-resident list (SORTED > 2048, or > 512 with the pre-screen)
template <typename BaseT, int LPR, int NCH, int MODE, class PSC>
__global__ void __launch_bounds__(kWave) query_filtered_kernel_lds(const FilteredQueryArgs a)
{
  using FILT = IdFilter;
#include "query_wave_lds_body.inc"
}

template <typename BaseT, int LPR, int NCH, int R, int MODE, class PSC, int HB = 0, bool EARLY = false>
__global__ void __launch_bounds__(kWave) __attribute__((
    amdgpu_waves_per_eu((R == 1 && NCH <= 3) ? filtered_waves<NCH, MODE, PSC, EARLY>() : 1)))
query_labeled_kernel(const FilteredQueryArgs a)
{
  static_assert(HB >= 0, "the filtered kernels keep their visited ring in LDS");
  using FILT = LabelFilter;
  constexpr bool GR = false;
#include "query_wave_body.inc"
}

// the LDS-resident list (SORTED > 2048, or > 512 with the pre-screen)
template <typename BaseT, int LPR, int NCH, int MODE, class PSC>
__global__ void __launch_bounds__(kWave) query_labeled_kernel_lds(const FilteredQueryArgs a)
{
  using FILT = LabelFilter;
#include "query_wave_lds_body.inc"
}

// Label sets.  One more register per lane is live from the request to the replay (the bitset word
// next to the label), and the eight wanted labels are scalar: the occupancy is the largest at which
// the early-rows squared-L2 kernels of float32 / uint8 rows have no private segment.
// At 7 waves (72 registers) the pre-screened early-rows kernels with two bucket registers go 12 / 28
// bytes into scratch memory on one- and three-chunk float rows as well, not only on two-chunk ones as
// under IdFilter: every pre-screened early-rows kernel gets 80 registers (6 waves).
template <class PSC, bool EARLY>
constexpr int labelset_waves()
{
  return (EARLY && PSC::enabled) ? 6 : 7;
}

template <typename BaseT, int LPR, int NCH, int R, int MODE, class PSC, int HB = 0, bool EARLY = false>
__global__ void __launch_bounds__(kWave) __attribute__((
    amdgpu_waves_per_eu((R == 1 && NCH <= 3) ? labelset_waves<PSC, EARLY>() : 1)))
query_labelset_kernel(const LabelSetQueryArgs a)
{
  static_assert(HB >= 0, "the filtered kernels keep their visited ring in LDS");
  static_assert(!PsExact<PSC>::value, "label sets: no kernels of exact distances from codes");
  using FILT = LabelSetFilter;
  constexpr bool GR = false;
#include "query_wave_body.inc"
}

// the LDS-resident list (SORTED > 2048, or > 512 with the pre-screen)
template <typename BaseT, int LPR, int NCH, int MODE, class PSC>
__global__ void __launch_bounds__(kWave) query_labelset_kernel_lds(const LabelSetQueryArgs a)
{
  using FILT = LabelSetFilter;
#include "query_wave_lds_body.inc"
}

// Label ranges.  LabelRangeFilter keeps per lane what LabelSetFilter keeps (key, label, bitset word)
// and per wave four (lo, span) pairs where that has eight wanted labels and a mask; the verdict is
// four subtract-and-compare pairs instead of eight compares.  The occupancy is chosen by the rule of labelset_waves -- the largest at which every
// early-rows squared-L2 kernel of float32 / uint8 rows has no private segment -- and the build gives
// the same answer.  Built with 7 waves (72 registers) throughout, the kernels read directly (float32
// and uint8 layout {8,1}) take 67-71 registers and no scratch memory, but five of the eight
// pre-screened early-rows squared-L2 kernels go 12-36 bytes into it, the headline kernels <float, 16,
// 2> with 20 and 36 bytes the most; at 6 waves (80 registers) they take 75 / 77 registers and none
// (tests/test_label_ranges.py).
template <class PSC, bool EARLY>
constexpr int labelrange_waves()
{
  return labelset_waves<PSC, EARLY>();
}

template <typename BaseT, int LPR, int NCH, int R, int MODE, class PSC, int HB = 0, bool EARLY = false>
__global__ void __launch_bounds__(kWave) __attribute__((
    amdgpu_waves_per_eu((R == 1 && NCH <= 3) ? labelrange_waves<PSC, EARLY>() : 1)))
query_labelrange_kernel(const LabelRangeQueryArgs a)
{
  static_assert(HB >= 0, "the filtered kernels keep their visited ring in LDS");
  static_assert(!PsExact<PSC>::value, "label ranges: no kernels of exact distances from codes");
  using FILT = LabelRangeFilter;
  constexpr bool GR = false;
#include "query_wave_body.inc"
}

// the LDS-resident list (SORTED > 2048, or > 512 with the pre-screen)
template <typename BaseT, int LPR, int NCH, int MODE, class PSC>
__global__ void __launch_bounds__(kWave) query_labelrange_kernel_lds(const LabelRangeQueryArgs a)
{
  using FILT = LabelRangeFilter;
#include "query_wave_lds_body.inc"
}

// Label masks.  LabelMaskFilter keeps per lane what LabelRangeFilter keeps (key, label, bitset word)
// and per wave two (mask, value, any) clauses where that has four (lo, span) pairs: six scalars for
// eight; the verdict is two ands and two compares per clause and a scalar test of any == 0.  The occupancy
// follows the rule of labelrange_waves -- the largest at which the kernel's private segment is 0, read
// from the built code object -- and the build gives the same answer: 6 waves for the pre-screened
// early-rows kernels, 7 for the others (tests/test_label_masks.py).
template <class PSC, bool EARLY>
constexpr int labelmask_waves()
{
  return labelrange_waves<PSC, EARLY>();
}

template <typename BaseT, int LPR, int NCH, int R, int MODE, class PSC, int HB = 0, bool EARLY = false>
__global__ void __launch_bounds__(kWave) __attribute__((
    amdgpu_waves_per_eu((R == 1 && NCH <= 3) ? labelmask_waves<PSC, EARLY>() : 1)))
query_labelmask_kernel(const LabelMaskQueryArgs a)
{
  static_assert(HB >= 0, "the filtered kernels keep their visited ring in LDS");
  static_assert(!PsExact<PSC>::value, "label masks: no kernels of exact distances from codes");
  using FILT = LabelMaskFilter;
  constexpr bool GR = false;
#include "query_wave_body.inc"
}

// the LDS-resident list (SORTED > 2048, or > 512 with the pre-screen)
template <typename BaseT, int LPR, int NCH, int MODE, class PSC>
__global__ void __launch_bounds__(kWave) query_labelmask_kernel_lds(const LabelMaskQueryArgs a)
{
  using FILT = LabelMaskFilter;
#include "query_wave_lds_body.inc"
}

// the kernel templates of a filter class
template <class FILT, typename BaseT, int LPR, int NCH, int R, int MODE, class PSC, int HB = 0,
          bool EARLY = false>
constexpr auto filtered_kernel()
{
  if constexpr (std::is_same<FILT, LabelMaskFilter>::value)
    return &query_labelmask_kernel<BaseT, LPR, NCH, R, MODE, PSC, HB, EARLY>;
  else if constexpr (std::is_same<FILT, LabelRangeFilter>::value)
    return &query_labelrange_kernel<BaseT, LPR, NCH, R, MODE, PSC, HB, EARLY>;
  else if constexpr (std::is_same<FILT, LabelSetFilter>::value)
    return &query_labelset_kernel<BaseT, LPR, NCH, R, MODE, PSC, HB, EARLY>;
  else if constexpr (std::is_same<FILT, LabelFilter>::value)
    return &query_labeled_kernel<BaseT, LPR, NCH, R, MODE, PSC, HB, EARLY>;
  else
    return &query_filtered_kernel<BaseT, LPR, NCH, R, MODE, PSC, HB, EARLY>;
}
template <class FILT, typename BaseT, int LPR, int NCH, int MODE, class PSC>
constexpr auto filtered_kernel_lds()
{
  if constexpr (std::is_same<FILT, LabelMaskFilter>::value)
    return &query_labelmask_kernel_lds<BaseT, LPR, NCH, MODE, PSC>;
  else if constexpr (std::is_same<FILT, LabelRangeFilter>::value)
    return &query_labelrange_kernel_lds<BaseT, LPR, NCH, MODE, PSC>;
  else if constexpr (std::is_same<FILT, LabelSetFilter>::value)
    return &query_labelset_kernel_lds<BaseT, LPR, NCH, MODE, PSC>;
  else if constexpr (std::is_same<FILT, LabelFilter>::value)
    return &query_labeled_kernel_lds<BaseT, LPR, NCH, MODE, PSC>;
  else
    return &query_filtered_kernel_lds<BaseT, LPR, NCH, MODE, PSC>;
}

// the kernel of one row layout, measure and pre-screen (launch_query_cfg, query_wave.hpp)
template <class FILT>
struct FilteredLadder {
  // (ARGS: FilteredQueryArgs, or LabelSetQueryArgs / LabelRangeQueryArgs / LabelMaskQueryArgs under
  // their filters)
  template <typename BaseT, int LPR, int NCH, int MODE, class PSC, class ARGS>
  static void launch(const ARGS& args, hipStream_t stream)
  {
    const uint32_t sorted = args.sorted;
    if constexpr (early_rows_layout<LPR, NCH, PSC>()) {
      // early rows + hashed visited set (hook QUERY_EARLY = 0: the plain order below, A/B and tests)
      const uint32_t hb = sorted <= 64 ? vis_hash_regs(args.cache - sorted) : 0;
      if (hb != 0 && args.KBuild <= 8 * kEarlySteps && hook(kHookQueryEarly) != 0) {
        const size_t qrow = DistEngine<BaseT, LPR, NCH, PSC::enabled>::kQueryLdsBytes;
        // (PSX: the two-phase variant for a base known to be lossless, as in QueryLadder)
        // (label sets, ranges and masks have no such variant: PSX = PSC and `exact` is false)
        using PSX = std::conditional_t<std::is_same<FILT, LabelSetFilter>::value ||
                                           std::is_same<FILT, LabelRangeFilter>::value ||
                                           std::is_same<FILT, LabelMaskFilter>::value,
                                       PSC, typename ExactOf<PSC>::type>;
        const bool exact = args.ps_lossless != 0 && !std::is_same<PSX, PSC>::value;
        if (hb == 1)
          launch_wave_per_query(exact ? filtered_kernel<FILT, BaseT, LPR, NCH, 1, MODE, PSX, 1, true>()
                                      : filtered_kernel<FILT, BaseT, LPR, NCH, 1, MODE, PSC, 1, true>(),
                                args, wave_lds_bytes(args.cache, 1) + qrow, stream);
        else
          launch_wave_per_query(exact ? filtered_kernel<FILT, BaseT, LPR, NCH, 1, MODE, PSX, 2, true>()
                                      : filtered_kernel<FILT, BaseT, LPR, NCH, 1, MODE, PSC, 2, true>(),
                                args, wave_lds_bytes(args.cache, 2) + qrow, stream);
        return;
      }
    }
    launch_query_ladder<PSC>(sorted, [&](auto regs) {
      constexpr int R = decltype(regs)::value;
      if constexpr (R == 0)
        launch_query_lds_list(filtered_kernel_lds<FILT, BaseT, LPR, NCH, MODE, PSC>(), args, stream);
      else
        launch_wave_per_query(filtered_kernel<FILT, BaseT, LPR, NCH, R, MODE, PSC>(), args,
                              wave_lds_bytes(args.cache), stream);
    });
  }
};

#ifdef GGNN_LABELS_TU
using TuFilter = LabelFilter;
#else
using TuFilter = IdFilter;
#endif

#ifdef GGNN_LABELMASK_TU
#ifdef GGNN_ROWS_16_TU
void launch_query_labelmask_16(const LabelMaskQueryArgs& args, ggnn_measure measure,
                               ggnn_dtype dtype, hipStream_t stream)
{
#define GGNN_LAUNCH_QF(T, LPR, NCH) \
  launch_query_cfg<FilteredLadder<LabelMaskFilter>, T, LPR, NCH>(args, false, measure, stream)
  GGNN_DISPATCH_DIST_16(dtype, args.D, GGNN_LAUNCH_QF);
#undef GGNN_LAUNCH_QF
}
#else
// base: filled by launch_query (query.hip); table: the filter table in base.filter_bits (or null)
// and the filter id per query (or null); mask: the label column and the queries' clauses
void launch_query_labelmask(const QueryArgs& base, const FilterTable& table,
                            const LabelMaskSpec& mask, bool use_ps, ggnn_measure measure,
                            ggnn_dtype dtype, hipStream_t stream)
{
  GGNN_REQUIRE(mask.labels != nullptr && mask.masks != nullptr, GGNN_INVALID_ARGUMENT,
               "the label column or the label masks are missing");
  GGNN_REQUIRE(mask.n_masks >= 1 && mask.n_masks <= kMaxLabelMasks, GGNN_INVALID_ARGUMENT,
               "a query has 1 or 2 label mask clauses");
  GGNN_REQUIRE(!table.query_labels, GGNN_INVALID_ARGUMENT,
               "label masks exclude the one-label form");
  GGNN_REQUIRE(!table.ids || !table.num_filters || (base.filter_bits && table.words),
               GGNN_INVALID_ARGUMENT, "filter ids into a table need the table");
  GGNN_REQUIRE(dtype != GGNN_I8, GGNN_UNSUPPORTED, "label masks are not built for int8 rows");
  GGNN_REQUIRE(base.N_base <= kMaxLabeledShardRows, GGNN_UNSUPPORTED,
               "label filters need shards of at most 2^30 base vectors");
  LabelMaskQueryArgs args{};
  static_cast<QueryArgs&>(args) = base;
  args.filter_table = table;
  args.mask = mask;
  if (dtype_is_16bit(dtype)) {
    launch_query_labelmask_16(args, measure, dtype, stream);
    return;
  }
#define GGNN_LAUNCH_QF(T, LPR, NCH) \
  launch_query_cfg<FilteredLadder<LabelMaskFilter>, T, LPR, NCH>(args, use_ps, measure, stream)
  GGNN_DISPATCH_DIST_32_8(dtype, args.D, GGNN_LAUNCH_QF);
#undef GGNN_LAUNCH_QF
}
#endif
#elif defined(GGNN_LABELRANGE_TU)
#ifdef GGNN_ROWS_16_TU
void launch_query_labelrange_16(const LabelRangeQueryArgs& args, ggnn_measure measure,
                                ggnn_dtype dtype, hipStream_t stream)
{
#define GGNN_LAUNCH_QF(T, LPR, NCH) \
  launch_query_cfg<FilteredLadder<LabelRangeFilter>, T, LPR, NCH>(args, false, measure, stream)
  GGNN_DISPATCH_DIST_16(dtype, args.D, GGNN_LAUNCH_QF);
#undef GGNN_LAUNCH_QF
}
#else
// base: filled by launch_query (query.hip); table: the filter table in base.filter_bits (or null)
// and the filter id per query (or null); range: the label column and the queries' intervals
void launch_query_labelrange(const QueryArgs& base, const FilterTable& table,
                             const LabelRangeSpec& range, bool use_ps, ggnn_measure measure,
                             ggnn_dtype dtype, hipStream_t stream)
{
  GGNN_REQUIRE(range.labels != nullptr && range.ranges != nullptr, GGNN_INVALID_ARGUMENT,
               "the label column or the label ranges are missing");
  GGNN_REQUIRE(range.n_ranges >= 1 && range.n_ranges <= kMaxLabelRanges, GGNN_INVALID_ARGUMENT,
               "a query has 1 to 4 label ranges");
  GGNN_REQUIRE(!table.query_labels, GGNN_INVALID_ARGUMENT,
               "label ranges exclude the one-label form");
  GGNN_REQUIRE(!table.ids || !table.num_filters || (base.filter_bits && table.words),
               GGNN_INVALID_ARGUMENT, "filter ids into a table need the table");
  GGNN_REQUIRE(dtype != GGNN_I8, GGNN_UNSUPPORTED, "label ranges are not built for int8 rows");
  GGNN_REQUIRE(base.N_base <= kMaxLabeledShardRows, GGNN_UNSUPPORTED,
               "label filters need shards of at most 2^30 base vectors");
  LabelRangeQueryArgs args{};
  static_cast<QueryArgs&>(args) = base;
  args.filter_table = table;
  args.range = range;
  if (dtype_is_16bit(dtype)) {
    launch_query_labelrange_16(args, measure, dtype, stream);
    return;
  }
#define GGNN_LAUNCH_QF(T, LPR, NCH) \
  launch_query_cfg<FilteredLadder<LabelRangeFilter>, T, LPR, NCH>(args, use_ps, measure, stream)
  GGNN_DISPATCH_DIST_32_8(dtype, args.D, GGNN_LAUNCH_QF);
#undef GGNN_LAUNCH_QF
}
#endif
#elif defined(GGNN_LABELSET_TU)
#ifdef GGNN_ROWS_16_TU
void launch_query_labelset_16(const LabelSetQueryArgs& args, ggnn_measure measure, ggnn_dtype dtype,
                              hipStream_t stream)
{
#define GGNN_LAUNCH_QF(T, LPR, NCH) \
  launch_query_cfg<FilteredLadder<LabelSetFilter>, T, LPR, NCH>(args, false, measure, stream)
  GGNN_DISPATCH_DIST_16(dtype, args.D, GGNN_LAUNCH_QF);
#undef GGNN_LAUNCH_QF
}
#else
// base: filled by launch_query (query.hip); table: the filter table in base.filter_bits (or null)
// and the filter id per query (or null); set: the label column and the queries' label sets
void launch_query_labelset(const QueryArgs& base, const FilterTable& table, const LabelSetSpec& set,
                           bool use_ps, ggnn_measure measure, ggnn_dtype dtype, hipStream_t stream)
{
  GGNN_REQUIRE(set.labels != nullptr && set.sets != nullptr, GGNN_INVALID_ARGUMENT,
               "the label column or the label sets are missing");
  GGNN_REQUIRE(set.width >= 1 && set.width <= kMaxLabelSet, GGNN_INVALID_ARGUMENT,
               "a label set has 1 to 8 entries");
  GGNN_REQUIRE(!table.query_labels, GGNN_INVALID_ARGUMENT,
               "label sets exclude the one-label form");
  GGNN_REQUIRE(!table.ids || !table.num_filters || (base.filter_bits && table.words),
               GGNN_INVALID_ARGUMENT, "filter ids into a table need the table");
  GGNN_REQUIRE(dtype != GGNN_I8, GGNN_UNSUPPORTED, "label sets are not built for int8 rows");
  GGNN_REQUIRE(base.N_base <= kMaxLabeledShardRows, GGNN_UNSUPPORTED,
               "label filters need shards of at most 2^30 base vectors");
  LabelSetQueryArgs args{};
  static_cast<QueryArgs&>(args) = base;
  args.filter_table = table;
  args.set = set;
  if (dtype_is_16bit(dtype)) {
    launch_query_labelset_16(args, measure, dtype, stream);
    return;
  }
#define GGNN_LAUNCH_QF(T, LPR, NCH) \
  launch_query_cfg<FilteredLadder<LabelSetFilter>, T, LPR, NCH>(args, use_ps, measure, stream)
  GGNN_DISPATCH_DIST_32_8(dtype, args.D, GGNN_LAUNCH_QF);
#undef GGNN_LAUNCH_QF
}
#endif
#elif defined(GGNN_ROWS_16_TU)
template <class FILT>
void launch_query_filtered_16(const FilteredQueryArgs& args, ggnn_measure measure, ggnn_dtype dtype,
                              hipStream_t stream)
{
#define GGNN_LAUNCH_QF(T, LPR, NCH) \
  launch_query_cfg<FilteredLadder<FILT>, T, LPR, NCH>(args, false, measure, stream)
  GGNN_DISPATCH_DIST_16(dtype, args.D, GGNN_LAUNCH_QF);
#undef GGNN_LAUNCH_QF
}
template void launch_query_filtered_16<TuFilter>(const FilteredQueryArgs&, ggnn_measure, ggnn_dtype,
                                                 hipStream_t);
#elif defined(GGNN_ROWS_I8_TU)
template <class FILT>
void launch_query_filtered_i8(const FilteredQueryArgs& args, ggnn_measure measure, ggnn_dtype dtype,
                              hipStream_t stream)
{
#define GGNN_LAUNCH_QF(T, LPR, NCH) \
  launch_query_cfg<FilteredLadder<FILT>, T, LPR, NCH>(args, false, measure, stream)
  GGNN_DISPATCH_DIST_I8(dtype, args.D, GGNN_LAUNCH_QF);
#undef GGNN_LAUNCH_QF
}
template void launch_query_filtered_i8<TuFilter>(const FilteredQueryArgs&, ggnn_measure, ggnn_dtype,
                                                 hipStream_t);
#else
#ifndef GGNN_LABELS_TU
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
#endif

// base: filled by launch_query (query.hip), filter_bits = the bitset, the table or the label column;
// table: the launch's per-query filters (IdFilter) or query labels (LabelFilter)
template <class FILT>
void launch_query_filtered(const QueryArgs& base, const FilterTable& table, bool use_ps,
                           ggnn_measure measure, ggnn_dtype dtype, hipStream_t stream)
{
  if (table.ids)
    GGNN_REQUIRE(table.words != 0 && table.num_filters != 0, GGNN_INVALID_ARGUMENT,
                 "filter ids need a filter table");
  if constexpr (std::is_same<FILT, LabelFilter>::value) {
    GGNN_REQUIRE(table.query_labels != nullptr && !table.ids, GGNN_INVALID_ARGUMENT,
                 "query labels are missing, or given together with filter ids");
    GGNN_REQUIRE(base.N_base <= kMaxLabeledShardRows, GGNN_UNSUPPORTED,
                 "label filters need shards of at most 2^30 base vectors");
  }
  FilteredQueryArgs args{};
  static_cast<QueryArgs&>(args) = base;
  args.filter_table = table;
  // (null without filter ids, so under labels too)
  ScratchGuard consts{filter_consts_scratch(table, stream), stream};
  if (consts.p)
    args.filter_table.consts = static_cast<const uint32_t*>(consts.p);
  if (dtype_is_16bit(dtype)) {
    launch_query_filtered_16<FILT>(args, measure, dtype, stream);
    return;
  }
  if (dtype == GGNN_I8) {
    launch_query_filtered_i8<FILT>(args, measure, dtype, stream);
    return;
  }
#define GGNN_LAUNCH_QF(T, LPR, NCH) \
  launch_query_cfg<FilteredLadder<FILT>, T, LPR, NCH>(args, use_ps, measure, stream)
  GGNN_DISPATCH_DIST_32_8(dtype, args.D, GGNN_LAUNCH_QF);
#undef GGNN_LAUNCH_QF
}
template void launch_query_filtered<TuFilter>(const QueryArgs&, const FilterTable&, bool, ggnn_measure,
                                              ggnn_dtype, hipStream_t);
#endif

}  // namespace ggnn_amd
