// What the query kernels -- unfiltered (query.hip), under an allowed-id bitset and under label
// filters (query_filtered.hip) -- and their launchers share, next to the wave program itself
// (query_wave_body.inc, query_wave_lds_body.inc).
#pragma once
#include "traversal.hpp"
#include "query_args.hpp"

namespace ggnn_amd {

// (the kernels of PrescreenExact also derive the certificate of exact distances from lossless codes)
template <class PSC, typename BaseT>
GGNN_DEV void load_prescreen(PSC& ps, const QueryArgs& a, const BaseT* qrow)
{
  if constexpr (PSC::enabled)
    ps.template load<PsExact<PSC>::value>(a.ps_codes, a.ps_params, a.ps_Dc,
                                          reinterpret_cast<const float*>(qrow), a.D);
}

// the filter of the wave of query n.  IdFilter: this wave's bitset is the call's, or the row of the
// table its query's filter id names
template <class FILT, class ARGS>
GGNN_DEV FILT wave_filter(const ARGS& a, const uint32_t n)
{
  if constexpr (std::is_same<FILT, LabelMaskFilter>::value)
    return LabelMaskFilter(a.filter_bits, a.filter_bit_offset, a.filter_table, a.mask, n);
  else if constexpr (std::is_same<FILT, LabelRangeFilter>::value)
    return LabelRangeFilter(a.filter_bits, a.filter_bit_offset, a.filter_table, a.range, n);
  else if constexpr (std::is_same<FILT, LabelSetFilter>::value)
    return LabelSetFilter(a.filter_bits, a.filter_bit_offset, a.filter_table, a.set, n);
  else if constexpr (std::is_same<FILT, LabelFilter>::value)
    return LabelFilter(a.filter_bits, a.filter_bit_offset, a.filter_table, n);
  else if constexpr (FILT::enabled)
    return IdFilter{wave_filter_bits(a.filter_bits, a.filter_table, n), a.filter_bit_offset, kEmptyKey,
                    0u};
  else
    return NoIdFilter{};
}

// the bit words of a filter go out in front of a pop's first-read rows: loads return in order, so
// the wait for the rows covers them and the replay finds them there
template <class FILT>
GGNN_DEV void request_filter_words(FILT& idf, const int cand)
{
  if constexpr (FILT::enabled)
    idf.request(cand);
}

// SortedList<.., SEL> of a query kernel: the push with selects and the one-block replay
// (traversal.hpp), except where that form costs the kernel registers it does not have.  Eight
// unfiltered kernels of two-chunk layouts keep the nested `if`: six early-rows kernels with the
// visited ring in LDS (GR = false: hook QUERY_GLOBAL_RING = 0, or a search that can wrap its ring),
// which would go 8-28 bytes into scratch memory, four of them from none, and the two cosine uint8
// tag-set kernels without pre-screen, which spill already and would spill 4 bytes more.
template <typename BaseT, int LPR, int NCH, int R, int MODE, class PSC, int HB, bool EARLY, bool GR,
          class FILT>
constexpr bool query_select_push()
{
  if (R != 1)
    return true;
  // (and where it costs one register at an occupancy step, 64 -> 65 or 80 -> 81: the ring-less
  // early-rows kernels of rows read directly with two bucket registers, the bfloat16 8 x 3 kernel
  // without a hashed set, and the bitset kernels of 16-bit 16 x 4 cosine rows)
  if (!PSC::enabled && !FILT::enabled && LPR == 8 && NCH == 1 && HB == 2 && EARLY && GR)
    return false;
  if (std::is_same_v<BaseT, bf16_t> && !PSC::enabled && !FILT::enabled && LPR == 8 && NCH == 3 &&
      MODE == kL2 && HB == 0 && !EARLY)
    return false;
  if (std::is_same_v<FILT, IdFilter> && sizeof(BaseT) == 2 && !PSC::enabled && LPR == 16 && NCH == 4 &&
      MODE == kCos && HB == 0)
    return false;
  if (FILT::enabled || NCH != 2)
    return true;
  if (std::is_same_v<BaseT, float> && PSC::enabled && EARLY && !GR) {
    if (LPR == 16)
      return HB != 2;
    if (LPR == 8)
      return MODE == kL2 ? !(HB == 1 || HB == 2) : !(HB == 0 || HB == 1);
  }
  if (is_byte_row<BaseT> && !PSC::enabled && !EARLY && !GR && LPR == 8 && MODE == kCos)
    return !is_tag_set(HB);
  return true;
}

// ---- host side: what the launchers of query.hip and query_filtered.hip share ----

// layouts whose first row read is 8 lanes x one 16-byte chunk: Prescreen<8,1> next to any float
// layout, or rows of <= 128 bytes read directly
template <int LPR, int NCH, class PSC>
constexpr bool early_rows_layout()
{
  return PSC::enabled ? (PsLayout<PSC>::lpr == 8 && PsLayout<PSC>::nch == 1) : (LPR == 8 && NCH == 1);
}

// every query kernel runs one wave per query
template <class ARGS>
void launch_wave_per_query(void (*kernel)(ARGS), const ARGS& args, size_t lds_bytes, hipStream_t stream)
{
  hipLaunchKernelGGL(kernel, grid_for(args.Nq), dim3(kWave), lds_bytes, stream, args);
}

template <int R>
using ListRegs = std::integral_constant<int, R>;

// The list of a sorted part that no special form took: R = 1, 2, 4, 8 registers per lane, then
// launch(ListRegs<R>{}) picks the kernel; ListRegs<0> is the LDS list (launch_query_lds_list).
// KQuery <= 1007 / 2031: 16 / 32 list registers per lane.  A push is then 16 / 32 lock-step
// register steps (~12 instructions each) instead of a walk through LDS with a round trip or
// two per 64 entries -- with K this large nearly every evaluated candidate is pushed, so
// the pushes ARE the search (K = 1000 / 4 000 iterations: 24 pushes per pop).  Launched
// without the pre-screen (launch_query_cfg): a loose criteria rejects nothing.
template <class PSC, class LAUNCH>
void launch_query_ladder(const uint32_t sorted, LAUNCH&& launch)
{
  if (sorted <= 64)
    launch(ListRegs<1>{});
  else if (sorted <= 128)
    launch(ListRegs<2>{});
  else if (sorted <= 256)
    launch(ListRegs<4>{});
  else if (sorted <= 512)  // KQuery <= 495: eight list registers per lane
    launch(ListRegs<8>{});
  else if constexpr (!PSC::enabled) {
    if (sorted <= 1024)
      launch(ListRegs<16>{});
    else if (sorted <= 2048)
      launch(ListRegs<32>{});
    else
      launch(ListRegs<0>{});
  }
  else
    launch(ListRegs<0>{});
}

// SORTED > 512: sorted list in LDS (keys [cache] + dists [sorted] + candidate scratch)
template <class ARGS>
void launch_query_lds_list(void (*kernel)(ARGS), const ARGS& args, hipStream_t stream)
{
  const size_t lds_big = (args.cache + args.sorted + WaveLds::extra_ints) * sizeof(int);
  GGNN_REQUIRE(lds_big <= 64 * 1024, GGNN_UNSUPPORTED, "cache too large for one workgroup");
  launch_wave_per_query(kernel, args, lds_big, stream);
}

// measure and pre-screen of a launch: the pre-screened kernels for float rows with a pre-screen copy
// and a sorted part of at most 512.  LADDER::launch<BaseT, LPR, NCH, MODE, PSC>(args, stream) picks
// the kernel (QueryLadder in query.hip, FilteredLadder<FILT> in query_filtered.hip)
template <class LADDER, typename BaseT, int LPR, int NCH, class ARGS>
void launch_query_cfg(const ARGS& args, bool use_ps, ggnn_measure measure, hipStream_t stream)
{
  if constexpr (std::is_same<BaseT, float>::value) {
    if (use_ps && args.sorted <= 512) {
      using PsL2 = typename PsFor<LPR, NCH, kL2>::type;
      using PsCos = typename PsFor<LPR, NCH, kCos>::type;
      if (measure == GGNN_EUCLIDEAN)
        LADDER::template launch<BaseT, LPR, NCH, kL2, PsL2>(args, stream);
      else
        LADDER::template launch<BaseT, LPR, NCH, kCos, PsCos>(args, stream);
      return;
    }
  }
  if (measure == GGNN_EUCLIDEAN)
    LADDER::template launch<BaseT, LPR, NCH, kL2, NoPrescreen>(args, stream);
  else
    LADDER::template launch<BaseT, LPR, NCH, kCos, NoPrescreen>(args, stream);
}

// The launchers of query_filtered.hip, FILT = IdFilter or LabelFilter: each is instantiated by the
// translation unit that holds its kernels (query_filtered / query_labeled, and their _16 units for
// float16 / bfloat16 rows)
template <class FILT>
void launch_query_filtered(const QueryArgs& base, const FilterTable& table, bool use_ps,
                           ggnn_measure measure, ggnn_dtype dtype, hipStream_t stream);
template <class FILT>
void launch_query_filtered_16(const FilteredQueryArgs& args, ggnn_measure measure, ggnn_dtype dtype,
                              hipStream_t stream);
// (and query_filtered_i8 / query_labeled_i8 for int8 rows)
template <class FILT>
void launch_query_filtered_i8(const FilteredQueryArgs& args, ggnn_measure measure, ggnn_dtype dtype,
                              hipStream_t stream);
// Label sets (LabelSetFilter): query_labelset for float32 / uint8 rows and query_labelset_16 for
// float16 / bfloat16 ones; there are no int8 kernels (GGNN_UNSUPPORTED)
void launch_query_labelset(const QueryArgs& base, const FilterTable& table, const LabelSetSpec& set,
                           bool use_ps, ggnn_measure measure, ggnn_dtype dtype, hipStream_t stream);
void launch_query_labelset_16(const LabelSetQueryArgs& args, ggnn_measure measure, ggnn_dtype dtype,
                              hipStream_t stream);
// Label ranges (LabelRangeFilter): query_labelrange / query_labelrange_16, likewise without int8
void launch_query_labelrange(const QueryArgs& base, const FilterTable& table,
                             const LabelRangeSpec& range, bool use_ps, ggnn_measure measure,
                             ggnn_dtype dtype, hipStream_t stream);
void launch_query_labelrange_16(const LabelRangeQueryArgs& args, ggnn_measure measure,
                                ggnn_dtype dtype, hipStream_t stream);
// Label masks (LabelMaskFilter): query_labelmask / query_labelmask_16, likewise without int8
void launch_query_labelmask(const QueryArgs& base, const FilterTable& table,
                            const LabelMaskSpec& mask, bool use_ps, ggnn_measure measure,
                            ggnn_dtype dtype, hipStream_t stream);
void launch_query_labelmask_16(const LabelMaskQueryArgs& args, ggnn_measure measure,
                               ggnn_dtype dtype, hipStream_t stream);

}  // namespace ggnn_amd
