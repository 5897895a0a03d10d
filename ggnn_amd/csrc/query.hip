// query kernel: best-first graph traversal, one wave64 per query.
// Reference: QueryKernel::operator(), src/ggnn/query/query_layer.cu:39-97; host sizing
// QueryKernelsImpl::query, src/ggnn/query/query_kernels.cu:50-186.
#include <algorithm>

#include "query_wave.hpp"

namespace ggnn_amd {

// occupancy target of the common instantiations (one register of list per lane, narrow rows):
// a tuning knob, 1 = leave it to the compiler
#ifndef GGNN_QUERY_WAVES
#define GGNN_QUERY_WAVES 7
#endif
// early rows: the requested code rows (15 registers) are live across the pop's bookkeeping and the
// membership test; with the float query row in LDS (DistEngine<.., QL>) the kernels still fit the
// 72 registers of 7 waves.  The global-ring variants spill 9-15 registers there: 80 (6 waves; they
// exist for caches whose LDS ring would allow fewer)
#ifndef GGNN_QUERY_WAVES_GR
#define GGNN_QUERY_WAVES_GR 7
#endif

// the wave program: query_wave_body.inc (EARLY, GR: there)
template <typename BaseT, int LPR, int NCH, int R, int MODE, class PSC, int HB = 0, bool EARLY = false,
          bool GR = false>
__global__ void __launch_bounds__(kWave) __attribute__((
    amdgpu_waves_per_eu((R == 1 && NCH <= 3) ? (GR ? GGNN_QUERY_WAVES_GR : GGNN_QUERY_WAVES) : 1)))
query_kernel(const QueryArgs a)
{
  using FILT = NoIdFilter;
#include "query_wave_body.inc"
}

// Same kernel with the LDS-resident list (SORTED > 512, i.e. KQuery > 495).
template <typename BaseT, int LPR, int NCH, int MODE, class PSC>
__global__ void __launch_bounds__(kWave) query_kernel_lds(const QueryArgs a)
{
  using FILT = NoIdFilter;
#include "query_wave_lds_body.inc"
}

#ifndef GGNN_ROWS_EXTRA_TU
void query_sizing(uint32_t D, uint32_t k_query, uint32_t max_iterations, uint32_t* cache_size,
                  uint32_t* sorted_size)
{
  // query_kernels.cu:55-110
  GGNN_REQUIRE(k_query >= 1 && k_query <= 6000, GGNN_INVALID_ARGUMENT, "KQuery must be in [1, 6000]");
  GGNN_REQUIRE(max_iterations <= 8192, GGNN_INVALID_ARGUMENT, "max_iterations must be <= 8192");
  GGNN_REQUIRE(D >= 1 && D <= 4096, GGNN_INVALID_ARGUMENT, "D must be in [1, 4096]");
  const uint32_t required_sorted = next_multiple32(k_query + 1 + 16);
  const uint32_t cache =
      std::max(std::max(256u, required_sorted + 32u), bit_ceil_u32(max_iterations));
  GGNN_REQUIRE(cache <= 8192, GGNN_INVALID_ARGUMENT, "cache size exceeds 8192");
  *cache_size = cache;
  *sorted_size = std::max(cache < 512u ? 64u : 32u, required_sorted);
}
#endif

// the kernel of one row layout, measure and pre-screen (launch_query_cfg, query_wave.hpp); comments
// elsewhere know this function by its earlier name, launch_query_r
struct QueryLadder {
  template <typename BaseT, int LPR, int NCH, int MODE, class PSC>
  static void launch(const QueryArgs& args, hipStream_t stream)
  {
    const uint32_t sorted = args.sorted;
    const size_t lds = wave_lds_bytes(args.cache);
    const auto go = [&](void (*kernel)(QueryArgs), size_t lds_bytes) {
      launch_wave_per_query(kernel, args, lds_bytes, stream);
    };
    // one list register per lane: the visited ring is mirrored in a hash set (traversal.hpp) when it
    // is short enough for one or two bucket registers
    // (not for the two-chunk float layouts without pre-screen: four rows of two chunks in flight leave
    // no register for it at 7 waves per SIMD -- measured 2.73 vs 2.54 ms with the spills)
    const bool fits = PSC::enabled || NCH == 1;
    const uint32_t hb = (sorted <= 64 && fits) ? vis_hash_regs(args.cache - sorted) : 0;
    // early rows (traversal.hpp): graph rows of <= 24 neighbours, first row read 8 lanes x 16 bytes
    // (hook QUERY_EARLY = 0: the round-1..4 order, A/B and test hook)
    if constexpr (early_rows_layout<LPR, NCH, PSC>()) {
      // Exact distances from lossless codes (traversal.hpp): when the caller knows the base's flag
      // the ring-less kernels are taken in their two-phase variant PSX.  Every other launch -- a
      // fractional base, the operator seam without the flag, hook PS_EXACT = 0 -- runs the kernels
      // of PSC, the code objects they always were.  (The variants that keep a visited ring in LDS
      // stay with PSC: at 7 waves per SIMD both phases would put 2-5 registers in scratch there.)
      using PSX = typename ExactOf<PSC>::type;
      const bool exact = args.ps_lossless != 0 && !std::is_same<PSX, PSC>::value;
      // the tag set of long rings (513..2016 iterations): early rows only when the search cannot
      // wrap its ring -- then the set is ring-less too (no store per pop: a store in flight turns
      // every wait for the requested rows into vmcnt(0)); otherwise the round-4 order below
      const bool tagged = hb == 0 && fits && args.ring && (args.tag_bits == 8 || args.tag_bits == 9);
      const bool tagged_ringless = tagged && args.max_iters <= args.cache - sorted &&
                                   hook(kHookQueryGlobalRing) != 0;
      if (args.KBuild <= 8 * kEarlySteps && sorted <= 64 && tagged_ringless &&
          hook(kHookQueryEarly) != 0) {
        const size_t tag_lds = tag_set_lds_bytes(sorted, args.cache - sorted) +
                               DistEngine<BaseT, LPR, NCH, PSC::enabled>::kQueryLdsBytes;
        if (args.tag_bits == 8)
          go(exact ? query_kernel<BaseT, LPR, NCH, 1, MODE, PSX, -8, true, true>
                   : query_kernel<BaseT, LPR, NCH, 1, MODE, PSC, -8, true, true>, tag_lds);
        else
          go(exact ? query_kernel<BaseT, LPR, NCH, 1, MODE, PSX, -9, true, true>
                   : query_kernel<BaseT, LPR, NCH, 1, MODE, PSC, -9, true, true>, tag_lds);
        return;
      }
      if (args.KBuild <= 8 * kEarlySteps && sorted <= 64 && !tagged && hook(kHookQueryEarly) != 0) {
        // (hook QUERY_LDS_PAD: extra bytes of LDS per wave -- occupancy experiments without a rebuild)
        const size_t qrow = DistEngine<BaseT, LPR, NCH, PSC::enabled>::kQueryLdsBytes +
                            static_cast<size_t>(std::clamp<int64_t>(hook(kHookQueryLdsPad), 0, 32768));
        // a search that cannot wrap its visited ring needs no ring: buckets + stash ARE the set
        // (SortedList<R, HB, true>; launch_query allocates the overflow lists then)
        const bool ringless = args.ring && args.tag_bits == 0;
        if (hb == 1 && ringless)
          go(exact ? query_kernel<BaseT, LPR, NCH, 1, MODE, PSX, 1, true, true>
                   : query_kernel<BaseT, LPR, NCH, 1, MODE, PSC, 1, true, true>,
             wave_lds_bytes(sorted, 1) + qrow);
        else if (hb == 1)
          go(query_kernel<BaseT, LPR, NCH, 1, MODE, PSC, 1, true>,
             wave_lds_bytes(args.cache, 1) + qrow);
        else if (hb == 2 && ringless)
          go(exact ? query_kernel<BaseT, LPR, NCH, 1, MODE, PSX, 2, true, true>
                   : query_kernel<BaseT, LPR, NCH, 1, MODE, PSC, 2, true, true>,
             wave_lds_bytes(sorted, 2) + qrow);
        else if (hb == 2)
          go(query_kernel<BaseT, LPR, NCH, 1, MODE, PSC, 2, true>,
             wave_lds_bytes(args.cache, 2) + qrow);
        else
          go(query_kernel<BaseT, LPR, NCH, 1, MODE, PSC, 0, true>, lds + qrow);
        return;
      }
    }
    // long rings (searches of 1000-2000 iterations): tag set + ring in global memory (traversal.hpp)
    if (hb == 0 && sorted <= 64 && fits && args.ring && args.tag_bits == 8)
      go(query_kernel<BaseT, LPR, NCH, 1, MODE, PSC, -8>,
         tag_set_lds_bytes(sorted, args.cache - sorted));
    else if (hb == 0 && sorted <= 64 && fits && args.ring && args.tag_bits == 9)
      go(query_kernel<BaseT, LPR, NCH, 1, MODE, PSC, -9>,
         tag_set_lds_bytes(sorted, args.cache - sorted));
    else if (hb == 1)
#ifdef GGNN_PHASE_CYCLES
      go(query_kernel<BaseT, LPR, NCH, 1, MODE, PSC, 1>, 16384 + 256);
#else
      go(query_kernel<BaseT, LPR, NCH, 1, MODE, PSC, 1>, wave_lds_bytes(args.cache, 1));
#endif
    else if (hb == 2)
      go(query_kernel<BaseT, LPR, NCH, 1, MODE, PSC, 2>, wave_lds_bytes(args.cache, 2));
    else
      launch_query_ladder<PSC>(sorted, [&](auto regs) {
        constexpr int R = decltype(regs)::value;
        if constexpr (R == 0)
          launch_query_lds_list(query_kernel_lds<BaseT, LPR, NCH, MODE, PSC>, args, stream);
        else
          go(query_kernel<BaseT, LPR, NCH, R, MODE, PSC>, lds);
      });
  }
};

#ifndef GGNN_ROWS_EXTRA_TU
// float16 / bfloat16 rows (no pre-screen): query_16.hip
void launch_query_16(const QueryArgs& args, ggnn_measure measure, ggnn_dtype dtype,
                     hipStream_t stream);
// int8 rows (no pre-screen): query_i8.hip
void launch_query_i8(const QueryArgs& args, ggnn_measure measure, ggnn_dtype dtype,
                     hipStream_t stream);

void launch_query(const QueryLaunch& a, hipStream_t stream)
{
  if (a.Nq == 0)
    return;
  check_vector_layout(a.base, a.D, a.dtype);
  check_vector_layout(a.query, a.D, a.dtype);
  QueryArgs args{};
  args.base = a.base;
  args.query = a.query;
  args.graph0 = a.graph0;
  args.start = a.start;
  args.nn1_stats = a.nn1_stats;
  args.ids = a.ids;
  args.dists = a.dists;
  args.n_dist = a.n_dist;
  args.n_pop = a.n_pop;
  args.n_rows = reinterpret_cast<uint2*>(a.n_rows);
  args.D = a.D;
  args.Nq = a.Nq;
  args.N_base = a.N_base;
  args.KBuild = a.KBuild;
  args.num_start = a.num_start;
  args.KQuery = a.k_query;
  query_sizing(a.D, a.k_query, a.max_iterations, &args.cache, &args.sorted);
  args.max_iters = a.max_iterations;
  args.shards_per_gpu = a.shards_per_gpu;
  args.on_gpu_shard = a.on_gpu_shard;
  args.tau = a.tau_query;
  args.vis_slots = vis_slots_hook();
  // long rings: per-query visited rings as stream-ordered scratch of this launch
  const uint32_t vis = args.cache - args.sorted;
  const bool use_ps = a.ps_codes && a.ps_params && a.dtype == GGNN_F32;
  // what launch_query_cfg / QueryLadder will pick for this shape, decided HERE so that the
  // per-query scratch below is only allocated for kernels that use it (round-5 advisor finding:
  // Nq x ring x 4 bytes -- 77 MB per 100k-query launch -- also went to layouts that keep the ring
  // in LDS): the early-rows layouts (first row read 8 lanes x 16 bytes: Prescreen<8, 1> next to
  // every float layout up to 128 dimensions, or rows of <= 128 bytes read directly) and the
  // layouts that carry a hashed / tag set at all (pre-screened, or one chunk per lane)
  const DistConfig dc = pick_dist_config(a.D, a.dtype);
  const bool ps_kernel = use_ps && args.sorted <= 512;
  const bool early_shape = ps_kernel ? !((dc.lpr == 16 && dc.nch == 4) || dc.lpr == 64)
                                     : (dc.lpr == 8 && dc.nch == 1);
  const bool set_shape = ps_kernel || dc.nch == 1;
  // ring-less hashed set (QueryLadder: early rows) when the search cannot wrap its ring: the
  // overflow lists of the launch (hook QUERY_GLOBAL_RING = 0: ring in LDS, A/B and test hook)
  const bool global_ring = args.sorted <= 64 && vis_hash_regs(vis) != 0 && a.max_iterations <= vis &&
                           a.KBuild <= 8 * kEarlySteps && hook(kHookQueryEarly) != 0 &&
                           hook(kHookQueryGlobalRing) != 0 && early_shape && set_shape;
  // (the filtered kernels keep their ring in LDS: no scratch)
  if (!a.filter_bits && !a.label_sets.labels && !a.label_ranges.labels && !a.label_masks.labels &&
      (global_ring || (args.sorted <= 64 && set_shape && tag_set_usable(vis, a.N_base) &&
                       hook(kHookVisTagSet) != 0))) {
    args.tag_bits = global_ring ? 0 : tag_set_bucket_bits(vis);
    try {
      args.ring = static_cast<int32_t*>(
          scratch_alloc(static_cast<size_t>(a.Nq) * vis * sizeof(int32_t), stream));
    }
    catch (const Error& e) {
      // no room for the rings (Nq x ring x 4 bytes): the ring-scan kernel needs none
      if (e.status != GGNN_OUT_OF_MEMORY)
        throw;
      (void)hipGetLastError();
      args.ring = nullptr;
    }
  }
  ScratchGuard ring_guard{args.ring, stream};
  if (use_ps) {
    GGNN_REQUIRE(a.ps_Dc == prescreen_code_dim(a.D), GGNN_INVALID_ARGUMENT,
                 "pre-screen code rows must have prescreen_code_dim(D) bytes");
    GGNN_REQUIRE((reinterpret_cast<uintptr_t>(a.ps_codes) & 15u) == 0 &&
                     (reinterpret_cast<uintptr_t>(a.ps_params) & 15u) == 0,
                 GGNN_INVALID_ARGUMENT, "pre-screen buffers must be 16-byte aligned");
    args.ps_codes = a.ps_codes;
    args.ps_params = a.ps_params;
    args.ps_Dc = a.ps_Dc;
    args.ps_lossless = (a.ps_lossless && a.measure == GGNN_EUCLIDEAN && hook(kHookPsExact) != 0) ? 1u : 0u;
  }

  if (a.label_masks.labels) {
    // the label's tag bits under one of up to 2 clauses per query, with an optional filter id
    // (query_labelmask.hip)
    GGNN_REQUIRE(!a.label_sets.labels && !a.label_ranges.labels, GGNN_INVALID_ARGUMENT,
                 "label masks cannot be combined with label sets or label ranges in one launch");
    args.filter_bits = a.filter_bits;
    args.filter_bit_offset = a.filter_bit_offset;
    launch_query_labelmask(args, a.filter_table, a.label_masks, use_ps, a.measure, a.dtype, stream);
  }
  else if (a.label_ranges.labels) {
    // the label in one of up to 4 intervals per query, with an optional filter id
    // (query_labelrange.hip)
    GGNN_REQUIRE(!a.label_sets.labels, GGNN_INVALID_ARGUMENT,
                 "label ranges and label sets cannot be combined in one launch");
    args.filter_bits = a.filter_bits;
    args.filter_bit_offset = a.filter_bit_offset;
    launch_query_labelrange(args, a.filter_table, a.label_ranges, use_ps, a.measure, a.dtype, stream);
  }
  else if (a.label_sets.labels) {
    // any of a set of labels per query, with an optional filter id (query_labelset.hip)
    args.filter_bits = a.filter_bits;
    args.filter_bit_offset = a.filter_bit_offset;
    launch_query_labelset(args, a.filter_table, a.label_sets, use_ps, a.measure, a.dtype, stream);
  }
  else if (a.filter_bits) {
    args.filter_bits = a.filter_bits;
    args.filter_bit_offset = a.filter_bit_offset;
    // restricted to an allowed-id bitset (query_filtered.hip) or to a label (query_labeled.hip)
    if (a.filter_table.query_labels)
      launch_query_filtered<LabelFilter>(args, a.filter_table, use_ps, a.measure, a.dtype, stream);
    else
      launch_query_filtered<IdFilter>(args, a.filter_table, use_ps, a.measure, a.dtype, stream);
  }
  else if (dtype_is_16bit(a.dtype)) {
    launch_query_16(args, a.measure, a.dtype, stream);
  }
  else if (a.dtype == GGNN_I8) {
    launch_query_i8(args, a.measure, a.dtype, stream);
  }
  else {
#define GGNN_LAUNCH_QUERY(T, LPR, NCH) \
  launch_query_cfg<QueryLadder, T, LPR, NCH>(args, use_ps, a.measure, stream)
    GGNN_DISPATCH_DIST_32_8(a.dtype, a.D, GGNN_LAUNCH_QUERY);
#undef GGNN_LAUNCH_QUERY
  }
  GGNN_HIP_CHECK(hipGetLastError());
}

#ifdef GGNN_PHASE_CYCLES
extern "C" int ggnn_debug_phase_cycles(unsigned long long* out16, int reset)
{
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_phase_acc), 16 * sizeof(unsigned long long)) != hipSuccess)
    return 1;
  if (reset) {
    unsigned long long z[16] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase_acc), z, sizeof(z)) != hipSuccess)
      return 1;
  }
  return 0;
}
#endif

#elif defined(GGNN_ROWS_16_TU)

void launch_query_16(const QueryArgs& args, ggnn_measure measure, ggnn_dtype dtype,
                     hipStream_t stream)
{
#define GGNN_LAUNCH_QUERY(T, LPR, NCH) \
  launch_query_cfg<QueryLadder, T, LPR, NCH>(args, false, measure, stream)
  GGNN_DISPATCH_DIST_16(dtype, args.D, GGNN_LAUNCH_QUERY);
#undef GGNN_LAUNCH_QUERY
}

#else  // GGNN_ROWS_I8_TU

void launch_query_i8(const QueryArgs& args, ggnn_measure measure, ggnn_dtype dtype,
                     hipStream_t stream)
{
#define GGNN_LAUNCH_QUERY(T, LPR, NCH) \
  launch_query_cfg<QueryLadder, T, LPR, NCH>(args, false, measure, stream)
  GGNN_DISPATCH_DIST_I8(dtype, args.D, GGNN_LAUNCH_QUERY);
#undef GGNN_LAUNCH_QUERY
}

#endif  // GGNN_ROWS_EXTRA_TU

}  // namespace ggnn_amd
