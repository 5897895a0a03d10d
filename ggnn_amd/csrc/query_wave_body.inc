// The wave program of the query kernels, written once: the BODY of query_kernel (query.hip),
// query_filtered_kernel and query_labeled_kernel (query_filtered.hip), included inside each of them.
// Not a header: it expects the kernel's template parameters BaseT, LPR, NCH, R, MODE, PSC, HB, EARLY,
// the names GR (bool) and FILT (NoIdFilter, IdFilter or LabelFilter), and the kernel argument `a`.
// (Text and not a function template: see DESIGN.md 4.9, "One wave program" -- a function body is
// optimised once on its own and once more inside the kernel, and the kernels come out different.)
//
// EARLY (R = 1, KBuild <= 24; traversal.hpp "Early rows"): the first-read rows of a pop's neighbours
// are requested before the pop's bookkeeping and the membership test instead of after them.
// GR (with EARLY and a hashed set): the visited ring in global memory (SortedList<R, HB, true>).
// (fetch_early<.., COUNT = false> -- the sorted part of the cache tested behind the verdicts, for the
// candidates still in the race -- is used by the merge kernel only: measured here on one box,
// round 6, it is 3 % SLOWER on 10 000-query batches (1.186 -> 1.225 ms headline, 7.36 -> 7.57 ms
// lowrank24 at 1.0 / 750: the per-candidate compare chain sits between the verdicts and the float
// rows of a wave that is bound by its own latency) and even on 100 000-query batches.)
//
// FILT (NoIdFilter, IdFilter, LabelFilter; DESIGN.md section 4.9): under a filter one rule is added
// to the search -- the push of a DENIED key never touches the best list [0, BEST): it is queued,
// popped and expanded like any other point, but never reported.  The start points are fetched like
// any candidate, dist[0] is the best ALLOWED distance (+inf until one is found), and unfilled slots
// keep (EMPTY, +inf), written as -1 + offset like the unfiltered kernel's.
  extern __shared__ __attribute__((aligned(16))) int lds_raw[];
  // tag-set form: the visited ring is not in LDS, the candidate scratch follows the sorted keys
  const WaveLds lds(lds_raw, (is_tag_set(HB) || GR) ? a.sorted : a.cache);
  const int lane = threadIdx.x;
  const uint32_t n = block_linear_index();
  if (n >= a.Nq)
    return;

  const BaseT* base = static_cast<const BaseT*>(a.base);
  const BaseT* query = static_cast<const BaseT*>(a.query);

  // query_layer.cu:48-50 (xi from the MAX nn1 distance, quirk Q4)
  const float nn1 = a.nn1_stats[1];
  const float xi = (MODE == kL2) ? (nn1 * nn1) * a.tau * a.tau : nn1 * a.tau;

  // early rows + pre-screen: the float query row waits in LDS behind the wave's other regions (its
  // registers are needed while the requested code rows are live across the membership test)
  using DE = DistEngine<BaseT, LPR, NCH, EARLY && PSC::enabled>;
  DE de;
  de.template load_query<MODE>(
      base, a.D, query + static_cast<size_t>(n) * a.D,
      lds_raw + (is_tag_set(HB) ? tag_set_lds_ints(a.sorted, static_cast<uint32_t>(-HB))
                                : wave_lds_ints(GR ? a.sorted : a.cache, HB)));
  PSC ps;
  // (PrescreenExact: with the certificate of exact distances from lossless codes, traversal.hpp)
  constexpr bool kExactCodes = PsExact<PSC>::value;
  static_assert(!kExactCodes || EARLY, "exact distances from codes: early-rows kernels only");
  load_prescreen(ps, a, query + static_cast<size_t>(n) * a.D);

  SortedList<R, HB, GR, query_select_push<BaseT, LPR, NCH, R, MODE, PSC, HB, EARLY, GR, FILT>()> sl;
  if constexpr (GR && !is_tag_set(HB))
    sl.init_global_ring(a.KQuery, a.sorted, a.cache, xi, lds.known, static_cast<int>(a.vis_slots),
                        a.ring + static_cast<size_t>(n) * (a.cache - a.sorted));
  else if constexpr (is_tag_set(HB))
    sl.init_tagged(a.KQuery, a.sorted, a.cache, xi, lds.known, static_cast<int>(a.vis_slots),
                   a.ring + static_cast<size_t>(n) * (a.cache - a.sorted));
  else
    sl.init(a.KQuery, a.sorted, a.cache, xi, lds.known, static_cast<int>(a.vis_slots));
  FILT idf = wave_filter<FILT>(a, n);

  uint32_t cnt_dist = 0, cnt_pop = 0;
  uint2 cnt_rows = make_uint2(0u, 0u);

  // fetch_unfiltered(d_starting_points, nullptr, S), query_layer.cu:54-55
  for (uint32_t i = 0; i < a.num_start; i += kKBlock) {
    const int cand = (lane < (int)kKBlock && i + lane < a.num_start) ? a.start[i + lane]
                                                                      : kEmptyKey;
    cnt_dist += fetch<MODE, false>(sl, de, lds, cand, nullptr, ps, cnt_rows, NoHook{}, idf);
  }

  // Speculation that hides one of the dependent memory latencies per pop: while the pre-screen
  // and distance phases of this pop run, the graph row of the current queue head is loaded; if
  // that key is still the head at the next pop (no closer candidate was pushed: 73 % of the pops)
  // the row is there.  The load is issued from fetch()'s after-filter hook, i.e. after the wait
  // for this pop's own graph row -- issued before it, the two waits merge into one vmcnt(0).
  int spec_key = kEmptyKey, spec_row = kEmptyKey;
#ifdef GGNN_PHASE_CYCLES
  phase_begin();
#endif
  for (uint32_t ite = 0; ite < a.max_iters; ++ite) {
    // query_layer.cu:58-63
    const float d0 = sl.dist_at(0);
    sl.xi = (MODE == kL2) ? fminf(xi, d0 * a.tau * a.tau) : fminf(xi, d0 * a.tau);
    if constexpr (EARLY) {
      // the same pop, reordered: decide -> graph row (speculated, else loaded now) -> request the
      // neighbours' first-read rows -> bookkeeping of the pop and membership test under that latency
      const int anchor = sl.peek(sl.criteria());
      if (anchor == kEmptyKey)
        break;
      ++cnt_pop;
      const bool in_row = lane < static_cast<int>(a.KBuild);  // KBuild <= 24 (host)
      int cand;
      if (anchor == spec_key)
        cand = in_row ? spec_row : kEmptyKey;
      else if constexpr (kExactCodes && !FILT::enabled) {
        // (the row's address as a scalar base + lane offset: the per-lane 64-bit address of the form
        // below is loop invariant, and the unfiltered two-phase kernels have no register pair left for it --
        // it went to scratch and its reload put a vmcnt(0) in front of this load)
        const uint64_t rp = reinterpret_cast<uint64_t>(
            a.graph0 + static_cast<size_t>(static_cast<uint32_t>(anchor)) * a.KBuild);
        // (a pointer made from an integer is a generic one -- a flat load, which also counts as an
        // LDS access and is waited for with lgkmcnt(0): the address space is stated)
        using GlobalRow = const __attribute__((address_space(1))) int32_t*;
        const GlobalRow row = reinterpret_cast<GlobalRow>(
            (static_cast<uint64_t>(static_cast<uint32_t>(uni(static_cast<int>(rp >> 32)))) << 32) |
            static_cast<uint32_t>(uni(static_cast<int>(rp))));
        cand = in_row ? row[lane] : kEmptyKey;
      }
      else
        cand = in_row ? a.graph0[static_cast<size_t>(static_cast<uint32_t>(anchor)) * a.KBuild + lane]
                      : kEmptyKey;
      // The speculative row is loaded UNCONDITIONALLY (an empty queue reads row 0, lanes past the
      // row its last entry; masked where the row is consumed): a load under a branch leaves the
      // two paths with different numbers of loads in flight, and the compiler then waits for the
      // requested code rows with vmcnt(0) -- i.e. also for this load, issued a moment earlier
      // (found in the ISA; the wait is vmcnt(1) now and the row travels during the verdicts).
      auto prefetch_head_row = [&]() {
        spec_key = sl.key_at(sl.BEST);
        spec_row = a.graph0[static_cast<size_t>(static_cast<uint32_t>(max(spec_key, 0))) * a.KBuild +
                            min(lane, static_cast<int>(a.KBuild) - 1)];
        __builtin_amdgcn_s_setprio(1);  // (the membership test is done: see below)
      };
      // Wave priority.  What a wave does WHILE its requested rows travel (bookkeeping of the pop,
      // membership test) is free as long as it finishes before they arrive; everything else --
      // verdicts -> float rows -> distances -> replay -> peek -> graph row -> the next requests --
      // is on the way to the wave's next memory request.  The seven waves of a SIMD compete for
      // its issue slots (VALU issue ~0.7 busy), so the first kind runs at priority 0 and yields
      // to waves of the second kind (priority 1): a pure scheduling hint, results unchanged.
      // Same box, alternating runs: 1M x 128 f32 1.234-1.242 -> 1.209-1.210 ms, uint8 0.883-0.885
      // -> 0.860-0.870, 12.5M x 96 2.014 -> 1.931 ms, 100k-query batches -1.5 ... -2.6 %.  (The
      // inverse assignment: +1 %; only the bookkeeping at low priority: +1 %; a third level for
      // peek -> requests: -0.3 %, inside the noise.)
      request_filter_words(idf, cand);  // (a filter's words go out in front of the rows)
      if constexpr (PSC::enabled) {
        EarlyRows<PSC> er;
        er.issue(ps, cand);
        __builtin_amdgcn_s_setprio(0);
        sl.pop_commit(anchor, lds.known);
        cnt_dist += fetch_early<MODE, true, kExactCodes>(sl, de, lds, cand, er, ps, cnt_rows,
                                                  prefetch_head_row, nullptr, idf);
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
    GGNN_TICK(0);  // pop
    if (anchor == kEmptyKey)
      break;
    ++cnt_pop;
    // query_layer.cu:69-77
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

#ifdef GGNN_PHASE_CYCLES
  phase_end();
#endif
  // write_best + dists, query_layer.cu:81-90 (EMPTY becomes -1 + offset, as in the reference)
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
