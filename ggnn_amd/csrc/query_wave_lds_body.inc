// The wave program of the query kernels with the LDS-resident list (SORTED > 2048, or > 512 with the
// pre-screen): the body of query_kernel_lds, query_filtered_kernel_lds and query_labeled_kernel_lds,
// included inside each of them as query_wave_body.inc is.  Expects BaseT, LPR, NCH, MODE, PSC, FILT, `a`.
  extern __shared__ __attribute__((aligned(16))) int lds_raw[];
  // [cache keys][sorted dists][ckeys 32 | cd0 32 | cd1 32]
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
  load_prescreen(ps, a, query + static_cast<size_t>(n) * a.D);
  LdsList sl;
  sl.init(a.KQuery, a.sorted, a.cache, xi, keys, dists);
  FILT idf = wave_filter<FILT>(a, n);
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
