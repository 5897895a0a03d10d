// Engine behind the C-ABI, part "query": query drivers: shard loop of one GPU, blocking / split / asynchronous batches, bf_query
// (gpu_instance.cu:626-790, ggnn.cu:278-330).
// The handle is declared in engine.hpp.
#include "engine.hpp"

void ggnn_handle::check_query(uint64_t Nq, uint32_t D, ggnn_dtype dtype, const void* q) const
{
  GGNN_REQUIRE(dtype == base_dtype, GGNN_INVALID_ARGUMENT,
               "query data type does not match base data type");
  GGNN_REQUIRE(D == base_D, GGNN_INVALID_ARGUMENT, "query dimension does not match the base");
  GGNN_REQUIRE(Nq < 0xffffffffull, GGNN_INVALID_ARGUMENT, "too many queries");
  GGNN_REQUIRE(!Nq || q != nullptr, GGNN_INVALID_ARGUMENT, "query pointer is null");
}

// query.referenceOnGPU (gpu_instance.cu:638-641): the full query set on ctx's GPU
ggnn_handle::Staged ggnn_handle::stage_query(DeviceCtx& ctx, const void* q, uint64_t Nq, uint32_t D, ggnn_dtype dtype,
                   ggnn_location loc, int q_gpu)
{
  Staged s;
  if (!Nq)
    return s;
  const size_t es = dtype_size(dtype);
  const bool padded = pad_D != base_D;
  if (loc == GGNN_GPU && q_gpu == ctx.device && !padded &&
      (reinterpret_cast<uintptr_t>(q) & 15u) == 0) {
    s.ptr = q;
    return s;
  }
  const hipMemcpyKind kind = loc == GGNN_GPU ? hipMemcpyDefault : hipMemcpyHostToDevice;
  s.owned.alloc(Nq * pad_D * es);
  if (padded) {
    GGNN_HIP_CHECK(hipMemsetAsync(s.owned.p, 0, s.owned.bytes, ctx.stream));
    GGNN_HIP_CHECK(
        hipMemcpy2DAsync(s.owned.p, pad_D * es, q, D * es, D * es, Nq, kind, ctx.stream));
  }
  else
    GGNN_HIP_CHECK(hipMemcpyAsync(s.owned.p, q, s.owned.bytes, kind, ctx.stream));
  s.ptr = s.owned.p;
  return s;
}

// the one place that fills a shard's QueryLaunch (the caller that collects counters adds them)
QueryLaunch ggnn_handle::shard_launch(const DeviceCtx& ctx, uint32_t si, const QueryRequest& r,
                                      const void* d_query, uint32_t nq, int32_t* d_ids,
                                      float* d_dists, bool use_prescreen,
                                      const DeviceFilter& df) const
{
  const Shard& sh = ctx.shards[si];
  QueryLaunch ql{shard_base(ctx, si),
                 d_query,
                 base_dtype,
                 cfg.N,
                 pad_D,
                 nq,
                 sh.graph,
                 cfg.KBuild,
                 sh.translation + cfg.STs_offsets[kLayers - 1],
                 cfg.S,
                 sh.nn1_stats,
                 r.k,
                 r.tau,
                 r.max_iterations,
                 r.measure,
                 shards_per_gpu,
                 si,
                 d_ids,
                 d_dists,
                 nullptr,
                 nullptr};
  if (use_prescreen) {
    ql.ps_codes = sh.ps_codes.as<uint8_t>();
    ql.ps_params = sh.ps_params.as<float>();
    ql.ps_Dc = prescreen_code_dim(pad_D);
    ql.ps_lossless = sh.ps_lossless;
  }
  ql.filter_bits = df.bits;
  ql.filter_bit_offset = sh.global_id * cfg.N;
  ql.filter_table = df.table;
  ql.label_sets = df.set;
  ql.label_ranges = df.ranges;
  ql.label_masks = df.masks;
  return ql;
}

// GPUInstance::query, gpu_instance.cu:626-743: all shards of one GPU into d_ids/d_dists
// [Nq, K * shards_per_gpu]
void ggnn_handle::query_device(DeviceCtx& ctx, const QueryRequest& r, const void* d_query,
                               int32_t* d_ids, float* d_dists, const QueryFilter& filter)
{
  hipStream_t stream = ctx.stream;
  const uint32_t spg = shards_per_gpu;
  const uint32_t nq = static_cast<uint32_t>(r.Nq);
  const ggnn_measure measure = r.measure;
  const DeviceFilter df = resolve_filter(ctx, filter, DeviceCtx::kBlockingLane);
  DeviceBuffer c_dist, c_pop, c_rows;
  if (collect_counters) {
    c_dist.alloc(static_cast<size_t>(nq) * 4);
    c_pop.alloc(static_cast<size_t>(nq) * 4);
    c_rows.alloc(static_cast<size_t>(nq) * 8);
  }
  ctx.query_ms = 0.f;
  ctx.n_dist = ctx.n_pop = ctx.n_float_rows = ctx.n_code_rows = 0;
  std::vector<uint32_t> h_cnt;
  // Several resident shards: one launch per shard, spread over a few streams and NOT separated
  // by host synchronisation, so the under-occupied tail of a 10k-wave launch is filled by the
  // next shard's waves (hook SHARD_OVERLAP = 0: one launch at a time, as for the work counters).
  const bool overlap = spg > 1 && !collect_counters && hook(kHookShardOverlap) != 0 && !ctx.swap;
  if (overlap) {
    for (uint32_t si = 0; si < spg; ++si)
      (void)ensure_prescreen(ctx, si, measure);  // may code a shard (synchronises): do it first
    ctx.ensure_shard_streams();
    GGNN_HIP_CHECK(hipEventRecord(ctx.ev_ready, stream));  // query staged, earlier work done
    for (int i = 0; i < DeviceCtx::kShardStreams; ++i)
      GGNN_HIP_CHECK(hipStreamWaitEvent(ctx.shard_stream[i], ctx.ev_ready, 0));
    GGNN_HIP_CHECK(hipEventRecord(ctx.ev_a, stream));
  }
  for (uint32_t si = 0; si < spg; ++si) {
    if (ctx.swap) {
      // out-of-core shards (swapInPart / waitForPart, gpu_instance.cu:661-688): this shard is
      // in its slot (uploaded as the previous one's prefetch, or right now), the next one
      // starts travelling on the copy stream while this one is searched
      SwapState& sw = *ctx.swap;
      acquire_shard(ctx, si, sw.io);
      GGNN_HIP_CHECK(hipStreamWaitEvent(stream, sw.uploaded[si % sw.slots], 0));
      if (si + 1 < spg && sw.slots > 1)
        acquire_shard(ctx, si + 1, sw.io);
    }
    const bool use_ps = ensure_prescreen(ctx, si, measure);
    const Shard& sh = ctx.shards[si];
    QueryLaunch ql = shard_launch(ctx, si, r, d_query, nq, d_ids, d_dists, use_ps, df);
    ql.n_dist = c_dist.as<uint32_t>();
    ql.n_pop = c_pop.as<uint32_t>();
    ql.n_rows = c_rows.as<uint32_t>();
    if (overlap) {
      launch_query(ql, ctx.shard_stream[si % DeviceCtx::kShardStreams]);
      continue;
    }
    EventTimer timer(stream, ctx.ev_a, ctx.ev_b);
    launch_query(ql, stream);
    if (ctx.swap)
      shard_consumed(ctx, si, stream);
    const float ms = timer.stop();
    ctx.query_ms += ms;
    GGNN_LOG(0, "[GPU: %d] query part %u => ms: %.3f [%u points query -> %.3f us/point]",
             ctx.device, sh.global_id, ms, nq, ms * 1000.f / static_cast<float>(nq));
    if (collect_counters) {
      h_cnt.resize(nq);
      GGNN_HIP_CHECK(hipMemcpy(h_cnt.data(), c_dist.p, nq * 4ull, hipMemcpyDeviceToHost));
      for (uint32_t v : h_cnt)
        ctx.n_dist += v;
      GGNN_HIP_CHECK(hipMemcpy(h_cnt.data(), c_pop.p, nq * 4ull, hipMemcpyDeviceToHost));
      for (uint32_t v : h_cnt)
        ctx.n_pop += v;
      h_cnt.resize(2ull * nq);
      GGNN_HIP_CHECK(hipMemcpy(h_cnt.data(), c_rows.p, nq * 8ull, hipMemcpyDeviceToHost));
      for (uint32_t i = 0; i < nq; ++i) {
        ctx.n_float_rows += h_cnt[2 * i];
        ctx.n_code_rows += h_cnt[2 * i + 1];
      }
    }
  }
  if (overlap) {
    // join: the main stream continues (timing event, row sort) after every shard stream
    for (int i = 0; i < DeviceCtx::kShardStreams; ++i) {
      GGNN_HIP_CHECK(hipEventRecord(ctx.shard_done[i], ctx.shard_stream[i]));
      GGNN_HIP_CHECK(hipStreamWaitEvent(stream, ctx.shard_done[i], 0));
    }
    GGNN_HIP_CHECK(hipEventRecord(ctx.ev_b, stream));
  }
  if (spg > 1)
    launch_sort_shard_results(nq, r.k * spg, d_ids, d_dists, stream);
  GGNN_HIP_CHECK(hipStreamSynchronize(stream));
  if (overlap) {
    GGNN_HIP_CHECK(hipEventElapsedTime(&ctx.query_ms, ctx.ev_a, ctx.ev_b));
    GGNN_LOG(0, "[GPU: %d] query parts %u..%u overlapped => ms: %.3f [%u points query]",
             ctx.device, ctx.first_shard, ctx.first_shard + spg - 1, ctx.query_ms, nq);
  }
}

// GGNNImpl::queryImpl, ggnn.cu:278-330
void ggnn_handle::query(const QueryRequest& r, const QueryFilter& filter)
{
  GGNN_REQUIRE(has_graph(), GGNN_INVALID_STATE, "There is no graph to query.");
  check_query(r.Nq, r.D, r.dtype, r.q);
  const bool direct = (r.out_loc == GGNN_GPU);
  GGNN_REQUIRE(!(direct && devs.size() > 1), GGNN_INVALID_STATE,
               "Returning query results on GPU is only possible when using a single GPU.");
  query_ms = 0.f;
  last_n_dist = last_n_pop = last_float_rows = last_code_rows = 0;
  if (!r.Nq)
    return;
  const uint32_t nq = static_cast<uint32_t>(r.Nq);
  const uint32_t k_query = r.k;
  int32_t* const ids_out = r.ids_out;
  float* const dists_out = r.dists_out;
  const size_t row = static_cast<size_t>(k_query) * shards_per_gpu;
  const size_t part = nq * row;

  // Several GPUs: a blocking batch is searched as TWO half-batches in flight, so that the
  // all-gather, the slice merges and the result copies of the first half overlap the search of
  // the second (the step is latency-bound: one ~2 ms kernel per GPU, then the exchange) -- the
  // caller gets the pipelining of query_async without having to use it.  Hook QUERY_SPLIT = 0
  // switches it off, 1 forces it from 2 queries on (tests).
  last_query_parts = 1;
  {
    const int64_t split = hook(kHookQuerySplit);
    const bool several = devs.size() > 1 || hook(kHookExchange) == 1;
    const bool want = split >= 0 ? split == 1 : nq >= 4096;
    if (several && !direct && !collect_counters && want && nq >= 2 && !swapping()) {
      query_split(r, filter);
      return;
    }
  }

  constexpr int lane = DeviceCtx::kBlockingLane;
  for_each_device([&](DeviceCtx& ctx) {
    Staged sq = stage_query(ctx, r.q, r.Nq, r.D, r.dtype, r.loc, r.gpu);
    int32_t* d_ids = ids_out;
    float* d_dists = dists_out;
    if (!direct) {
      DeviceCtx::grow(ctx.xb[lane].r_pack, 2 * part * 4);
      d_ids = ctx.xb[lane].r_pack.as<int32_t>();
      d_dists = reinterpret_cast<float*>(d_ids + part);
    }
    query_device(ctx, r, sq.ptr, d_ids, d_dists, filter);
  });
  for (const DeviceCtx& ctx : devs) {
    query_ms = std::max(query_ms, ctx.query_ms);  // GPUs run concurrently
    last_n_dist += ctx.n_dist;
    last_n_pop += ctx.n_pop;
    last_float_rows += ctx.n_float_rows;
    last_code_rows += ctx.n_code_rows;
  }
  if (direct)
    return;

  const bool force_rccl = hook(kHookExchange) == 1;
  if (devs.size() == 1 && !force_rccl) {
    // ResultMerger::merge for one GPU: first K of each pre-sorted row (result_merger.cpp:55-73)
    DeviceCtx& d0 = devs[0];
    d0.activate();
    const int32_t* rows = d0.xb[lane].r_pack.as<int32_t>();
    GGNN_HIP_CHECK(hipMemcpy2DAsync(ids_out, k_query * 4ull, rows, row * 4, k_query * 4ull, nq,
                                    hipMemcpyDeviceToHost, d0.stream));
    GGNN_HIP_CHECK(hipMemcpy2DAsync(dists_out, k_query * 4ull, rows + part, row * 4,
                                    k_query * 4ull, nq, hipMemcpyDeviceToHost, d0.stream));
    GGNN_HIP_CHECK(hipStreamSynchronize(d0.stream));
    last_exchange = "none";
    return;
  }
  exchange(lane, nq, k_query, row, ids_out, dists_out, /*blocking=*/true);
}

// blocking multi-GPU query as two half-batches on the asynchronous lanes 0 and 1 (see query())
void ggnn_handle::query_split(const QueryRequest& r, const QueryFilter& filter)
{
  const uint32_t nq = static_cast<uint32_t>(r.Nq);
  const uint32_t k_query = r.k;
  const size_t row = static_cast<size_t>(k_query) * shards_per_gpu;
  const size_t es = dtype_size(r.dtype);
  const uint32_t first[2] = {0u, nq / 2};
  const uint32_t count[2] = {nq / 2, nq - nq / 2};
  std::vector<Staged> staged(devs.size());
  // the whole query set once per GPU, both halves enqueued on their lanes; nothing waits yet
  for (size_t g = 0; g < devs.size(); ++g) {
    DeviceCtx& ctx = devs[g];
    ctx.activate();
    for (uint32_t si = 0; si < shards_per_gpu; ++si)
      (void)ensure_prescreen(ctx, si, r.measure);
    ctx.ensure_shard_streams();
    staged[g] = stage_query(ctx, r.q, nq, r.D, r.dtype, r.loc, r.gpu);
    const DeviceFilter df = resolve_filter(ctx, filter, DeviceCtx::kBlockingLane);
    GGNN_HIP_CHECK(hipEventRecord(ctx.ev_ready, ctx.stream));
    GGNN_HIP_CHECK(hipEventRecord(ctx.ev_a, ctx.stream));
    for (int half = 0; half < 2; ++half) {
      if (!count[half])
        continue;
      const int lane = half;
      hipStream_t st = ctx.lane_stream(lane);
      GGNN_HIP_CHECK(hipStreamWaitEvent(st, ctx.ev_ready, 0));
      DeviceCtx::ExchangeBufs& x = ctx.xb[lane];
      if (&ctx != &devs[0] && devs[0].xb[lane].consumed)
        GGNN_HIP_CHECK(hipStreamWaitEvent(st, devs[0].xb[lane].consumed, 0));
      const size_t part = count[half] * row;
      grow_lane(ctx, lane, x.r_pack, 2 * part * 4);
      int32_t* rows = x.r_pack.as<int32_t>();
      const uint8_t* qh = static_cast<const uint8_t*>(staged[g].ptr) +
                          static_cast<size_t>(first[half]) * pad_D * es;
      // (each half sees its own half of the filter ids)
      enqueue_local_search(ctx, lane, r, qh, count[half], rows,
                           reinterpret_cast<float*>(rows + part), df.from(first[half]));
      GGNN_HIP_CHECK(hipEventRecord(ctx.shard_done[lane], st));
      GGNN_HIP_CHECK(hipStreamWaitEvent(ctx.stream, ctx.shard_done[lane], 0));
    }
    GGNN_HIP_CHECK(hipEventRecord(ctx.ev_b, ctx.stream));  // both halves searched on this GPU
  }
  // the first half is exchanged, merged and copied out while the second is still being searched
  for (int half = 0; half < 2; ++half)
    if (count[half])
      exchange(half, count[half], k_query, row,
               r.ids_out + static_cast<size_t>(first[half]) * k_query,
               r.dists_out + static_cast<size_t>(first[half]) * k_query, /*blocking=*/true);
  for (DeviceCtx& ctx : devs) {
    ctx.activate();
    GGNN_HIP_CHECK(hipStreamSynchronize(ctx.stream));
    float ms = 0.f;
    GGNN_HIP_CHECK(hipEventElapsedTime(&ms, ctx.ev_a, ctx.ev_b));
    ctx.query_ms = ms;
    query_ms = std::max(query_ms, ms);
    GGNN_LOG(0, "[GPU: %d] query parts %u..%u, two half-batches in flight => ms: %.3f [%u points "
                "query]", ctx.device, ctx.first_shard, ctx.first_shard + shards_per_gpu - 1, ms, nq);
  }
  last_query_parts = 2;
}

// Grows one exchange buffer of a lane.  Batches in flight on the lane may still use the old
// allocation -- also from ANOTHER GPU's stream (peer copies read r_pack, RCCL kernels write
// g_pack), which the hipFree of the owning device does not wait for: every GPU's stream of the
// lane is drained first.  Rare: the first batch on a lane, or a larger one than any before.
void ggnn_handle::grow_lane(DeviceCtx& owner, int lane, DeviceBuffer& b, size_t bytes)
{
  if (b.bytes >= bytes)
    return;
  for (DeviceCtx& ctx : devs) {
    hipStream_t st = ctx.lane_stream(lane);
    if (!st)
      continue;
    ctx.activate();
    GGNN_HIP_CHECK(hipStreamSynchronize(st));
  }
  owner.activate();
  b.alloc(bytes);
}

// Extension for serving: enqueue one query batch and return.  Consecutive batches given
// different slots run on different streams, so the under-occupied tail of one batch's launch
// overlaps with the head of the next (a lone 10k-query launch is latency-bound).
//
// One GPU: query and result arrays already on that GPU (nothing is staged); results are the
// sorted [Nq, K * shards] rows of results-on-GPU mode (ggnn.cuh:108-113).
// Several GPUs: the query may live on any GPU of the node or in page-locked host memory (it is
// copied to every GPU on the slot's stream), results are the MERGED [Nq, K] arrays, written
// by asynchronous copies (device memory of any GPU, or page-locked host memory; with pageable
// memory the copies degrade to synchronous ones).  Local search, the RCCL all-gather, the
// slice merges and the result copies of batch i+1 are all enqueued while batch i runs.
// Valid after synchronize() / synchronize_slot(slot).
//
// Ordering contract with the blocking query(): both may be used on one handle from one
// thread; a blocking call does not wait for batches in flight (its buffers and stream are its
// own), and a call that has to re-code the pre-screen copy for another measure first drains
// every slot.
void ggnn_handle::query_async(const QueryRequest& r, uint32_t slot, const QueryFilter& filter)
{
  const void* const d_query = r.q;
  const uint64_t Nq = r.Nq;
  const ggnn_location loc = r.loc;
  const int q_gpu = r.gpu;
  const uint32_t k_query = r.k;
  const ggnn_measure measure = r.measure;
  int32_t* const d_ids = r.ids_out;
  float* const d_dists = r.dists_out;
  GGNN_REQUIRE(has_graph(), GGNN_INVALID_STATE, "There is no graph to query.");
  check_query(Nq, r.D, r.dtype, d_query);
  GGNN_REQUIRE(!Nq || (d_ids != nullptr && d_dists != nullptr), GGNN_INVALID_ARGUMENT,
               "result pointers are null");
  GGNN_REQUIRE(!swapping(), GGNN_UNSUPPORTED,
               "asynchronous queries need every shard resident on its GPU (the shards of this "
               "handle take turns in GPU memory)");
  if (!Nq)
    return;
  const uint32_t nq = static_cast<uint32_t>(Nq);
  const int lane = static_cast<int>(slot % DeviceCtx::kShardStreams);
  // the pre-screen copy of another measure is replaced below: nothing may still read it
  bool recode = false;
  for (const DeviceCtx& ctx : devs)
    for (const Shard& sh : ctx.shards)
      recode = recode || (sh.ps_state != 0 && sh.ps_measure != measure);
  if (recode)
    synchronize();
  const bool force_rccl = hook(kHookExchange) == 1;
  if (devs.size() == 1 && !force_rccl) {
    DeviceCtx& ctx = devs[0];
    GGNN_REQUIRE(loc == GGNN_GPU && q_gpu == ctx.device, GGNN_INVALID_ARGUMENT,
                 "asynchronous queries need the query on the engine's GPU");
    GGNN_REQUIRE(pad_D == base_D && (reinterpret_cast<uintptr_t>(d_query) & 15u) == 0,
                 GGNN_UNSUPPORTED,
                 "asynchronous queries need 16-byte aligned rows (no padding is staged)");
    ctx.activate();
    for (uint32_t si = 0; si < shards_per_gpu; ++si)
      (void)ensure_prescreen(ctx, si, measure);
    ctx.ensure_shard_streams();
    // (filter ids: device memory on this GPU like the query, used in place)
    enqueue_local_search(ctx, lane, r, d_query, nq, d_ids, d_dists,
                         resolve_filter(ctx, filter, lane));
    return;
  }
  GGNN_REQUIRE(pad_D == base_D, GGNN_UNSUPPORTED,
               "asynchronous queries need 16-byte rows (no padding is staged)");
  const size_t row = static_cast<size_t>(k_query) * shards_per_gpu;
  const size_t part = nq * row;
  const size_t qbytes = Nq * static_cast<size_t>(pad_D) * dtype_size(r.dtype);
  for (DeviceCtx& ctx : devs) {
    ctx.activate();
    for (uint32_t si = 0; si < shards_per_gpu; ++si)
      (void)ensure_prescreen(ctx, si, measure);
    ctx.ensure_shard_streams();
    DeviceCtx::ExchangeBufs& x = ctx.xb[lane];
    hipStream_t st = ctx.lane_stream(lane);
    const void* q_here = d_query;
    if (!(loc == GGNN_GPU && q_gpu == ctx.device &&
          (reinterpret_cast<uintptr_t>(d_query) & 15u) == 0)) {
      grow_lane(ctx, lane, x.q_stage, qbytes);
      GGNN_HIP_CHECK(hipMemcpyAsync(x.q_stage.p, d_query, qbytes, hipMemcpyDefault, st));
      q_here = x.q_stage.p;
    }
    // the filter ids follow the query's memory rule: used in place on their own GPU, else copied
    // on the lane's stream
    const DeviceFilter df = resolve_filter(ctx, filter, lane);
    // (copy exchange: the first GPU may still be copying this lane's previous rows)
#ifndef GGNN_EXP_NO_CONSUMED_WAIT  // (test-the-test hook)
    if (&ctx != &devs[0] && devs[0].xb[lane].consumed)
      GGNN_HIP_CHECK(hipStreamWaitEvent(st, devs[0].xb[lane].consumed, 0));
#endif
    grow_lane(ctx, lane, x.r_pack, 2 * part * 4);
    int32_t* rows = x.r_pack.as<int32_t>();
    enqueue_local_search(ctx, lane, r, q_here, nq, rows, reinterpret_cast<float*>(rows + part), df);
  }
  exchange(lane, nq, k_query, row, d_ids, d_dists, /*blocking=*/false);
}

// the shards of one GPU on one lane's stream, nothing waits
void ggnn_handle::enqueue_local_search(DeviceCtx& ctx, int lane, const QueryRequest& r,
                                       const void* d_query, uint32_t nq, int32_t* d_ids,
                                       float* d_dists, const DeviceFilter& df)
{
  hipStream_t stream = ctx.lane_stream(lane);
  for (uint32_t si = 0; si < shards_per_gpu; ++si) {
    const Shard& sh = ctx.shards[si];
    const bool use_ps = sh.ps_state > 0 && sh.ps_measure == r.measure;
    launch_query(shard_launch(ctx, si, r, d_query, nq, d_ids, d_dists, use_ps, df), stream);
  }
  if (shards_per_gpu > 1)
    launch_sort_shard_results(nq, r.k * shards_per_gpu, d_ids, d_dists, stream);
}

// wait for the batches enqueued on one slot only (the other slots keep running)
void ggnn_handle::synchronize_slot(uint32_t slot)
{
  for (DeviceCtx& ctx : devs) {
    ctx.activate();
    hipStream_t st = ctx.shard_stream[slot % DeviceCtx::kShardStreams];
    if (st)
      GGNN_HIP_CHECK(hipStreamSynchronize(st));
  }
}

void ggnn_handle::synchronize()
{
  for (DeviceCtx& ctx : devs) {
    ctx.activate();
    GGNN_HIP_CHECK(hipStreamSynchronize(ctx.stream));
    for (int i = 0; i < DeviceCtx::kShardStreams; ++i)
      if (ctx.shard_stream[i])
        GGNN_HIP_CHECK(hipStreamSynchronize(ctx.shard_stream[i]));
  }
}

// The whole base on the one GPU of an exhaustive call (bf_query, bf_range_query): the resident base,
// or -- no graph yet -- the base made resident on the (first) selected GPU.
DeviceCtx& ggnn_handle::bf_context(uint64_t Nq, uint32_t D, ggnn_dtype dtype, const void* q)
{
  GGNN_REQUIRE(base_set, GGNN_INVALID_STATE,
               "There is no base dataset loaded which could be queried.");
  GGNN_REQUIRE(devs.size() <= 1, GGNN_INVALID_STATE,
               "The brute-force query only supports a single GPU.");
  check_query(Nq, D, dtype, q);
  if (devs.empty()) {
    // no graph yet: make the whole base resident on the (first) selected GPU
    const std::vector<int> gpus = resolve_gpus();
    devs.resize(1);
    devs[0].device = gpus[0];
    stage_base_slice(devs[0], 0, base_N);
  }
  devs[0].activate();
  return devs[0];
}

// ... and with out-of-core shards whose rows are on the host: the exhaustive scan needs the whole
// base on the GPU for the duration of the call (fails with GGNN_OUT_OF_MEMORY if that is too much);
// `whole_base` owns that copy
const void* ggnn_handle::bf_whole_base(DeviceCtx& ctx, DeviceBuffer& whole_base)
{
  if (!(ctx.swap && !ctx.swap->base_borrowed))
    return ctx.d_base;
  const size_t es = dtype_size(base_dtype);
  whole_base.alloc(base_N * pad_D * es);
  const hipMemcpyKind kind = base_loc == GGNN_GPU ? hipMemcpyDefault : hipMemcpyHostToDevice;
  if (pad_D != base_D) {
    GGNN_HIP_CHECK(hipMemsetAsync(whole_base.p, 0, whole_base.bytes, ctx.stream));
    GGNN_HIP_CHECK(hipMemcpy2DAsync(whole_base.p, pad_D * es, base_src, base_D * es, base_D * es,
                                    base_N, kind, ctx.stream));
  }
  else
    GGNN_HIP_CHECK(hipMemcpyAsync(whole_base.p, base_src, whole_base.bytes, kind, ctx.stream));
  return whole_base.p;
}

// GGNNImpl::bfQueryImpl, ggnn.cu:332-390
void ggnn_handle::bf_query(const QueryRequest& r, const QueryFilter& filter)
{
  const uint64_t Nq = r.Nq;
  const uint32_t k_gt = r.k;
  int32_t* const ids_out = r.ids_out;
  float* const dists_out = r.dists_out;
  DeviceCtx& ctx = bf_context(Nq, r.D, r.dtype, r.q);
  bf_ms = 0.f;
  last_bf_matrix_path = 0;
  if (!Nq)
    return;
  DeviceBuffer whole_base;
  const void* bf_base = bf_whole_base(ctx, whole_base);
  Staged sq = stage_query(ctx, r.q, Nq, r.D, r.dtype, r.loc, r.gpu);
  const uint32_t nq = static_cast<uint32_t>(Nq);
  const bool direct = (r.out_loc == GGNN_GPU);
  DeviceBuffer r_ids, r_dists;
  int32_t* d_ids = ids_out;
  float* d_dists = dists_out;
  if (!direct) {
    r_ids.alloc(static_cast<size_t>(nq) * k_gt * 4);
    r_dists.alloc(static_cast<size_t>(nq) * k_gt * 4);
    d_ids = r_ids.as<int32_t>();
    d_dists = r_dists.as<float>();
  }
  if (!ctx.bf_rescanned.p)
    ctx.bf_rescanned.alloc(sizeof(uint32_t));
  BfLaunch bl{bf_base, sq.ptr, base_dtype, static_cast<uint32_t>(base_N), pad_D, nq, k_gt,
              r.measure,  d_ids,  d_dists,    ctx.bf_rescanned.as<uint32_t>()};
  const DeviceFilter df = resolve_filter(ctx, filter, DeviceCtx::kBlockingLane);
  bl.filter_bits = df.bits;
  bl.filter_table = df.table;
  bl.label_sets = df.set;
  bl.label_ranges = df.ranges;
  bl.label_masks = df.masks;
  // (one launch over the whole base: "every shard" is this launch)
  last_bf_matrix_path = 0;
  bl.matrix_path = &last_bf_matrix_path;
  EventTimer timer(ctx.stream, ctx.ev_a, ctx.ev_b);
  launch_bf_query(bl, ctx.stream);
  bf_ms = timer.stop();
  GGNN_HIP_CHECK(hipMemcpyAsync(&last_bf_rescanned, ctx.bf_rescanned.p, sizeof(uint32_t),
                                hipMemcpyDeviceToHost, ctx.stream));
  GGNN_LOG(0, "[GPU: %d] brute-force query: => ms: %.3f [%u points query -> %.3f us/point]",
           ctx.device, bf_ms, nq, bf_ms * 1000.f / static_cast<float>(nq));
  if (!direct) {
    GGNN_HIP_CHECK(hipMemcpyAsync(ids_out, d_ids, static_cast<size_t>(nq) * k_gt * 4,
                                  hipMemcpyDeviceToHost, ctx.stream));
    GGNN_HIP_CHECK(hipMemcpyAsync(dists_out, d_dists, static_cast<size_t>(nq) * k_gt * 4,
                                  hipMemcpyDeviceToHost, ctx.stream));
  }
  GGNN_HIP_CHECK(hipStreamSynchronize(ctx.stream));
}

// Exact range search over the whole base (launch_bf_range_query): bf_query's staging, a CSR result.
// lims is host memory; ids / dists follow r.out_loc and are written only if the total fits.
void ggnn_handle::bf_range_query(const QueryRequest& r, const float* radii, uint64_t capacity,
                                 uint64_t* lims_out, const QueryFilter& filter)
{
  const uint64_t Nq = r.Nq;
  GGNN_REQUIRE(lims_out != nullptr, GGNN_INVALID_ARGUMENT, "lims is null");
  GGNN_REQUIRE(!Nq || radii != nullptr, GGNN_INVALID_ARGUMENT, "the radius array is null");
  GGNN_REQUIRE(capacity == 0 || (r.ids_out != nullptr && r.dists_out != nullptr),
               GGNN_INVALID_ARGUMENT, "ids / dists are null with capacity > 0");
  for (uint64_t i = 0; i < Nq; ++i)
    GGNN_REQUIRE(radii[i] == radii[i], GGNN_INVALID_ARGUMENT,
                 "the radius of query " + std::to_string(i) + " is NaN");
  GGNN_REQUIRE(filter.kind == QueryFilter::None || filter.kind == QueryFilter::Bitset ||
                   filter.kind == QueryFilter::TableIds || filter.kind == QueryFilter::Labels,
               GGNN_UNSUPPORTED, "range search takes a bitset, filter ids or one label per query");
  DeviceCtx& ctx = bf_context(Nq, r.D, r.dtype, r.q);
  bf_ms = 0.f;
  lims_out[0] = 0;
  if (!Nq)
    return;
  DeviceBuffer whole_base;
  const void* bf_base = bf_whole_base(ctx, whole_base);
  Staged sq = stage_query(ctx, r.q, Nq, r.D, r.dtype, r.loc, r.gpu);
  const uint32_t nq = static_cast<uint32_t>(Nq);
  const bool direct = (r.out_loc == GGNN_GPU);
  DeviceBuffer d_radii, d_lims, r_ids, r_dists;
  d_radii.alloc(Nq * sizeof(float));
  d_lims.alloc((Nq + 1) * sizeof(uint64_t));
  GGNN_HIP_CHECK(hipMemcpyAsync(d_radii.p, radii, Nq * sizeof(float), hipMemcpyHostToDevice,
                                ctx.stream));
  int32_t* d_ids = r.ids_out;
  float* d_dists = r.dists_out;
  if (!direct && capacity) {
    r_ids.alloc(capacity * 4);
    r_dists.alloc(capacity * 4);
    d_ids = r_ids.as<int32_t>();
    d_dists = r_dists.as<float>();
  }
  BfRangeLaunch bl{bf_base,   sq.ptr,   base_dtype, static_cast<uint32_t>(base_N),
                   pad_D,     nq,       r.measure,  d_radii.as<float>(),
                   capacity,  d_lims.as<uint64_t>(), d_ids, d_dists};
  const DeviceFilter df = resolve_filter(ctx, filter, DeviceCtx::kBlockingLane);
  bl.filter_bits = df.bits;
  bl.filter_table = df.table;
  EventTimer timer(ctx.stream, ctx.ev_a, ctx.ev_b);
  launch_bf_range_query(bl, ctx.stream);
  bf_ms = timer.stop();
  GGNN_HIP_CHECK(hipMemcpyAsync(lims_out, d_lims.p, (Nq + 1) * sizeof(uint64_t),
                                hipMemcpyDeviceToHost, ctx.stream));
  GGNN_HIP_CHECK(hipStreamSynchronize(ctx.stream));
  GGNN_LOG(0, "[GPU: %d] brute-force range query: => ms: %.3f [%u points query, %llu results]",
           ctx.device, bf_ms, nq, static_cast<unsigned long long>(lims_out[Nq]));
  const uint64_t total = lims_out[Nq];
  if (!direct && total && total <= capacity) {
    GGNN_HIP_CHECK(hipMemcpyAsync(r.ids_out, d_ids, total * 4, hipMemcpyDeviceToHost, ctx.stream));
    GGNN_HIP_CHECK(hipMemcpyAsync(r.dists_out, d_dists, total * 4, hipMemcpyDeviceToHost,
                                  ctx.stream));
    GGNN_HIP_CHECK(hipStreamSynchronize(ctx.stream));
  }
}

// ---- the filter of one call: validated as the caller gave it, then resolved per GPU -------------
QueryFilter QueryFilter::bitset(const ggnn_handle& h, const uint32_t* bits, uint64_t n_bits,
                                ggnn_location loc, int gpu)
{
  GGNN_REQUIRE(bits != nullptr, GGNN_INVALID_ARGUMENT, "the filter bitset is null");
  GGNN_REQUIRE(!h.base_set || n_bits == h.base_N, GGNN_INVALID_ARGUMENT,
               "the filter needs one bit per base vector (n_bits must equal N)");
  GGNN_REQUIRE(h.base_set, GGNN_INVALID_STATE, "There is no base dataset the filter could refer to.");
  return {Bitset, bits, n_bits, loc, gpu};
}

QueryFilter QueryFilter::table_ids(const ggnn_handle& h, const int32_t* ids, uint64_t Nq,
                                   ggnn_location loc, int gpu, bool read_host_ids)
{
  GGNN_REQUIRE(h.num_filters != 0, GGNN_INVALID_STATE,
               "There is no filter table the filter ids could refer to (ggnn_set_filters).");
  GGNN_REQUIRE(!Nq || ids != nullptr, GGNN_INVALID_ARGUMENT, "the filter id array is null");
  if (read_host_ids && loc == GGNN_CPU)
    for (uint64_t i = 0; i < Nq; ++i)
      GGNN_REQUIRE(ids[i] >= -1 && ids[i] < static_cast<int64_t>(h.num_filters),
                   GGNN_INVALID_ARGUMENT,
                   "filter id " + std::to_string(ids[i]) + " of query " + std::to_string(i) +
                       " is outside [-1, " + std::to_string(h.num_filters) + ")");
  return {TableIds, ids, Nq, loc, gpu};
}

QueryFilter QueryFilter::labels(const ggnn_handle& h, const int32_t* query_labels, uint64_t Nq,
                                ggnn_location loc, int gpu)
{
  GGNN_REQUIRE(!h.labels_host.empty(), GGNN_INVALID_STATE,
               "There are no labels the query labels could refer to (ggnn_set_labels).");
  GGNN_REQUIRE(!Nq || query_labels != nullptr, GGNN_INVALID_ARGUMENT,
               "the query label array is null");
  // (every int32 is a valid label: nothing to validate)
  return {Labels, query_labels, Nq, loc, gpu};
}

QueryFilter QueryFilter::label_sets(const ggnn_handle& h, const int32_t* sets, uint32_t width,
                                    uint64_t Nq, ggnn_location loc, int gpu, const int32_t* ids,
                                    ggnn_location ids_loc, int ids_gpu, bool read_host_ids)
{
  GGNN_REQUIRE(width >= 1 && width <= GGNN_MAX_LABEL_SET, GGNN_INVALID_ARGUMENT,
               "set_width " + std::to_string(width) + " is outside [1, " +
                   std::to_string(GGNN_MAX_LABEL_SET) + "]");
  GGNN_REQUIRE(sets != nullptr, GGNN_INVALID_ARGUMENT, "the label set array is null");
  GGNN_REQUIRE(!h.labels_host.empty(), GGNN_INVALID_STATE,
               "There are no labels the label sets could refer to (ggnn_set_labels).");
  QueryFilter f{LabelSets, sets, Nq * width, loc, gpu};
  f.width = width;
  if (ids) {
    // (the rules of the filter ids of ggnn_query_filtered_by)
    const QueryFilter t = table_ids(h, ids, Nq, ids_loc, ids_gpu, read_host_ids);
    f.ids = ids;
    f.ids_loc = t.loc;
    f.ids_gpu = t.gpu;
  }
  GGNN_REQUIRE(h.base_dtype != GGNN_I8, GGNN_UNSUPPORTED,
               "label sets are not built for int8 bases");
  return f;
}

QueryFilter QueryFilter::label_ranges(const ggnn_handle& h, const int32_t* ranges,
                                      uint32_t n_ranges, uint64_t Nq, ggnn_location loc, int gpu,
                                      const int32_t* ids, ggnn_location ids_loc, int ids_gpu,
                                      bool read_host_ids)
{
  GGNN_REQUIRE(n_ranges >= 1 && n_ranges <= GGNN_MAX_LABEL_RANGES, GGNN_INVALID_ARGUMENT,
               "n_ranges " + std::to_string(n_ranges) + " is outside [1, " +
                   std::to_string(GGNN_MAX_LABEL_RANGES) + "]");
  GGNN_REQUIRE(ranges != nullptr, GGNN_INVALID_ARGUMENT, "the label range array is null");
  GGNN_REQUIRE(!h.labels_host.empty(), GGNN_INVALID_STATE,
               "There are no labels the label ranges could refer to (ggnn_set_labels).");
  QueryFilter f{LabelRanges, ranges, Nq * n_ranges * 2, loc, gpu};
  f.width = n_ranges;
  if (ids) {
    // (the rules of the filter ids of ggnn_query_filtered_by)
    const QueryFilter t = table_ids(h, ids, Nq, ids_loc, ids_gpu, read_host_ids);
    f.ids = ids;
    f.ids_loc = t.loc;
    f.ids_gpu = t.gpu;
  }
  GGNN_REQUIRE(h.base_dtype != GGNN_I8, GGNN_UNSUPPORTED,
               "label ranges are not built for int8 bases");
  return f;
}

QueryFilter QueryFilter::label_masks(const ggnn_handle& h, const int32_t* masks, uint32_t n_masks,
                                     uint64_t Nq, ggnn_location loc, int gpu, const int32_t* ids,
                                     ggnn_location ids_loc, int ids_gpu, bool read_host_ids)
{
  GGNN_REQUIRE(n_masks >= 1 && n_masks <= GGNN_MAX_LABEL_MASKS, GGNN_INVALID_ARGUMENT,
               "n_masks " + std::to_string(n_masks) + " is outside [1, " +
                   std::to_string(GGNN_MAX_LABEL_MASKS) + "]");
  GGNN_REQUIRE(masks != nullptr, GGNN_INVALID_ARGUMENT, "the label mask array is null");
  GGNN_REQUIRE(!h.labels_host.empty(), GGNN_INVALID_STATE,
               "There are no labels the label masks could refer to (ggnn_set_labels).");
  QueryFilter f{LabelMasks, masks, Nq * n_masks * 3, loc, gpu};
  f.width = n_masks;
  if (ids) {
    // (the rules of the filter ids of ggnn_query_filtered_by)
    const QueryFilter t = table_ids(h, ids, Nq, ids_loc, ids_gpu, read_host_ids);
    f.ids = ids;
    f.ids_loc = t.loc;
    f.ids_gpu = t.gpu;
  }
  GGNN_REQUIRE(h.base_dtype != GGNN_I8, GGNN_UNSUPPORTED,
               "label masks are not built for int8 bases");
  return f;
}

// label sets, label ranges and label masks -- a per-query int32 array of f.stride() words, plus
// optional ids: the resident column and (with filter ids) the resident table; the rows and the ids
// are used in place on their own GPU, else staged behind one another in the lane's id stage
DeviceFilter ggnn_handle::resolve_label_rows(DeviceCtx& ctx, const QueryFilter& f, int lane,
                                             const int32_t*& column, const int32_t*& rows)
{
  DeviceFilter d;
  column = place_labels(ctx);
  if (f.ids) {
    d.bits = place_filter_table(ctx);
    d.table.words = filter_words;
    d.table.num_filters = num_filters;
  }
  const bool blocking = lane == DeviceCtx::kBlockingLane;
  const auto in_place = [&](const void* p, ggnn_location loc, int gpu) {
    return loc == GGNN_GPU && gpu == ctx.device && (reinterpret_cast<uintptr_t>(p) & 3u) == 0;
  };
  const size_t set_bytes = static_cast<size_t>(f.count) * 4;
  const size_t id_bytes = f.ids ? static_cast<size_t>(f.count / f.stride()) * 4 : 0;
  const bool stage_sets = !in_place(f.ptr, f.loc, f.gpu);
  const bool stage_ids = f.ids && !in_place(f.ids, f.ids_loc, f.ids_gpu);
  DeviceBuffer& stage = blocking ? ctx.filter_ids_stage : ctx.xb[lane].f_stage;
  const size_t bytes = (stage_sets ? set_bytes : 0) + (stage_ids ? id_bytes : 0);
  if (bytes) {
    if (blocking)
      DeviceCtx::grow(stage, bytes);
    else
      grow_lane(ctx, lane, stage, bytes);
  }
  uint8_t* at = static_cast<uint8_t*>(stage.p);
  const auto here = [&](const void* p, bool staged, size_t n, ggnn_location loc) {
    if (!staged)
      return p;
    GGNN_HIP_CHECK(hipMemcpyAsync(at, p, n, loc == GGNN_GPU ? hipMemcpyDefault : hipMemcpyHostToDevice,
                                  ctx.lane_stream(lane)));
    const void* r = at;
    at += n;
    return r;
  };
  rows = static_cast<const int32_t*>(here(f.ptr, stage_sets, set_bytes, f.loc));
  if (f.ids)
    d.table.ids = static_cast<const int32_t*>(here(f.ids, stage_ids, id_bytes, f.ids_loc));
  return d;
}

DeviceFilter ggnn_handle::resolve_label_sets(DeviceCtx& ctx, const QueryFilter& f, int lane)
{
  const int32_t *column = nullptr, *rows = nullptr;
  DeviceFilter d = resolve_label_rows(ctx, f, lane, column, rows);
  d.set = LabelSetSpec{column, rows, f.width};
  return d;
}

DeviceFilter ggnn_handle::resolve_label_ranges(DeviceCtx& ctx, const QueryFilter& f, int lane)
{
  const int32_t *column = nullptr, *rows = nullptr;
  DeviceFilter d = resolve_label_rows(ctx, f, lane, column, rows);
  d.ranges = LabelRangeSpec{column, rows, f.width};
  return d;
}

DeviceFilter ggnn_handle::resolve_label_masks(DeviceCtx& ctx, const QueryFilter& f, int lane)
{
  const int32_t *column = nullptr, *rows = nullptr;
  DeviceFilter d = resolve_label_rows(ctx, f, lane, column, rows);
  d.masks = LabelMaskSpec{column, rows, f.width};
  return d;
}

DeviceFilter ggnn_handle::resolve_filter(DeviceCtx& ctx, const QueryFilter& f, int lane)
{
  DeviceFilter d;
  if (f.kind == QueryFilter::None)
    return d;
  if (f.kind == QueryFilter::LabelSets)
    return resolve_label_sets(ctx, f, lane);
  if (f.kind == QueryFilter::LabelRanges)
    return resolve_label_ranges(ctx, f, lane);
  if (f.kind == QueryFilter::LabelMasks)
    return resolve_label_masks(ctx, f, lane);
  // what is resident: the filter table, or the label column (the kernels read it through
  // filter_bits, common.hpp: the only place that casts it)
  if (f.kind == QueryFilter::TableIds) {
    d.bits = place_filter_table(ctx);
    d.table.words = filter_words;
    d.table.num_filters = num_filters;
    d.table.consts = d.bits + static_cast<size_t>(num_filters) * filter_words;
  }
  else if (f.kind == QueryFilter::Labels)
    d.bits = reinterpret_cast<const uint32_t*>(place_labels(ctx));
  // what the caller brought (bitset words, filter ids, query labels): used in place on its own
  // GPU, else copied on the lane's stream
  const bool blocking = lane == DeviceCtx::kBlockingLane;
  const void* here = f.ptr;
  if (!(f.loc == GGNN_GPU && f.gpu == ctx.device && (reinterpret_cast<uintptr_t>(f.ptr) & 3u) == 0)) {
    const bool bitset = f.kind == QueryFilter::Bitset;
    const size_t bytes = static_cast<size_t>(bitset ? (f.count + 31) / 32 : f.count) * 4;
    DeviceBuffer& stage = bitset     ? ctx.filter_stage
                          : blocking ? ctx.filter_ids_stage
                                     : ctx.xb[lane].f_stage;
    if (blocking)
      DeviceCtx::grow(stage, bytes);
    else
      grow_lane(ctx, lane, stage, bytes);
    GGNN_HIP_CHECK(hipMemcpyAsync(stage.p, f.ptr, bytes,
                                  f.loc == GGNN_GPU ? hipMemcpyDefault : hipMemcpyHostToDevice,
                                  ctx.lane_stream(lane)));
    here = stage.p;
  }
  switch (f.kind) {
    case QueryFilter::Bitset: d.bits = static_cast<const uint32_t*>(here); break;
    case QueryFilter::TableIds: d.table.ids = static_cast<const int32_t*>(here); break;
    case QueryFilter::Labels: d.table.query_labels = static_cast<const int32_t*>(here); break;
    case QueryFilter::LabelSets:
    case QueryFilter::LabelRanges:
    case QueryFilter::LabelMasks:
    case QueryFilter::None: break;
  }
  return d;
}

// ---- per-query filters: resident filter table, one filter id per query ------------------------
void ggnn_handle::drop_filters()
{
  synchronize();
  DeviceRestoreGuard keep;
  filter_table_host.clear();
  filter_table_host.shrink_to_fit();
  num_filters = 0;
  filter_words = 0;
  ++filter_epoch;
  for (DeviceCtx& ctx : devs) {
    (void)hipSetDevice(ctx.device);
    ctx.filter_table.release();
    ctx.filter_table_epoch = 0;
  }
}

void ggnn_handle::set_filters(const uint32_t* bits, uint32_t F, uint64_t n_bits, ggnn_location loc,
                              int gpu)
{
  if (F == 0) {
    drop_filters();
    return;
  }
  GGNN_REQUIRE(bits != nullptr, GGNN_INVALID_ARGUMENT, "the filter table is null");
  GGNN_REQUIRE(!base_set || n_bits == base_N, GGNN_INVALID_ARGUMENT,
               "a filter needs one bit per base vector (n_bits must equal N)");
  GGNN_REQUIRE(base_set, GGNN_INVALID_STATE, "There is no base dataset the filters could refer to.");
  const uint32_t words = static_cast<uint32_t>((n_bits + 31) / 32);
  std::vector<uint32_t> table(static_cast<size_t>(F) * words);
  if (loc == GGNN_GPU) {
    GGNN_HIP_CHECK(hipSetDevice(gpu));
    GGNN_HIP_CHECK(hipMemcpy(table.data(), bits, table.size() * sizeof(uint32_t),
                             hipMemcpyDeviceToHost));
  }
  else
    std::copy(bits, bits + table.size(), table.begin());
  // batches in flight read the old table: drain them before it is freed
  synchronize();
  filter_table_host = std::move(table);
  num_filters = F;
  filter_words = words;
  ++filter_epoch;
  try {
    place_filter_tables();
  }
  catch (...) {
    drop_filters();
    throw;
  }
}

void ggnn_handle::update_filter(uint32_t index, const uint32_t* bits, uint64_t n_bits,
                                ggnn_location loc, int gpu)
{
  GGNN_REQUIRE(num_filters != 0, GGNN_INVALID_STATE, "There is no filter table (ggnn_set_filters).");
  GGNN_REQUIRE(index < num_filters, GGNN_OUT_OF_RANGE,
               "filter index " + std::to_string(index) + " is outside the table of " +
                   std::to_string(num_filters) + " filters");
  GGNN_REQUIRE(bits != nullptr, GGNN_INVALID_ARGUMENT, "the filter bitset is null");
  GGNN_REQUIRE(n_bits == base_N, GGNN_INVALID_ARGUMENT,
               "a filter needs one bit per base vector (n_bits must equal N)");
  uint32_t* row = filter_table_host.data() + static_cast<size_t>(index) * filter_words;
  const size_t bytes = static_cast<size_t>(filter_words) * sizeof(uint32_t);
  // no batch in flight may see a half-written row
  synchronize();
  if (loc == GGNN_GPU) {
    GGNN_HIP_CHECK(hipSetDevice(gpu));
    GGNN_HIP_CHECK(hipMemcpy(row, bits, bytes, hipMemcpyDeviceToHost));
  }
  else
    std::copy(bits, bits + filter_words, row);
  for (DeviceCtx& ctx : devs) {
    if (ctx.filter_table_epoch != filter_epoch)
      continue;  // (not placed yet: placed whole when it is first needed)
    ctx.activate();
    GGNN_HIP_CHECK(hipMemcpy(ctx.filter_table.as<uint32_t>() + static_cast<size_t>(index) * filter_words,
                             row, bytes, hipMemcpyHostToDevice));
  }
}

const uint32_t* ggnn_handle::place_filter_table(DeviceCtx& ctx)
{
  GGNN_REQUIRE(num_filters != 0, GGNN_INVALID_STATE, "There is no filter table (ggnn_set_filters).");
  if (ctx.filter_table_epoch == filter_epoch && ctx.filter_table.p)
    return ctx.filter_table.as<uint32_t>();
  ctx.activate();
  const size_t row = static_cast<size_t>(filter_words) * sizeof(uint32_t);
  const size_t rows = static_cast<size_t>(num_filters);
  ctx.filter_table_epoch = 0;
  ctx.filter_table.alloc((rows + 2) * row);
  uint8_t* p = static_cast<uint8_t*>(ctx.filter_table.p);
  GGNN_HIP_CHECK(hipMemcpy(p, filter_table_host.data(), rows * row, hipMemcpyHostToDevice));
  GGNN_HIP_CHECK(hipMemset(p + rows * row, 0xff, row));  // id -1: everything allowed
  GGNN_HIP_CHECK(hipMemset(p + (rows + 1) * row, 0, row));  // any other id: nothing allowed
  GGNN_HIP_CHECK(hipDeviceSynchronize());
  ctx.filter_table_epoch = filter_epoch;
  return ctx.filter_table.as<uint32_t>();
}

void ggnn_handle::place_filter_tables()
{
  if (!num_filters)
    return;
  DeviceRestoreGuard keep;
  for (DeviceCtx& ctx : devs)
    (void)place_filter_table(ctx);
}

// ---- label filters: a resident int32 label per base vector, one label per query ----------------
void ggnn_handle::drop_labels()
{
  synchronize();
  DeviceRestoreGuard keep;
  labels_host.clear();
  labels_host.shrink_to_fit();
  ++labels_epoch;
  for (DeviceCtx& ctx : devs) {
    (void)hipSetDevice(ctx.device);
    ctx.labels.release();
    ctx.labels_epoch = 0;
  }
}

void ggnn_handle::set_labels(const int32_t* labels, uint64_t n, ggnn_location loc, int gpu)
{
  if (!labels) {
    drop_labels();
    return;
  }
  GGNN_REQUIRE(!base_set || n == base_N, GGNN_INVALID_ARGUMENT,
               "labels need one entry per base vector (n must equal N)");
  GGNN_REQUIRE(base_set, GGNN_INVALID_STATE, "There is no base dataset the labels could refer to.");
  std::vector<int32_t> column(n);
  if (loc == GGNN_GPU) {
    GGNN_HIP_CHECK(hipSetDevice(gpu));
    GGNN_HIP_CHECK(hipMemcpy(column.data(), labels, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  else
    std::copy(labels, labels + n, column.begin());
  // batches in flight read the old column: drain them before it is freed
  synchronize();
  labels_host = std::move(column);
  ++labels_epoch;
  try {
    place_labels_everywhere();
  }
  catch (...) {
    drop_labels();
    throw;
  }
}

void ggnn_handle::update_labels(const int64_t* ids, const int32_t* values, uint64_t count,
                                ggnn_location loc, int gpu)
{
  GGNN_REQUIRE(!labels_host.empty(), GGNN_INVALID_STATE, "There are no labels (ggnn_set_labels).");
  if (!count)
    return;
  GGNN_REQUIRE(ids != nullptr && values != nullptr, GGNN_INVALID_ARGUMENT,
               "the id or the value array is null");
  std::vector<int64_t> h_ids(count);
  std::vector<int32_t> h_values(count);
  if (loc == GGNN_GPU) {
    GGNN_HIP_CHECK(hipSetDevice(gpu));
    GGNN_HIP_CHECK(hipMemcpy(h_ids.data(), ids, count * sizeof(int64_t), hipMemcpyDeviceToHost));
    GGNN_HIP_CHECK(
        hipMemcpy(h_values.data(), values, count * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  else {
    std::copy(ids, ids + count, h_ids.begin());
    std::copy(values, values + count, h_values.begin());
  }
  // validate everything before anything changes
  const int64_t N = static_cast<int64_t>(labels_host.size());
  for (uint64_t i = 0; i < count; ++i)
    GGNN_REQUIRE(h_ids[i] >= 0 && h_ids[i] < N, GGNN_OUT_OF_RANGE,
                 "label id " + std::to_string(h_ids[i]) + " (pair " + std::to_string(i) +
                     ") is outside [0, " + std::to_string(N) + ")");
  // no batch in flight may see a half-relabelled column
  synchronize();
  // in order on the host, so the last pair of a repeated id wins; the GPUs are then sent the FINAL
  // label of every id named, so duplicates write equal values and the scatter is deterministic
  std::vector<uint32_t> rows(count);
  for (uint64_t i = 0; i < count; ++i) {
    rows[i] = static_cast<uint32_t>(h_ids[i]);
    labels_host[rows[i]] = h_values[i];
  }
  for (uint64_t i = 0; i < count; ++i)
    h_values[i] = labels_host[rows[i]];
  DeviceRestoreGuard keep;
  for (DeviceCtx& ctx : devs) {
    if (ctx.labels_epoch != labels_epoch || !ctx.labels.p)
      continue;  // (not placed yet: placed whole when it is first needed)
    ctx.activate();
    DeviceBuffer d_rows, d_values;
    d_rows.alloc(count * sizeof(uint32_t));
    d_values.alloc(count * sizeof(int32_t));
    GGNN_HIP_CHECK(hipMemcpyAsync(d_rows.p, rows.data(), count * sizeof(uint32_t),
                                  hipMemcpyHostToDevice, ctx.stream));
    GGNN_HIP_CHECK(hipMemcpyAsync(d_values.p, h_values.data(), count * sizeof(int32_t),
                                  hipMemcpyHostToDevice, ctx.stream));
    launch_scatter_labels(ctx.labels.as<int32_t>(), labels_host.size(), d_rows.as<uint32_t>(),
                          d_values.as<int32_t>(), count, ctx.stream);
    GGNN_HIP_CHECK(hipStreamSynchronize(ctx.stream));
  }
}

const int32_t* ggnn_handle::place_labels(DeviceCtx& ctx)
{
  GGNN_REQUIRE(!labels_host.empty(), GGNN_INVALID_STATE, "There are no labels (ggnn_set_labels).");
  if (ctx.labels_epoch == labels_epoch && ctx.labels.p)
    return ctx.labels.as<int32_t>();
  ctx.activate();
  ctx.labels_epoch = 0;
  ctx.labels.alloc(labels_host.size() * sizeof(int32_t));
  GGNN_HIP_CHECK(hipMemcpy(ctx.labels.p, labels_host.data(), labels_host.size() * sizeof(int32_t),
                           hipMemcpyHostToDevice));
  GGNN_HIP_CHECK(hipDeviceSynchronize());
  ctx.labels_epoch = labels_epoch;
  return ctx.labels.as<int32_t>();
}

void ggnn_handle::place_labels_everywhere()
{
  if (labels_host.empty())
    return;
  DeviceRestoreGuard keep;
  for (DeviceCtx& ctx : devs)
    (void)place_labels(ctx);
}
