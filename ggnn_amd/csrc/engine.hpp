// Engine behind the C-ABI (include/ggnn_c.h): shard residency, build schedule, query / bf_query
// drivers.  Replaces, for the hot path only, GGNNImpl (src/ggnn/base/ggnn.cu:124-413),
// GPUInstance::build/query (src/ggnn/base/gpu_instance.cu:499-584, 626-790) and
// GraphConstructionImpl::build/refine (src/ggnn/construction/graph_construction.cu:128-147).
//
// MI355X-first choices: every shard of the base and its graph stay resident in HBM (288 GB), so
// the reference's GPU<->CPU<->disk swapping is not reproduced; one engine drives one GPU
// (multi-GPU = one process per GPU, shards exchanged with an RCCL all-gather, see
// ggnn_amd/distributed.py and DESIGN.md).
//
// engine.hpp: the handle and its helper types; the member functions live in
//   engine_residency.cpp  base staging, prepare, pre-screen copies, store / load
//   engine_swap.cpp       out-of-core shards: GPU slots <-> pinned host buffers <-> part files
//   engine_build.cpp      build / refine schedule of one GPU
//   engine_query.cpp      shard loop, blocking / split / asynchronous query, bf_query
//   engine_exchange.cpp   candidates between the GPUs of one handle: RCCL all-gather, peer copies
//   engine_cabi.cpp       extern "C" entry points (include/ggnn_c.h)
#pragma once
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <exception>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "common.hpp"
#include "hooks.hpp"

namespace ggnn_amd {

struct DeviceBuffer {
  void* p{nullptr};
  size_t bytes{0};
  DeviceBuffer() = default;
  explicit DeviceBuffer(size_t n) { alloc(n); }
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  DeviceBuffer(DeviceBuffer&& o) noexcept : p(o.p), bytes(o.bytes)
  {
    o.p = nullptr;
    o.bytes = 0;
  }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept
  {
    if (this != &o) {
      release();
      p = o.p;
      bytes = o.bytes;
      o.p = nullptr;
      o.bytes = 0;
    }
    return *this;
  }
  ~DeviceBuffer() { release(); }
  void alloc(size_t n)
  {
    release();
    if (n) {
      GGNN_HIP_CHECK(hipMalloc(&p, n));
      bytes = n;
    }
  }
  void release()
  {
    if (p)
      (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <typename T>
  T* as() const
  {
    return static_cast<T*>(p);
  }
};

// page-locked host memory (slice copies of the multi-GPU exchange: a D2H copy into pageable
// memory is staged and serialised by the runtime)
struct PinnedBuffer {
  void* p{nullptr};
  size_t bytes{0};
  PinnedBuffer() = default;
  PinnedBuffer(const PinnedBuffer&) = delete;
  PinnedBuffer& operator=(const PinnedBuffer&) = delete;
  PinnedBuffer(PinnedBuffer&& o) noexcept : p(o.p), bytes(o.bytes)
  {
    o.p = nullptr;
    o.bytes = 0;
  }
  PinnedBuffer& operator=(PinnedBuffer&& o) noexcept
  {
    if (this != &o) {
      release();
      p = o.p;
      bytes = o.bytes;
      o.p = nullptr;
      o.bytes = 0;
    }
    return *this;
  }
  ~PinnedBuffer() { release(); }
  void grow(size_t n)
  {
    if (bytes >= n)
      return;
    release();
    GGNN_HIP_CHECK(hipHostMalloc(&p, n, hipHostMallocDefault));
    bytes = n;
  }
  void release()
  {
    if (p)
      (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
  }
};

// HIP-event stopwatch on one stream, on two events owned by the caller (DeviceCtx creates them
// once: creating and destroying events costs ~10 us per query() otherwise)
struct EventTimer {
  hipEvent_t a, b;
  hipStream_t s;
  EventTimer(hipStream_t stream, hipEvent_t ev_a, hipEvent_t ev_b) : a(ev_a), b(ev_b), s(stream)
  {
    GGNN_HIP_CHECK(hipEventRecord(a, s));
  }
  float stop()
  {
    float ms = 0.f;
    GGNN_HIP_CHECK(hipEventRecord(b, s));
    GGNN_HIP_CHECK(hipEventSynchronize(b));
    GGNN_HIP_CHECK(hipEventElapsedTime(&ms, a, b));
    return ms;
  }
};

// graph pool of one shard, reference layout (src/ggnn/base/graph.cpp:48-91):
// [N_all x K int32 graph][ST_all int32 translation][ST_all int32 selection][2 float nn1_stats]
struct Shard {
  uint32_t global_id{0};
  DeviceBuffer pool;
  int32_t* graph{nullptr};
  int32_t* translation{nullptr};
  int32_t* selection{nullptr};
  float* nn1_stats{nullptr};
  bool ready{false};
  // 8-bit pre-screen copy of this shard's rows (prescreen.hip) for ps_measure, made when a
  // float32 build or query first needs it: 0 = not attempted, 1 = usable, -1 = data not codable
  // (non-finite values)
  DeviceBuffer ps_codes, ps_params;
  int ps_state{0};
  bool ps_lossless{false};  // params[5] of the copy: lossless on a power-of-two grid (squared L2)
  ggnn_measure ps_measure{GGNN_EUCLIDEAN};

  static size_t pool_bytes(const ggnn_graph_config& c)
  {
    return (static_cast<size_t>(c.N_all) * c.KBuild + 2 * static_cast<size_t>(c.ST_all)) * 4 +
           2 * sizeof(float);
  }
  // out-of-core shards: the pool is a slot buffer of the GPU's SwapState
  void view(const ggnn_graph_config& c, void* slot_pool)
  {
    graph = static_cast<int32_t*>(slot_pool);
    translation = graph + static_cast<size_t>(c.N_all) * c.KBuild;
    selection = translation + c.ST_all;
    nn1_stats = reinterpret_cast<float*>(selection + c.ST_all);
  }
  void allocate(const ggnn_graph_config& c)
  {
    pool.alloc(align8(pool_bytes(c)));
    graph = pool.as<int32_t>();
    translation = graph + static_cast<size_t>(c.N_all) * c.KBuild;
    selection = translation + c.ST_all;
    nn1_stats = reinterpret_cast<float*>(selection + c.ST_all);
  }
};

}  // namespace ggnn_amd

using namespace ggnn_amd;

// the engine switches devices (hipSetDevice) while it works, and so does destroying a DeviceCtx;
// callers such as PyTorch keep their own notion of the current device, so every entry point leaves
// it as it found it
struct DeviceRestoreGuard {
  int prev{-1};
  DeviceRestoreGuard() { (void)hipGetDevice(&prev); }
  ~DeviceRestoreGuard()
  {
    int now = -1;
    if (prev >= 0 && hipGetDevice(&now) == hipSuccess && now != prev)
      (void)hipSetDevice(prev);
  }
};

// RCCL entry points, resolved at run time the first time a handle that drives several GPUs
// exchanges results: single-GPU use never loads the library (torch ships its own copy of
// librccl.so.1; the loader hands back that copy when it is already in the process).
struct Rccl {
  decltype(&ncclCommInitAll) CommInitAll{nullptr};
  decltype(&ncclCommDestroy) CommDestroy{nullptr};
  decltype(&ncclAllGather) AllGather{nullptr};
  decltype(&ncclGroupStart) GroupStart{nullptr};
  decltype(&ncclGroupEnd) GroupEnd{nullptr};
  decltype(&ncclGetErrorString) GetErrorString{nullptr};
  decltype(&ncclCommCount) CommCount{nullptr};  // optional (tracing only)
  bool ok{false};

  static const Rccl& get()
  {
    static const Rccl r = [] {
      Rccl x;
      void* lib = nullptr;
      for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (lib)
          break;
      }
      if (!lib)
        return x;
      auto sym = [&](const char* n) { return dlsym(lib, n); };
      x.CommInitAll = reinterpret_cast<decltype(x.CommInitAll)>(sym("ncclCommInitAll"));
      x.CommDestroy = reinterpret_cast<decltype(x.CommDestroy)>(sym("ncclCommDestroy"));
      x.AllGather = reinterpret_cast<decltype(x.AllGather)>(sym("ncclAllGather"));
      x.GroupStart = reinterpret_cast<decltype(x.GroupStart)>(sym("ncclGroupStart"));
      x.GroupEnd = reinterpret_cast<decltype(x.GroupEnd)>(sym("ncclGroupEnd"));
      x.GetErrorString = reinterpret_cast<decltype(x.GetErrorString)>(sym("ncclGetErrorString"));
      x.CommCount = reinterpret_cast<decltype(x.CommCount)>(sym("ncclCommCount"));
      x.ok = x.CommInitAll && x.CommDestroy && x.AllGather && x.GroupStart && x.GroupEnd &&
             x.GetErrorString;
      return x;
    }();
    return r;
  }
};
// a failed RCCL call: the only kind of error the exchange answers with its peer-copy fallback
struct RcclError : Error {
  using Error::Error;
};
#define GGNN_RCCL_CHECK(expr)                                                              \
  do {                                                                                     \
    ncclResult_t _r = (expr);                                                              \
    if (_r != ncclSuccess)                                                                 \
      throw RcclError(GGNN_DEVICE_ERROR, std::string(#expr) + ": " +           \
                                                         Rccl::get().GetErrorString(_r));  \
  } while (0)

// Out-of-core shards of one GPU (reference: GPUInstance's d_buffers / h_buffers /
// part files, gpu_instance.cu:135-227, 371-497).  Only when the shards of a GPU do not fit next
// to each other -- at every BASELINE configuration they do, and then none of this exists:
//   * `slots` GPU buffers (graph pool + base shard); local shard s lives in slot s % slots;
//   * `host.size()` page-locked host buffers for the graph pools (shard s in buffer s % host
//     buffers; ggnn_set_cpu_memory_limit bounds them), the rest as part_<shard>.ggnn files in
//     the working directory -- the reference's three tiers;
//   * one copy stream: the shard a query needs next is uploaded while the current one is
//     searched (the reference uses one io thread per buffer for the same purpose).
struct SwapState {
  int device{0};
  uint32_t slots{0};
  std::vector<DeviceBuffer> pool, base;     // [slots]
  std::vector<int> pool_shard, base_shard;  // local shard held, -1: none
  std::vector<PinnedBuffer> host;           // [host buffers]
  std::vector<int> host_shard;
  std::vector<uint8_t> on_disk;             // [shards per GPU]: part file is current
  hipStream_t io{nullptr};
  std::vector<hipEvent_t> uploaded, consumed;  // [slots]: copies done (io) / last kernel done (ctx)
  bool base_borrowed{false};                // the base slice is device memory of this GPU already
  SwapState() = default;
  SwapState(const SwapState&) = delete;
  SwapState& operator=(const SwapState&) = delete;
  ~SwapState()
  {
    if (io || !uploaded.empty()) {
      (void)hipSetDevice(device);
      for (hipEvent_t e : uploaded)
        if (e)
          (void)hipEventDestroy(e);
      for (hipEvent_t e : consumed)
        if (e)
          (void)hipEventDestroy(e);
      if (io)
        (void)hipStreamDestroy(io);
    }
  }
};

// everything one GPU owns (GPUInstance of the reference, gpu_instance.cuh:60-221, reduced to
// resident shards)
struct DeviceCtx {
  int device{0};
  hipStream_t stream{nullptr};
  hipEvent_t ev_a{nullptr}, ev_b{nullptr};  // timing events, created with the stream
  DeviceBuffer base_copy;       // this GPU's slice of the base unless it is borrowed
  const void* d_base{nullptr};  // first row of the slice
  uint32_t first_shard{0};      // global id of shards[0]
  std::vector<Shard> shards;
  float build_ms{0.f}, query_ms{0.f};
  uint64_t n_dist{0}, n_pop{0}, n_float_rows{0}, n_code_rows{0};
  // several resident shards: their query kernels run on a few extra streams so that the thin tail
  // of one launch overlaps with the head of the next (the reference also uses per-shard streams,
  // gpu_instance.cu:626-743)
  static constexpr int kShardStreams = 4;
  hipStream_t shard_stream[kShardStreams] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t shard_done[kShardStreams] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_ready{nullptr};
  DeviceBuffer bf_rescanned;    // one uint32: queries of the last bf_query answered by the scan
  // staging of a blocking call's filter when the caller's memory is not on this GPU (resolve_filter):
  // the allowed-id bitset, and the filter ids / query labels
  DeviceBuffer filter_stage, filter_ids_stage;
  // per-query filters: this GPU's copy of the handle's filter table, [(F + 2) x words] -- the F
  // rows, then the all-ones and the all-zero row that the ids -1 / out of range read -- current when
  // filter_table_epoch equals the handle's
  DeviceBuffer filter_table;
  uint64_t filter_table_epoch{0};
  // label filters: this GPU's copy of the handle's label column, int32 [N] over the global ids,
  // current when labels_epoch equals the handle's
  DeviceBuffer labels;
  uint64_t labels_epoch{0};
  std::unique_ptr<SwapState> swap;  // out-of-core shards (null: every shard resident)
  // Result staging of query() / query_async(): grown on demand, kept between calls.  One set per
  // lane: lanes [0, kShardStreams) belong to the asynchronous slots (their streams), lane
  // kBlockingLane to the blocking query(): its staging, exchange and result copies run on `stream`,
  // but with several resident shards its per-shard search launches are spread over the SAME
  // shard_stream[] the asynchronous slots use (ordered behind whatever a slot has in flight there;
  // the blocking call waits for all of them before it returns).  Ids and distance bit patterns share ONE
  // buffer so that the exchange is one collective: r_pack = [ids: Nq x row][dists: Nq x row].
  static constexpr int kBlockingLane = kShardStreams;
  struct ExchangeBufs {
    DeviceBuffer q_stage;  // the query set on this GPU when it has to be copied (async lanes)
    DeviceBuffer f_stage;  // ... and its filter ids (query_async with filter ids)
    DeviceBuffer r_pack;   // this GPU's sorted rows, ids then distances
    DeviceBuffer g_pack;   // r_pack of all GPUs after the exchange, [G][2 * Nq * row]
    DeviceBuffer m_pack;   // merged results, [ids: Nq x K][dists: Nq x K] (this GPU's slice filled)
    PinnedBuffer h_pack;   // the merged slice on the host, [ids: count x K][dists: count x K]
    hipEvent_t done{nullptr};  // local search of this lane finished (copy exchange)
    // (first GPU, copy exchange of asynchronous batches) the rows of every GPU have been copied
    // out: their owners may overwrite them with the next batch of this lane
    hipEvent_t consumed{nullptr};
  };
  ExchangeBufs xb[kShardStreams + 1];
  hipStream_t lane_stream(int lane) const
  {
    return lane == kBlockingLane ? stream : shard_stream[lane];
  }
  static void grow(DeviceBuffer& b, size_t bytes)
  {
    if (b.bytes < bytes)
      b.alloc(bytes);
  }

  DeviceCtx() = default;
  DeviceCtx(const DeviceCtx&) = delete;
  DeviceCtx& operator=(const DeviceCtx&) = delete;
  DeviceCtx(DeviceCtx&& o) noexcept { *this = std::move(o); }
  DeviceCtx& operator=(DeviceCtx&& o) noexcept
  {
    device = o.device;
    stream = o.stream;
    ev_a = o.ev_a;
    ev_b = o.ev_b;
    ev_ready = o.ev_ready;
    for (int i = 0; i < kShardStreams; ++i) {
      shard_stream[i] = o.shard_stream[i];
      shard_done[i] = o.shard_done[i];
      o.shard_stream[i] = nullptr;
      o.shard_done[i] = nullptr;
    }
    o.stream = nullptr;
    o.ev_a = o.ev_b = o.ev_ready = nullptr;
    base_copy = std::move(o.base_copy);
    bf_rescanned = std::move(o.bf_rescanned);
    filter_table = std::move(o.filter_table);
    filter_table_epoch = o.filter_table_epoch;
    o.filter_table_epoch = 0;
    labels = std::move(o.labels);
    labels_epoch = o.labels_epoch;
    o.labels_epoch = 0;
    for (int i = 0; i <= kShardStreams; ++i) {
      xb[i].q_stage = std::move(o.xb[i].q_stage);
      xb[i].f_stage = std::move(o.xb[i].f_stage);
      xb[i].r_pack = std::move(o.xb[i].r_pack);
      xb[i].g_pack = std::move(o.xb[i].g_pack);
      xb[i].m_pack = std::move(o.xb[i].m_pack);
      xb[i].h_pack = std::move(o.xb[i].h_pack);
      xb[i].done = o.xb[i].done;
      o.xb[i].done = nullptr;
      xb[i].consumed = o.xb[i].consumed;
      o.xb[i].consumed = nullptr;
    }
    d_base = o.d_base;
    first_shard = o.first_shard;
    shards = std::move(o.shards);
    swap = std::move(o.swap);
    return *this;
  }
  ~DeviceCtx()
  {
    if (stream) {
      (void)hipSetDevice(device);
      (void)hipEventDestroy(ev_a);
      (void)hipEventDestroy(ev_b);
      if (ev_ready)
        (void)hipEventDestroy(ev_ready);
      for (int i = 0; i < kShardStreams; ++i)
        if (shard_stream[i]) {
          (void)hipEventDestroy(shard_done[i]);
          (void)hipStreamDestroy(shard_stream[i]);
        }
      for (int i = 0; i <= kShardStreams; ++i) {
        if (xb[i].done)
          (void)hipEventDestroy(xb[i].done);
        if (xb[i].consumed)
          (void)hipEventDestroy(xb[i].consumed);
      }
      (void)hipStreamDestroy(stream);
    }
  }
  void activate()
  {
    GGNN_HIP_CHECK(hipSetDevice(device));
    if (!stream) {
      GGNN_HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
      GGNN_HIP_CHECK(hipEventCreate(&ev_a));
      GGNN_HIP_CHECK(hipEventCreate(&ev_b));
    }
  }
  // (after activate(); created with the first multi-shard query)
  void ensure_shard_streams()
  {
    if (shard_stream[0])
      return;
    GGNN_HIP_CHECK(hipEventCreateWithFlags(&ev_ready, hipEventDisableTiming));
    for (int i = 0; i < kShardStreams; ++i) {
      GGNN_HIP_CHECK(hipStreamCreateWithFlags(&shard_stream[i], hipStreamNonBlocking));
      GGNN_HIP_CHECK(hipEventCreateWithFlags(&shard_done[i], hipEventDisableTiming));
    }
  }
};

struct ggnn_handle;

// One blocking or asynchronous call as the C-ABI received it: the query set, the search parameters
// and where the results go (bf_query reads neither tau nor max_iterations).
struct QueryRequest {
  const void* q;
  uint64_t Nq;
  uint32_t D;
  ggnn_dtype dtype;
  ggnn_location loc;
  int gpu;
  uint32_t k;
  ggnn_measure measure;
  int32_t* ids_out;
  float* dists_out;
  ggnn_location out_loc;
  float tau{0.f};
  uint32_t max_iterations{0};
};

// The filter of one call as the caller gave it: nothing, one allowed-id bitset for the whole batch
// (count = n_bits), a row of the resident filter table per query, or a label per query (count =
// Nq).  The three constructors validate against the handle; a search is filtered iff it is handed
// one of these, never by anything the handle remembers.
struct QueryFilter {
  enum Kind { None, Bitset, TableIds, Labels, LabelSets, LabelRanges, LabelMasks } kind{None};
  const void* ptr{nullptr};
  uint64_t count{0};
  ggnn_location loc{GGNN_CPU};
  int gpu{0};
  // LabelSets: ptr is the [Nq x width] label sets (count = Nq * width) and ids the filter id per
  // query ([Nq], or null: labels only), each with its own location.  LabelRanges: the same with
  // ptr the [Nq x width x 2] (lo, hi) pairs, width = n_ranges (count = Nq * width * 2).  LabelMasks:
  // ptr the [Nq x width x 3] (mask, value, any) clauses, width = n_masks (count = Nq * width * 3)
  uint32_t width{0};
  // int32 words of ptr per query
  uint32_t stride() const
  {
    return kind == LabelMasks ? 3 * width : kind == LabelRanges ? 2 * width : width;
  }
  const int32_t* ids{nullptr};
  ggnn_location ids_loc{GGNN_CPU};
  int ids_gpu{0};
  static QueryFilter bitset(const ggnn_handle& h, const uint32_t* bits, uint64_t n_bits,
                            ggnn_location loc, int gpu);
  // read_host_ids: ids in host memory are range-checked here (the blocking calls; the asynchronous
  // ones do not read them, include/ggnn_c.h)
  static QueryFilter table_ids(const ggnn_handle& h, const int32_t* ids, uint64_t Nq,
                               ggnn_location loc, int gpu, bool read_host_ids = true);
  static QueryFilter labels(const ggnn_handle& h, const int32_t* query_labels, uint64_t Nq,
                            ggnn_location loc, int gpu);
  static QueryFilter label_sets(const ggnn_handle& h, const int32_t* sets, uint32_t width,
                                uint64_t Nq, ggnn_location loc, int gpu, const int32_t* ids,
                                ggnn_location ids_loc, int ids_gpu, bool read_host_ids = true);
  // (the range values are not validated: every int32 is a valid bound)
  static QueryFilter label_ranges(const ggnn_handle& h, const int32_t* ranges, uint32_t n_ranges,
                                  uint64_t Nq, ggnn_location loc, int gpu, const int32_t* ids,
                                  ggnn_location ids_loc, int ids_gpu, bool read_host_ids = true);
  // (no clause value is invalid: only n_masks is checked)
  static QueryFilter label_masks(const ggnn_handle& h, const int32_t* masks, uint32_t n_masks,
                                 uint64_t Nq, ggnn_location loc, int gpu, const int32_t* ids,
                                 ggnn_location ids_loc, int ids_gpu, bool read_host_ids = true);
};

// A QueryFilter on one GPU, as a launch takes it (filter_bits / filter_table of QueryLaunch and
// BfLaunch): bits is the bitset, the resident table (table.ids set) or the resident label column
// (table.query_labels set); all null: unfiltered.  Label sets: set.labels is the resident label column
// and bits / table.ids the resident table and the filter ids, or null; label ranges: the same with
// `ranges` in place of `set`; label masks: with `masks`.
struct DeviceFilter {
  const uint32_t* bits{nullptr};
  FilterTable table{};
  LabelSetSpec set{};
  LabelRangeSpec ranges{};
  LabelMaskSpec masks{};
  // ... of the queries from `first` on (a half-batch; a bitset is shared by all queries)
  DeviceFilter from(uint32_t first) const
  {
    DeviceFilter d = *this;
    if (d.table.ids)
      d.table.ids += first;
    if (d.table.query_labels)
      d.table.query_labels += first;
    if (d.set.sets)
      d.set.sets += static_cast<size_t>(first) * d.set.width;
    if (d.ranges.ranges)
      d.ranges.ranges += static_cast<size_t>(first) * d.ranges.n_ranges * 2;
    if (d.masks.masks)
      d.masks.masks += static_cast<size_t>(first) * d.masks.n_masks * 3;
    return d;
  }
};

struct ggnn_handle {
  // configuration (GGNNConfig, ggnn.cu:52-59)
  std::filesystem::path graph_dir{};
  size_t cpu_memory_limit{static_cast<size_t>(-1)};
  size_t reserved_gpu_memory{0};
  std::vector<int> gpu_ids{};
  uint32_t N_shard{0};
  bool return_results_on_gpu{false};
  bool collect_counters{false};
  bool prescreen{hook(kHookPrescreen) != 0};  // ggnn_set_prescreen() per handle

  // deterministic-build hooks (ggnn_set_build_hooks): injected selection random numbers
  // ([layers-1][N_shard], shard-local) and sym launched one point at a time in ascending order
  std::vector<float> hook_rng;
  int hook_serial_sym{0};  // 1: one point per sym launch, 2: deterministic sym (sym.hip)

  // base as handed over by the caller
  const void* base_src{nullptr};
  ggnn_location base_loc{GGNN_CPU};
  int base_gpu{0};
  std::vector<uint8_t> base_host_copy;
  bool base_host_copy_registered{false};  // page-locked (hipHostRegister) while shards swap
  void pin_host_copy();
  void drop_host_copy();
  DeviceBuffer base_dev_copy;
  uint64_t base_N{0};
  uint32_t base_D{0};  // dimension as given by the caller
  uint32_t pad_D{0};   // row length the kernels see: rows are zero-padded to a multiple of 16 bytes
                       // (zeros change neither the L2 nor the cosine distance)
  ggnn_dtype base_dtype{GGNN_F32};
  bool base_set{false};

  // graph: one DeviceCtx per GPU, shards_per_gpu resident shards each
  bool prepared{false};
  ggnn_graph_config cfg{};
  uint32_t shards_per_gpu{0};
  std::vector<DeviceCtx> devs;

  // tracing
  float build_ms{0.f}, query_ms{0.f}, bf_ms{0.f};
  uint64_t last_n_dist{0}, last_n_pop{0}, last_float_rows{0}, last_code_rows{0};
  ggnn_build_work build_work{};  // collect_counters during build(): see ggnn_last_build_work
  std::mutex build_work_mutex;   // one host thread per GPU accounts into it
  uint32_t last_bf_rescanned{0};
  int last_bf_matrix_path{0};  // the last bf_query ran the tile kernels (bf_mfma.hip) on every shard
  // per-query filters.  The table as ggnn_set_filters copied it, [num_filters x filter_words]
  // words on the host (placed on a GPU when a context exists: place_filter_table)
  std::vector<uint32_t> filter_table_host;
  uint32_t num_filters{0};
  uint32_t filter_words{0};
  uint64_t filter_epoch{0};  // counts ggnn_set_filters calls: a context with another value is stale
  // label filters.  The label column as ggnn_set_labels copied it, one int32 per base vector on the
  // host (placed on a GPU when a context exists: place_labels); empty: no labels
  std::vector<int32_t> labels_host;
  uint64_t labels_epoch{0};  // counts ggnn_set_labels calls: a context with another value is stale

  std::string last_error;

  // one RCCL communicator per GPU of a multi-GPU handle (created with the first exchange)
  std::vector<ncclComm_t> comms;
  int rccl_state{0};  // 0 = not tried, 1 = communicators ready, -1 = unavailable (peer copies)
  uint32_t rccl_fallbacks{0};  // exchanges that failed inside RCCL and were served by peer copies
  const char* last_exchange{"none"};
  uint32_t last_query_parts{1};  // half-batches the last blocking query was searched in

  ~ggnn_handle()
  {
    destroy_comms();
    if (base_host_copy_registered)
      (void)hipHostUnregister(base_host_copy.data());
  }
  void destroy_comms();
  bool ensure_comms();

  size_t row_bytes() const { return static_cast<size_t>(pad_D) * dtype_size(base_dtype); }
  uint32_t num_shards() const { return shards_per_gpu * static_cast<uint32_t>(devs.size()); }
  bool has_graph() const;
  void rollback_graph();

  // runs f(ctx) for every GPU -- inline for one GPU, one host thread per GPU otherwise (the
  // reference does the same, ggnn.cu:218-230,308-326); the first failure is rethrown
  template <typename F>
  void for_each_device(F&& f)
  {
    if (devs.size() == 1) {
      devs[0].activate();
      f(devs[0]);
      return;
    }
    std::vector<std::thread> pool;
    std::vector<std::exception_ptr> errors(devs.size());
    for (size_t i = 0; i < devs.size(); ++i)
      pool.emplace_back([&, i] {
        try {
          devs[i].activate();
          f(devs[i]);
        }
        catch (...) {
          errors[i] = std::current_exception();
        }
      });
    for (auto& t : pool)
      t.join();
    for (auto& e : errors)
      if (e)
        std::rethrow_exception(e);
  }

  std::vector<int> resolve_gpus() const;

  void stage_base_slice(DeviceCtx& ctx, uint64_t row0, uint64_t rows);

  const void* shard_base(const DeviceCtx& ctx, uint32_t local_shard) const;

  // ---- out-of-core shards (SwapState) -----------------------------------------------------------
  bool swapping() const { return !devs.empty() && devs[0].swap != nullptr; }

  uint32_t plan_gpu_slots(const DeviceCtx& ctx, uint32_t spg, bool base_on_this_gpu) const;

  void setup_swap(DeviceCtx& ctx, uint32_t slots, bool base_on_this_gpu);

  void upload_base_shard(DeviceCtx& ctx, uint32_t si, hipStream_t st);

  void* host_pool_of(DeviceCtx& ctx, uint32_t si);

  void acquire_shard(DeviceCtx& ctx, uint32_t si, hipStream_t st, bool with_graph = true);
  void shard_consumed(DeviceCtx& ctx, uint32_t si, hipStream_t st);
  void retire_built_shard(DeviceCtx& ctx, uint32_t si);
  void write_part(uint32_t global_shard, const void* host);
  void read_part(uint32_t global_shard, void* host);

  void prepare(uint32_t KBuild);

  void build_device(DeviceCtx& ctx, float tau_build, uint32_t refinement_iterations,
                    ggnn_measure measure);

  void build(uint32_t KBuild, float tau_build, uint32_t refinement_iterations,
             ggnn_measure measure);

  void release_caller_copy();

  struct Staged {
    const void* ptr{nullptr};
    DeviceBuffer owned;
  };
  void check_query(uint64_t Nq, uint32_t D, ggnn_dtype dtype, const void* q) const;
  Staged stage_query(DeviceCtx& ctx, const void* q, uint64_t Nq, uint32_t D, ggnn_dtype dtype,
                     ggnn_location loc, int q_gpu);

  bool ensure_prescreen(DeviceCtx& ctx, uint32_t si, ggnn_measure measure);

  // the filter of a call on ctx's GPU: the caller's memory where it lives there, else copied on
  // the lane's stream (blocking lane: ctx.filter_stage / filter_ids_stage, a slot's lane: its
  // f_stage); the resident table or label column is placed if it is missing or stale
  DeviceFilter resolve_filter(DeviceCtx& ctx, const QueryFilter& f, int lane);
  // label sets, label ranges and label masks: the resident column (`column`) and table, and the
  // queries' int32 rows (f.stride() words each, returned in `rows`) and ids in place or staged
  DeviceFilter resolve_label_rows(DeviceCtx& ctx, const QueryFilter& f, int lane,
                                  const int32_t*& column, const int32_t*& rows);
  DeviceFilter resolve_label_sets(DeviceCtx& ctx, const QueryFilter& f, int lane);
  DeviceFilter resolve_label_ranges(DeviceCtx& ctx, const QueryFilter& f, int lane);
  DeviceFilter resolve_label_masks(DeviceCtx& ctx, const QueryFilter& f, int lane);

  // the search of local shard si for nq queries of request r, without work counters
  QueryLaunch shard_launch(const DeviceCtx& ctx, uint32_t si, const QueryRequest& r,
                           const void* d_query, uint32_t nq, int32_t* d_ids, float* d_dists,
                           bool use_prescreen, const DeviceFilter& df) const;

  void query_device(DeviceCtx& ctx, const QueryRequest& r, const void* d_query, int32_t* d_ids,
                    float* d_dists, const QueryFilter& filter);

  void query(const QueryRequest& r, const QueryFilter& filter);
  void query_split(const QueryRequest& r, const QueryFilter& filter);

  // per-query filters (engine_query.cpp)
  void set_filters(const uint32_t* bits, uint32_t F, uint64_t n_bits, ggnn_location loc, int gpu);
  void update_filter(uint32_t index, const uint32_t* bits, uint64_t n_bits, ggnn_location loc,
                     int gpu);
  void drop_filters();
  // ctx's copy of the table, placed now if it is missing or stale (synchronous; ctx is active)
  const uint32_t* place_filter_table(DeviceCtx& ctx);
  void place_filter_tables();  // ... on every context there is

  // label filters (engine_query.cpp)
  void set_labels(const int32_t* labels, uint64_t n, ggnn_location loc, int gpu);
  void update_labels(const int64_t* ids, const int32_t* values, uint64_t count, ggnn_location loc,
                     int gpu);
  void drop_labels();
  // ctx's copy of the label column, placed now if it is missing or stale (synchronous; ctx is
  // active)
  const int32_t* place_labels(DeviceCtx& ctx);
  void place_labels_everywhere();  // ... on every context there is

  void grow_lane(DeviceCtx& owner, int lane, DeviceBuffer& b, size_t bytes);

  void exchange(int lane, uint32_t nq, uint32_t k_query, size_t row, int32_t* ids_out,
                float* dists_out, bool blocking);

  static void slice_of(uint32_t nq, size_t G, size_t g, uint32_t* first, uint32_t* count);

  void return_slice(DeviceCtx& ctx, int lane, uint32_t nq, uint32_t k_query, uint32_t first,
                    uint32_t count, int32_t* ids_out, float* dists_out, bool blocking);
  void finish_slices(int lane, uint32_t nq, uint32_t k_query, size_t G_slices, int32_t* ids_out,
                     float* dists_out);

  void exchange_rccl(int lane, uint32_t nq, uint32_t k_query, size_t row, int32_t* ids_out,
                     float* dists_out, bool blocking);

  void exchange_peer_copies(int lane, uint32_t nq, uint32_t k_query, size_t row, int32_t* ids_out,
                            float* dists_out, bool blocking);
  void merge_slices(int lane, uint32_t nq, uint32_t k_query, size_t row, int32_t* ids_out,
                    float* dists_out, bool blocking);
  void exchange_gather_copies(int lane, uint32_t nq, uint32_t k_query, size_t row, int32_t* ids_out,
                              float* dists_out);

  void query_async(const QueryRequest& r, uint32_t slot, const QueryFilter& filter);

  void enqueue_local_search(DeviceCtx& ctx, int lane, const QueryRequest& r, const void* d_query,
                            uint32_t nq, int32_t* d_ids, float* d_dists, const DeviceFilter& df);
  void synchronize_slot(uint32_t slot);
  void synchronize();

  void bf_query(const QueryRequest& r, const QueryFilter& filter);
  // r.k is not used; radii[Nq] and lims_out[Nq + 1] are host memory, r.ids_out / r.dists_out hold
  // `capacity` entries at r.out_loc
  void bf_range_query(const QueryRequest& r, const float* radii, uint64_t capacity,
                      uint64_t* lims_out, const QueryFilter& filter);
  // the staging of the exhaustive calls (engine_query.cpp)
  DeviceCtx& bf_context(uint64_t Nq, uint32_t D, ggnn_dtype dtype, const void* q);
  const void* bf_whole_base(DeviceCtx& ctx, DeviceBuffer& whole_base);

  std::filesystem::path part_file(uint32_t shard) const;

  void store();

  void load(uint32_t KBuild);
  void load_shards();
};
