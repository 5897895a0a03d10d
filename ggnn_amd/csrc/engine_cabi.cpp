// extern "C" entry points of libggnn_amd.so (include/ggnn_c.h): handle API and operator seam.
// Every call is guarded: exceptions become status codes + ggnn_last_error().
#include "engine.hpp"
#include "traversal.hpp"

namespace {
thread_local std::string g_create_error;

template <typename F>
ggnn_status guarded(ggnn_t* h, F&& f)
{
  DeviceRestoreGuard restore;
  try {
    f();
    return GGNN_OK;
  }
  catch (const Error& e) {
    (h ? h->last_error : g_create_error) = e.what();
    return e.status;
  }
  catch (const std::bad_alloc&) {
    (h ? h->last_error : g_create_error) = "out of host memory";
    return GGNN_OUT_OF_MEMORY;
  }
  catch (const std::exception& e) {
    (h ? h->last_error : g_create_error) = e.what();
    return GGNN_DEVICE_ERROR;
  }
}

#define GGNN_NEED_HANDLE(h) \
  if (!(h))                 \
  return GGNN_INVALID_ARGUMENT

// the request of the ggnn_query_async* calls: the query lives on GPU gpu_id or (gpu_id < 0) in host
// memory, and the results go where the exchange puts them
QueryRequest async_request(const void* query, uint64_t Nq, uint32_t D, ggnn_dtype dtype,
                           int gpu_id, uint32_t k_query, float tau_query, uint32_t max_iterations,
                           ggnn_measure measure, int32_t* ids_out, float* dists_out)
{
  return {query, Nq, D, dtype, gpu_id < 0 ? GGNN_CPU : GGNN_GPU, gpu_id, k_query, measure,
          ids_out, dists_out, GGNN_GPU, tau_query, max_iterations};
}

// the QueryLaunch of the ggnn_op_query* seam calls (codes / params / n_rows may be null)
QueryLaunch seam_query(const void* base, ggnn_dtype dtype, uint32_t N_base, uint32_t D,
                       const uint8_t* codes, const float* params, const void* query, uint32_t Nq,
                       const int32_t* graph0, uint32_t KBuild, const int32_t* start,
                       uint32_t num_start, const float* nn1_stats, uint32_t k_query,
                       float tau_query, uint32_t max_iterations, ggnn_measure measure,
                       uint32_t shards_per_gpu, uint32_t on_gpu_shard, int32_t* ids, float* dists,
                       uint32_t* n_dist, uint32_t* n_pop, uint32_t* n_rows)
{
  GGNN_REQUIRE(!codes == !params, GGNN_INVALID_ARGUMENT,
               "pre-screen codes and params go together");
  GGNN_REQUIRE(!codes || dtype == GGNN_F32, GGNN_INVALID_ARGUMENT,
               "the pre-screen needs a float32 base");
  QueryLaunch q{base,      query,          dtype,    N_base,         D,         Nq,
                graph0,    KBuild,         start,    num_start,      nn1_stats, k_query,
                tau_query, max_iterations, measure,  shards_per_gpu, on_gpu_shard, ids,
                dists,     n_dist,         n_pop};
  if (codes) {
    q.ps_codes = codes;
    q.ps_params = params;
    q.ps_Dc = prescreen_code_dim(D);
  }
  q.n_rows = n_rows;
  return q;
}

// the table arguments of the *_filtered_by seam calls as a launch sees them
FilterTable seam_filter_table(const uint32_t* filter_table, uint32_t num_filters, uint64_t n_bits,
                              const int32_t* filter_ids, uint32_t filter_bit_offset,
                              uint32_t N_base)
{
  GGNN_REQUIRE(filter_table != nullptr && num_filters > 0, GGNN_INVALID_ARGUMENT,
               "the filter table is null or empty");
  GGNN_REQUIRE(filter_ids != nullptr, GGNN_INVALID_ARGUMENT, "the filter id array is null");
  GGNN_REQUIRE(n_bits >= static_cast<uint64_t>(filter_bit_offset) + N_base &&
                   n_bits <= 0xffffffffull,
               GGNN_INVALID_ARGUMENT, "a filter needs filter_bit_offset + N_base bits");
  FilterTable t{};
  t.ids = filter_ids;
  t.words = static_cast<uint32_t>((n_bits + 31) / 32);
  t.num_filters = num_filters;
  return t;
}

// the label arguments of the *_labeled seam calls as a launch sees them
FilterTable seam_labels(const int32_t* labels, uint64_t n_labels, const int32_t* query_labels,
                        uint32_t filter_bit_offset, uint32_t N_base)
{
  GGNN_REQUIRE(labels != nullptr, GGNN_INVALID_ARGUMENT, "the label column is null");
  GGNN_REQUIRE(query_labels != nullptr, GGNN_INVALID_ARGUMENT, "the query label array is null");
  GGNN_REQUIRE(n_labels >= static_cast<uint64_t>(filter_bit_offset) + N_base &&
                   n_labels <= 0xffffffffull,
               GGNN_INVALID_ARGUMENT, "the label column needs filter_bit_offset + N_base entries");
  FilterTable t{};
  t.query_labels = query_labels;
  return t;
}

// the label-set arguments of the *_labeled_in seam calls as a launch sees them: fills label_sets,
// filter_bits, filter_bit_offset and filter_table of a QueryLaunch / BfLaunch
template <class LAUNCH>
void seam_label_sets(LAUNCH& l, const int32_t* labels, uint64_t n_labels,
                     const int32_t* query_label_sets, uint32_t set_width,
                     const uint32_t* filter_table, uint32_t num_filters, uint64_t n_bits,
                     const int32_t* filter_ids, uint32_t filter_bit_offset, uint32_t N_base)
{
  GGNN_REQUIRE(labels != nullptr, GGNN_INVALID_ARGUMENT, "the label column is null");
  GGNN_REQUIRE(set_width >= 1 && set_width <= GGNN_MAX_LABEL_SET, GGNN_INVALID_ARGUMENT,
               "set_width must be in [1, 8]");
  GGNN_REQUIRE(query_label_sets != nullptr, GGNN_INVALID_ARGUMENT, "the label set array is null");
  GGNN_REQUIRE(n_labels >= static_cast<uint64_t>(filter_bit_offset) + N_base &&
                   n_labels <= 0xffffffffull,
               GGNN_INVALID_ARGUMENT, "the label column needs filter_bit_offset + N_base entries");
  GGNN_REQUIRE((filter_table != nullptr) == (num_filters > 0), GGNN_INVALID_ARGUMENT,
               "filter_table and num_filters go together");
  GGNN_REQUIRE(!filter_table || (n_bits >= static_cast<uint64_t>(filter_bit_offset) + N_base &&
                                 n_bits <= 0xffffffffull),
               GGNN_INVALID_ARGUMENT, "a filter needs filter_bit_offset + N_base bits");
  l.label_sets.labels = labels;
  l.label_sets.sets = query_label_sets;
  l.label_sets.width = set_width;
  l.filter_bits = filter_ids ? filter_table : nullptr;
  l.filter_bit_offset = filter_bit_offset;
  l.filter_table = FilterTable{};
  if (filter_ids) {
    l.filter_table.ids = filter_ids;
    l.filter_table.words = filter_table ? static_cast<uint32_t>((n_bits + 31) / 32) : 0u;
    l.filter_table.num_filters = num_filters;
  }
}

// the label-range arguments of the *_labeled_range seam calls, likewise: fills label_ranges,
// filter_bits, filter_bit_offset and filter_table
template <class LAUNCH>
void seam_label_ranges(LAUNCH& l, const int32_t* labels, uint64_t n_labels,
                       const int32_t* query_label_ranges, uint32_t n_ranges,
                       const uint32_t* filter_table, uint32_t num_filters, uint64_t n_bits,
                       const int32_t* filter_ids, uint32_t filter_bit_offset, uint32_t N_base)
{
  GGNN_REQUIRE(n_ranges >= 1 && n_ranges <= GGNN_MAX_LABEL_RANGES, GGNN_INVALID_ARGUMENT,
               "n_ranges must be in [1, 4]");
  GGNN_REQUIRE(query_label_ranges != nullptr, GGNN_INVALID_ARGUMENT,
               "the label range array is null");
  // (the column, the table and the ids: the checks and the fields of the label-set seam)
  seam_label_sets(l, labels, n_labels, query_label_ranges, 1, filter_table, num_filters, n_bits,
                  filter_ids, filter_bit_offset, N_base);
  l.label_sets = LabelSetSpec{};
  l.label_ranges.labels = labels;
  l.label_ranges.ranges = query_label_ranges;
  l.label_ranges.n_ranges = n_ranges;
}

// the label-mask arguments of the *_labeled_mask seam calls, likewise: fills label_masks,
// filter_bits, filter_bit_offset and filter_table
template <class LAUNCH>
void seam_label_masks(LAUNCH& l, const int32_t* labels, uint64_t n_labels,
                      const int32_t* query_label_masks, uint32_t n_masks,
                      const uint32_t* filter_table, uint32_t num_filters, uint64_t n_bits,
                      const int32_t* filter_ids, uint32_t filter_bit_offset, uint32_t N_base)
{
  GGNN_REQUIRE(n_masks >= 1 && n_masks <= GGNN_MAX_LABEL_MASKS, GGNN_INVALID_ARGUMENT,
               "n_masks must be in [1, 2]");
  GGNN_REQUIRE(query_label_masks != nullptr, GGNN_INVALID_ARGUMENT,
               "the label mask array is null");
  // (the column, the table and the ids: the checks and the fields of the label-set seam)
  seam_label_sets(l, labels, n_labels, query_label_masks, 1, filter_table, num_filters, n_bits,
                  filter_ids, filter_bit_offset, N_base);
  l.label_sets = LabelSetSpec{};
  l.label_masks.labels = labels;
  l.label_masks.masks = query_label_masks;
  l.label_masks.n_masks = n_masks;
}
}  // namespace

extern "C" {

const char* ggnn_version(void)
{
  return "ggnn_amd 0.1.0 (gfx950)";
}

ggnn_status ggnn_create(ggnn_t** out)
{
  if (!out)
    return GGNN_INVALID_ARGUMENT;
  return guarded(nullptr, [&] { *out = new ggnn_handle(); });
}

void ggnn_destroy(ggnn_t* h)
{
  DeviceRestoreGuard restore;
  delete h;
}

const char* ggnn_last_error(const ggnn_t* h)
{
  return h ? h->last_error.c_str() : g_create_error.c_str();
}

void ggnn_set_log_level(int level)
{
  g_log_level = level;
}

ggnn_status ggnn_set_working_directory(ggnn_t* h, const char* dir)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    // ggnn.cu:69-76
    const std::filesystem::path p = dir ? dir : "";
    const auto target = p.empty() ? std::filesystem::current_path() : std::filesystem::absolute(p);
    // graph parts of out-of-core shards live in the directory they were written to: store() skips
    // them as "already on disk" and read_part() would look for them in the new place
    if (target != h->graph_dir)
      for (const auto& ctx : h->devs)
        if (ctx.swap)
          for (const uint8_t on_disk : ctx.swap->on_disk)
            GGNN_REQUIRE(!on_disk, GGNN_INVALID_STATE,
                         "the working directory cannot change while graph parts of out-of-core "
                         "shards live in " + h->graph_dir.string());
    h->graph_dir = target;
    std::error_code ec;
    std::filesystem::create_directories(h->graph_dir, ec);
    GGNN_REQUIRE(!ec, GGNN_IO_ERROR, "cannot create working directory " + h->graph_dir.string());
  });
}

ggnn_status ggnn_set_cpu_memory_limit(ggnn_t* h, size_t memory_limit)
{
  GGNN_NEED_HANDLE(h);
  h->cpu_memory_limit = memory_limit;
  return GGNN_OK;
}

ggnn_status ggnn_set_reserved_gpu_memory(ggnn_t* h, size_t reserved_memory)
{
  GGNN_NEED_HANDLE(h);
  h->reserved_gpu_memory = reserved_memory;
  return GGNN_OK;
}

ggnn_status ggnn_set_gpus(ggnn_t* h, const int* gpu_ids, size_t num_gpus)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    int count = 0;
    (void)hipGetDeviceCount(&count);
    for (size_t i = 0; i < num_gpus; ++i) {
      // ggnn.cu:94-97 (accepts gpu_id == device count, quirk Q5)
      GGNN_REQUIRE(gpu_ids[i] >= 0 && gpu_ids[i] <= count, GGNN_OUT_OF_RANGE,
                   "Invalid GPU index " + std::to_string(gpu_ids[i]) + " given.");
    }
    h->gpu_ids.assign(gpu_ids, gpu_ids + num_gpus);
  });
}

ggnn_status ggnn_set_shard_size(ggnn_t* h, uint32_t n_shard)
{
  GGNN_NEED_HANDLE(h);
  h->N_shard = n_shard;
  return GGNN_OK;
}

ggnn_status ggnn_set_return_results_on_gpu(ggnn_t* h, int v)
{
  GGNN_NEED_HANDLE(h);
  h->return_results_on_gpu = v != 0;
  return GGNN_OK;
}

ggnn_status ggnn_last_query_rows_read(const ggnn_t* h, uint64_t* float_rows, uint64_t* code_rows)
{
  if (!h)
    return GGNN_INVALID_ARGUMENT;
  if (float_rows)
    *float_rows = h->last_float_rows;
  if (code_rows)
    *code_rows = h->last_code_rows;
  return GGNN_OK;
}

ggnn_status ggnn_set_prescreen(ggnn_t* h, int enable)
{
  GGNN_NEED_HANDLE(h);
  h->prescreen = enable != 0;
  return GGNN_OK;
}

ggnn_status ggnn_last_query_parts(const ggnn_t* h, uint32_t* parts)
{
  GGNN_NEED_HANDLE(h);
  if (!parts)
    return GGNN_INVALID_ARGUMENT;
  *parts = h->last_query_parts;
  return GGNN_OK;
}

ggnn_status ggnn_last_build_work(const ggnn_t* h, ggnn_build_work* out)
{
  GGNN_NEED_HANDLE(h);
  if (!out)
    return GGNN_INVALID_ARGUMENT;
  *out = h->build_work;
  return GGNN_OK;
}

ggnn_status ggnn_set_hook(const char* name, int64_t value)
{
  const int h = ggnn_amd::hook_by_name(name);
  if (h < 0)
    return GGNN_INVALID_ARGUMENT;
  ggnn_amd::hook_set(static_cast<ggnn_amd::Hook>(h), value);
  return GGNN_OK;
}

ggnn_status ggnn_reset_hook(const char* name)
{
  const int h = ggnn_amd::hook_by_name(name);
  if (h < 0)
    return GGNN_INVALID_ARGUMENT;
  ggnn_amd::hook_reset(static_cast<ggnn_amd::Hook>(h));
  return GGNN_OK;
}

ggnn_status ggnn_get_hook(const char* name, int64_t* value)
{
  const int h = ggnn_amd::hook_by_name(name);
  if (h < 0 || !value)
    return GGNN_INVALID_ARGUMENT;
  *value = ggnn_amd::hook(static_cast<ggnn_amd::Hook>(h));
  return GGNN_OK;
}

ggnn_status ggnn_get_shard_layout(const ggnn_t* h, uint32_t* num_shards, uint32_t* shards_per_gpu,
                                  uint32_t* n_shard)
{
  GGNN_NEED_HANDLE(h);
  if (!h->has_graph())
    return GGNN_INVALID_STATE;
  if (num_shards)
    *num_shards = h->num_shards();
  if (shards_per_gpu)
    *shards_per_gpu = h->shards_per_gpu;
  if (n_shard)
    *n_shard = h->cfg.N;
  return GGNN_OK;
}

ggnn_status ggnn_set_collect_counters(ggnn_t* h, int enable)
{
  GGNN_NEED_HANDLE(h);
  h->collect_counters = enable != 0;
  return GGNN_OK;
}

ggnn_status ggnn_set_base(ggnn_t* h, const void* data, uint64_t N, uint32_t D, ggnn_dtype dtype,
                          ggnn_location location, int gpu_id, int take_copy)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    // ggnn.cu:146-152
    GGNN_REQUIRE(!h->prepared, GGNN_INVALID_STATE,
                 "The base cannot be changed once the GPU instances are setup.");
    GGNN_REQUIRE(dtype == GGNN_F32 || dtype == GGNN_U8 || dtype == GGNN_F16 || dtype == GGNN_BF16 ||
                     dtype == GGNN_I8,
                 GGNN_INVALID_ARGUMENT, "unsupported datatype for base");
    // ggnn.cu:466-487: the element type is fixed by the first set_base
    GGNN_REQUIRE(!h->base_set || h->base_dtype == dtype, GGNN_INVALID_ARGUMENT,
                 "base has already been set with a different data type");
    GGNN_REQUIRE(data != nullptr && N > 0 && D > 0, GGNN_INVALID_ARGUMENT, "empty base");
    const size_t bytes = N * D * dtype_size(dtype);
    h->drop_host_copy();
    h->base_dev_copy.release();
    if (h->num_filters)
      h->drop_filters();  // a filter table is over the ids of the base it was set for
    if (!h->labels_host.empty())
      h->drop_labels();  // ... and so is a label column
    h->devs.clear();  // a base staged for an earlier bf_query() is stale now
    h->base_src = data;
    h->base_loc = location;
    h->base_gpu = gpu_id;
    if (take_copy) {
      if (location == GGNN_CPU) {
        h->base_host_copy.assign(static_cast<const uint8_t*>(data),
                                 static_cast<const uint8_t*>(data) + bytes);
        h->base_src = h->base_host_copy.data();
      }
      else {
        GGNN_HIP_CHECK(hipSetDevice(gpu_id));
        h->base_dev_copy.alloc(bytes);
        GGNN_HIP_CHECK(hipMemcpy(h->base_dev_copy.p, data, bytes, hipMemcpyDeviceToDevice));
        h->base_src = h->base_dev_copy.p;
      }
    }
    h->base_N = N;
    h->base_D = D;
    const uint32_t epc = dtype_elems_per_chunk(dtype);
    h->pad_D = (D + epc - 1) / epc * epc;
    h->base_dtype = dtype;
    h->base_set = true;
  });
}

ggnn_status ggnn_build(ggnn_t* h, uint32_t k_build, float tau_build,
                       uint32_t refinement_iterations, ggnn_measure measure)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] { h->build(k_build, tau_build, refinement_iterations, measure); });
}

ggnn_status ggnn_device_clock_hz(int device, double* clock_hz)
{
  return guarded(nullptr, [&] {
    GGNN_REQUIRE(clock_hz != nullptr, GGNN_INVALID_ARGUMENT, "null output");
    int khz = 0;
    GGNN_HIP_CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, device));
    *clock_hz = static_cast<double>(khz) * 1e3;
  });
}

ggnn_status ggnn_set_build_hooks(ggnn_t* h, const float* rng, uint64_t n_rng, int serial_sym)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    GGNN_REQUIRE(rng != nullptr || n_rng == 0, GGNN_INVALID_ARGUMENT, "rng is null");
    h->hook_rng.assign(rng, rng + n_rng);
    GGNN_REQUIRE(serial_sym >= 0 && serial_sym <= 2, GGNN_INVALID_ARGUMENT,
                 "serial_sym must be 0, 1 or 2");
    h->hook_serial_sym = serial_sym;
  });
}

ggnn_status ggnn_store(ggnn_t* h)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] { h->store(); });
}

ggnn_status ggnn_load(ggnn_t* h, uint32_t k_build)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] { h->load(k_build); });
}

ggnn_status ggnn_query(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D, ggnn_dtype dtype,
                       ggnn_location location, int gpu_id, uint32_t k_query, float tau_query,
                       uint32_t max_iterations, ggnn_measure measure, int32_t* ids_out,
                       float* dists_out, ggnn_location out_location)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    h->query({query, Nq, D, dtype, location, gpu_id, k_query, measure, ids_out, dists_out,
              out_location, tau_query, max_iterations},
             QueryFilter{});
  });
}

ggnn_status ggnn_query_async(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                             ggnn_dtype dtype, int gpu_id, uint32_t k_query, float tau_query,
                             uint32_t max_iterations, ggnn_measure measure, int32_t* ids_out,
                             float* dists_out, uint32_t slot)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    h->query_async(async_request(query, Nq, D, dtype, gpu_id, k_query, tau_query, max_iterations,
                                 measure, ids_out, dists_out),
                   slot, QueryFilter{});
  });
}

ggnn_status ggnn_synchronize(ggnn_t* h)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] { h->synchronize(); });
}

ggnn_status ggnn_synchronize_slot(ggnn_t* h, uint32_t slot)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] { h->synchronize_slot(slot); });
}

ggnn_status ggnn_bf_query(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                          ggnn_dtype dtype, ggnn_location location, int gpu_id,
                          uint32_t k_gt, ggnn_measure measure, int32_t* ids_out, float* dists_out,
                          ggnn_location out_location)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    h->bf_query({query, Nq, D, dtype, location, gpu_id, k_gt, measure, ids_out, dists_out,
                 out_location},
                QueryFilter{});
  });
}

// The filtered calls: the filter is an argument of query() / bf_query() like the request.  Its
// constructor runs before the call, so a filter that is wrong is reported before anything else.
ggnn_status ggnn_query_filtered(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                uint32_t k_query, float tau_query, uint32_t max_iterations,
                                ggnn_measure measure, int32_t* ids_out, float* dists_out,
                                ggnn_location out_location, const uint32_t* allowed_bits,
                                uint64_t n_bits, ggnn_location filter_location, int filter_gpu_id)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    h->query({query, Nq, D, dtype, location, gpu_id, k_query, measure, ids_out, dists_out,
              out_location, tau_query, max_iterations},
             QueryFilter::bitset(*h, allowed_bits, n_bits, filter_location, filter_gpu_id));
  });
}

ggnn_status ggnn_bf_query_filtered(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                   ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                   uint32_t k_gt, ggnn_measure measure, int32_t* ids_out,
                                   float* dists_out, ggnn_location out_location,
                                   const uint32_t* allowed_bits, uint64_t n_bits,
                                   ggnn_location filter_location, int filter_gpu_id)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    h->bf_query({query, Nq, D, dtype, location, gpu_id, k_gt, measure, ids_out, dists_out,
                 out_location},
                QueryFilter::bitset(*h, allowed_bits, n_bits, filter_location, filter_gpu_id));
  });
}

ggnn_status ggnn_set_filters(ggnn_t* h, const uint32_t* bits, uint32_t num_filters,
                             uint64_t n_bits, ggnn_location location, int gpu_id)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] { h->set_filters(bits, num_filters, n_bits, location, gpu_id); });
}

ggnn_status ggnn_update_filter(ggnn_t* h, uint32_t index, const uint32_t* bits, uint64_t n_bits,
                               ggnn_location location, int gpu_id)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] { h->update_filter(index, bits, n_bits, location, gpu_id); });
}

ggnn_status ggnn_get_num_filters(const ggnn_t* h, uint32_t* num_filters)
{
  GGNN_NEED_HANDLE(h);
  if (!num_filters)
    return GGNN_INVALID_ARGUMENT;
  *num_filters = h->num_filters;
  return GGNN_OK;
}

ggnn_status ggnn_query_filtered_by(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                   ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                   uint32_t k_query, float tau_query, uint32_t max_iterations,
                                   ggnn_measure measure, int32_t* ids_out, float* dists_out,
                                   ggnn_location out_location, const int32_t* filter_ids,
                                   ggnn_location ids_location, int ids_gpu_id)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    h->query({query, Nq, D, dtype, location, gpu_id, k_query, measure, ids_out, dists_out,
              out_location, tau_query, max_iterations},
             QueryFilter::table_ids(*h, filter_ids, Nq, ids_location, ids_gpu_id));
  });
}

ggnn_status ggnn_bf_query_filtered_by(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                      ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                      uint32_t k_gt, ggnn_measure measure, int32_t* ids_out,
                                      float* dists_out, ggnn_location out_location,
                                      const int32_t* filter_ids, ggnn_location ids_location,
                                      int ids_gpu_id)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    h->bf_query({query, Nq, D, dtype, location, gpu_id, k_gt, measure, ids_out, dists_out,
                 out_location},
                QueryFilter::table_ids(*h, filter_ids, Nq, ids_location, ids_gpu_id));
  });
}

ggnn_status ggnn_query_async_filtered_by(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                         ggnn_dtype dtype, int gpu_id, uint32_t k_query,
                                         float tau_query, uint32_t max_iterations,
                                         ggnn_measure measure, int32_t* ids_out, float* dists_out,
                                         uint32_t slot, const int32_t* filter_ids)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    const QueryRequest r = async_request(query, Nq, D, dtype, gpu_id, k_query, tau_query,
                                         max_iterations, measure, ids_out, dists_out);
    // (the ids live where the query lives and are not read on the host)
    h->query_async(r, slot, QueryFilter::table_ids(*h, filter_ids, Nq, r.loc, r.gpu,
                                                   /*read_host_ids=*/false));
  });
}

ggnn_status ggnn_set_labels(ggnn_t* h, const int32_t* labels, uint64_t n, ggnn_location location,
                            int gpu_id)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] { h->set_labels(labels, n, location, gpu_id); });
}

ggnn_status ggnn_update_labels(ggnn_t* h, const int64_t* ids, const int32_t* values,
                               uint64_t count, ggnn_location location, int gpu_id)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] { h->update_labels(ids, values, count, location, gpu_id); });
}

ggnn_status ggnn_get_num_labels(const ggnn_t* h, uint64_t* n)
{
  GGNN_NEED_HANDLE(h);
  if (!n)
    return GGNN_INVALID_ARGUMENT;
  *n = h->labels_host.size();
  return GGNN_OK;
}

ggnn_status ggnn_label_index_build(const int32_t* labels, uint64_t n, int32_t* keys,
                                   uint32_t* offsets, int32_t* rows, uint32_t* n_keys)
{
  return guarded(nullptr, [&] { label_index_build(labels, n, keys, offsets, rows, n_keys); });
}

ggnn_status ggnn_query_labeled(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                               ggnn_dtype dtype, ggnn_location location, int gpu_id,
                               uint32_t k_query, float tau_query, uint32_t max_iterations,
                               ggnn_measure measure, int32_t* ids_out, float* dists_out,
                               ggnn_location out_location, const int32_t* query_labels,
                               ggnn_location labels_location, int labels_gpu_id)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    h->query({query, Nq, D, dtype, location, gpu_id, k_query, measure, ids_out, dists_out,
              out_location, tau_query, max_iterations},
             QueryFilter::labels(*h, query_labels, Nq, labels_location, labels_gpu_id));
  });
}

ggnn_status ggnn_bf_query_labeled(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                  ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                  uint32_t k_gt, ggnn_measure measure, int32_t* ids_out,
                                  float* dists_out, ggnn_location out_location,
                                  const int32_t* query_labels, ggnn_location labels_location,
                                  int labels_gpu_id)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    h->bf_query({query, Nq, D, dtype, location, gpu_id, k_gt, measure, ids_out, dists_out,
                 out_location},
                QueryFilter::labels(*h, query_labels, Nq, labels_location, labels_gpu_id));
  });
}

// Exact range search (bf_range.hip): the bf_query calls with a radius per query and a CSR result.
#define GGNN_RANGE_REQUEST \
  QueryRequest{query, Nq, D, dtype, location, gpu_id, 0u, measure, ids_out, dists_out, out_location}
ggnn_status ggnn_bf_range_query(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                const float* radii, ggnn_measure measure, uint64_t capacity,
                                uint64_t* lims_out, int32_t* ids_out, float* dists_out,
                                ggnn_location out_location)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    h->bf_range_query(GGNN_RANGE_REQUEST, radii, capacity, lims_out, QueryFilter{});
  });
}

ggnn_status ggnn_bf_range_query_filtered(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                         ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                         const float* radii, ggnn_measure measure,
                                         uint64_t capacity, uint64_t* lims_out, int32_t* ids_out,
                                         float* dists_out, ggnn_location out_location,
                                         const uint32_t* allowed_bits, uint64_t n_bits,
                                         ggnn_location filter_location, int filter_gpu_id)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    h->bf_range_query(GGNN_RANGE_REQUEST, radii, capacity, lims_out,
                      QueryFilter::bitset(*h, allowed_bits, n_bits, filter_location, filter_gpu_id));
  });
}

ggnn_status ggnn_bf_range_query_filtered_by(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                            ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                            const float* radii, ggnn_measure measure,
                                            uint64_t capacity, uint64_t* lims_out,
                                            int32_t* ids_out, float* dists_out,
                                            ggnn_location out_location, const int32_t* filter_ids,
                                            ggnn_location ids_location, int ids_gpu_id)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    h->bf_range_query(GGNN_RANGE_REQUEST, radii, capacity, lims_out,
                      QueryFilter::table_ids(*h, filter_ids, Nq, ids_location, ids_gpu_id));
  });
}

ggnn_status ggnn_bf_range_query_labeled(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                        ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                        const float* radii, ggnn_measure measure,
                                        uint64_t capacity, uint64_t* lims_out, int32_t* ids_out,
                                        float* dists_out, ggnn_location out_location,
                                        const int32_t* query_labels, ggnn_location labels_location,
                                        int labels_gpu_id)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    h->bf_range_query(GGNN_RANGE_REQUEST, radii, capacity, lims_out,
                      QueryFilter::labels(*h, query_labels, Nq, labels_location, labels_gpu_id));
  });
}
#undef GGNN_RANGE_REQUEST

ggnn_status ggnn_query_async_labeled(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                     ggnn_dtype dtype, int gpu_id, uint32_t k_query,
                                     float tau_query, uint32_t max_iterations,
                                     ggnn_measure measure, int32_t* ids_out, float* dists_out,
                                     uint32_t slot, const int32_t* query_labels)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    const QueryRequest r = async_request(query, Nq, D, dtype, gpu_id, k_query, tau_query,
                                         max_iterations, measure, ids_out, dists_out);
    h->query_async(r, slot, QueryFilter::labels(*h, query_labels, Nq, r.loc, r.gpu));
  });
}

ggnn_status ggnn_query_labeled_in(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                  ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                  uint32_t k_query, float tau_query, uint32_t max_iterations,
                                  ggnn_measure measure, int32_t* ids_out, float* dists_out,
                                  ggnn_location out_location, const int32_t* query_label_sets,
                                  uint32_t set_width, ggnn_location sets_location, int sets_gpu_id,
                                  const int32_t* filter_ids, ggnn_location ids_location,
                                  int ids_gpu_id)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    h->query({query, Nq, D, dtype, location, gpu_id, k_query, measure, ids_out, dists_out,
              out_location, tau_query, max_iterations},
             QueryFilter::label_sets(*h, query_label_sets, set_width, Nq, sets_location,
                                     sets_gpu_id, filter_ids, ids_location, ids_gpu_id));
  });
}

ggnn_status ggnn_bf_query_labeled_in(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                     ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                     uint32_t k_gt, ggnn_measure measure, int32_t* ids_out,
                                     float* dists_out, ggnn_location out_location,
                                     const int32_t* query_label_sets, uint32_t set_width,
                                     ggnn_location sets_location, int sets_gpu_id,
                                     const int32_t* filter_ids, ggnn_location ids_location,
                                     int ids_gpu_id)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    h->bf_query({query, Nq, D, dtype, location, gpu_id, k_gt, measure, ids_out, dists_out,
                 out_location},
                QueryFilter::label_sets(*h, query_label_sets, set_width, Nq, sets_location,
                                        sets_gpu_id, filter_ids, ids_location, ids_gpu_id));
  });
}

ggnn_status ggnn_query_async_labeled_in(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                        ggnn_dtype dtype, int gpu_id, uint32_t k_query,
                                        float tau_query, uint32_t max_iterations,
                                        ggnn_measure measure, int32_t* ids_out, float* dists_out,
                                        uint32_t slot, const int32_t* query_label_sets,
                                        uint32_t set_width, const int32_t* filter_ids)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    const QueryRequest r = async_request(query, Nq, D, dtype, gpu_id, k_query, tau_query,
                                         max_iterations, measure, ids_out, dists_out);
    // (sets and ids live where the query lives and are not read on the host)
    h->query_async(r, slot,
                   QueryFilter::label_sets(*h, query_label_sets, set_width, Nq, r.loc, r.gpu,
                                           filter_ids, r.loc, r.gpu, /*read_host_ids=*/false));
  });
}

ggnn_status ggnn_query_labeled_range(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                     ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                     uint32_t k_query, float tau_query, uint32_t max_iterations,
                                     ggnn_measure measure, int32_t* ids_out, float* dists_out,
                                     ggnn_location out_location,
                                     const int32_t* query_label_ranges, uint32_t n_ranges,
                                     ggnn_location ranges_location, int ranges_gpu_id,
                                     const int32_t* filter_ids, ggnn_location ids_location,
                                     int ids_gpu_id)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    h->query({query, Nq, D, dtype, location, gpu_id, k_query, measure, ids_out, dists_out,
              out_location, tau_query, max_iterations},
             QueryFilter::label_ranges(*h, query_label_ranges, n_ranges, Nq, ranges_location,
                                       ranges_gpu_id, filter_ids, ids_location, ids_gpu_id));
  });
}

ggnn_status ggnn_bf_query_labeled_range(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                        ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                        uint32_t k_gt, ggnn_measure measure, int32_t* ids_out,
                                        float* dists_out, ggnn_location out_location,
                                        const int32_t* query_label_ranges, uint32_t n_ranges,
                                        ggnn_location ranges_location, int ranges_gpu_id,
                                        const int32_t* filter_ids, ggnn_location ids_location,
                                        int ids_gpu_id)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    h->bf_query({query, Nq, D, dtype, location, gpu_id, k_gt, measure, ids_out, dists_out,
                 out_location},
                QueryFilter::label_ranges(*h, query_label_ranges, n_ranges, Nq, ranges_location,
                                          ranges_gpu_id, filter_ids, ids_location, ids_gpu_id));
  });
}

ggnn_status ggnn_query_async_labeled_range(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                           ggnn_dtype dtype, int gpu_id, uint32_t k_query,
                                           float tau_query, uint32_t max_iterations,
                                           ggnn_measure measure, int32_t* ids_out,
                                           float* dists_out, uint32_t slot,
                                           const int32_t* query_label_ranges, uint32_t n_ranges,
                                           const int32_t* filter_ids)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    const QueryRequest r = async_request(query, Nq, D, dtype, gpu_id, k_query, tau_query,
                                         max_iterations, measure, ids_out, dists_out);
    // (ranges and ids live where the query lives and are not read on the host)
    h->query_async(r, slot,
                   QueryFilter::label_ranges(*h, query_label_ranges, n_ranges, Nq, r.loc, r.gpu,
                                             filter_ids, r.loc, r.gpu, /*read_host_ids=*/false));
  });
}

ggnn_status ggnn_query_labeled_mask(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                    ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                    uint32_t k_query, float tau_query, uint32_t max_iterations,
                                    ggnn_measure measure, int32_t* ids_out, float* dists_out,
                                    ggnn_location out_location,
                                    const int32_t* query_label_masks, uint32_t n_masks,
                                    ggnn_location masks_location, int masks_gpu_id,
                                    const int32_t* filter_ids, ggnn_location ids_location,
                                    int ids_gpu_id)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    h->query({query, Nq, D, dtype, location, gpu_id, k_query, measure, ids_out, dists_out,
              out_location, tau_query, max_iterations},
             QueryFilter::label_masks(*h, query_label_masks, n_masks, Nq, masks_location,
                                      masks_gpu_id, filter_ids, ids_location, ids_gpu_id));
  });
}

ggnn_status ggnn_bf_query_labeled_mask(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                       ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                       uint32_t k_gt, ggnn_measure measure, int32_t* ids_out,
                                       float* dists_out, ggnn_location out_location,
                                       const int32_t* query_label_masks, uint32_t n_masks,
                                       ggnn_location masks_location, int masks_gpu_id,
                                       const int32_t* filter_ids, ggnn_location ids_location,
                                       int ids_gpu_id)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    h->bf_query({query, Nq, D, dtype, location, gpu_id, k_gt, measure, ids_out, dists_out,
                 out_location},
                QueryFilter::label_masks(*h, query_label_masks, n_masks, Nq, masks_location,
                                         masks_gpu_id, filter_ids, ids_location, ids_gpu_id));
  });
}

ggnn_status ggnn_query_async_labeled_mask(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                          ggnn_dtype dtype, int gpu_id, uint32_t k_query,
                                          float tau_query, uint32_t max_iterations,
                                          ggnn_measure measure, int32_t* ids_out,
                                          float* dists_out, uint32_t slot,
                                          const int32_t* query_label_masks, uint32_t n_masks,
                                          const int32_t* filter_ids)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    const QueryRequest r = async_request(query, Nq, D, dtype, gpu_id, k_query, tau_query,
                                         max_iterations, measure, ids_out, dists_out);
    // (clauses and ids live where the query lives and are not read on the host)
    h->query_async(r, slot,
                   QueryFilter::label_masks(*h, query_label_masks, n_masks, Nq, r.loc, r.gpu,
                                            filter_ids, r.loc, r.gpu, /*read_host_ids=*/false));
  });
}

ggnn_status ggnn_get_graph(ggnn_t* h, uint32_t global_shard_id, ggnn_graph_view* out)
{
  GGNN_NEED_HANDLE(h);
  return guarded(h, [&] {
    GGNN_REQUIRE(out != nullptr, GGNN_INVALID_ARGUMENT, "null output");
    // ggnn.cu:392-413
    GGNN_REQUIRE(h->has_graph(), GGNN_INVALID_STATE, "No graph has been built or loaded yet.");
    GGNN_REQUIRE(global_shard_id < h->num_shards(), GGNN_INVALID_STATE,
                 "Shard " + std::to_string(global_shard_id) + " does not exist.");
    DeviceCtx& ctx = h->devs[global_shard_id / h->shards_per_gpu];
    if (ctx.swap) {
      // out-of-core shards: the view is valid until another shard takes the slot
      ctx.activate();
      h->acquire_shard(ctx, global_shard_id % h->shards_per_gpu, ctx.stream);
      GGNN_HIP_CHECK(hipStreamSynchronize(ctx.stream));
    }
    const Shard& sh = ctx.shards[global_shard_id % h->shards_per_gpu];
    out->config = h->cfg;
    out->config.D = h->base_D;  // caller-visible dimension (rows are padded internally)
    out->graph = sh.graph;
    out->translation = sh.translation;
    out->selection = sh.selection;
    out->nn1_stats = sh.nn1_stats;
    out->gpu_id = ctx.device;
  });
}

ggnn_status ggnn_last_timing_ms(const ggnn_t* h, float* build_ms, float* query_ms, float* bf_ms)
{
  GGNN_NEED_HANDLE(h);
  if (build_ms)
    *build_ms = h->build_ms;
  if (query_ms)
    *query_ms = h->query_ms;
  if (bf_ms)
    *bf_ms = h->bf_ms;
  return GGNN_OK;
}

const char* ggnn_last_exchange(const ggnn_t* h)
{
  return h ? h->last_exchange : "none";
}

ggnn_status ggnn_rccl_ranks(const ggnn_t* h, uint32_t* ranks)
{
  GGNN_NEED_HANDLE(h);
  uint32_t n = 0;
  if (!h->comms.empty() && h->comms[0] && Rccl::get().ok && Rccl::get().CommCount) {
    int count = 0;
    if (Rccl::get().CommCount(h->comms[0], &count) == ncclSuccess && count > 0)
      n = static_cast<uint32_t>(count);
  }
  if (ranks)
    *ranks = n;
  return GGNN_OK;
}

ggnn_status ggnn_last_bf_query_rescanned(const ggnn_t* h, uint32_t* n_rescanned)
{
  GGNN_NEED_HANDLE(h);
  if (n_rescanned)
    *n_rescanned = h->last_bf_rescanned;
  return GGNN_OK;
}

ggnn_status ggnn_last_bf_query_matrix_path(const ggnn_t* h, int* out)
{
  GGNN_NEED_HANDLE(h);
  if (!out)
    return GGNN_INVALID_ARGUMENT;
  *out = h->last_bf_matrix_path;
  return GGNN_OK;
}

ggnn_status ggnn_last_query_counters(const ggnn_t* h, uint64_t* n_dist, uint64_t* n_pop)
{
  GGNN_NEED_HANDLE(h);
  if (n_dist)
    *n_dist = h->last_n_dist;
  if (n_pop)
    *n_pop = h->last_n_pop;
  return GGNN_OK;
}

// ---- Section 2: operator seam ----------------------------------------------------------------

ggnn_status ggnn_graph_config_init(uint32_t N, uint32_t D, uint32_t KBuild,
                                   ggnn_graph_config* out)
{
  return guarded(nullptr, [&] { graph_config_init(N, D, KBuild, out); });
}

ggnn_status ggnn_query_sizing(uint32_t D, uint32_t k_query, uint32_t max_iterations,
                              uint32_t* cache_size, uint32_t* sorted_size)
{
  return guarded(nullptr, [&] { query_sizing(D, k_query, max_iterations, cache_size, sorted_size); });
}

ggnn_status ggnn_op_dist_layout(uint32_t D, ggnn_dtype dtype, uint32_t* lanes_per_row,
                                uint32_t* chunks_per_lane)
{
  return guarded(nullptr, [&] {
    GGNN_REQUIRE(dtype == GGNN_F32 || dtype == GGNN_U8 || dtype == GGNN_F16 || dtype == GGNN_BF16 ||
                     dtype == GGNN_I8,
                 GGNN_INVALID_ARGUMENT, "unknown dtype");
    GGNN_REQUIRE(lanes_per_row && chunks_per_lane, GGNN_INVALID_ARGUMENT, "null output pointer");
    const DistConfig dc = pick_dist_config(D, dtype);
    *lanes_per_row = static_cast<uint32_t>(dc.lpr);
    *chunks_per_lane = static_cast<uint32_t>(dc.nch);
  });
}

ggnn_status ggnn_op_query(const void* base, ggnn_dtype dtype, uint32_t N_base, uint32_t D,
                          const void* query, uint32_t Nq, const int32_t* graph0,
                          uint32_t KBuild, const int32_t* start, uint32_t num_start,
                          const float* nn1_stats, uint32_t k_query, float tau_query,
                          uint32_t max_iterations, ggnn_measure measure,
                          uint32_t shards_per_gpu, uint32_t on_gpu_shard, int32_t* ids,
                          float* dists, uint32_t* n_dist, uint32_t* n_pop, void* stream)
{
  return guarded(nullptr, [&] {
    launch_query(seam_query(base, dtype, N_base, D, nullptr, nullptr, query, Nq, graph0, KBuild,
                            start, num_start, nn1_stats, k_query, tau_query, max_iterations,
                            measure, shards_per_gpu, on_gpu_shard, ids, dists, n_dist, n_pop,
                            nullptr),
                 static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_prescreen_sizes(uint32_t N_base, uint32_t D, ggnn_measure measure,
                                 uint32_t* code_dim, size_t* param_floats, size_t* scratch_floats)
{
  return guarded(nullptr, [&] {
    GGNN_REQUIRE(D >= 1 && D <= 4096 && D % 4 == 0, GGNN_INVALID_ARGUMENT,
                 "D must be a multiple of 4 in [4, 4096]");
    if (code_dim)
      *code_dim = prescreen_code_dim(D);
    if (param_floats)
      *param_floats = prescreen_param_floats(D);
    if (scratch_floats)
      *scratch_floats = prescreen_scratch_floats(N_base, D, measure);
  });
}

ggnn_status ggnn_op_prescreen_encode(const float* base, uint32_t N_base, uint32_t D,
                                     ggnn_measure measure, uint8_t* codes, float* params,
                                     float* scratch, void* stream)
{
  return guarded(nullptr, [&] {
    launch_prescreen_encode(base, N_base, D, measure, codes, params, scratch,
                            static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_prescreen_probe(const uint8_t* codes, const float* params, uint32_t D,
                                    ggnn_measure measure, const float* query, uint32_t Nq,
                                    const int32_t* cand, uint32_t M, const float* crit,
                                    int32_t* reject, float* s_out, void* stream)
{
  return guarded(nullptr, [&] {
    launch_prescreen_probe(codes, params, D, measure, query, Nq, cand, M, crit, reject, s_out,
                           static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_query_prescreened(const float* base, uint32_t N_base, uint32_t D,
                                      const uint8_t* codes, const float* params,
                                      const float* query, uint32_t Nq, const int32_t* graph0,
                                      uint32_t KBuild, const int32_t* start, uint32_t num_start,
                                      const float* nn1_stats, uint32_t k_query, float tau_query,
                                      uint32_t max_iterations, ggnn_measure measure,
                                      uint32_t shards_per_gpu, uint32_t on_gpu_shard, int32_t* ids,
                                      float* dists, uint32_t* n_dist, uint32_t* n_pop,
                                      uint32_t* n_rows, void* stream)
{
  return guarded(nullptr, [&] {
    GGNN_REQUIRE(codes && params, GGNN_INVALID_ARGUMENT, "pre-screen buffers are null");
    launch_query(seam_query(base, GGNN_F32, N_base, D, codes, params, query, Nq, graph0, KBuild,
                            start, num_start, nn1_stats, k_query, tau_query, max_iterations,
                            measure, shards_per_gpu, on_gpu_shard, ids, dists, n_dist, n_pop,
                            n_rows),
                 static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_query_filtered(const void* base, ggnn_dtype dtype, uint32_t N_base, uint32_t D,
                                   const uint8_t* codes, const float* params, const void* query,
                                   uint32_t Nq, const int32_t* graph0, uint32_t KBuild,
                                   const int32_t* start, uint32_t num_start,
                                   const float* nn1_stats, uint32_t k_query, float tau_query,
                                   uint32_t max_iterations, ggnn_measure measure,
                                   uint32_t shards_per_gpu, uint32_t on_gpu_shard, int32_t* ids,
                                   float* dists, uint32_t* n_dist, uint32_t* n_pop,
                                   uint32_t* n_rows, const uint32_t* filter_bits,
                                   uint32_t filter_bit_offset, void* stream)
{
  return guarded(nullptr, [&] {
    GGNN_REQUIRE(filter_bits != nullptr, GGNN_INVALID_ARGUMENT, "the filter bitset is null");
    QueryLaunch q = seam_query(base, dtype, N_base, D, codes, params, query, Nq, graph0, KBuild,
                               start, num_start, nn1_stats, k_query, tau_query, max_iterations,
                               measure, shards_per_gpu, on_gpu_shard, ids, dists, n_dist, n_pop,
                               n_rows);
    q.filter_bits = filter_bits;
    q.filter_bit_offset = filter_bit_offset;
    launch_query(q, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_bf_query_filtered(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                      uint32_t D, const void* query, uint32_t Nq,
                                      uint32_t k_query, ggnn_measure measure, int32_t* ids,
                                      float* dists, const uint32_t* filter_bits,
                                      uint32_t filter_bit_offset, void* stream)
{
  return guarded(nullptr, [&] {
    GGNN_REQUIRE(filter_bits != nullptr, GGNN_INVALID_ARGUMENT, "the filter bitset is null");
    BfLaunch b{base, query, dtype, N_base, D, Nq, k_query, measure, ids, dists};
    b.filter_bits = filter_bits;
    b.filter_bit_offset = filter_bit_offset;
    launch_bf_query(b, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_bf_query_filtered_certified(const void* base, ggnn_dtype dtype,
                                                uint32_t N_base, uint32_t D, const void* query,
                                                uint32_t Nq, uint32_t k_query,
                                                ggnn_measure measure, int32_t* ids, float* dists,
                                                const uint32_t* filter_bits,
                                                uint32_t filter_bit_offset, uint32_t* n_rescanned,
                                                int* matrix_path, void* stream)
{
  return guarded(nullptr, [&] {
    GGNN_REQUIRE(filter_bits != nullptr, GGNN_INVALID_ARGUMENT, "the filter bitset is null");
    BfLaunch b{base, query, dtype, N_base, D, Nq, k_query, measure, ids, dists, n_rescanned};
    b.filter_bits = filter_bits;
    b.filter_bit_offset = filter_bit_offset;
    b.matrix_path = matrix_path;
    launch_bf_query(b, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_query_filtered_by(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                      uint32_t D, const uint8_t* codes, const float* params,
                                      const void* query, uint32_t Nq, const int32_t* graph0,
                                      uint32_t KBuild, const int32_t* start, uint32_t num_start,
                                      const float* nn1_stats, uint32_t k_query, float tau_query,
                                      uint32_t max_iterations, ggnn_measure measure,
                                      uint32_t shards_per_gpu, uint32_t on_gpu_shard, int32_t* ids,
                                      float* dists, uint32_t* n_dist, uint32_t* n_pop,
                                      uint32_t* n_rows, const uint32_t* filter_table,
                                      uint32_t num_filters, uint64_t n_bits,
                                      const int32_t* filter_ids, uint32_t filter_bit_offset,
                                      void* stream)
{
  return guarded(nullptr, [&] {
    QueryLaunch q = seam_query(base, dtype, N_base, D, codes, params, query, Nq, graph0, KBuild,
                               start, num_start, nn1_stats, k_query, tau_query, max_iterations,
                               measure, shards_per_gpu, on_gpu_shard, ids, dists, n_dist, n_pop,
                               n_rows);
    q.filter_table =
        seam_filter_table(filter_table, num_filters, n_bits, filter_ids, filter_bit_offset, N_base);
    q.filter_bits = filter_table;
    q.filter_bit_offset = filter_bit_offset;
    launch_query(q, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_bf_query_filtered_by(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                         uint32_t D, const void* query, uint32_t Nq,
                                         uint32_t k_query, ggnn_measure measure, int32_t* ids,
                                         float* dists, const uint32_t* filter_table,
                                         uint32_t num_filters, uint64_t n_bits,
                                         const int32_t* filter_ids, uint32_t filter_bit_offset,
                                         void* stream)
{
  return guarded(nullptr, [&] {
    BfLaunch b{base, query, dtype, N_base, D, Nq, k_query, measure, ids, dists};
    b.filter_table =
        seam_filter_table(filter_table, num_filters, n_bits, filter_ids, filter_bit_offset, N_base);
    b.filter_bits = filter_table;
    b.filter_bit_offset = filter_bit_offset;
    launch_bf_query(b, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_bf_query_filtered_by_certified(
    const void* base, ggnn_dtype dtype, uint32_t N_base, uint32_t D, const void* query, uint32_t Nq,
    uint32_t k_query, ggnn_measure measure, int32_t* ids, float* dists,
    const uint32_t* filter_table, uint32_t num_filters, uint64_t n_bits, const int32_t* filter_ids,
    uint32_t filter_bit_offset, uint32_t* n_rescanned, int* matrix_path, void* stream)
{
  return guarded(nullptr, [&] {
    BfLaunch b{base, query, dtype, N_base, D, Nq, k_query, measure, ids, dists, n_rescanned};
    b.filter_table =
        seam_filter_table(filter_table, num_filters, n_bits, filter_ids, filter_bit_offset, N_base);
    b.filter_bits = filter_table;
    b.filter_bit_offset = filter_bit_offset;
    b.matrix_path = matrix_path;
    launch_bf_query(b, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_query_labeled(const void* base, ggnn_dtype dtype, uint32_t N_base, uint32_t D,
                                  const uint8_t* codes, const float* params, const void* query,
                                  uint32_t Nq, const int32_t* graph0, uint32_t KBuild,
                                  const int32_t* start, uint32_t num_start, const float* nn1_stats,
                                  uint32_t k_query, float tau_query, uint32_t max_iterations,
                                  ggnn_measure measure, uint32_t shards_per_gpu,
                                  uint32_t on_gpu_shard, int32_t* ids, float* dists,
                                  uint32_t* n_dist, uint32_t* n_pop, uint32_t* n_rows,
                                  const int32_t* labels, uint64_t n_labels,
                                  const int32_t* query_labels, uint32_t filter_bit_offset,
                                  void* stream)
{
  return guarded(nullptr, [&] {
    QueryLaunch q = seam_query(base, dtype, N_base, D, codes, params, query, Nq, graph0, KBuild,
                               start, num_start, nn1_stats, k_query, tau_query, max_iterations,
                               measure, shards_per_gpu, on_gpu_shard, ids, dists, n_dist, n_pop,
                               n_rows);
    q.filter_table = seam_labels(labels, n_labels, query_labels, filter_bit_offset, N_base);
    q.filter_bits = reinterpret_cast<const uint32_t*>(labels);
    q.filter_bit_offset = filter_bit_offset;
    launch_query(q, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_bf_query_labeled(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                     uint32_t D, const void* query, uint32_t Nq, uint32_t k_query,
                                     ggnn_measure measure, int32_t* ids, float* dists,
                                     const int32_t* labels, uint64_t n_labels,
                                     const int32_t* query_labels, uint32_t filter_bit_offset,
                                     void* stream)
{
  return guarded(nullptr, [&] {
    BfLaunch b{base, query, dtype, N_base, D, Nq, k_query, measure, ids, dists};
    b.filter_table = seam_labels(labels, n_labels, query_labels, filter_bit_offset, N_base);
    b.filter_bits = reinterpret_cast<const uint32_t*>(labels);
    b.filter_bit_offset = filter_bit_offset;
    launch_bf_query(b, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_bf_query_label_index(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                         uint32_t D, const void* query, uint32_t Nq,
                                         uint32_t k_query, ggnn_measure measure,
                                         const int32_t* keys, uint32_t n_keys,
                                         const uint32_t* offsets, const int32_t* rows,
                                         const int32_t* query_labels, int32_t* ids, float* dists,
                                         void* stream)
{
  return guarded(nullptr, [&] {
    GGNN_REQUIRE(!Nq || (ids != nullptr && dists != nullptr), GGNN_INVALID_ARGUMENT,
                 "result pointers are null");
    const LabelIndexLaunch l{base, query, dtype,  N_base,  D,    Nq,          k_query, measure,
                             ids,  dists, keys,   n_keys,  offsets, rows, query_labels};
    launch_label_index_scan(l, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_label_index_classify(const int32_t* keys, uint32_t n_keys,
                                         const uint32_t* offsets, const int32_t* query_labels,
                                         uint32_t Nq, uint32_t cutoff, uint32_t* routed_list,
                                         uint32_t* rest_list, uint32_t* counts, void* stream)
{
  return guarded(nullptr, [&] {
    launch_label_index_classify(keys, n_keys, offsets, query_labels, Nq, cutoff, routed_list,
                                rest_list, counts, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_label_spans_resolve(const int32_t* keys, uint32_t n_keys,
                                        const uint32_t* offsets, int mode, const int32_t* sel,
                                        uint32_t n_sel, uint32_t Nq, uint32_t* spans,
                                        uint32_t* totals, void* stream)
{
  return guarded(nullptr, [&] {
    launch_label_spans_resolve(keys, n_keys, offsets, mode, sel, n_sel, Nq, spans, totals,
                               static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_bf_query_label_spans(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                         uint32_t D, const void* query, uint32_t Nq,
                                         uint32_t k_query, ggnn_measure measure,
                                         const int32_t* rows, const uint32_t* spans,
                                         uint32_t span_limit, const uint32_t* filter_table,
                                         uint32_t num_filters, uint64_t n_bits,
                                         const int32_t* filter_ids, int32_t* ids, float* dists,
                                         void* stream)
{
  return guarded(nullptr, [&] {
    GGNN_REQUIRE((filter_table != nullptr) == (num_filters > 0), GGNN_INVALID_ARGUMENT,
                 "filter_table and num_filters go together");
    GGNN_REQUIRE(!filter_table || (n_bits >= N_base && n_bits <= 0xffffffffull),
                 GGNN_INVALID_ARGUMENT, "a filter needs N_base bits");
    LabelSpansLaunch l{base, query, dtype, N_base, D, Nq, k_query, measure, ids, dists, rows, spans};
    l.span_limit = span_limit;
    l.filter_table = filter_table;
    l.num_filters = num_filters;
    l.words = filter_table ? static_cast<uint32_t>((n_bits + 31) / 32) : 0u;
    l.filter_ids = filter_ids;
    launch_label_spans_scan(l, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_label_spans_classify(const uint32_t* totals, uint32_t Nq, uint32_t cutoff,
                                         uint32_t* routed_list, uint32_t* rest_list,
                                         uint32_t* counts, void* stream)
{
  return guarded(nullptr, [&] {
    launch_label_spans_classify(totals, Nq, cutoff, routed_list, rest_list, counts,
                                static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_bf_query_labeled_certified(const void* base, ggnn_dtype dtype,
                                               uint32_t N_base, uint32_t D, const void* query,
                                               uint32_t Nq, uint32_t k_query, ggnn_measure measure,
                                               int32_t* ids, float* dists, const int32_t* labels,
                                               uint64_t n_labels, const int32_t* query_labels,
                                               uint32_t filter_bit_offset, uint32_t* n_rescanned,
                                               int* matrix_path, void* stream)
{
  return guarded(nullptr, [&] {
    BfLaunch b{base, query, dtype, N_base, D, Nq, k_query, measure, ids, dists, n_rescanned};
    b.filter_table = seam_labels(labels, n_labels, query_labels, filter_bit_offset, N_base);
    b.filter_bits = reinterpret_cast<const uint32_t*>(labels);
    b.filter_bit_offset = filter_bit_offset;
    b.matrix_path = matrix_path;
    launch_bf_query(b, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_query_labeled_in(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                     uint32_t D, const uint8_t* codes, const float* params,
                                     const void* query, uint32_t Nq, const int32_t* graph0,
                                     uint32_t KBuild, const int32_t* start, uint32_t num_start,
                                     const float* nn1_stats, uint32_t k_query, float tau_query,
                                     uint32_t max_iterations, ggnn_measure measure,
                                     uint32_t shards_per_gpu, uint32_t on_gpu_shard, int32_t* ids,
                                     float* dists, uint32_t* n_dist, uint32_t* n_pop,
                                     uint32_t* n_rows, const int32_t* labels, uint64_t n_labels,
                                     const int32_t* query_label_sets, uint32_t set_width,
                                     const uint32_t* filter_table, uint32_t num_filters,
                                     uint64_t n_bits, const int32_t* filter_ids,
                                     uint32_t filter_bit_offset, void* stream)
{
  return guarded(nullptr, [&] {
    QueryLaunch q = seam_query(base, dtype, N_base, D, codes, params, query, Nq, graph0, KBuild,
                               start, num_start, nn1_stats, k_query, tau_query, max_iterations,
                               measure, shards_per_gpu, on_gpu_shard, ids, dists, n_dist, n_pop,
                               n_rows);
    seam_label_sets(q, labels, n_labels, query_label_sets, set_width, filter_table, num_filters,
                    n_bits, filter_ids, filter_bit_offset, N_base);
    launch_query(q, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_bf_query_labeled_in(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                        uint32_t D, const void* query, uint32_t Nq,
                                        uint32_t k_query, ggnn_measure measure, int32_t* ids,
                                        float* dists, const int32_t* labels, uint64_t n_labels,
                                        const int32_t* query_label_sets, uint32_t set_width,
                                        const uint32_t* filter_table, uint32_t num_filters,
                                        uint64_t n_bits, const int32_t* filter_ids,
                                        uint32_t filter_bit_offset, void* stream)
{
  return guarded(nullptr, [&] {
    BfLaunch b{base, query, dtype, N_base, D, Nq, k_query, measure, ids, dists};
    seam_label_sets(b, labels, n_labels, query_label_sets, set_width, filter_table, num_filters,
                    n_bits, filter_ids, filter_bit_offset, N_base);
    launch_bf_query(b, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_query_labeled_range(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                        uint32_t D, const uint8_t* codes, const float* params,
                                        const void* query, uint32_t Nq, const int32_t* graph0,
                                        uint32_t KBuild, const int32_t* start, uint32_t num_start,
                                        const float* nn1_stats, uint32_t k_query, float tau_query,
                                        uint32_t max_iterations, ggnn_measure measure,
                                        uint32_t shards_per_gpu, uint32_t on_gpu_shard,
                                        int32_t* ids, float* dists, uint32_t* n_dist,
                                        uint32_t* n_pop, uint32_t* n_rows, const int32_t* labels,
                                        uint64_t n_labels, const int32_t* query_label_ranges,
                                        uint32_t n_ranges, const uint32_t* filter_table,
                                        uint32_t num_filters, uint64_t n_bits,
                                        const int32_t* filter_ids, uint32_t filter_bit_offset,
                                        void* stream)
{
  return guarded(nullptr, [&] {
    QueryLaunch q = seam_query(base, dtype, N_base, D, codes, params, query, Nq, graph0, KBuild,
                               start, num_start, nn1_stats, k_query, tau_query, max_iterations,
                               measure, shards_per_gpu, on_gpu_shard, ids, dists, n_dist, n_pop,
                               n_rows);
    seam_label_ranges(q, labels, n_labels, query_label_ranges, n_ranges, filter_table, num_filters,
                      n_bits, filter_ids, filter_bit_offset, N_base);
    launch_query(q, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_bf_query_labeled_range(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                           uint32_t D, const void* query, uint32_t Nq,
                                           uint32_t k_query, ggnn_measure measure, int32_t* ids,
                                           float* dists, const int32_t* labels, uint64_t n_labels,
                                           const int32_t* query_label_ranges, uint32_t n_ranges,
                                           const uint32_t* filter_table, uint32_t num_filters,
                                           uint64_t n_bits, const int32_t* filter_ids,
                                           uint32_t filter_bit_offset, void* stream)
{
  return guarded(nullptr, [&] {
    BfLaunch b{base, query, dtype, N_base, D, Nq, k_query, measure, ids, dists};
    seam_label_ranges(b, labels, n_labels, query_label_ranges, n_ranges, filter_table, num_filters,
                      n_bits, filter_ids, filter_bit_offset, N_base);
    launch_bf_query(b, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_query_labeled_mask(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                       uint32_t D, const uint8_t* codes, const float* params,
                                       const void* query, uint32_t Nq, const int32_t* graph0,
                                       uint32_t KBuild, const int32_t* start, uint32_t num_start,
                                       const float* nn1_stats, uint32_t k_query, float tau_query,
                                       uint32_t max_iterations, ggnn_measure measure,
                                       uint32_t shards_per_gpu, uint32_t on_gpu_shard,
                                       int32_t* ids, float* dists, uint32_t* n_dist,
                                       uint32_t* n_pop, uint32_t* n_rows, const int32_t* labels,
                                       uint64_t n_labels, const int32_t* query_label_masks,
                                       uint32_t n_masks, const uint32_t* filter_table,
                                       uint32_t num_filters, uint64_t n_bits,
                                       const int32_t* filter_ids, uint32_t filter_bit_offset,
                                       void* stream)
{
  return guarded(nullptr, [&] {
    QueryLaunch q = seam_query(base, dtype, N_base, D, codes, params, query, Nq, graph0, KBuild,
                               start, num_start, nn1_stats, k_query, tau_query, max_iterations,
                               measure, shards_per_gpu, on_gpu_shard, ids, dists, n_dist, n_pop,
                               n_rows);
    seam_label_masks(q, labels, n_labels, query_label_masks, n_masks, filter_table, num_filters,
                     n_bits, filter_ids, filter_bit_offset, N_base);
    launch_query(q, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_bf_query_labeled_mask(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                          uint32_t D, const void* query, uint32_t Nq,
                                          uint32_t k_query, ggnn_measure measure, int32_t* ids,
                                          float* dists, const int32_t* labels, uint64_t n_labels,
                                          const int32_t* query_label_masks, uint32_t n_masks,
                                          const uint32_t* filter_table, uint32_t num_filters,
                                          uint64_t n_bits, const int32_t* filter_ids,
                                          uint32_t filter_bit_offset, void* stream)
{
  return guarded(nullptr, [&] {
    BfLaunch b{base, query, dtype, N_base, D, Nq, k_query, measure, ids, dists};
    seam_label_masks(b, labels, n_labels, query_label_masks, n_masks, filter_table, num_filters,
                     n_bits, filter_ids, filter_bit_offset, N_base);
    launch_bf_query(b, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_pack_filters(const uint8_t* masks, uint32_t num_filters, uint64_t N,
                                 uint32_t* words, void* stream)
{
  return guarded(nullptr, [&] {
    launch_pack_filters(masks, num_filters, N, words, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_bf_query(const void* base, ggnn_dtype dtype, uint32_t N_base, uint32_t D,
                             const void* query, uint32_t Nq, uint32_t k_query,
                             ggnn_measure measure, int32_t* ids, float* dists, void* stream)
{
  return guarded(nullptr, [&] {
    BfLaunch b{base, query, dtype, N_base, D, Nq, k_query, measure, ids, dists};
    launch_bf_query(b, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_bf_query_certified(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                       uint32_t D, const void* query, uint32_t Nq,
                                       uint32_t k_query, ggnn_measure measure, int32_t* ids,
                                       float* dists, uint32_t* n_rescanned, void* stream)
{
  return guarded(nullptr, [&] {
    BfLaunch b{base, query, dtype, N_base, D, Nq, k_query, measure, ids, dists, n_rescanned};
    launch_bf_query(b, static_cast<hipStream_t>(stream));
  });
}

// the range-search seam calls: lims [Nq + 1] uint64, ids / dists [capacity] (all device memory)
#define GGNN_RANGE_LAUNCH \
  BfRangeLaunch{base, query, dtype, N_base, D, Nq, measure, radii, capacity, lims, ids, dists}
ggnn_status ggnn_op_bf_range_query(const void* base, ggnn_dtype dtype, uint32_t N_base, uint32_t D,
                                   const void* query, uint32_t Nq, const float* radii,
                                   ggnn_measure measure, uint64_t capacity, uint64_t* lims,
                                   int32_t* ids, float* dists, void* stream)
{
  return guarded(nullptr, [&] {
    launch_bf_range_query(GGNN_RANGE_LAUNCH, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_bf_range_query_filtered(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                            uint32_t D, const void* query, uint32_t Nq,
                                            const float* radii, ggnn_measure measure,
                                            uint64_t capacity, uint64_t* lims, int32_t* ids,
                                            float* dists, const uint32_t* filter_bits,
                                            uint32_t filter_bit_offset, void* stream)
{
  return guarded(nullptr, [&] {
    GGNN_REQUIRE(filter_bits != nullptr, GGNN_INVALID_ARGUMENT, "the filter bitset is null");
    BfRangeLaunch b = GGNN_RANGE_LAUNCH;
    b.filter_bits = filter_bits;
    b.filter_bit_offset = filter_bit_offset;
    launch_bf_range_query(b, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_bf_range_query_filtered_by(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                               uint32_t D, const void* query, uint32_t Nq,
                                               const float* radii, ggnn_measure measure,
                                               uint64_t capacity, uint64_t* lims, int32_t* ids,
                                               float* dists, const uint32_t* filter_table,
                                               uint32_t num_filters, uint64_t n_bits,
                                               const int32_t* filter_ids,
                                               uint32_t filter_bit_offset, void* stream)
{
  return guarded(nullptr, [&] {
    BfRangeLaunch b = GGNN_RANGE_LAUNCH;
    b.filter_table =
        seam_filter_table(filter_table, num_filters, n_bits, filter_ids, filter_bit_offset, N_base);
    b.filter_bits = filter_table;
    b.filter_bit_offset = filter_bit_offset;
    launch_bf_range_query(b, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_bf_range_query_labeled(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                           uint32_t D, const void* query, uint32_t Nq,
                                           const float* radii, ggnn_measure measure,
                                           uint64_t capacity, uint64_t* lims, int32_t* ids,
                                           float* dists, const int32_t* labels, uint64_t n_labels,
                                           const int32_t* query_labels, uint32_t filter_bit_offset,
                                           void* stream)
{
  return guarded(nullptr, [&] {
    BfRangeLaunch b = GGNN_RANGE_LAUNCH;
    b.filter_table = seam_labels(labels, n_labels, query_labels, filter_bit_offset, N_base);
    b.filter_bits = reinterpret_cast<const uint32_t*>(labels);
    b.filter_bit_offset = filter_bit_offset;
    launch_bf_range_query(b, static_cast<hipStream_t>(stream));
  });
}
#undef GGNN_RANGE_LAUNCH

ggnn_status ggnn_op_top(const void* base, ggnn_dtype dtype, uint32_t D, ggnn_measure measure,
                        uint32_t KBuild, const int32_t* translation_layer, uint32_t N_layer,
                        uint32_t S, uint32_t S_offset, uint32_t layer, int32_t* graph_layer,
                        float* nn1_dist_buffer, void* stream)
{
  return guarded(nullptr, [&] {
    TopLaunch t{base, dtype, D, measure, KBuild, translation_layer, N_layer, S, S_offset, layer,
                graph_layer, nn1_dist_buffer};
    launch_top(t, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_merge(const void* base, ggnn_dtype dtype, ggnn_measure measure,
                          const ggnn_graph_config* cfg, const int32_t* graph_all,
                          const int32_t* translation_all, const int32_t* selection_all,
                          const float* nn1_stats, float tau_build, uint32_t layer_top,
                          uint32_t layer_btm, int32_t* graph_buffer, float* nn1_dist_buffer,
                          uint32_t* n_dist, void* stream)
{
  return guarded(nullptr, [&] {
    GGNN_REQUIRE(cfg != nullptr, GGNN_INVALID_ARGUMENT, "null graph config");
    MergeLaunch m{base,      dtype,     measure,   *cfg,         graph_all,       translation_all,
                  selection_all, nn1_stats, tau_build, layer_top, layer_btm,      graph_buffer,
                  nn1_dist_buffer, n_dist};
    launch_merge(m, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_merge_prescreened(const float* base, const uint8_t* codes, const float* params,
                                      ggnn_measure measure, const ggnn_graph_config* cfg,
                                      const int32_t* graph_all,
                                      const int32_t* translation_all,
                                      const int32_t* selection_all, const float* nn1_stats,
                                      float tau_build, uint32_t layer_top, uint32_t layer_btm,
                                      int32_t* graph_buffer, float* nn1_dist_buffer,
                                      uint32_t* n_dist, void* stream)
{
  return guarded(nullptr, [&] {
    GGNN_REQUIRE(cfg != nullptr, GGNN_INVALID_ARGUMENT, "null graph config");
    GGNN_REQUIRE(codes && params, GGNN_INVALID_ARGUMENT, "pre-screen buffers are null");
    MergeLaunch m{base,          GGNN_F32,  measure,        *cfg,      graph_all, translation_all,
                  selection_all, nn1_stats, tau_build,      layer_top, layer_btm, graph_buffer,
                  nn1_dist_buffer, n_dist};
    m.ps_codes = codes;
    m.ps_params = params;
    m.ps_Dc = prescreen_code_dim(cfg->D);
    launch_merge(m, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_select(const ggnn_graph_config* cfg, uint32_t layer,
                           const float* nn1_dist_buffer, const float* rng,
                           int32_t* translation_all, int32_t* selection_all, void* stream)
{
  return guarded(nullptr, [&] {
    GGNN_REQUIRE(cfg != nullptr, GGNN_INVALID_ARGUMENT, "null graph config");
    launch_select(*cfg, layer, nn1_dist_buffer, rng, translation_all, selection_all,
                  static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_uniform(float* out, uint32_t n, uint64_t seed, uint64_t stream_id,
                            void* stream)
{
  return guarded(nullptr,
                 [&] { launch_uniform(out, n, seed, stream_id, static_cast<hipStream_t>(stream)); });
}

ggnn_status ggnn_op_sym(const void* base, ggnn_dtype dtype, ggnn_measure measure, uint32_t D,
                        uint32_t KBuild, const int32_t* graph_layer,
                        const int32_t* translation_layer, uint32_t N_layer,
                        const float* nn1_stats, float tau_build, int32_t* sym_buffer,
                        uint32_t* sym_atomic, uint32_t first_n, uint32_t count, void* stream)
{
  return guarded(nullptr, [&] {
    SymLaunch s{base,      dtype,     measure,    D,          KBuild,  graph_layer, translation_layer,
                N_layer,   nn1_stats, tau_build,  sym_buffer, sym_atomic, first_n,  count};
    launch_sym(s, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_sym_prescreened(const float* base, const uint8_t* codes, const float* params,
                                    ggnn_measure measure, uint32_t D, uint32_t KBuild,
                                    const int32_t* graph_layer, const int32_t* translation_layer,
                                    uint32_t N_layer, const float* nn1_stats, float tau_build,
                                    int32_t* sym_buffer, uint32_t* sym_atomic, uint32_t first_n,
                                    uint32_t count, void* stream)
{
  return guarded(nullptr, [&] {
    GGNN_REQUIRE(codes && params, GGNN_INVALID_ARGUMENT, "pre-screen buffers are null");
    SymLaunch s{base,    GGNN_F32,  measure,   D,          KBuild,     graph_layer, translation_layer,
                N_layer, nn1_stats, tau_build, sym_buffer, sym_atomic, first_n,     count};
    s.ps_codes = codes;
    s.ps_params = params;
    s.ps_Dc = prescreen_code_dim(D);
    launch_sym(s, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_sym_requests(const void* base, ggnn_dtype dtype, const uint8_t* codes,
                                 const float* params, ggnn_measure measure, uint32_t D,
                                 uint32_t KBuild, const int32_t* graph_layer,
                                 const int32_t* translation_layer, uint32_t N_layer,
                                 const float* nn1_stats, float tau_build, int32_t* sym_buffer,
                                 uint32_t* sym_atomic, int32_t* requests, uint32_t first_n,
                                 uint32_t count, void* stream)
{
  return guarded(nullptr, [&] {
    GGNN_REQUIRE(requests != nullptr, GGNN_INVALID_ARGUMENT, "requests is null");
    GGNN_REQUIRE(!codes == !params, GGNN_INVALID_ARGUMENT,
                 "pre-screen codes and params go together");
    GGNN_REQUIRE(!codes || dtype == GGNN_F32, GGNN_INVALID_ARGUMENT,
                 "the pre-screen needs a float32 base");
    SymLaunch s{base,    dtype,     measure,   D,          KBuild,     graph_layer, translation_layer,
                N_layer, nn1_stats, tau_build, sym_buffer, sym_atomic, first_n,     count};
    if (codes) {
      s.ps_codes = codes;
      s.ps_params = params;
      s.ps_Dc = prescreen_code_dim(D);
    }
    s.requests = requests;
    launch_sym(s, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_sym_assign(uint32_t KBuild, uint32_t N_layer, const int32_t* requests,
                               uint32_t* sym_atomic, int32_t* sym_buffer, void* stream)
{
  return guarded(nullptr, [&] {
    GGNN_REQUIRE(requests && sym_atomic && sym_buffer, GGNN_INVALID_ARGUMENT,
                 "sym_assign: null buffer");
    launch_sym_assign(KBuild, N_layer, requests, sym_atomic, sym_buffer,
                      static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_sym_buffer_merge(uint32_t KBuild, uint32_t N_layer, int32_t* sym_buffer,
                                     const uint32_t* sym_atomic, int32_t* graph_layer,
                                     void* stream)
{
  return guarded(nullptr, [&] {
    launch_sym_buffer_merge(KBuild, N_layer, sym_buffer, sym_atomic, graph_layer,
                            static_cast<hipStream_t>(stream));
  });
}

size_t ggnn_nn1_stats_scratch_floats(void)
{
  return 3 * kStatsBlocks;
}

ggnn_status ggnn_op_nn1_stats(const float* nn1_dist_buffer, uint32_t N, float* scratch,
                              float* out, void* stream)
{
  return guarded(nullptr, [&] {
    launch_nn1_stats(nn1_dist_buffer, N, scratch, out, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_sort_shard_results(uint32_t Nq, uint32_t row_len, int32_t* ids, float* dists,
                                       void* stream)
{
  return guarded(nullptr, [&] {
    launch_sort_shard_results(Nq, row_len, ids, dists, static_cast<hipStream_t>(stream));
  });
}

ggnn_status ggnn_op_merge_results(uint32_t Nq, uint32_t k, uint32_t num_parts, uint32_t stride,
                                  uint32_t id_offset_per_part, const int32_t* parts_ids,
                                  const float* parts_dists, int32_t* ids_out, float* dists_out,
                                  void* stream)
{
  return guarded(nullptr, [&] {
    launch_merge_results(Nq, k, num_parts, stride, id_offset_per_part, parts_ids, parts_dists,
                         ids_out, dists_out, static_cast<hipStream_t>(stream));
  });
}

}  // extern "C"
