/*
 * ggnn_c.h -- C-ABI of the MI355X-native GGNN query+build engine (libggnn_amd.so).
 *
 * The reference (cgtuebingen/ggnn v0.9.1) has no C-ABI: its nanobind module wraps the C++
 * class ggnn::GGNN<int32_t,float> directly (src/ggnn/python/nanobind.cu:184-268).  This header
 * is the thin C boundary a binding for that class binds instead; every entry point cites the
 * reference interface it replaces (paths relative to the reference tree).
 *
 *  - Section 1 mirrors the public class           include/ggnn/base/ggnn.cuh:42-182
 *  - Section 2 mirrors the internal operator seam  include/ggnn/query/query_kernels.cuh:33-61
 *                                                  include/ggnn/construction/graph_construction.cuh:35-59
 *    (one function per kernel, device pointers + HIP stream; used by the engine itself and by
 *    the per-kernel parity tests with injected inputs)
 *
 * Conventions: plain pointers and sizes only.  Every call returns a ggnn_status; the message
 * of the last failure is available through ggnn_last_error().  API misuse maps to the
 * exceptions the reference throws (INVALID_STATE/INVALID_ARGUMENT -> std::runtime_error,
 * OUT_OF_RANGE -> std::out_of_range); see INTEGRATION.md.
 * Distances are squared L2 (no sqrt) or |1 - cos|, ids are int32, as in the reference.
 */
#ifndef GGNN_C_H
#define GGNN_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  GGNN_OK = 0,
  GGNN_INVALID_ARGUMENT = 1, /* std::runtime_error / glog CHECK in the reference */
  GGNN_INVALID_STATE = 2,    /* std::runtime_error ("base needs to be set", ...) */
  GGNN_OUT_OF_RANGE = 3,     /* std::out_of_range (ggnn.cu:96) */
  GGNN_OUT_OF_MEMORY = 4,
  GGNN_DEVICE_ERROR = 5,
  GGNN_UNSUPPORTED = 6,
  GGNN_IO_ERROR = 7
} ggnn_status;

/* include/ggnn/base/def.h:27-30 */
typedef enum { GGNN_EUCLIDEAN = 0, GGNN_COSINE = 1 } ggnn_measure;
/* include/ggnn/base/dataset.cuh (DataType): base / query element type.
 * GGNN_F16 (IEEE binary16) and GGNN_BF16 (bfloat16) have no reference counterpart: the kernels
 * widen every element exactly to float32 and compute all distances in float32 with the
 * operations of the float32 path (no intermediate is rounded to 16 bits), so a 16-bit base gives
 * the results of a float32 base holding the widened values.  Distances returned stay float32.
 * Rows are padded to 16 bytes as for the other types (8 elements).  No pre-screen: see
 * ggnn_set_prescreen.
 * GGNN_I8 (signed 8-bit, D bytes per row) has no reference counterpart either.  Base and query
 * have the same type.  Squared L2: the exact integer sum (o - q)^2, formed in 32-bit integer
 * arithmetic and converted once to float32 -- bit for bit the value of the GGNN_U8 path on the rows
 * x ^ 0x80 (2 * 255^2 * 4096 < 2^32: nothing wraps).  Cosine: the signed dot product and the row's
 * sum of squares are exact integers where the GGNN_U8 path forms integers, the query's sum of
 * squares is a float fmaf chain over the sign-extended elements, then |1 - dot / sqrt(|q|^2 |o|^2)|
 * as for every type; a zero row or a zero query gives 1.  Rows are padded with zeros to 16 bytes
 * (16 elements) by the handle; the ggnn_op_* entry points require D % 16 == 0.  No pre-screen
 * (8-bit rows are the compact copy already): ggnn_set_prescreen is accepted and has no effect.
 * Code 4 is reserved and refused (GGNN_INVALID_ARGUMENT). */
typedef enum { GGNN_F32 = 0, GGNN_U8 = 1, GGNN_F16 = 2, GGNN_BF16 = 3, GGNN_I8 = 5 } ggnn_dtype;
/* include/ggnn/base/data.cuh (MemoryLocation) reduced to what the boundary needs */
typedef enum { GGNN_CPU = 0, GGNN_GPU = 1 } ggnn_location;

typedef struct ggnn_handle ggnn_t;

/* ------------------------------------------------------------------------------------------
 * Section 1: ggnn::GGNN<int32_t,float>
 * ---------------------------------------------------------------------------------------- */

/* GGNN::GGNN() ggnn.cu:415-418 */
ggnn_status ggnn_create(ggnn_t** out);
void ggnn_destroy(ggnn_t* h);
/* message of the last failed call on this handle (or of ggnn_create when h == NULL) */
const char* ggnn_last_error(const ggnn_t* h);
const char* ggnn_version(void);

/* setWorkingDirectory ggnn.cuh:66-71 */
ggnn_status ggnn_set_working_directory(ggnn_t* h, const char* dir);
/* setCPUMemoryLimit ggnn.cuh:72-77 (accepted; all shards stay resident in 288 GB HBM) */
ggnn_status ggnn_set_cpu_memory_limit(ggnn_t* h, size_t memory_limit);
/* setReservedGPUMemory ggnn.cuh:79-84 */
ggnn_status ggnn_set_reserved_gpu_memory(ggnn_t* h, size_t reserved_memory);
/* setGPUs ggnn.cuh:86-98, ggnn.cu:89-100 (same range check, incl. quirk Q5) */
ggnn_status ggnn_set_gpus(ggnn_t* h, const int* gpu_ids, size_t num_gpus);
/* setShardSize ggnn.cuh:100-106 */
ggnn_status ggnn_set_shard_size(ggnn_t* h, uint32_t n_shard);
/* setReturnResultsOnGPU ggnn.cuh:108-114 */
ggnn_status ggnn_set_return_results_on_gpu(ggnn_t* h, int return_results_on_gpu);

/* setBase / setBaseReference ggnn.cuh:116-128, ggnn.cu:456-497.
 * take_copy != 0: the engine copies the data (setBase with an owning dataset, and what the
 * Python binding does, nanobind.cu:102-110).  take_copy == 0: borrow (setBaseReference); the
 * caller keeps the memory alive.  Host data is staged to the device at build()/bf_query(). */
ggnn_status ggnn_set_base(ggnn_t* h, const void* data, uint64_t N, uint32_t D, ggnn_dtype dtype,
                          ggnn_location location, int gpu_id, int take_copy);

/* build ggnn.cuh:130-137, ggnn.cu:205-240 */
ggnn_status ggnn_build(ggnn_t* h, uint32_t k_build, float tau_build,
                       uint32_t refinement_iterations, ggnn_measure measure);
/* store / load ggnn.cuh:138-147, ggnn.cu:242-276 ; files <workdir>/part_<shard>.ggnn with the
 * reference's pool layout (graph.cpp:48-91) */
ggnn_status ggnn_store(ggnn_t* h);
ggnn_status ggnn_load(ggnn_t* h, uint32_t k_build);

/* query ggnn.cuh:149-160, ggnn.cu:518-541.
 * ids_out/dists_out: [Nq x KQuery] (or [Nq x KQuery*shards] unmerged when results are returned
 * on the GPU, ggnn.cuh:108-113) in memory of kind out_location. */
ggnn_status ggnn_query(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D, ggnn_dtype dtype,
                       ggnn_location location, int gpu_id, uint32_t k_query, float tau_query,
                       uint32_t max_iterations, ggnn_measure measure, int32_t* ids_out,
                       float* dists_out, ggnn_location out_location);

/* Extension for serving (no counterpart in the reference, whose query() blocks,
 * gpu_instance.cu:687-712): enqueue one batch and return.  Batches given different `slot`s run on
 * different streams, so the thin tail of one batch's launch overlaps with the next batch.
 * Handle on one GPU: `query`, `ids_out`, `dists_out` are device memory on that GPU (gpu_id),
 * rows 16-byte aligned; the results are the sorted [Nq, k_query * shards] rows of
 * results-on-GPU mode.
 * Handle on several GPUs (ggnn_set_gpus): `query` is device memory of GPU gpu_id (any GPU of
 * the node) or, with gpu_id < 0, page-locked host memory; it is copied to every GPU on the
 * slot's stream.  The results are the MERGED [Nq, k_query] arrays (local searches, one packed
 * RCCL all-gather, per-GPU slice merges: replaces ggnn.cu:308-329 + result_merger.cpp:51-149),
 * written by asynchronous copies: ids_out / dists_out must be device memory or page-locked host
 * memory (pageable memory works but makes the copies synchronous).
 * Everything is valid after ggnn_synchronize() / ggnn_synchronize_slot(slot); `query`,
 * `ids_out` and `dists_out` must stay alive and untouched until then.
 * Ordering with ggnn_query(): both may be used on one handle from one thread; a blocking call
 * has its own stream and staging and does not wait for batches in flight.  A call whose
 * measure differs from the one the pre-screen copy was coded for drains every slot first. */
ggnn_status ggnn_query_async(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                             ggnn_dtype dtype, int gpu_id, uint32_t k_query, float tau_query,
                             uint32_t max_iterations, ggnn_measure measure, int32_t* ids_out,
                             float* dists_out, uint32_t slot);
ggnn_status ggnn_synchronize(ggnn_t* h);
/* wait for the batches of one slot only (slots are taken modulo the number of streams, 4) */
ggnn_status ggnn_synchronize_slot(ggnn_t* h, uint32_t slot);

/* bfQuery ggnn.cuh:162-172, ggnn.cu:543-564 */
ggnn_status ggnn_bf_query(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                          ggnn_dtype dtype, ggnn_location location, int gpu_id, uint32_t k_gt,
                          ggnn_measure measure, int32_t* ids_out, float* dists_out,
                          ggnn_location out_location);

/* Filtered search (an extension: the reference has no filter).  ggnn_query / ggnn_bf_query
 * restricted to the base vectors a bitset allows: here one filter per call, shared by all queries
 * of the batch (per-query filters: ggnn_set_filters below), over the GLOBAL base ids -- uint32 words, id i is allowed iff bit (i & 31) of word
 * (i >> 5) is set, ceil(n_bits / 32) words, bits at and above n_bits are ignored.  n_bits must
 * equal the base's N (GGNN_INVALID_ARGUMENT otherwise, also for a null bitset).  The bitset
 * may live on the host (filter_location GGNN_CPU; copied per call) or on GPU filter_gpu_id;
 * every GPU of the handle gets the whole bitset.
 * ggnn_query_filtered: the traversal of ggnn_query in which a denied vector still routes the
 * search (it is evaluated, queued, popped and expanded) but never enters the best list; the
 * termination rule then widens by itself until k_query ALLOWED vectors are found.  An all-ones
 * filter gives the result of ggnn_query bit for bit; slots that could not be filled hold
 * distance +inf and id -1 (plus the shard's id offset, as ggnn_query writes an unfilled slot).
 * Raise max_iterations / tau_query as the filter narrows; for very selective filters
 * ggnn_bf_query_filtered is the better call.  Works with several shards per GPU, several GPUs and
 * out-of-core shards; counters and timings are reported as for ggnn_query.
 * ggnn_bf_query_filtered: the exact k_gt nearest among the allowed vectors (ties: lower id first),
 * on the exhaustive scan kernels (there is no filtered matrix-core path). */
ggnn_status ggnn_query_filtered(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                uint32_t k_query, float tau_query, uint32_t max_iterations,
                                ggnn_measure measure, int32_t* ids_out, float* dists_out,
                                ggnn_location out_location, const uint32_t* allowed_bits,
                                uint64_t n_bits, ggnn_location filter_location, int filter_gpu_id);
ggnn_status ggnn_bf_query_filtered(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                   ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                   uint32_t k_gt, ggnn_measure measure, int32_t* ids_out,
                                   float* dists_out, ggnn_location out_location,
                                   const uint32_t* allowed_bits, uint64_t n_bits,
                                   ggnn_location filter_location, int filter_gpu_id);

/* Per-query filters: a resident filter table and one filter id per query.
 * The table is num_filters bitsets of the format above ([num_filters x ceil(n_bits / 32)] words,
 * n_bits must equal the base's N: GGNN_INVALID_ARGUMENT otherwise and for a null table with
 * num_filters > 0; GGNN_INVALID_STATE before ggnn_set_base).  ggnn_set_filters COPIES it (from
 * the host, or from GPU gpu_id): the engine keeps it on the host and places it on every GPU of
 * the handle as soon as those are known -- again after ggnn_build / ggnn_load / ggnn_set_gpus --
 * about num_filters * ceil(N / 32) * 4 bytes per GPU (plus two constant rows);
 * GGNN_OUT_OF_MEMORY if that cannot be allocated.  num_filters == 0 drops the table, and so does
 * ggnn_set_base.  ggnn_set_filters and ggnn_update_filter (replaces row `index` on every GPU;
 * GGNN_OUT_OF_RANGE for index >= num_filters) SYNCHRONISE: they first wait for every asynchronous
 * slot, so no batch in flight sees a half-written row.
 *
 * The *_filtered_by calls take one int32 filter id per query (filter_ids[Nq]) instead of a bitset:
 *   id f in [0, num_filters)  the result of ggnn_query_filtered / ggnn_bf_query_filtered of that
 *                             query with row f, bit for bit (ids, distances, counters);
 *   id -1                     unfiltered: the result of ggnn_query / ggnn_bf_query, bit for bit;
 *   any other id              an empty result: every slot (-1 + id offset, +inf).
 * No id value makes a kernel read outside the table.  The blocking calls read an id array in host
 * memory first and answer anything outside [-1, num_filters) with GGNN_INVALID_ARGUMENT (an id
 * array in device memory is not read back: there the rule above holds).  GGNN_INVALID_STATE
 * without a table.  Everything else is ggnn_query / ggnn_bf_query: shards, GPUs, exchange modes,
 * out-of-core shards, result location, counters and timings.
 * ggnn_query_async_filtered_by is ggnn_query_async with filter ids.  The ids follow the memory
 * rule of `query` in that call: handle on one GPU -- device memory on that GPU; several GPUs --
 * device memory of GPU gpu_id or, with gpu_id < 0, page-locked host memory, copied on the slot's
 * stream.  They must stay alive and untouched until the slot is synchronised.  Nothing is staged
 * per call but the ids, which is why the table is resident. */
ggnn_status ggnn_set_filters(ggnn_t* h, const uint32_t* bits, uint32_t num_filters,
                             uint64_t n_bits, ggnn_location location, int gpu_id);
ggnn_status ggnn_update_filter(ggnn_t* h, uint32_t index, const uint32_t* bits, uint64_t n_bits,
                               ggnn_location location, int gpu_id);
ggnn_status ggnn_get_num_filters(const ggnn_t* h, uint32_t* num_filters);
ggnn_status ggnn_query_filtered_by(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                   ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                   uint32_t k_query, float tau_query, uint32_t max_iterations,
                                   ggnn_measure measure, int32_t* ids_out, float* dists_out,
                                   ggnn_location out_location, const int32_t* filter_ids,
                                   ggnn_location ids_location, int ids_gpu_id);
ggnn_status ggnn_bf_query_filtered_by(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                      ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                      uint32_t k_gt, ggnn_measure measure, int32_t* ids_out,
                                      float* dists_out, ggnn_location out_location,
                                      const int32_t* filter_ids, ggnn_location ids_location,
                                      int ids_gpu_id);
ggnn_status ggnn_query_async_filtered_by(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                         ggnn_dtype dtype, int gpu_id, uint32_t k_query,
                                         float tau_query, uint32_t max_iterations,
                                         ggnn_measure measure, int32_t* ids_out, float* dists_out,
                                         uint32_t slot, const int32_t* filter_ids);

/* Label filters: one int32 label per base vector and one int32 label per query.
 * For many categories (tenants) the filter table above costs num_filters * N / 8 bytes per GPU; a
 * label column costs 4 * N bytes whatever the number of categories.  A base vector may be reported
 * to a query iff their labels are EQUAL.  Query n with label L gives, bit for bit (ids, distances,
 * counters), the result of ggnn_query_filtered / ggnn_bf_query_filtered of that query with the
 * bitset (labels == L); label -1 searches unfiltered (ggnn_query / ggnn_bf_query), whatever the
 * base labels are.  There is no invalid label value: a label that no row carries gives an empty
 * result, every slot (-1 + id offset, +inf).  Labels are int32 only; a query selects by equality
 * here and by membership in a small set below (*_labeled_in).
 *
 * ggnn_set_labels COPIES labels[n] (int32 over the global base ids, from the host or from GPU
 * gpu_id; n must equal the base's N: GGNN_INVALID_ARGUMENT otherwise, GGNN_INVALID_STATE before
 * ggnn_set_base): the engine keeps the column on the host and places it on every GPU of the handle
 * as soon as those are known -- again after ggnn_build / ggnn_load / ggnn_set_gpus, and on first
 * use by a ggnn_bf_query_labeled without a graph -- 4 * N bytes per GPU; GGNN_OUT_OF_MEMORY if
 * that cannot be allocated.  A null pointer drops the labels, and so does ggnn_set_base.
 * ggnn_update_labels relabels `count` rows: labels[ids[i]] = values[i], applied in order (the last
 * pair of a repeated id wins).  An id outside [0, N) is GGNN_OUT_OF_RANGE and nothing is changed;
 * GGNN_INVALID_STATE when no labels are set.  Both calls SYNCHRONISE: they first wait for every
 * asynchronous slot.  ggnn_get_num_labels gives N, or 0 when no labels are set.
 *
 * The *_labeled calls are the *_filtered_by calls with query_labels[Nq] in place of filter_ids --
 * the same memory rules, nothing is validated because every value is valid -- and
 * GGNN_INVALID_STATE without labels.  These calls take no bitset: see *_labeled_in. */
ggnn_status ggnn_set_labels(ggnn_t* h, const int32_t* labels, uint64_t n, ggnn_location location,
                            int gpu_id);
ggnn_status ggnn_update_labels(ggnn_t* h, const int64_t* ids, const int32_t* values,
                               uint64_t count, ggnn_location location, int gpu_id);
ggnn_status ggnn_get_num_labels(const ggnn_t* h, uint64_t* n);
ggnn_status ggnn_query_labeled(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                               ggnn_dtype dtype, ggnn_location location, int gpu_id,
                               uint32_t k_query, float tau_query, uint32_t max_iterations,
                               ggnn_measure measure, int32_t* ids_out, float* dists_out,
                               ggnn_location out_location, const int32_t* query_labels,
                               ggnn_location labels_location, int labels_gpu_id);
ggnn_status ggnn_bf_query_labeled(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                  ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                  uint32_t k_gt, ggnn_measure measure, int32_t* ids_out,
                                  float* dists_out, ggnn_location out_location,
                                  const int32_t* query_labels, ggnn_location labels_location,
                                  int labels_gpu_id);
ggnn_status ggnn_query_async_labeled(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                     ggnn_dtype dtype, int gpu_id, uint32_t k_query,
                                     float tau_query, uint32_t max_iterations,
                                     ggnn_measure measure, int32_t* ids_out, float* dists_out,
                                     uint32_t slot, const int32_t* query_labels);

/* Exact range search (an extension): EVERY base vector within a radius of each query, where
 * ggnn_bf_query returns the k_gt best.  Base row i belongs to the answer of query n iff the call's
 * filter admits it and d(n, i) <= radii[n], compared in float32; d is the float32 value the scan
 * kernels of ggnn_bf_query report for the pair, bit for bit.
 *   *** A Euclidean radius is in SQUARED units: d is the squared L2 distance (no square root). ***
 *   Cosine: d = |1 - cos|; a zero row or a zero query gives 1.0.
 * radii[Nq] is HOST memory, one radius per query: +inf admits every allowed row whose distance is not
 * NaN, a negative radius admits nothing, a NaN radius is GGNN_INVALID_ARGUMENT.
 * The result is CSR-shaped: lims_out[Nq + 1] (HOST memory, always written: lims_out[0] = 0,
 * lims_out[Nq] the total), and the rows of query n at ids_out / dists_out [lims_out[n], lims_out[n + 1])
 * in ASCENDING ID.  ids_out / dists_out hold `capacity` entries at out_location.  If lims_out[Nq] >
 * capacity they are left untouched and the call still returns GGNN_OK: compare lims_out[Nq] with the
 * capacity, and call again with enough room.  ids_out == dists_out == NULL with capacity == 0 is the
 * count-only call.  Every call evaluates all distances twice (a counting pass and a filling pass;
 * once when capacity == 0); no atomics decide a position, so results do not vary from run to run.
 * The *_filtered, *_filtered_by and *_labeled forms take the filter of the ggnn_bf_query call of the
 * same name, with the same rules (label -1 / filter id -1: every row).  Label sets, label ranges and
 * label masks have no range form.  Single GPU, any state of the handle after ggnn_set_base, exactly
 * as ggnn_bf_query; always scan kernels (hook BF_RANGE_SLICES forces their slice count). */
ggnn_status ggnn_bf_range_query(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                const float* radii, ggnn_measure measure, uint64_t capacity,
                                uint64_t* lims_out, int32_t* ids_out, float* dists_out,
                                ggnn_location out_location);
ggnn_status ggnn_bf_range_query_filtered(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                         ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                         const float* radii, ggnn_measure measure,
                                         uint64_t capacity, uint64_t* lims_out, int32_t* ids_out,
                                         float* dists_out, ggnn_location out_location,
                                         const uint32_t* allowed_bits, uint64_t n_bits,
                                         ggnn_location filter_location, int filter_gpu_id);
ggnn_status ggnn_bf_range_query_filtered_by(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                            ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                            const float* radii, ggnn_measure measure,
                                            uint64_t capacity, uint64_t* lims_out,
                                            int32_t* ids_out, float* dists_out,
                                            ggnn_location out_location, const int32_t* filter_ids,
                                            ggnn_location ids_location, int ids_gpu_id);
ggnn_status ggnn_bf_range_query_labeled(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                        ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                        const float* radii, ggnn_measure measure,
                                        uint64_t capacity, uint64_t* lims_out, int32_t* ids_out,
                                        float* dists_out, ggnn_location out_location,
                                        const int32_t* query_labels, ggnn_location labels_location,
                                        int labels_gpu_id);

/* Label index: a label's rows found without reading the label column.
 * The index is the label column grouped by label (CSR over the global base ids: the distinct labels
 * ascending, and the ids of every label ascending), 4 * N + 8 * L + 4 bytes for L distinct labels.
 * ggnn_op_bf_query_label_index (section 2) answers every query exactly from the rows of its label
 * alone, at about one distance evaluation per row of the label however large the base is, and
 * ggnn_op_label_index_classify says which queries of a batch have a label of at most `cutoff` rows.
 * Label sets and label ranges go through the same index: a closed label interval is one contiguous run
 * of its rows, a set of eight labels at most eight (ggnn_op_label_spans_resolve,
 * ggnn_op_bf_query_label_spans, ggnn_op_label_spans_classify, section 2) -- for int8 rows the only way
 * to search by a label set or a label range.  Label masks have no index form: tag bits are not a sort
 * key.  The handle's *_labeled calls do not use an index: they search as described above, and a caller
 * that wants small labels or narrow ranges answered from their rows routes with these operators.
 * (Routing inside the handle was tried and taken out again: with it in the tree an out-of-core build
 * faulted on the GPU, and the cause has not been found.) */
/* The index of a label column (pure host): keys[n_keys] the distinct labels in ascending signed
 * order, offsets[n_keys + 1] with offsets[0] = 0 and offsets[n_keys] = n, rows[n] the ids sorted by
 * (label, id).  The caller provides keys[n], offsets[n + 1], rows[n].  n must be in [1, 2^30]:
 * GGNN_INVALID_ARGUMENT otherwise, and nothing is written. */
ggnn_status ggnn_label_index_build(const int32_t* labels, uint64_t n, int32_t* keys,
                                   uint32_t* offsets, int32_t* rows, uint32_t* n_keys);

/* Label sets: "any of these labels", combined with a filter id.
 * Query n carries a label SET -- row n of query_label_sets[Nq x set_width], 1 <= set_width <=
 * GGNN_MAX_LABEL_SET -- and, optionally, a filter id filter_ids[n] into the resident filter table
 * of ggnn_set_filters (the whole array may be null).  Base vector i may be reported to query n iff
 *   labels[i] equals at least one entry of the set, or some entry of the set is -1 (the wildcard of
 *   ggnn_query_labeled; entries may repeat, so a short set is padded by repeating an entry; every
 *   other value is valid and only compared, never used as an index), AND
 *   the filter id admits i under the rules of ggnn_query_filtered_by: -1 or a null array admits
 *   every vector, an id in [0, num_filters) needs the vector's bit in that row, any other id
 *   admits none.
 * Query n gives, bit for bit (ids, distances, counters), the result of ggnn_query_filtered /
 * ggnn_bf_query_filtered of that query with the bitset isin(labels, set n) & row(filter_ids[n]);
 * an empty predicate gives every slot (-1 + id offset, +inf).  set_width 1 with null ids is
 * ggnn_query_labeled, an all -1 set with ids is ggnn_query_filtered_by.
 * The sets follow the memory rules of query_labels in the *_labeled calls and the ids those of
 * filter_ids in the *_filtered_by calls (ggnn_query_async_labeled_in: both live where the query
 * lives and are not read on the host).  GGNN_INVALID_ARGUMENT for a set_width outside [1, 8], a
 * null set array and host-resident ids outside [-1, num_filters); GGNN_INVALID_STATE without
 * labels, and with ids but no filter table; GGNN_UNSUPPORTED on an int8 base and for shards of more
 * than 2^30 vectors.  Everything else is ggnn_query / ggnn_bf_query.  ggnn_bf_query_labeled_in
 * always runs the scan kernels: ggnn_last_bf_query_matrix_path reports 0.
 * What remains: at most 8 labels per query (numeric predicates: the label ranges below), int32
 * labels only, no int8 rows, no matrix-core path. */
#define GGNN_MAX_LABEL_SET 8
ggnn_status ggnn_query_labeled_in(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                  ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                  uint32_t k_query, float tau_query, uint32_t max_iterations,
                                  ggnn_measure measure, int32_t* ids_out, float* dists_out,
                                  ggnn_location out_location, const int32_t* query_label_sets,
                                  uint32_t set_width, ggnn_location sets_location, int sets_gpu_id,
                                  const int32_t* filter_ids, ggnn_location ids_location,
                                  int ids_gpu_id);
ggnn_status ggnn_bf_query_labeled_in(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                     ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                     uint32_t k_gt, ggnn_measure measure, int32_t* ids_out,
                                     float* dists_out, ggnn_location out_location,
                                     const int32_t* query_label_sets, uint32_t set_width,
                                     ggnn_location sets_location, int sets_gpu_id,
                                     const int32_t* filter_ids, ggnn_location ids_location,
                                     int ids_gpu_id);
ggnn_status ggnn_query_async_labeled_in(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                        ggnn_dtype dtype, int gpu_id, uint32_t k_query,
                                        float tau_query, uint32_t max_iterations,
                                        ggnn_measure measure, int32_t* ids_out, float* dists_out,
                                        uint32_t slot, const int32_t* query_label_sets,
                                        uint32_t set_width, const int32_t* filter_ids);

/* Label ranges: "the label lies in one of these intervals", combined with a filter id.
 * Query n carries n_ranges closed intervals -- row n of query_label_ranges[Nq x n_ranges x 2], int32
 * pairs (lo, hi), 1 <= n_ranges <= GGNN_MAX_LABEL_RANGES -- and, optionally, a filter id
 * filter_ids[n] into the resident filter table of ggnn_set_filters (the whole array may be null).
 * Base vector i may be reported to query n iff
 *   lo_j <= labels[i] <= hi_j for at least one j, compared as SIGNED int32, AND
 *   the filter id admits i under the rules of ggnn_query_filtered_by: -1 or a null array admits
 *   every vector, an id in [0, num_filters) needs the vector's bit in that row, any other id
 *   admits none.
 * Query n gives, bit for bit (ids, distances, counters), the result of ggnn_query_filtered /
 * ggnn_bf_query_filtered of that query with the bitset any_j(lo_j <= labels <= hi_j) &
 * row(filter_ids[n]); an empty predicate gives every slot (-1 + id offset, +inf).
 *   An interval with lo > hi is EMPTY: it contains nothing, it is neither wrapped around nor
 *   swapped.  A short list is padded by repeating an interval or with an empty one such as (1, 0);
 *   a query whose intervals are all empty has an empty result.
 *   There is NO WILDCARD value, unlike *_labeled and *_labeled_in: -1 is an ordinary label here --
 *   (-5, 5) admits the rows labelled -5 .. 5 and nothing else -- and (INT32_MIN, INT32_MAX) admits
 *   every label.  Every int32 value is a valid bound: bounds are compared, never used as an index.
 * One interval (L, L) with L != -1 and null ids is ggnn_query_labeled with label L; intervals (a, a),
 * (b, b), ... are ggnn_query_labeled_in with the set {a, b, ...} when no entry is -1; (INT32_MIN,
 * INT32_MAX) with ids is ggnn_query_filtered_by, and with null ids ggnn_query.
 * The ranges follow the memory rules of query_label_sets and the ids those of filter_ids in the
 * *_labeled_in calls (ggnn_query_async_labeled_range: both live where the query lives and are not
 * read on the host).  GGNN_INVALID_ARGUMENT for n_ranges outside [1, 4], a null range array and
 * host-resident ids outside [-1, num_filters); GGNN_INVALID_STATE without labels, and with ids but
 * no filter table; GGNN_UNSUPPORTED on an int8 base and for shards of more than 2^30 vectors.
 * Everything else is ggnn_query / ggnn_bf_query.  ggnn_bf_query_labeled_range always runs the scan
 * kernels: ggnn_last_bf_query_matrix_path reports 0.
 * What remains: at most 4 intervals per query, one int32 column (float32 attributes: map them to
 * int32 in order first), closed intervals only, no int8 rows, no matrix-core path. */
#define GGNN_MAX_LABEL_RANGES 4
ggnn_status ggnn_query_labeled_range(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                     ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                     uint32_t k_query, float tau_query, uint32_t max_iterations,
                                     ggnn_measure measure, int32_t* ids_out, float* dists_out,
                                     ggnn_location out_location,
                                     const int32_t* query_label_ranges, uint32_t n_ranges,
                                     ggnn_location ranges_location, int ranges_gpu_id,
                                     const int32_t* filter_ids, ggnn_location ids_location,
                                     int ids_gpu_id);
ggnn_status ggnn_bf_query_labeled_range(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                        ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                        uint32_t k_gt, ggnn_measure measure, int32_t* ids_out,
                                        float* dists_out, ggnn_location out_location,
                                        const int32_t* query_label_ranges, uint32_t n_ranges,
                                        ggnn_location ranges_location, int ranges_gpu_id,
                                        const int32_t* filter_ids, ggnn_location ids_location,
                                        int ids_gpu_id);
ggnn_status ggnn_query_async_labeled_range(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                           ggnn_dtype dtype, int gpu_id, uint32_t k_query,
                                           float tau_query, uint32_t max_iterations,
                                           ggnn_measure measure, int32_t* ids_out,
                                           float* dists_out, uint32_t slot,
                                           const int32_t* query_label_ranges, uint32_t n_ranges,
                                           const int32_t* filter_ids);

/* Label masks: the label of a base vector read as 32 TAG BITS, combined with a filter id.
 * Query n carries n_masks clauses -- row n of query_label_masks[Nq x n_masks x 3], int32 triples
 * (mask, value, any), 1 <= n_masks <= GGNN_MAX_LABEL_MASKS -- and, optionally, a filter id
 * filter_ids[n] into the resident filter table of ggnn_set_filters (the whole array may be null).
 * Base vector i passes a clause iff
 *   (labels[i] & mask) == value  AND  (any == 0 OR (labels[i] & any) != 0)
 * and may be reported to query n iff it passes at least one of the query's clauses AND the filter id
 * admits i under the rules of ggnn_query_filtered_by: -1 or a null array admits every vector, an id
 * in [0, num_filters) needs the vector's bit in that row, any other id admits none.
 * Query n gives, bit for bit (ids, distances, counters), the result of ggnn_query_filtered /
 * ggnn_bf_query_filtered of that query with the bitset
 *   any_j(((labels & mask_j) == value_j) & ((any_j == 0) | ((labels & any_j) != 0))) & row(filter_ids[n]);
 * an empty predicate gives every slot (-1 + id offset, +inf).
 *   (0, 0, 0) admits every vector.  There is NO WILDCARD value.  Bit 31 is a bit like any other.
 *   A clause whose value has a bit outside its mask admits NOTHING: that is the definition, not an
 *   error, and value is never pre-masked.  No clause value is invalid.  A short list is padded by
 *   repeating a clause.
 * One clause says "all of A, none of B, any of C" as mask = A | B, value = A, any = C, and "field
 * equals v" with mask = the field's bits, value = v at the field's position; two clauses say "mine or
 * public".  (~0, L, 0) with null ids is ggnn_query_labeled with label L != -1.
 * The clauses follow the memory rules of query_label_ranges and the ids those of filter_ids in the
 * *_labeled_range calls (ggnn_query_async_labeled_mask: both live where the query lives and are not
 * read on the host).  GGNN_INVALID_ARGUMENT for n_masks outside [1, 2], a null clause array and
 * host-resident ids outside [-1, num_filters); GGNN_INVALID_STATE without labels, and with ids but
 * no filter table; GGNN_UNSUPPORTED on an int8 base and for shards of more than 2^30 vectors.
 * Everything else is ggnn_query / ggnn_bf_query.  ggnn_bf_query_labeled_mask always runs the scan
 * kernels: ggnn_last_bf_query_matrix_path reports 0.
 * What remains: at most 2 clauses per query, one int32 column, no int8 rows, no matrix-core path. */
#define GGNN_MAX_LABEL_MASKS 2
ggnn_status ggnn_query_labeled_mask(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                    ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                    uint32_t k_query, float tau_query, uint32_t max_iterations,
                                    ggnn_measure measure, int32_t* ids_out, float* dists_out,
                                    ggnn_location out_location,
                                    const int32_t* query_label_masks, uint32_t n_masks,
                                    ggnn_location masks_location, int masks_gpu_id,
                                    const int32_t* filter_ids, ggnn_location ids_location,
                                    int ids_gpu_id);
ggnn_status ggnn_bf_query_labeled_mask(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                       ggnn_dtype dtype, ggnn_location location, int gpu_id,
                                       uint32_t k_gt, ggnn_measure measure, int32_t* ids_out,
                                       float* dists_out, ggnn_location out_location,
                                       const int32_t* query_label_masks, uint32_t n_masks,
                                       ggnn_location masks_location, int masks_gpu_id,
                                       const int32_t* filter_ids, ggnn_location ids_location,
                                       int ids_gpu_id);
ggnn_status ggnn_query_async_labeled_mask(ggnn_t* h, const void* query, uint64_t Nq, uint32_t D,
                                          ggnn_dtype dtype, int gpu_id, uint32_t k_query,
                                          float tau_query, uint32_t max_iterations,
                                          ggnn_measure measure, int32_t* ids_out,
                                          float* dists_out, uint32_t slot,
                                          const int32_t* query_label_masks, uint32_t n_masks,
                                          const int32_t* filter_ids);

/* layout of one graph shard, include/ggnn/base/graph_config.h:31-112 */
typedef struct {
  uint32_t N, D, KBuild;
  uint32_t KF, G, S, S0, S0_off, SG, SG_off;
  uint32_t N_all, ST_all;
  uint32_t Bs[4], Ns[4], Ns_offsets[4], STs_offsets[4];
} ggnn_graph_config;

/* getGraph ggnn.cuh:174-175 + Graph (graph.h:38-71): device views of one shard, valid until
 * the handle is destroyed.  graph [N_all x KBuild], translation/selection [ST_all],
 * nn1_stats [2] = {mean, max}. */
typedef struct {
  ggnn_graph_config config;
  const int32_t* graph;
  const int32_t* translation;
  const int32_t* selection;
  const float* nn1_stats;
  int gpu_id;
} ggnn_graph_view;
ggnn_status ggnn_get_graph(ggnn_t* h, uint32_t global_shard_id, ggnn_graph_view* out);

/* tracing (reference: cudaEvent timings printed through glog, gpu_instance.cu:536-545,687-712).
 * Sum of the HIP-event durations (ms) of the kernels of the last build / query / bf_query. */
ggnn_status ggnn_last_timing_ms(const ggnn_t* h, float* build_ms, float* query_ms, float* bf_ms);
/* per-query work counters of the last ggnn_query (sum over queries and shards): number of
 * distance evaluations and of successful pops; used for the roofline figure. */
ggnn_status ggnn_last_query_counters(const ggnn_t* h, uint64_t* n_dist, uint64_t* n_pop);
/* how the last ggnn_query combined the per-GPU results (replaces the D2H + CPU heap merge of
 * ggnn.cu:308-329 / result_merger.cpp:51-149): "none" (one GPU), "rccl" (grouped ncclAllGather
 * over xGMI + per-GPU slice merge) "copy" (peer copies to the first GPU: contexts sharing one
 * device, or no librccl) or "gather" (hook EXCHANGE = 3).  Hook EXCHANGE (ggnn_set_hook) forces
 * one of them. */
const char* ggnn_last_exchange(const ggnn_t* h);
/* ranks of the RCCL communicator the handle's exchange runs on (ncclCommCount of its first
 * communicator): the number of GPUs of the handle once an "rccl" exchange has run, 0 before that,
 * without librccl, or after a fallback to peer copies.  A multi-GPU benchmark line that says
 * "rccl" must carry this number equal to its GPU count. */
ggnn_status ggnn_rccl_ranks(const ggnn_t* h, uint32_t* ranks);
/* number of half-batches the last blocking multi-GPU ggnn_query was searched in: 2 when the search
 * of the second half overlapped the exchange and merge of the first (hook QUERY_SPLIT), else 1 */
ggnn_status ggnn_last_query_parts(const ggnn_t* h, uint32_t* parts);
/* queries of the last ggnn_bf_query that were answered by the exhaustive scan because the
 * matrix-core pre-selection could not be certified exact (tracing; results are exact either way) */
ggnn_status ggnn_last_bf_query_rescanned(const ggnn_t* h, uint32_t* n_rescanned);
/* *out = 1 if the last ggnn_bf_query* call of the handle (filtered or not) ran the matrix-core
 * tile kernel on every shard, else 0 (the scan kernels; also before the first call and after a
 * call without queries).  Results are bit-identical on either path: this getter is how a caller
 * or a test tells which one ran.  out == NULL: GGNN_INVALID_ARGUMENT.
 * ggnn_last_bf_query_rescanned covers the filtered calls as well. */
ggnn_status ggnn_last_bf_query_matrix_path(const ggnn_t* h, int* out);
ggnn_status ggnn_set_collect_counters(ggnn_t* h, int enable);
/* rows the last ggnn_query read for those evaluations (needs collect_counters): float rows
 * (4*D bytes each) and, with the pre-screen, 8-bit code rows (prescreen_code_dim(D) bytes each: a power of two up to 64, multiples of 64 above). */
ggnn_status ggnn_last_query_rows_read(const ggnn_t* h, uint64_t* float_rows, uint64_t* code_rows);
/* Work of the construction kernels of the last ggnn_build, summed over every launch and shard
 * (needs ggnn_set_collect_counters before the build; the build then synchronises after every
 * merge / sym launch to time it with its own HIP events and to read the per-point counters, so it
 * is a diagnostic mode).  For SURVEY 8(d)'s build roofline ("sum over kernel launches"):
 * bytes of a kernel = float_rows x 4D + code_rows x prescreen_code_dim(D) + pops x graph-row bytes
 * (merge: KBuild x 4; sym: (KBuild + KBuild/2) x 4: graph row + pending inverse links)
 * + points x (own row 4D + result row). */
typedef struct {
  uint64_t launches, points;   /* kernel launches and points (= waves) they processed */
  uint64_t n_dist;             /* distance evaluations of the reference's algorithm */
  uint64_t float_rows;         /* 4D-byte rows actually read */
  uint64_t code_rows;          /* pre-screen code rows read */
  uint64_t pops;               /* graph rows read */
  double ms;                   /* sum of the launches' HIP-event durations */
} ggnn_kernel_work;
typedef struct {
  ggnn_kernel_work merge, sym;
} ggnn_build_work;
ggnn_status ggnn_last_build_work(const ggnn_t* h, ggnn_build_work* out);
/* Exact pre-screen of the float32 query and merge kernels (no reference counterpart; results
 * are identical with it on or off, see ggnn_op_prescreen_encode).  On by default; hook PRESCREEN = 0
 * (ggnn_set_hook) turns the default of handles created afterwards off.  Accepted on a uint8,
 * float16 or bfloat16 base, where it has no effect (those rows have no pre-screen codes). */
ggnn_status ggnn_set_prescreen(ggnn_t* h, int enable);
/* Deterministic build (no reference counterpart; the reference's build is not reproducible:
 * cuRAND stream graph_construction.cu:96-102,168-169, atomics and cross-block reads in sym
 * sym_query_layer.cu:102-104,124-141).  `rng` (host, may be null with n_rng = 0): uniform (0,1]
 * numbers for the selection kernel, [3][N_shard], layer l of every shard reads rng[l * N_shard
 * + n] instead of the engine's generator; `serial_sym` != 0 launches the sym kernel one point
 * at a time in ascending order.  With both, ggnn_build follows one fixed serialisation of
 * GraphConstructionImpl::build/refine (graph_construction.cu:128-147) that a CPU restatement can
 * be compared with bit for bit.  Slow; off by default.  `serial_sym` = 2 instead: the sym
 * searches of a pass run concurrently but do not read the inverse links requested in that pass,
 * and the slots are then handed out in ascending order of the requesting point (one wave; a
 * point already holding a slot at a candidate is not given a second) -- a build that is the
 * same on every run (with the engine's own seeded generator), not the reference's schedule.
 * Also slow: the hand-out is serial (bench.py uses it only for --dump-outputs runs). */
ggnn_status ggnn_set_build_hooks(ggnn_t* h, const float* rng, uint64_t n_rng, int serial_sym);
/* shard layout chosen by ggnn_build / ggnn_load (GGNNImpl::prepare, ggnn.cu:154-203): total
 * number of shards, shards per GPU (the width factor of results returned on the GPU,
 * ggnn.cu:299-306) and points per shard.  GGNN_INVALID_STATE without a graph. */
ggnn_status ggnn_get_shard_layout(const ggnn_t* h, uint32_t* num_shards, uint32_t* shards_per_gpu,
                                  uint32_t* n_shard);
/* tracing: peak engine clock the device reports (hipDeviceAttributeClockRate), in Hz; used to
 * turn SQ cycle counters into utilisation figures instead of assuming a nominal clock */
ggnn_status ggnn_device_clock_hz(int device, double* clock_hz);
/* nanobind.cu:151 set_log_level */
void ggnn_set_log_level(int level);

/* Test and tuning hooks (no reference counterpart): process-wide named integers that select a
 * code path or a tuning constant.  NONE changes a result -- every value yields the same ids and
 * distances; they exist so that tests can force rarely taken paths and so that A/B measurements
 * need no rebuild.  Precedence: ggnn_set_hook > the environment variable GGNN_<NAME>, which is
 * consulted ONLY while GGNN_TEST_HOOKS=1 is set (a production process that merely inherits such a
 * variable is not steered by it) > the default.  Unknown name: GGNN_INVALID_ARGUMENT.
 *
 *   name             default  values
 *   PRESCREEN           1     default of ggnn_set_prescreen for handles created afterwards
 *   EXCHANGE            0     0 auto | 1 ("rccl") RCCL all-gather, also on one GPU (1-rank world)
 *                             | 2 ("copy") peer copies to the first GPU | 3 ("gather", blocking
 *                             calls) every GPU gathers all rows by peer copies and merges its
 *                             1/G slice: the RCCL path's structure without RCCL, for handles whose
 *                             contexts share a device
 *   SYM_PRESCREEN      -1     sym kernel with the pre-screen: -1 auto (rows >= 1 KB) | 0 | 1
 *   SHARD_OVERLAP       1     0 = resident shards of one GPU searched one launch at a time
 *   VIS_SLOTS           8     usable keys per bucket of the hashed visited set, 1..8 (small values
 *                             exercise stash, overflow and removal paths)
 *   VIS_TAG_SET         1     0 = visited rings of 481..2016 keys (searches of 513..2048 iterations)
 *                             are scanned instead of probed through the 16-bit tag set
 *   QUERY_SPLIT        -1     blocking ggnn_query on several GPUs as two half-batches in flight:
 *                             -1 auto (from 4096 queries) | 0 never | 1 always (from 2 queries)
 *   RESIDENT_SHARDS     0     GPU slots per device for its shards: 0 = decided from the free device
 *                             memory (all resident whenever they fit); n < shards per GPU forces the
 *                             out-of-core mode (shards take turns: GPU <-> pinned host <-> part files)
 *   XCD_MAP             3     bit 0: merge kernel, bit 1: sym kernel -- workgroups of one XCD take a
 *                             contiguous range of points (consecutive points share neighbourhoods)
 *   BF_POOL_KEEP_MB  1024     bytes the private bf_query scratch pool keeps between calls
 *   BF_NO_I8            0     1 = uint8 bf_query through the float matrix-core kernels
 *   BF_I8_V1            0     1 = LDS-list i8 kernel instead of the register-set one
 *   BF_SLICES           0     0 auto | base slices per query block (1..64)
 *   BF_NO_CENTER        0     1 = float32 rows not shifted by the column mean (exercises the re-scan)
 *   BF_TILES            3     2 | 3 | 4 base tiles per accumulator group (D > 128)
 *   BF_I8_NOSHARE       0     1 = slices of the i8 kernel do not share their bound
 *   BF_I8_RANKS        -1     bit mask of the K-best set positions the slices of the i8 kernel
 *                             exchange (bit i = the i-th of {0,1,2,4,9} for sets of 10); -1 = auto
 *                             (ONE position chosen from the number of slices: the default), 31 = all
 *                             five, 16 = only the last entry (the single shared bound of rounds 3-4)
 *   BF_I8_REFRESH      64     stages of 128 rows between those exchanges (before that: at stages
 *                             1, 2, 4, ...)
 *   BF_I8_SEED          0     rows of an optional seeding launch of the i8 kernel (the K-th best
 *                             distance over the head of the base as every slice's first bound);
 *                             0 = none (measured: the launch costs what its fewer hits save)
 *   BF_SCAN             0     1 = scan kernels instead of the matrix-core brute force
 *   RCCL_FAIL_AFTER     0     fault injection: the n-th multi-GPU exchange of the process reports an
 *                             RCCL failure (exercises the peer-copy fallback); 0 = never
 *   QUERY_EARLY         1     query kernel, graphs with KBuild <= 24: 1 = the first-read rows of a
 *                             pop's neighbours (pre-screen codes, or rows of <= 128 bytes) are
 *                             requested BEFORE the pop's bookkeeping and the membership test;
 *                             0 = after them (the order of rounds 1-4; same results)
 *   MERGE_EARLY         1     the same switch for the merge kernel
 *   QUERY_LDS_PAD       0     extra bytes of LDS per wave of the early-rows query kernels (lowers the
 *                             occupancy: measurements of its effect without a rebuild)
 *   QUERY_GLOBAL_RING   1     early-rows query kernels whose search cannot wrap its visited ring
 *                             (max_iterations <= ring length): 1 = no ring at all, the hashed set's
 *                             buckets and stash ARE the visited keys (overflow list in global
 *                             memory); 0 = ring in LDS mirrored by the set
 *   MERGE_COUNTING      0     merge launches WITHOUT work counters (every production build) run a
 *                             kernel that tests a candidate against the sorted part of the cache
 *                             only once it has passed the pre-screen; 1 = they run the counting
 *                             kernel, which scans the sorted part for every candidate first (same
 *                             graph; A/B and test hook)
 *   PS_EXACT            1     early-rows query kernels on a float32 base whose pre-screen copy is
 *                             lossless on a power-of-two grid (integer or dyadic data, squared L2)
 *                             take a candidate's distance from its codes when the query lies on
 *                             the grid too, and read no float row (kernel variants of their own,
 *                             launched by the engine, which knows the copy's flag; the operator
 *                             seam always runs the float rows); 0 = always the float rows (same
 *                             results; A/B and test hook)
 *   LABEL_INDEX_SLICES  0     slices the index scans (one label, label spans) cut a query's rows into
 *                             (1..64): 0 = chosen from the longest segment the call can touch -- for
 *                             spans, span_limit -- and the number of queries (same results for every
 *                             count; test hook)
 *   BF_RANGE_SLICES     0     slices the range search cuts the base into per query (1..64): 0 = chosen
 *                             like the scan's, from the number of queries and rows (same results
 *                             for every count; test hook) */
ggnn_status ggnn_set_hook(const char* name, int64_t value);
/* back to environment / default */
ggnn_status ggnn_reset_hook(const char* name);
/* the value a use of the hook would see right now */
ggnn_status ggnn_get_hook(const char* name, int64_t* value);

/* ------------------------------------------------------------------------------------------
 * Section 2: operator seam (device pointers, explicit stream).  `stream` is a hipStream_t.
 * ---------------------------------------------------------------------------------------- */

/* GraphConfig(params) src/ggnn/base/graph_config.cpp:30-113 (pure host) */
ggnn_status ggnn_graph_config_init(uint32_t N, uint32_t D, uint32_t KBuild,
                                   ggnn_graph_config* out);
/* host sizing of the query kernel, src/ggnn/query/query_kernels.cu:55-110 */
ggnn_status ggnn_query_sizing(uint32_t D, uint32_t k_query, uint32_t max_iterations,
                              uint32_t* cache_size, uint32_t* sorted_size);
/* row layout of every distance kernel for rows of D elements of `dtype` (pure host, test entry):
 * *lanes_per_row lanes hold *chunks_per_lane 16-byte chunks each (pick_dist_config) */
ggnn_status ggnn_op_dist_layout(uint32_t D, ggnn_dtype dtype, uint32_t* lanes_per_row,
                                uint32_t* chunks_per_lane);

/* QueryKernels::query  query_kernels.cu:50-186 -> query_layer.cu:39-97 (one shard).
 * graph0 [N_base x KBuild], start [num_start] (= translation[L-1]), nn1_stats [2].
 * Writes ids/dists rows (n*shards_per_gpu + on_gpu_shard) of width k_query, ids offset by
 * on_gpu_shard*N_base.  n_dist/n_pop: optional per-query counters [Nq]. */
ggnn_status ggnn_op_query(const void* base, ggnn_dtype dtype, uint32_t N_base, uint32_t D,
                          const void* query, uint32_t Nq, const int32_t* graph0,
                          uint32_t KBuild, const int32_t* start, uint32_t num_start,
                          const float* nn1_stats, uint32_t k_query, float tau_query,
                          uint32_t max_iterations, ggnn_measure measure,
                          uint32_t shards_per_gpu, uint32_t on_gpu_shard, int32_t* ids,
                          float* dists, uint32_t* n_dist, uint32_t* n_pop, void* stream);

/* Pre-screen copy of a float32 base (no reference counterpart; an exact pruning aid of
 * query_layer.cu:69-77 / simple_knn_cache.cuh:268-286): every row is stored a second time as
 * 8-bit codes c with x^_d = o_d + s*c_d plus a bound e_max >= max_rows ||x - x^|| (cosine: of the
 * row normalised to unit length).  During a float32 query or merge a candidate whose lower
 * bound (||q^ - x^|| - e_q - e_max)^2 already reaches the criteria is dropped without reading
 * its float row -- exactly the candidates the reference evaluates and then discards -- so ids,
 * distances and counters do not change.  The copy is specific to the measure it was made for.
 * code_dim = prescreen_code_dim(D) (a power of two up to 64, multiples of 64 above: rows do not
 * straddle more memory lines than their length needs); codes [N_base x code_dim] bytes; params [param_floats] floats
 * ([0] s, [1] 1/s, [2] e_max, [3] ||o||, [4] usable (0 when the data holds non-finite values),
 * [5..6] internal, [7] measure, [8..] o_d); scratch [scratch_floats] floats.  D must be a
 * multiple of 4. */
ggnn_status ggnn_prescreen_sizes(uint32_t N_base, uint32_t D, ggnn_measure measure,
                                 uint32_t* code_dim, size_t* param_floats, size_t* scratch_floats);
ggnn_status ggnn_op_prescreen_encode(const float* base, uint32_t N_base, uint32_t D,
                                     ggnn_measure measure, uint8_t* codes, float* params,
                                     float* scratch, void* stream);
/* Validation probe: for query n and candidate cand[n*M+j], reject[n*M+j] = 1 iff the pre-screen
 * would drop the candidate at criteria crit[n*M+j]; s_out (optional) receives the coded squared
 * distance in code units.  A correct bound never rejects at a criteria above the float
 * distance of the pair. */
ggnn_status ggnn_op_prescreen_probe(const uint8_t* codes, const float* params, uint32_t D,
                                    ggnn_measure measure, const float* query, uint32_t Nq,
                                    const int32_t* cand, uint32_t M, const float* crit,
                                    int32_t* reject, float* s_out, void* stream);
/* ggnn_op_query for float32 with the pre-screen copy made for `measure` (params[4] must be 1).
 * n_rows: optional [Nq x 2], float rows and code rows read per query. */
ggnn_status ggnn_op_query_prescreened(const float* base, uint32_t N_base, uint32_t D,
                                      const uint8_t* codes, const float* params,
                                      const float* query, uint32_t Nq, const int32_t* graph0,
                                      uint32_t KBuild, const int32_t* start, uint32_t num_start,
                                      const float* nn1_stats, uint32_t k_query, float tau_query,
                                      uint32_t max_iterations, ggnn_measure measure,
                                      uint32_t shards_per_gpu, uint32_t on_gpu_shard, int32_t* ids,
                                      float* dists, uint32_t* n_dist, uint32_t* n_pop,
                                      uint32_t* n_rows, void* stream);

/* ggnn_op_query restricted to an allowed-id bitset (device memory): candidate key k of this
 * shard is allowed iff bit (k + filter_bit_offset) of filter_bits is set (filter_bit_offset: the
 * shard's first global id).  codes / params: the pre-screen copy of a float32 base, or both NULL
 * (no pre-screen).  n_rows: optional [Nq x 2]. */
ggnn_status ggnn_op_query_filtered(const void* base, ggnn_dtype dtype, uint32_t N_base, uint32_t D,
                                   const uint8_t* codes, const float* params, const void* query,
                                   uint32_t Nq, const int32_t* graph0, uint32_t KBuild,
                                   const int32_t* start, uint32_t num_start,
                                   const float* nn1_stats, uint32_t k_query, float tau_query,
                                   uint32_t max_iterations, ggnn_measure measure,
                                   uint32_t shards_per_gpu, uint32_t on_gpu_shard, int32_t* ids,
                                   float* dists, uint32_t* n_dist, uint32_t* n_pop,
                                   uint32_t* n_rows, const uint32_t* filter_bits,
                                   uint32_t filter_bit_offset, void* stream);
/* ggnn_op_bf_query among the allowed rows only; unfilled slots are (-1, +inf).  Large batches
 * (Nq >= 256, N_base >= 4096, k_query <= 112) run the filtered matrix-core tile kernels, checked
 * by the same exactness certificate as ggnn_op_bf_query; the scan kernels answer the rest:
 * smaller calls, uint8 rows under squared L2 with D <= 128 (the integer kernels have no filtered
 * form), a bitset or filter table whose filter_bit_offset is not a multiple of 32, and every call
 * under hook BF_SCAN = 1.  Results are bit-identical on either path. */
ggnn_status ggnn_op_bf_query_filtered(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                      uint32_t D, const void* query, uint32_t Nq,
                                      uint32_t k_query, ggnn_measure measure, int32_t* ids,
                                      float* dists, const uint32_t* filter_bits,
                                      uint32_t filter_bit_offset, void* stream);

/* The two calls above with a filter table and one filter id per query (all device memory):
 * filter_table is [num_filters x ceil(n_bits / 32)] words, n_bits >= filter_bit_offset + N_base;
 * query n searches under row filter_ids[n], -1 = unfiltered, any other id = empty result (the
 * constant rows those two read are made in scratch memory of the launch). */
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
                                      void* stream);
ggnn_status ggnn_op_bf_query_filtered_by(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                         uint32_t D, const void* query, uint32_t Nq,
                                         uint32_t k_query, ggnn_measure measure, int32_t* ids,
                                         float* dists, const uint32_t* filter_table,
                                         uint32_t num_filters, uint64_t n_bits,
                                         const int32_t* filter_ids, uint32_t filter_bit_offset,
                                         void* stream);
/* ggnn_op_query_filtered / ggnn_op_bf_query_filtered with a label column and one label per query
 * (all device memory): labels is int32 [n_labels], n_labels >= filter_bit_offset + N_base, local
 * id i has the label labels[i + filter_bit_offset]; query n may be given the rows whose label
 * equals query_labels[n], -1 = unfiltered. */
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
                                  void* stream);
ggnn_status ggnn_op_bf_query_labeled(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                     uint32_t D, const void* query, uint32_t Nq, uint32_t k_query,
                                     ggnn_measure measure, int32_t* ids, float* dists,
                                     const int32_t* labels, uint64_t n_labels,
                                     const int32_t* query_labels, uint32_t filter_bit_offset,
                                     void* stream);
/* Range search at the seam (all device memory, stream-ordered: a counting launch, a prefix launch and
 * a filling launch on `stream`, nothing waits for the host): ggnn_bf_range_query's semantics with
 * radii[Nq], lims[Nq + 1] (uint64) and ids / dists [capacity] in device memory.  lims is always
 * written; ids / dists only if lims[Nq] <= capacity (they may be null with capacity 0), rows in
 * ascending id whatever the number of slices.  A Euclidean radius is in SQUARED units.  A NaN radius
 * admits nothing here (the handle refuses it).  The filter arguments are those of
 * ggnn_op_bf_query_filtered / _filtered_by / _labeled; any filter_bit_offset (there is no matrix-core
 * path), 8-bit rows need D % 16 == 0, labels at most 2^30 rows. */
ggnn_status ggnn_op_bf_range_query(const void* base, ggnn_dtype dtype, uint32_t N_base, uint32_t D,
                                   const void* query, uint32_t Nq, const float* radii,
                                   ggnn_measure measure, uint64_t capacity, uint64_t* lims,
                                   int32_t* ids, float* dists, void* stream);
ggnn_status ggnn_op_bf_range_query_filtered(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                            uint32_t D, const void* query, uint32_t Nq,
                                            const float* radii, ggnn_measure measure,
                                            uint64_t capacity, uint64_t* lims, int32_t* ids,
                                            float* dists, const uint32_t* filter_bits,
                                            uint32_t filter_bit_offset, void* stream);
ggnn_status ggnn_op_bf_range_query_filtered_by(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                               uint32_t D, const void* query, uint32_t Nq,
                                               const float* radii, ggnn_measure measure,
                                               uint64_t capacity, uint64_t* lims, int32_t* ids,
                                               float* dists, const uint32_t* filter_table,
                                               uint32_t num_filters, uint64_t n_bits,
                                               const int32_t* filter_ids,
                                               uint32_t filter_bit_offset, void* stream);
ggnn_status ggnn_op_bf_range_query_labeled(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                           uint32_t D, const void* query, uint32_t Nq,
                                           const float* radii, ggnn_measure measure,
                                           uint64_t capacity, uint64_t* lims, int32_t* ids,
                                           float* dists, const int32_t* labels, uint64_t n_labels,
                                           const int32_t* query_labels, uint32_t filter_bit_offset,
                                           void* stream);
/* ggnn_op_bf_query_labeled through a label index (ggnn_label_index_build of the column, copied to
 * the device: keys[n_keys], offsets[n_keys + 1], rows[N_base]): every query reads only the rows of its
 * label.  Every output bit equals what ggnn_op_bf_query_labeled gives for the same base, labels and
 * query labels (ids, distance bits, unfilled slots); label -1 scans the whole base, a label that is no
 * key gives an empty row.  Every element type, both measures, k_query <= 6000; always scan kernels.
 * Hook LABEL_INDEX_SLICES forces the number of slices a label's rows are cut into. */
ggnn_status ggnn_op_bf_query_label_index(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                         uint32_t D, const void* query, uint32_t Nq,
                                         uint32_t k_query, ggnn_measure measure,
                                         const int32_t* keys, uint32_t n_keys,
                                         const uint32_t* offsets, const int32_t* rows,
                                         const int32_t* query_labels, int32_t* ids, float* dists,
                                         void* stream);
/* Which queries a label index of cutoff `cutoff` answers (all device memory): routed_list[Nq] gets
 * the queries n with query_labels[n] != -1 whose label has at most `cutoff` rows (a label that is no
 * key has 0), rest_list[Nq] the others, both in ascending order of n; counts[0] and counts[1] their
 * lengths.  The same input gives the same lists. */
ggnn_status ggnn_op_label_index_classify(const int32_t* keys, uint32_t n_keys,
                                         const uint32_t* offsets, const int32_t* query_labels,
                                         uint32_t Nq, uint32_t cutoff, uint32_t* routed_list,
                                         uint32_t* rest_list, uint32_t* counts, void* stream);
/* Label sets and label ranges through a label index: three operators (all device memory).
 *
 * rows[] of the index is sorted by (label, id), so the rows of one label -- and of one closed label
 * interval -- are one contiguous run of positions.  ggnn_op_label_spans_resolve turns every query's
 * label set or label ranges into at most eight such runs:
 *   mode 0  sel is int32 [Nq x n_sel], 1 <= n_sel <= GGNN_MAX_LABEL_SET, the label sets of
 *           ggnn_op_bf_query_labeled_in: an entry that is a key gives that key's rows, an entry that is
 *           no key nothing, an entry -1 the whole index; entries may repeat
 *   mode 1  sel is int32 [Nq x n_sel x 2], 1 <= n_sel <= GGNN_MAX_LABEL_RANGES, the closed signed
 *           intervals (lo, hi) of ggnn_op_bf_query_labeled_range: the rows of every key in [lo, hi];
 *           lo > hi and an interval without a key give nothing; there is no wildcard
 * spans is uint32 [Nq x 8 x 2], (begin, end) positions into rows[], in normal form: sorted by begin,
 * overlapping and touching spans merged (pairwise disjoint, never end == next begin), none empty,
 * unused slots (0, 0) at the tail -- the same input always gives the same words, and no row is
 * reachable twice whatever repeats or overlaps in sel.  totals[Nq] is the sum of a query's span
 * lengths: the number of rows the query will read.
 *
 * ggnn_op_bf_query_label_spans is the exact K nearest of every query among the rows at the positions
 * of its spans, and -- with filter_ids -- whose bit of the query's row of filter_table is set, under
 * the rules of ggnn_op_bf_query_labeled_in with filter_bit_offset 0: id -1 admits every row, f in
 * [0, num_filters) tests bit `row id` of row f, any other id gives an empty result without reading a
 * base row; filter_ids == NULL: spans only (the table is then not read); filter_table may be NULL
 * with num_filters == 0, and n_bits >= N_base when there is one (GGNN_INVALID_ARGUMENT otherwise).
 * The K-best list is ordered by the pair (distance, id): positions ascend with the id inside one
 * label only, and the K smallest pairs are what the scan of the whole base in ascending id with its
 * stable insert keeps.  Every output bit therefore equals ggnn_op_bf_query_labeled_in /
 * ggnn_op_bf_query_labeled_range on the same column, sets / ranges and table (ids, distance bits,
 * unfilled slots (-1, +inf)).  Every element type -- for int8 rows, which those two refuse, this is
 * the only way to search by a label set or a label range --, both measures, 1 <= k_query <= 6000
 * (GGNN_INVALID_ARGUMENT), N_base <= 2^30 (GGNN_UNSUPPORTED); always scan kernels.  A denied row costs
 * its id and its bitset word, not a base row.  span_limit: the cutoff the caller classified with, or
 * 0 for "unknown": it only sizes the slices a query's positions are cut into when the batch is small
 * (hook LABEL_INDEX_SLICES forces the count); a query with more rows is still answered in full.
 * Label masks have no such form: tag bits are not a sort key.
 *
 * ggnn_op_label_spans_classify is ggnn_op_label_index_classify by totals: routed iff totals[n] <=
 * cutoff (a wildcard set has total N_base, so it is routed only when cutoff >= N_base).  Nq == 0
 * launches nothing in all three (classify then zeroes counts). */
ggnn_status ggnn_op_label_spans_resolve(const int32_t* keys, uint32_t n_keys,
                                        const uint32_t* offsets, int mode, const int32_t* sel,
                                        uint32_t n_sel, uint32_t Nq, uint32_t* spans,
                                        uint32_t* totals, void* stream);
ggnn_status ggnn_op_bf_query_label_spans(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                         uint32_t D, const void* query, uint32_t Nq,
                                         uint32_t k_query, ggnn_measure measure,
                                         const int32_t* rows, const uint32_t* spans,
                                         uint32_t span_limit, const uint32_t* filter_table,
                                         uint32_t num_filters, uint64_t n_bits,
                                         const int32_t* filter_ids, int32_t* ids, float* dists,
                                         void* stream);
ggnn_status ggnn_op_label_spans_classify(const uint32_t* totals, uint32_t Nq, uint32_t cutoff,
                                         uint32_t* routed_list, uint32_t* rest_list,
                                         uint32_t* counts, void* stream);
/* ggnn_op_query_labeled / ggnn_op_bf_query_labeled with a label SET per query and an optional
 * filter table (all device memory): query_label_sets is int32 [Nq x set_width], 1 <= set_width <=
 * GGNN_MAX_LABEL_SET; local id i may be given to query n iff labels[i + filter_bit_offset] equals
 * one of the set's entries (or one of them is -1) AND filter_ids[n] admits it -- -1: every id, f in
 * [0, num_filters): bit i + filter_bit_offset of row f, anything else: none.  filter_ids may be
 * NULL (labels only) and so may filter_table with num_filters == 0 (then an id is -1 or admits
 * nothing); n_bits >= filter_bit_offset + N_base when there is a table.  No int8 rows
 * (GGNN_UNSUPPORTED); ggnn_op_bf_query_labeled_in always runs the scan kernels. */
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
                                     uint32_t filter_bit_offset, void* stream);
ggnn_status ggnn_op_bf_query_labeled_in(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                        uint32_t D, const void* query, uint32_t Nq,
                                        uint32_t k_query, ggnn_measure measure, int32_t* ids,
                                        float* dists, const int32_t* labels, uint64_t n_labels,
                                        const int32_t* query_label_sets, uint32_t set_width,
                                        const uint32_t* filter_table, uint32_t num_filters,
                                        uint64_t n_bits, const int32_t* filter_ids,
                                        uint32_t filter_bit_offset, void* stream);
/* ggnn_op_query_labeled_in / ggnn_op_bf_query_labeled_in with label RANGES in place of label sets:
 * query_label_ranges is int32 [Nq x n_ranges x 2], (lo, hi) pairs, 1 <= n_ranges <=
 * GGNN_MAX_LABEL_RANGES; local id i may be given to query n iff lo <= labels[i + filter_bit_offset]
 * <= hi (signed) for one of its pairs AND filter_ids[n] admits it, as above.  lo > hi is an empty
 * interval and there is no wildcard value (see ggnn_query_labeled_range).  No int8 rows
 * (GGNN_UNSUPPORTED); ggnn_op_bf_query_labeled_range always runs the scan kernels. */
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
                                        void* stream);
ggnn_status ggnn_op_bf_query_labeled_range(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                           uint32_t D, const void* query, uint32_t Nq,
                                           uint32_t k_query, ggnn_measure measure, int32_t* ids,
                                           float* dists, const int32_t* labels, uint64_t n_labels,
                                           const int32_t* query_label_ranges, uint32_t n_ranges,
                                           const uint32_t* filter_table, uint32_t num_filters,
                                           uint64_t n_bits, const int32_t* filter_ids,
                                           uint32_t filter_bit_offset, void* stream);
/* ggnn_op_query_labeled_range / ggnn_op_bf_query_labeled_range with label MASKS in place of label
 * ranges: query_label_masks is int32 [Nq x n_masks x 3], (mask, value, any) triples, 1 <= n_masks <=
 * GGNN_MAX_LABEL_MASKS; local id i may be given to query n iff L = labels[i + filter_bit_offset] has
 * (L & mask) == value and (any == 0 or (L & any) != 0) for one of its triples AND filter_ids[n] admits
 * it, as above.  value is never pre-masked and there is no wildcard value (see
 * ggnn_query_labeled_mask).  No int8 rows (GGNN_UNSUPPORTED); ggnn_op_bf_query_labeled_mask always
 * runs the scan kernels. */
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
                                       void* stream);
ggnn_status ggnn_op_bf_query_labeled_mask(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                          uint32_t D, const void* query, uint32_t Nq,
                                          uint32_t k_query, ggnn_measure measure, int32_t* ids,
                                          float* dists, const int32_t* labels, uint64_t n_labels,
                                          const int32_t* query_label_masks, uint32_t n_masks,
                                          const uint32_t* filter_table, uint32_t num_filters,
                                          uint64_t n_bits, const int32_t* filter_ids,
                                          uint32_t filter_bit_offset, void* stream);
/* ggnn_op_bf_query_filtered, _filtered_by and _labeled, reporting how they ran (modelled on
 * ggnn_op_bf_query_certified): *n_rescanned (DEVICE memory, may be NULL) receives the number of
 * queries the matrix-core pre-selection could not certify and the filtered scan answered instead;
 * *matrix_path (HOST memory, may be NULL) is set before the call returns to 1 if the launch ran
 * the tile kernels and to 0 if it ran the scan. */
ggnn_status ggnn_op_bf_query_filtered_certified(const void* base, ggnn_dtype dtype,
                                                uint32_t N_base, uint32_t D, const void* query,
                                                uint32_t Nq, uint32_t k_query,
                                                ggnn_measure measure, int32_t* ids, float* dists,
                                                const uint32_t* filter_bits,
                                                uint32_t filter_bit_offset, uint32_t* n_rescanned,
                                                int* matrix_path, void* stream);
ggnn_status ggnn_op_bf_query_filtered_by_certified(
    const void* base, ggnn_dtype dtype, uint32_t N_base, uint32_t D, const void* query, uint32_t Nq,
    uint32_t k_query, ggnn_measure measure, int32_t* ids, float* dists,
    const uint32_t* filter_table, uint32_t num_filters, uint64_t n_bits, const int32_t* filter_ids,
    uint32_t filter_bit_offset, uint32_t* n_rescanned, int* matrix_path, void* stream);
ggnn_status ggnn_op_bf_query_labeled_certified(const void* base, ggnn_dtype dtype,
                                               uint32_t N_base, uint32_t D, const void* query,
                                               uint32_t Nq, uint32_t k_query, ggnn_measure measure,
                                               int32_t* ids, float* dists, const int32_t* labels,
                                               uint64_t n_labels, const int32_t* query_labels,
                                               uint32_t filter_bit_offset, uint32_t* n_rescanned,
                                               int* matrix_path, void* stream);
/* [num_filters x N] byte masks (non-zero: allowed) -> [num_filters x ceil(N / 32)] bitset words,
 * padding bits zero; both in device memory.  A table made from a label column on the GPU needs
 * no host round trip. */
ggnn_status ggnn_op_pack_filters(const uint8_t* masks, uint32_t num_filters, uint64_t N,
                                 uint32_t* words, void* stream);

/* QueryKernels::bruteForceQuery  query_kernels.cu:188-264 -> bf_query_layer.cu:39-65 */
ggnn_status ggnn_op_bf_query(const void* base, ggnn_dtype dtype, uint32_t N_base, uint32_t D,
                             const void* query, uint32_t Nq, uint32_t k_query,
                             ggnn_measure measure, int32_t* ids, float* dists, void* stream);
/* same, and *n_rescanned (device memory, may be NULL) receives the number of queries whose
 * matrix-core pre-selection could not be certified exact and which were therefore answered by the
 * exhaustive scan kernel (0 on paths that scan anyway).  The answers are exact either way. */
ggnn_status ggnn_op_bf_query_certified(const void* base, ggnn_dtype dtype, uint32_t N_base,
                                       uint32_t D, const void* query, uint32_t Nq,
                                       uint32_t k_query, ggnn_measure measure, int32_t* ids,
                                       float* dists, uint32_t* n_rescanned, void* stream);

/* top  graph_construction.cu:201-237 -> top_merge_layer.cu:40-82.  graph_layer/translation are
 * the views of `layer` (translation NULL on layer 0). */
ggnn_status ggnn_op_top(const void* base, ggnn_dtype dtype, uint32_t D, ggnn_measure measure,
                        uint32_t KBuild, const int32_t* translation_layer, uint32_t N_layer,
                        uint32_t S, uint32_t S_offset, uint32_t layer, int32_t* graph_layer,
                        float* nn1_dist_buffer, void* stream);

/* mergeLayer  graph_construction.cu:239-296 -> merge_layer.cu:63-158 (without the final D2D
 * copy).  graph_all [N_all x K], translation_all/selection_all [ST_all] (views "starting at
 * layer 1", i.e. indexed with STs_offsets), writes graph_buffer [Ns[btm] x K]. */
ggnn_status ggnn_op_merge(const void* base, ggnn_dtype dtype, ggnn_measure measure,
                          const ggnn_graph_config* cfg, const int32_t* graph_all,
                          const int32_t* translation_all, const int32_t* selection_all,
                          const float* nn1_stats, float tau_build, uint32_t layer_top,
                          uint32_t layer_btm, int32_t* graph_buffer, float* nn1_dist_buffer,
                          uint32_t* n_dist, void* stream);
/* ggnn_op_merge for float32 with the pre-screen copy of the base made for `measure`
 * (ggnn_op_prescreen_encode, params[4] must be 1); same outputs. */
ggnn_status ggnn_op_merge_prescreened(const float* base, const uint8_t* codes, const float* params,
                                      ggnn_measure measure, const ggnn_graph_config* cfg,
                                      const int32_t* graph_all,
                                      const int32_t* translation_all,
                                      const int32_t* selection_all, const float* nn1_stats,
                                      float tau_build, uint32_t layer_top, uint32_t layer_btm,
                                      int32_t* graph_buffer, float* nn1_dist_buffer,
                                      uint32_t* n_dist, void* stream);

/* select  graph_construction.cu:163-187 -> wrs_select_layer.cu:41-102.  rng [Ns[layer]] uniform
 * (0,1] numbers (the reference draws them with cuRAND XORWOW; injected here). */
ggnn_status ggnn_op_select(const ggnn_graph_config* cfg, uint32_t layer,
                           const float* nn1_dist_buffer, const float* rng,
                           int32_t* translation_all, int32_t* selection_all, void* stream);
/* uniform (0,1] generator used by ggnn_build in place of curandGenerateUniform
 * (graph_construction.cu:96-102,168-169); counter based, seed 1234 by default. */
ggnn_status ggnn_op_uniform(float* out, uint32_t n, uint64_t seed, uint64_t stream_id,
                            void* stream);

/* sym  graph_construction.cu:298-379 -> sym_query_layer.cu:39-145 (blocks first_n ..
 * first_n+count-1; sym_buffer/sym_atomic must have been cleared by the caller) */
ggnn_status ggnn_op_sym(const void* base, ggnn_dtype dtype, ggnn_measure measure, uint32_t D,
                        uint32_t KBuild, const int32_t* graph_layer,
                        const int32_t* translation_layer, uint32_t N_layer,
                        const float* nn1_stats, float tau_build, int32_t* sym_buffer,
                        uint32_t* sym_atomic, uint32_t first_n, uint32_t count, void* stream);
/* ggnn_op_sym for float32 with the pre-screen copy of the base made for `measure`
 * (ggnn_op_prescreen_encode, params[4] must be 1); same outputs. */
ggnn_status ggnn_op_sym_prescreened(const float* base, const uint8_t* codes, const float* params,
                                    ggnn_measure measure, uint32_t D, uint32_t KBuild,
                                    const int32_t* graph_layer, const int32_t* translation_layer,
                                    uint32_t N_layer, const float* nn1_stats, float tau_build,
                                    int32_t* sym_buffer, uint32_t* sym_atomic, uint32_t first_n,
                                    uint32_t count, void* stream);

/* The two steps of the deterministic sym schedule (ggnn_set_build_hooks, serial_sym = 2; no
 * reference counterpart), for tests.
 * Request pass: ggnn_op_sym / ggnn_op_sym_prescreened (codes and params non-null: float32 with
 * the pre-screen, dtype must be GGNN_F32) with `requests` [N_layer x (KBuild - KBuild / 2) x
 * KBuild / 2]: the searches treat the pending inverse links as empty and neither read nor write
 * sym_buffer / sym_atomic (which may be null); per point and local neighbour the row is -1
 * everywhere if the search met the point, else its best list, nearest first, -1 from the first
 * unused entry on. */
ggnn_status ggnn_op_sym_requests(const void* base, ggnn_dtype dtype, const uint8_t* codes,
                                 const float* params, ggnn_measure measure, uint32_t D,
                                 uint32_t KBuild, const int32_t* graph_layer,
                                 const int32_t* translation_layer, uint32_t N_layer,
                                 const float* nn1_stats, float tau_build, int32_t* sym_buffer,
                                 uint32_t* sym_atomic, int32_t* requests, uint32_t first_n,
                                 uint32_t count, void* stream);
/* Assign step (one wave; a whole pass starts from sym_atomic = 0, sym_buffer = -1): the request
 * rows in ascending (point n, local neighbour) order; the candidates c of a row up to the first
 * -1 or id >= N_layer: if n is among sym_buffer[c][0 .. min(sym_atomic[c], KF)) the row is done;
 * else pos = sym_atomic[c]++, and pos < KF stores n at sym_buffer[c][pos] and ends the row. */
ggnn_status ggnn_op_sym_assign(uint32_t KBuild, uint32_t N_layer, const int32_t* requests,
                               uint32_t* sym_atomic, int32_t* sym_buffer, void* stream);

/* sym_buffer_merge  sym_buffer_merge_layer.cu:36-99 (sym_buffer is used as scratch) */
ggnn_status ggnn_op_sym_buffer_merge(uint32_t KBuild, uint32_t N_layer, int32_t* sym_buffer,
                                     const uint32_t* sym_atomic, int32_t* graph_layer,
                                     void* stream);
/* computeNN1Stats + divide  graph_construction.cu:381-393,79-83 ; out = {mean, max};
 * scratch: >= ggnn_nn1_stats_scratch_floats() floats of device memory */
size_t ggnn_nn1_stats_scratch_floats(void);
ggnn_status ggnn_op_nn1_stats(const float* nn1_dist_buffer, uint32_t N, float* scratch,
                              float* out, void* stream);

/* GPUInstance::sortQueryResults  gpu_instance.cu:745-790: stable ascending sort of every
 * [row_len] row by distance (in place). */
ggnn_status ggnn_op_sort_shard_results(uint32_t Nq, uint32_t row_len, int32_t* ids, float* dists,
                                       void* stream);
/* ResultMerger::merge  result_merger.cpp:51-149 on the device: `parts` = num_parts consecutive
 * [Nq x stride] blocks (e.g. the RCCL all-gather buffer), each row sorted ascending; writes the
 * k best per query with id + part*id_offset_per_part.  Ties: lower part first. */
ggnn_status ggnn_op_merge_results(uint32_t Nq, uint32_t k, uint32_t num_parts, uint32_t stride,
                                  uint32_t id_offset_per_part, const int32_t* parts_ids,
                                  const float* parts_dists, int32_t* ids_out, float* dists_out,
                                  void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GGNN_C_H */
