// Shared host/device definitions of the MI355X GGNN engine (libggnn_amd.so).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>

#include "../../include/ggnn_c.h"

namespace ggnn_amd {

constexpr int kWave = 64;
constexpr int32_t kEmptyKey = -1;
constexpr uint32_t kLayers = 4;  // reference: graph_config.h:42-44
constexpr uint32_t kKBlock = 32; // reference: K_BLOCK in query_layer.cu:42, merge_layer.cu:67

struct Error : std::runtime_error {
  ggnn_status status;
  Error(ggnn_status s, const std::string& msg) : std::runtime_error(msg), status(s) {}
};

#define GGNN_HIP_CHECK(expr)                                                                  \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      throw ::ggnn_amd::Error(_e == hipErrorOutOfMemory ? GGNN_OUT_OF_MEMORY                  \
                                                        : GGNN_DEVICE_ERROR,                  \
                              std::string(#expr) + ": " + hipGetErrorString(_e));            \
  } while (0)

#define GGNN_REQUIRE(cond, status, msg)        \
  do {                                         \
    if (!(cond))                               \
      throw ::ggnn_amd::Error((status), (msg)); \
  } while (0)

// bytes per element of a base / query row (every dtype the C-ABI accepts)
inline size_t dtype_size(ggnn_dtype t)
{
  switch (t) {
    case GGNN_F32: return 4;
    case GGNN_U8:
    case GGNN_I8: return 1;
    case GGNN_F16:
    case GGNN_BF16: return 2;
  }
  throw Error(GGNN_INVALID_ARGUMENT, "unknown dtype");
}
// elements per 16-byte chunk: the unit of every row load and of the row padding
inline uint32_t dtype_elems_per_chunk(ggnn_dtype t)
{
  return 16u / static_cast<uint32_t>(dtype_size(t));
}
inline bool dtype_is_16bit(ggnn_dtype t)
{
  return t == GGNN_F16 || t == GGNN_BF16;
}

// include/ggnn/base/def.h:37-62 of the reference (host helpers, restated)
inline uint32_t bit_ceil_u32(uint32_t v)
{
  if (v <= 1)
    return 1;
  --v;
  v |= v >> 1;
  v |= v >> 2;
  v |= v >> 4;
  v |= v >> 8;
  v |= v >> 16;
  return v + 1;
}
inline uint32_t next_multiple32(uint32_t v)
{
  return (v + 31u) / 32u * 32u;
}
inline size_t align8(size_t s)
{
  return (s + 7) / 8 * 8;
}

// The AQL dispatch packet stores the grid size per dimension in WORK-ITEMS as 32 bits, so a 1-D
// launch of more than 2^32 / block_threads workgroups is silently truncated (one wave per point
// breaks beyond 2^26 points).  Large launches therefore use a 2-D grid; kernels recover the
// linear workgroup index with block_linear_index() and guard against the rounded-up tail.
constexpr uint32_t kMaxGridX = 1u << 20;
inline dim3 grid_for(uint64_t blocks)
{
  if (blocks <= kMaxGridX)
    return dim3(static_cast<uint32_t>(blocks ? blocks : 1));
  return dim3(kMaxGridX, static_cast<uint32_t>((blocks + kMaxGridX - 1) / kMaxGridX));
}
#if defined(__HIPCC__)
__device__ __forceinline__ uint32_t block_linear_index()
{
  return blockIdx.y * gridDim.x + blockIdx.x;
}
// XCD-aware block -> item mapping for kernels whose consecutive items share data (the construction
// kernels: consecutive points share their neighbourhoods).  Workgroup b runs on XCD b % 8 (observed,
// MI355X_MICROARCH.md; only speed depends on it) and every XCD has its own L2: with the identity
// mapping each XCD works on every 8th point and all eight L2s fetch the same rows.  Here XCD x gets
// the CONTIGUOUS items [x * per, (x + 1) * per), per = ceil(n / 8); launch xcd_grid_blocks(n)
// workgroups and drop the indices >= n.
__device__ __forceinline__ uint32_t xcd_contiguous_index(uint32_t b, uint32_t n, bool enabled)
{
  if (!enabled)
    return b;
  const uint32_t per = (n + 7u) >> 3;
  const uint32_t i = b >> 3;
  return i < per ? (b & 7u) * per + i : 0xffffffffu;
}
#endif
inline uint64_t xcd_grid_blocks(uint64_t n, bool enabled)
{
  return enabled ? ((n + 7) / 8) * 8 : n;
}

extern int g_log_level;
#define GGNN_LOG(level, ...)                 \
  do {                                       \
    if (::ggnn_amd::g_log_level >= (level)) { \
      std::fprintf(stderr, "[ggnn_amd] ");   \
      std::fprintf(stderr, __VA_ARGS__);     \
      std::fprintf(stderr, "\n");            \
    }                                        \
  } while (0)

// ---- host-side launchers implemented in the .hip files ---------------------------------------
// Per-query filters: filter_bits of a launch is a table of [num_filters x words] bitsets and
// query n searches under row ids[n] (-1: unfiltered, any other value outside [0, num_filters): empty
// result).  ids == nullptr is the per-call form: filter_bits is ONE bitset shared by every query.
// consts: [2 x words] device words, all ones then all zeros -- what the ids -1 / out of range read;
// when it is null the launcher makes the two rows in stream-ordered scratch of the launch.
//
// Label filters: query_labels != nullptr (ids is then null).  filter_bits of the launch is the
// label column, one int32 per global base id, and query n with label L = query_labels[n] may be
// given a base vector iff that vector's label equals L; L == -1 searches unfiltered.  No label
// value is invalid and none addresses memory: the labels are compared, never used as an index.
struct FilterTable {
  const int32_t* ids{nullptr};      // [Nq] (device) or null
  const uint32_t* consts{nullptr};  // [2 x words]
  uint32_t words{0};                // words per filter: ceil(bits / 32) over the global ids
  uint32_t num_filters{0};
  const int32_t* query_labels{nullptr};  // [Nq] (device) or null
};
// Label sets (with a label column): query n carries width <= 8 labels, sets[n * width + j], and a
// base vector may be given to it iff its label equals one of them; an entry -1 admits every label,
// entries may repeat.  A launch with labels != nullptr is a label-set launch: filter_bits is then the
// filter table or null, filter_table.ids the filter id per query or null (both null: labels only),
// and a vector must ALSO have its bit set in the query's row -- id -1 admits every vector, an id
// outside [0, num_filters) none.  filter_table.consts and query_labels are not used; filter_bit_offset
// is the shard's first global id in the column and in the table alike.
struct LabelSetSpec {
  const int32_t* labels{nullptr};  // [>= offset + N_base] (device)
  const int32_t* sets{nullptr};    // [Nq x width] (device)
  uint32_t width{0};               // 1 .. 8 (GGNN_MAX_LABEL_SET)
};
// Label ranges (with a label column): query n carries n_ranges <= 4 closed intervals of signed int32
// labels, (ranges[(n * n_ranges + j) * 2], ranges[(n * n_ranges + j) * 2 + 1]) = (lo, hi), and a base
// vector may be given to it iff lo <= its label <= hi for at least one of them.  lo > hi is an empty
// interval; there is no wildcard value (-1 is an ordinary label); every int32 value is a valid bound.
// A launch with labels != nullptr is a label-range launch; filter_bits, filter_table.ids and
// filter_bit_offset are what they are under LabelSetSpec.
struct LabelRangeSpec {
  const int32_t* labels{nullptr};  // [>= offset + N_base] (device)
  const int32_t* ranges{nullptr};  // [Nq x n_ranges x 2] (device)
  uint32_t n_ranges{0};            // 1 .. 4 (GGNN_MAX_LABEL_RANGES)
};
// Label masks (with a label column read as 32 tag bits): query n carries n_masks <= 2 clauses of
// three int32 words, masks[(n * n_masks + j) * 3 + 0 .. 2] = (mask, value, any), and a base vector may
// be given to it iff, for at least one clause, (label & mask) == value AND (any == 0 OR (label & any)
// != 0).  (0, 0, 0) admits every row; a value with a bit outside its mask admits none (value is never
// pre-masked); there is no wildcard value and no invalid clause.  A launch with labels != nullptr is
// a label-mask launch; filter_bits, filter_table.ids and filter_bit_offset are what they are under
// LabelSetSpec.
struct LabelMaskSpec {
  const int32_t* labels{nullptr};  // [>= offset + N_base] (device)
  const int32_t* masks{nullptr};   // [Nq x n_masks x 3] (device)
  uint32_t n_masks{0};             // 1 .. 2 (GGNN_MAX_LABEL_MASKS)
};
// the two constant rows for a launch that was given none (null if ids is null); free with
// scratch_free(p, stream) after the launch
uint32_t* filter_consts_scratch(const FilterTable& t, hipStream_t stream);

struct QueryLaunch {
  const void* base;
  const void* query;
  ggnn_dtype dtype;
  uint32_t N_base, D, Nq;
  const int32_t* graph0;
  uint32_t KBuild;
  const int32_t* start;
  uint32_t num_start;
  const float* nn1_stats;
  uint32_t k_query;
  float tau_query;
  uint32_t max_iterations;
  ggnn_measure measure;
  uint32_t shards_per_gpu, on_gpu_shard;
  int32_t* ids;
  float* dists;
  uint32_t* n_dist;
  uint32_t* n_pop;
  // optional pre-screen copy of the base (launch_prescreen_encode, same measure); ignored unless float32
  const uint8_t* ps_codes{nullptr};
  const float* ps_params{nullptr};
  uint32_t ps_Dc{0};
  // the caller knows that params[5] of this copy is set (lossless on a power-of-two grid, squared
  // L2): the launch may take the kernels that read exact distances from the codes (traversal.hpp)
  bool ps_lossless{false};
  uint32_t* n_rows{nullptr};  // optional [Nq x 2]: float rows and code rows read per query
  // optional allowed-id bitset (device; bit (id + filter_bit_offset) of the uint32 words): the
  // search reports allowed ids only (query_filtered.hip)
  const uint32_t* filter_bits{nullptr};
  uint32_t filter_bit_offset{0};
  // per-query filters: filter_bits is then a table (see FilterTable)
  FilterTable filter_table{};
  // label-set filters (labels != nullptr: see LabelSetSpec)
  LabelSetSpec label_sets{};
  // label-range filters (labels != nullptr: see LabelRangeSpec)
  LabelRangeSpec label_ranges{};
  // label-mask filters (labels != nullptr: see LabelMaskSpec)
  LabelMaskSpec label_masks{};
};
void launch_query(const QueryLaunch& a, hipStream_t stream);

// 8-bit pre-screen copy of a float32 base for one distance measure (prescreen.hip): codes
// [N x Dc], Dc = D rounded up to 16; params [prescreen_param_floats(D)] floats; scratch
// [prescreen_scratch_floats(N, D, measure)] floats.
constexpr int kPsHeaderFloats = 8;
// Code-row length: rows must not straddle more memory lines than their length needs -- a
// 96-byte code row at a 96-byte pitch touches 2.5 64-byte granules on average instead of 2 and a
// 128-byte line boundary three times in four (profiles/r03_d96: 1.40x the algorithmic bytes on the
// fabric).  Up to 64 dimensions the pitch is a power of two (several rows per line, none split),
// above that a multiple of 64 bytes; padding codes are zero on both sides of every difference.
inline uint32_t prescreen_code_dim(uint32_t D)
{
  if (D <= 64) {
    uint32_t p = 16;
    while (p < D)
      p <<= 1;
    return p;
  }
  return (D + 63u) / 64u * 64u;
}
size_t prescreen_param_floats(uint32_t D);
size_t prescreen_scratch_floats(uint32_t N, uint32_t D, ggnn_measure measure);
void launch_prescreen_encode(const float* base, uint32_t N, uint32_t D, ggnn_measure measure,
                             uint8_t* codes, float* params, float* scratch, hipStream_t stream);
void launch_prescreen_probe(const uint8_t* codes, const float* params, uint32_t D,
                            ggnn_measure measure, const float* query, uint32_t Nq,
                            const int32_t* cand, uint32_t M, const float* crit, int32_t* reject,
                            float* s_out, hipStream_t stream);

struct BfLaunch {
  const void* base;
  const void* query;
  ggnn_dtype dtype;
  uint32_t N_base, D, Nq, k_query;
  ggnn_measure measure;
  int32_t* ids;
  float* dists;
  // optional (device): number of queries the matrix-core path could not certify and answered
  // with the scan kernel instead (0 on the scan path)
  uint32_t* n_rescanned{nullptr};
  // optional allowed-id bitset (device; bit (row + filter_bit_offset)): the exact K nearest among
  // the allowed rows (bf_query.hip: launch_bf_query says which filtered calls run the tile kernels)
  const uint32_t* filter_bits{nullptr};
  uint32_t filter_bit_offset{0};
  // per-query filters: filter_bits is then a table (see FilterTable)
  FilterTable filter_table{};
  // optional (HOST): 1 if the launch ran the tile kernels of bf_mfma.hip, 0 if it ran the scan --
  // decided on the host before anything is enqueued; results are bit-identical either way
  int* matrix_path{nullptr};
  // label-set filters (labels != nullptr: see LabelSetSpec); always the scan
  LabelSetSpec label_sets{};
  // label-range filters (labels != nullptr: see LabelRangeSpec); always the scan
  LabelRangeSpec label_ranges{};
  // label-mask filters (labels != nullptr: see LabelMaskSpec); always the scan
  LabelMaskSpec label_masks{};
};
void launch_bf_query(const BfLaunch& a, hipStream_t stream);

// Exact range search (bf_range.hip): every base row i that the filter admits and whose distance to
// query n -- the float32 value launch_bf_query's scan kernel reports for the pair: squared L2 or
// |1 - cos| -- is <= radii[n].  CSR result: lims[Nq + 1] (lims[0] = 0, lims[Nq] the total), and the
// rows of query n at ids / dists [lims[n], lims[n + 1]) in ascending id.  lims is always written; ids /
// dists only if the total fits `capacity` entries (they may be null with capacity 0: count only).
// A NaN radius and a negative one admit nothing.  All device memory, nothing waits for the host.
// Filters: none, a bitset (filter_bits), a filter table (filter_table.ids) or one label per query
// (filter_table.query_labels) -- BfLaunch's rules.
struct BfRangeLaunch {
  const void* base;
  const void* query;
  ggnn_dtype dtype;
  uint32_t N_base, D, Nq;
  ggnn_measure measure;
  const float* radii;  // [Nq]
  uint64_t capacity;
  uint64_t* lims;  // [Nq + 1]
  int32_t* ids;    // [capacity] or null
  float* dists;    // [capacity] or null
  const uint32_t* filter_bits{nullptr};
  uint32_t filter_bit_offset{0};
  FilterTable filter_table{};
};
void launch_bf_range_query(const BfRangeLaunch& a, hipStream_t stream);

// Label index (label_index.hip): the label column in CSR form over the global base ids -- keys[n_keys]
// the distinct labels ascending, offsets[n_keys + 1] uint32 positions (offsets[0] = 0, offsets[n_keys]
// = N), rows[N] the base ids sorted by (label, id).  label_index_build is a host function (n in
// [1, 2^30]; keys / rows of n entries, offsets of n + 1).
void label_index_build(const int32_t* labels, uint64_t n, int32_t* keys, uint32_t* offsets,
                       int32_t* rows, uint32_t* n_keys);
// The exact K nearest of every query among the rows of its label, read through the index: bit for bit
// launch_bf_query under the same label column and query labels (label -1: every row; a label that is
// no key: an empty result).
struct LabelIndexLaunch {
  const void* base;
  const void* query;
  ggnn_dtype dtype;
  uint32_t N_base, D, Nq, k_query;
  ggnn_measure measure;
  int32_t* ids;  // [Nq x k_query]
  float* dists;
  const int32_t* keys;
  uint32_t n_keys;
  const uint32_t* offsets;
  const int32_t* rows;
  const int32_t* query_labels;  // [Nq]
};
void launch_label_index_scan(const LabelIndexLaunch& a, hipStream_t stream);
// routed_list / rest_list [Nq]: the queries with label != -1 and at most `cutoff` rows under their label
// (a label that is no key: 0 rows), and the others, both in ascending query order; counts[0 .. 1] their
// lengths.  Deterministic.
void launch_label_index_classify(const int32_t* keys, uint32_t n_keys, const uint32_t* offsets,
                                 const int32_t* query_labels, uint32_t Nq, uint32_t cutoff,
                                 uint32_t* routed_list, uint32_t* rest_list, uint32_t* counts,
                                 hipStream_t stream);

// Label spans (label_spans.hip): a label set or up to four label ranges of a query as at most eight
// spans [begin, end) of positions into rows[] of a label index, in normal form -- sorted by begin,
// pairwise disjoint, not touching, non-empty, unused slots (0, 0) at the tail -- so that no row is
// reachable twice.  spans [Nq x 8 x 2], totals [Nq] (the sum of a query's span lengths).
constexpr uint32_t kMaxLabelSpans = 8;
enum LabelSpanMode : int { kLabelSpanSets = 0, kLabelSpanRanges = 1 };
// sel: kLabelSpanSets [Nq x n_sel] labels (n_sel 1 .. 8; -1: the whole index; entries may repeat, an
// entry that is no key gives nothing); kLabelSpanRanges [Nq x n_sel x 2] closed signed intervals
// (n_sel 1 .. 4; lo > hi and intervals without a key give nothing; no wildcard)
void launch_label_spans_resolve(const int32_t* keys, uint32_t n_keys, const uint32_t* offsets,
                                int mode, const int32_t* sel, uint32_t n_sel, uint32_t Nq,
                                uint32_t* spans, uint32_t* totals, hipStream_t stream);
// The exact K nearest of every query among the rows at its spans' positions and, with filter ids, whose
// bit of the query's row of the filter table is set (FilterTable's rules, bit offset 0).  Ranked by
// (distance, id): bit for bit what the scan of the whole base gives under the same label set or ranges.
struct LabelSpansLaunch {
  const void* base;
  const void* query;
  ggnn_dtype dtype;
  uint32_t N_base, D, Nq, k_query;
  ggnn_measure measure;
  int32_t* ids;  // [Nq x k_query]
  float* dists;
  const int32_t* rows;    // [N_base]
  const uint32_t* spans;  // [Nq x 8 x 2]
  // the cutoff the caller classified with (0: unknown): sizes the slices only; longer queries are
  // still answered in full
  uint32_t span_limit{0};
  const uint32_t* filter_table{nullptr};  // [num_filters x words] or null
  uint32_t num_filters{0}, words{0};
  const int32_t* filter_ids{nullptr};  // [Nq] or null: spans only
};
void launch_label_spans_scan(const LabelSpansLaunch& a, hipStream_t stream);
// launch_label_index_classify by totals: routed iff totals[n] <= cutoff
void launch_label_spans_classify(const uint32_t* totals, uint32_t Nq, uint32_t cutoff,
                                 uint32_t* routed_list, uint32_t* rest_list, uint32_t* counts,
                                 hipStream_t stream);

struct TopLaunch {
  const void* base;
  ggnn_dtype dtype;
  uint32_t D;
  ggnn_measure measure;
  uint32_t KBuild;
  const int32_t* translation;
  uint32_t N_layer, S, S_offset, layer;
  int32_t* graph_layer;
  float* nn1_dist_buffer;
};
void launch_top(const TopLaunch& a, hipStream_t stream);

struct MergeLaunch {
  const void* base;
  ggnn_dtype dtype;
  ggnn_measure measure;
  ggnn_graph_config cfg;
  const int32_t* graph_all;
  const int32_t* translation_all;
  const int32_t* selection_all;
  const float* nn1_stats;
  float tau_build;
  uint32_t layer_top, layer_btm;
  int32_t* graph_buffer;
  float* nn1_dist_buffer;
  uint32_t* n_dist;
  // optional pre-screen copy of the base (launch_prescreen_encode, same measure); ignored unless float32
  const uint8_t* ps_codes{nullptr};
  const float* ps_params{nullptr};
  uint32_t ps_Dc{0};
  // optional [N_btm x 4]: distance evaluations, float rows, code rows, pops per point
  uint32_t* n_work{nullptr};
};
void launch_merge(const MergeLaunch& a, hipStream_t stream);

struct SymLaunch {
  const void* base;
  ggnn_dtype dtype;
  ggnn_measure measure;
  uint32_t D, KBuild;
  const int32_t* graph_layer;
  const int32_t* translation;
  uint32_t N_layer;
  const float* nn1_stats;
  float tau_build;
  int32_t* sym_buffer;
  uint32_t* sym_atomic;
  uint32_t first_n, count;
  // optional pre-screen copy of the base (launch_prescreen_encode, same measure); ignored unless float32
  const uint8_t* ps_codes{nullptr};
  const float* ps_params{nullptr};
  uint32_t ps_Dc{0};
  // optional [N_layer x 4]: distance evaluations, float rows, code rows, pops per point
  uint32_t* n_work{nullptr};
  // optional [N_layer x (KBuild - KBuild / 2) x KBuild / 2]: deterministic mode (sym.hip), the
  // slots are then handed out by launch_sym_assign
  int32_t* requests{nullptr};
};
void launch_sym(const SymLaunch& a, hipStream_t stream);
void launch_sym_assign(uint32_t KBuild, uint32_t N_layer, const int32_t* requests,
                       uint32_t* sym_atomic, int32_t* sym_buffer, hipStream_t stream);

void launch_select(const ggnn_graph_config& cfg, uint32_t layer, const float* nn1_dist_buffer,
                   const float* rng, int32_t* translation_all, int32_t* selection_all,
                   hipStream_t stream);
void launch_uniform(float* out, uint32_t n, uint64_t seed, uint64_t stream_id,
                    hipStream_t stream);
void launch_sym_buffer_merge(uint32_t KBuild, uint32_t N_layer, int32_t* sym_buffer,
                             const uint32_t* sym_atomic, int32_t* graph_layer,
                             hipStream_t stream);
constexpr uint32_t kStatsBlocks = 1024;
void launch_nn1_stats(const float* nn1, uint32_t N, float* scratch, float* out,
                      hipStream_t stream);
// [F x N] byte masks (non-zero = allowed) -> [F x ceil(N / 32)] bitset words, padding bits zero
void launch_pack_filters(const uint8_t* masks, uint32_t F, uint64_t N, uint32_t* words,
                         hipStream_t stream);
// labels[ids[i]] = values[i] for i < count (device memory; every ids[i] < N)
void launch_scatter_labels(int32_t* labels, uint64_t N, const uint32_t* ids, const int32_t* values,
                           uint64_t count, hipStream_t stream);
void launch_sort_shard_results(uint32_t Nq, uint32_t row_len, int32_t* ids, float* dists,
                               hipStream_t stream);
void launch_merge_results(uint32_t Nq, uint32_t k, uint32_t num_parts, uint32_t stride,
                          uint32_t id_offset_per_part, const int32_t* parts_ids,
                          const float* parts_dists, int32_t* ids_out, float* dists_out,
                          hipStream_t stream);

// merge_results for the queries qlist[0, *qcount) only (device memory; null = all queries)
void launch_merge_results_subset(uint32_t Nq, uint32_t k, uint32_t num_parts, uint32_t stride,
                                 uint32_t id_offset_per_part, const int32_t* parts_ids,
                                 const float* parts_dists, int32_t* ids_out, float* dists_out,
                                 const uint32_t* qlist, const uint32_t* qcount,
                                 hipStream_t stream);

// ... and for the queries [first, first + count) only (every GPU of a multi-GPU handle merges its
// own slice of the query set); outputs are indexed by the query number.  part_elems: distance
// (in elements) between the rows of consecutive parts, 0 = Nq * stride (parts stored back to
// back); the packed exchange keeps every part's ids and distances in one block of 2 * Nq * stride
void launch_merge_results_range(uint32_t Nq, uint32_t k, uint32_t num_parts, uint32_t stride,
                                uint32_t id_offset_per_part, const int32_t* parts_ids,
                                const float* parts_dists, int32_t* ids_out, float* dists_out,
                                const uint32_t* qlist, const uint32_t* qcount, uint32_t first,
                                uint32_t count, hipStream_t stream, size_t part_elems = 0);

// stream-ordered scratch of one launch from a private, bounded pool per device (scratch.cpp)
void* scratch_alloc(size_t bytes, hipStream_t stream);
void scratch_free(void* p, hipStream_t stream);
// frees a launch's scratch (null: nothing) at scope exit, on the launch's stream
struct ScratchGuard {
  void* p;
  hipStream_t stream;
  ~ScratchGuard() { scratch_free(p, stream); }
};

// host layout math (graph_config.cpp)
void graph_config_init(uint32_t N, uint32_t D, uint32_t KBuild, ggnn_graph_config* out);
void query_sizing(uint32_t D, uint32_t k_query, uint32_t max_iterations, uint32_t* cache_size,
                  uint32_t* sorted_size);
uint32_t merge_sorted_size(uint32_t KBuild);
uint32_t sym_sorted_size(uint32_t KBuild);

}  // namespace ggnn_amd
