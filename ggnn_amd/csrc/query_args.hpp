// Kernel arguments of the query kernels (query.hip).
#pragma once
#include "common.hpp"

namespace ggnn_amd {

struct QueryArgs {
  const void* base;
  const void* query;
  const int32_t* graph0;
  const int32_t* start;
  const float* nn1_stats;
  int32_t* ids;
  float* dists;
  uint32_t* n_dist;
  uint32_t* n_pop;
  uint2* n_rows;
  uint32_t D, Nq, N_base, KBuild, num_start, KQuery, sorted, cache, max_iters;
  uint32_t shards_per_gpu, on_gpu_shard;
  float tau;
  // optional pre-screen copy of the base coded for this measure (prescreen.hip); float32 only
  const uint8_t* ps_codes;
  const float* ps_params;
  uint32_t ps_Dc;
  uint32_t vis_slots;  // usable keys per bucket of the hashed visited set (kVisSlots; test hook)
  // tag-set form (long rings, traversal.hpp kTagSet): [Nq x (cache - sorted)] visited rings in
  // global memory (scratch of the launch) and the bucket bits of the set
  int32_t* ring;
  uint32_t tag_bits;
  // filtered search (query_filtered.hip): allowed-id bitset over the global ids and the first
  // global id of this shard; null for the unfiltered kernels (with per-query filters: the table,
  // see FilteredQueryArgs)
  const uint32_t* filter_bits;
  uint32_t filter_bit_offset;
  // HOST side only (in the struct's tail padding: size and every offset are what they were, and
  // no kernel reads it): the launch may pick the kernels that take exact distances from lossless
  // pre-screen codes (ExactOf in traversal.hpp; QueryLaunch::ps_lossless and hook PS_EXACT)
  uint32_t ps_lossless;
};

// Arguments of the filtered kernels (query_filtered.hip): per-query filters make filter_bits a
// table and add the id array beside it.  A struct of its own, so that the unfiltered kernels keep
// their argument block -- and stay the same code objects -- whatever the filters grow into.
struct FilteredQueryArgs : QueryArgs {
  FilterTable filter_table;
};

// Arguments of the label-set kernels (query_labelset.hip): the label column and the queries' sets
// beside the optional filter table.  Derived once more, so that FilteredQueryArgs stays what it is.
struct LabelSetQueryArgs : FilteredQueryArgs {
  LabelSetSpec set;
};

// Arguments of the label-range kernels (query_labelrange.hip), likewise: the label column and the
// queries' intervals beside the optional filter table.
struct LabelRangeQueryArgs : FilteredQueryArgs {
  LabelRangeSpec range;
};

// Arguments of the label-mask kernels (query_labelmask.hip), likewise: the label column and the
// queries' clauses beside the optional filter table.
struct LabelMaskQueryArgs : FilteredQueryArgs {
  LabelMaskSpec mask;
};

}  // namespace ggnn_amd
