// The range tile kernels with 256 queries per workgroup (bf_range_i8.hip, bf_range_f16.hip) stage a
// bitset filter with thread = query: every thread picks the bitset row of its own query once, then loads
// one word of it per tile.  (FilterStage of bf_mfma.hip is laid out for 128 queries per workgroup.)
#pragma once
#include "bf_common.hpp"

namespace ggnn_amd {

// The bitset row of query q, chosen as wave_filter_bits() chooses it (that helper takes a wave-uniform
// query): the call's bitset without filter ids, else the table row of an id in [0, num_filters) -- an
// UNSIGNED compare --, the all-ones row for -1 and the all-zero row for everything else.  No id value
// forms an address outside table / consts.  q >= Nq (padding) reads the id of the last query.
GGNN_DEV const uint32_t* bf_thread_filter_row(const uint32_t* filter_bits, const FilterTable& t,
                                              uint32_t q, uint32_t Nq)
{
  if (!t.ids)
    return filter_bits;
  const int32_t f = t.ids[min(q, Nq - 1)];
  return static_cast<uint32_t>(f) < t.num_filters
             ? filter_bits + static_cast<size_t>(static_cast<uint32_t>(f)) * t.words
             : t.consts + (f == -1 ? 0u : t.words);
}

}  // namespace ggnn_amd
