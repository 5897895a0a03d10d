// Device helpers that the kernels reading rows through a label index share: label_index.hip (one
// label per query) and label_spans.hip (label sets and label ranges as spans of positions).
#pragma once

#include "traversal.hpp"

namespace ggnn_amd {

// position of label L in keys, or n_keys.  Every lane computes the same thing when L is wave-uniform;
// the classify and resolve kernels call it per lane.
GGNN_DEV uint32_t label_index_find(const int32_t* keys, const uint32_t n_keys, const int32_t L)
{
  uint32_t lo = 0, hi = n_keys;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (keys[mid] < L)
      lo = mid + 1;
    else
      hi = mid;
  }
  return (lo < n_keys && keys[lo] == L) ? lo : n_keys;
}

// the distances of one batch into s_d: rows idv of lanes [0, ROWS * STEPS) (bf_query.hip's sequence)
template <typename BaseT, int LPR, int NCH, int MODE, class DE>
GGNN_DEV void label_index_batch(const DE& de, const int idv, float* s_d)
{
  constexpr int ROWS = kWave / LPR;
  constexpr int STEPS = StepsOf<LPR, NCH>::value;
  using Chunk = typename DE::Chunk;
  const int grp = threadIdx.x / LPR;
  Chunk v[STEPS][NCH];
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    const int id = __shfl(idv, s * ROWS + grp);
    const bool valid = id >= 0;
    const BaseT* rp = de.row_ptr(valid ? id : 0);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      v[s][c] = ChunkOf<BaseT>::zero();
      if (valid && de.chunk_valid(c))
        v[s][c] = de.load_chunk(rp, c);
    }
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    float x, y;
    de.template partial<MODE>(v[s], x, y);
    x = group_sum<LPR>(x);
    if (MODE == kCos)
      y = group_sum<LPR>(y);
    if (de.g == 0)
      s_d[s * ROWS + grp] = (MODE == kCos) ? de.finish_cos(x, y) : x;
  }
  __syncthreads();
}

// label_index_compact_kernel (label_index.hip) on a flag word per 64 queries: the two order-preserving
// lists and their lengths
void launch_label_index_compact(const unsigned long long* flags, uint32_t Nq, uint32_t* routed_list,
                                uint32_t* rest_list, uint32_t* counts, hipStream_t stream);

}  // namespace ggnn_amd
