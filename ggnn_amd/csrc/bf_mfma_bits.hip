// bf_mfma_kernel under a bitset filter (the per-call bitset or a filter table with one id per
// query): the tile kernel templates of bf_mfma.hip with FM = kBfBits, in a translation unit of
// their own so that the unfiltered kernels stay what they were and the build compiles both in
// parallel
#define GGNN_BF_FILTER_TU 1
#include "bf_mfma.hip"
