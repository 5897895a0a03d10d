// query kernels under label filters, float32 / uint8 rows: the templates of query_filtered.hip
// with LabelFilter in place of the bitset filter, in a translation unit of their own so that the
// bitset kernels stay what they were and the build compiles both in parallel
#define GGNN_LABELS_TU
#include "query_filtered.hip"
