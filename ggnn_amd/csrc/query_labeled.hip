// query kernels under label filters, float32 / uint8 rows: query_filtered.hip instantiated for
// LabelFilter (query_labeled_kernel*) instead of the bitset filter, in a translation unit of its own
// so that the bitset kernels stay what they were and the build compiles both in parallel
#define GGNN_LABELS_TU
#include "query_filtered.hip"
