// query kernels under label-range filters, float32 / uint8 rows: query_filtered.hip instantiated for
// LabelRangeFilter (query_labelrange_kernel*), in a translation unit of its own like query_labelset.hip
#define GGNN_LABELRANGE_TU
#include "query_filtered.hip"
