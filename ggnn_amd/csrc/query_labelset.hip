// query kernels under label-set filters, float32 / uint8 rows: query_filtered.hip instantiated for
// LabelSetFilter (query_labelset_kernel*), in a translation unit of its own like query_labeled.hip
#define GGNN_LABELSET_TU
#include "query_filtered.hip"
