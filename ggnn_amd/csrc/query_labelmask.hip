// query kernels under label-mask filters, float32 / uint8 rows: query_filtered.hip instantiated for
// LabelMaskFilter (query_labelmask_kernel*), in a translation unit of its own like query_labelrange.hip
#define GGNN_LABELMASK_TU
#include "query_filtered.hip"
