// query kernels under label-mask filters on float16 / bfloat16 rows (see query_labelmask.hip and
// query_filtered_16.hip)
#define GGNN_LABELMASK_TU
#define GGNN_ROWS_16_TU
#include "query_filtered.hip"
