// query kernels under label-range filters on float16 / bfloat16 rows (see query_labelrange.hip and
// query_filtered_16.hip)
#define GGNN_LABELRANGE_TU
#define GGNN_ROWS_16_TU
#include "query_filtered.hip"
