// query kernels under label-set filters on float16 / bfloat16 rows (see query_labelset.hip and
// query_filtered_16.hip)
#define GGNN_LABELSET_TU
#define GGNN_ROWS_16_TU
#include "query_filtered.hip"
