// query kernels under label filters on float16 / bfloat16 rows (see query_labeled.hip and
// query_filtered_16.hip)
#define GGNN_LABELS_TU
#define GGNN_ROWS_16_TU
#include "query_filtered.hip"
