// query kernels under label filters on int8 rows (GGNN_I8): see query_labeled.hip and query_i8.hip
#define GGNN_LABELS_TU
#define GGNN_ROWS_I8_TU
#include "query_filtered.hip"
