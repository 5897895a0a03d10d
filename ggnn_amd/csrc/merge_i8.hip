// merge kernels on int8 rows (GGNN_I8): see query_i8.hip
#define GGNN_ROWS_I8_TU
#include "merge.hip"
