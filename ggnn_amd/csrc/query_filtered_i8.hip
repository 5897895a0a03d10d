// query kernels under an allowed-id bitset on int8 rows (GGNN_I8): see query_i8.hip and
// query_filtered_16.hip
#define GGNN_ROWS_I8_TU
#include "query_filtered.hip"
