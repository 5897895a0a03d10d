// query kernels on int8 rows (GGNN_I8): the templates of query.hip instantiated for signed bytes
// only, in a translation unit of their own (see query_16.hip)
#define GGNN_ROWS_I8_TU
#include "query.hip"
