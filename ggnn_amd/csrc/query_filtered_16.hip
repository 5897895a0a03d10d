// filtered query kernels on float16 / bfloat16 rows: the templates of query_filtered.hip
// instantiated for the 16-bit element types only, in a translation unit of their own so that the
// build compiles them in parallel with the float32 / uint8 kernels
#define GGNN_ROWS_16_TU
#include "query_filtered.hip"
