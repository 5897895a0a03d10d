// merge kernels on float16 / bfloat16 rows (GGNN_F16, GGNN_BF16): the templates of merge.hip
// instantiated for the 16-bit element types only, in a translation unit of their own so that the
// build compiles them in parallel with the float32 / uint8 kernels of merge.hip
#define GGNN_ROWS_16_TU
#include "merge.hip"
