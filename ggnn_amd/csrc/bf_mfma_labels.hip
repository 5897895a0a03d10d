// bf_mfma_kernel under label filters: the tile kernel templates of bf_mfma.hip with
// FM = kBfLabels, in a translation unit of their own (see bf_mfma_bits.hip)
#define GGNN_BF_FILTER_TU 2
#include "bf_mfma.hip"
