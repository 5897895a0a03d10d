// bf_mfma_kernel under a label predicate (a label set, label ranges or label masks per query, with
// or without a filter table): the tile kernel templates of bf_mfma.hip with FM = kBfPredicate, in a
// translation unit of their own (see bf_mfma_bits.hip).  One kernel per shape serves all three
// families: the family is a launch-uniform switch of FilterStage<kBfPredicate>
#define GGNN_BF_FILTER_TU 3
#include "bf_mfma.hip"
