// Test and tuning hooks of libggnn_amd.so: process-wide named integers.
//
// Set with ggnn_set_hook(name, value) (include/ggnn_c.h documents every name and its values).
// The environment is consulted ONLY when GGNN_TEST_HOOKS=1 is set (variable GGNN_<NAME>, read at
// every use), so that a production process that merely inherits such a variable is not steered
// by it.  Precedence: ggnn_set_hook > environment (with GGNN_TEST_HOOKS=1) > built-in default.
#pragma once
#include <cstdint>

namespace ggnn_amd {

enum Hook {
  kHookPrescreen = 0,   // PRESCREEN        default of new handles: 1 = exact pre-screen on
  kHookExchange,        // EXCHANGE         0 auto | 1 "rccl" | 2 "copy" | 3 "gather"
  kHookSymPrescreen,    // SYM_PRESCREEN    -1 auto (rows >= 1 KB) | 0 | 1
  kHookShardOverlap,    // SHARD_OVERLAP    1 = resident shards searched concurrently
  kHookVisSlots,        // VIS_SLOTS        usable keys per bucket of the hashed visited set (1..8)
  kHookVisTagSet,       // VIS_TAG_SET      0 = rings of 481..2016 keys scanned instead of the tag set
  kHookQuerySplit,      // QUERY_SPLIT      -1 auto | 0 | 1: blocking multi-GPU query as two half-batches
  kHookResidentShards,  // RESIDENT_SHARDS  0 auto (by free memory) | GPU slots per device for its shards
  kHookXcdMap,          // XCD_MAP          bit 0: merge, bit 1: sym -- XCD-contiguous point ranges
  kHookBfPoolKeepMb,    // BF_POOL_KEEP_MB  release threshold of the bf scratch pool
  kHookBfNoI8,          // BF_NO_I8         1 = uint8 bf_query through the float kernels
  kHookBfI8V1,          // BF_I8_V1         1 = LDS-list i8 kernel instead of the register-set one
  kHookBfSlices,        // BF_SLICES        0 auto | base slices per query block
  kHookBfNoCenter,      // BF_NO_CENTER     1 = rows not shifted by the column mean
  kHookBfTiles,         // BF_TILES         2 | 4 base tiles per accumulator group (D > 128)
  kHookBfI8NoShare,     // BF_I8_NOSHARE    1 = slices do not share their bound
  kHookBfI8Ranks,       // BF_I8_RANKS      bit mask of the set positions the slices exchange (-1 = auto: one, 31 = all)
  kHookBfScan,          // BF_SCAN          1 = scan kernels instead of the matrix-core path
  kHookRcclFailAfter,   // RCCL_FAIL_AFTER  fault injection: the n-th exchange (1-based) reports an
                        //                  RCCL failure (0 = never); exercises the peer-copy fallback
  kHookQueryEarly,      // QUERY_EARLY      0 = the query kernel's round-1..4 order (rows requested after
                        //                  the membership test); 1 = early rows where the layout allows
  kHookMergeEarly,      // MERGE_EARLY      the same switch for the merge kernel
  kHookQueryLdsPad,     // QUERY_LDS_PAD    extra bytes of LDS per wave of the early-rows query kernels
  kHookQueryGlobalRing, // QUERY_GLOBAL_RING 0 = early-rows kernels keep a visited ring in LDS even when it cannot wrap
  kHookBfI8Refresh,     // BF_I8_REFRESH    stages between bound exchanges of the i8 kernel's slices
  kHookBfI8Seed,        // BF_I8_SEED       rows of the i8 kernel's seeding launch (0 = none)
  kHookMergeCounting,   // MERGE_COUNTING   1 = merge launches without counters use the counting kernel too
  kHookPsExact,         // PS_EXACT         0 = query kernels always run the float phase, also on a lossless-grid base
  kHookLabelIndexSlices, // LABEL_INDEX_SLICES 0 auto | slices a label's rows are cut into by the index scan
  kHookBfRangeSlices,   // BF_RANGE_SLICES  0 auto | base slices per query of the range search (bf_range.hip)
  kHookBfRangePath,     // BF_RANGE_PATH    0 auto | 1 scan always | 2 tile kernels whenever dtype / D / filter allow
  kHookBfRangeCand,     // BF_RANGE_CAND    0 auto | entries of the tile path's candidate buffer (bf_range_mfma.hip)
  kHookBfRangeI8,       // BF_RANGE_I8      0 auto | 1 never | 2 integer tile kernels whenever dtype / measure / D / filter allow (bf_range_i8.hip)
  kHookBfF16,           // BF_F16           0 auto | 1 never | 2 16-bit tile kernels whenever dtype / measure / D / k allow (bf_f16.hip)
  kHookBfRangeF16,      // BF_RANGE_F16     0 auto | 1 never | 2 16-bit range tile kernels whenever dtype / measure / D / filter allow (bf_range_f16.hip)
  kHookBfI8Wide,        // BF_I8_WIDE       0 auto | 1 never | 2 wide-row integer kernel of bf_query whenever dtype / measure / D / k / shape allow (bf_i8_wide.hip)
  kHookBfI8Filtered,    // BF_I8_FILTERED   0 auto | 1 never | 2 filtered integer kernels of bf_query whenever dtype / measure / D / k / filter allow (bf_i8_filtered.hip)
  kHookBfLabelTiles,    // BF_LABEL_TILES   0 auto | 1 never | 2 float tile kernels for bf_query under label sets / ranges / masks whenever dtype / D / k / shape allow (bf_mfma_pred.hip)
  kHookBfI8Cos,         // BF_I8_COS        0 auto | 1 never | 2 integer cosine kernel of bf_query whenever dtype / measure / D / k / shape allow (bf_i8_cos.hip)
  kHookBfRangeI8Cos,    // BF_RANGE_I8_COS  0 auto | 1 never | 2 integer cosine tile kernels of the range search whenever dtype / measure / D / filter allow (bf_range_i8_cos.hip)
  kHookCount
};

int64_t hook(Hook h);
const char* hook_name(Hook h);
// -1: unknown name
int hook_by_name(const char* name);
void hook_set(Hook h, int64_t value);
void hook_reset(Hook h);

}  // namespace ggnn_amd
