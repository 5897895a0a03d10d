// Shared between bf_mfma.hip (f32 / LDS-list kernels, host side) and bf_i8.hip (the register-set
// uint8 / int8 kernel, compiled with the VGPR form of the MFMA instructions).
#pragma once
#include "traversal.hpp"

namespace ggnn_amd {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBfQueriesPerBlock = 128;
constexpr int kBfTileRows = 32;
constexpr uint32_t kBfMaxKP = 120;  // lists of 128 queries must fit into LDS next to the tiles

struct BfMfmaArgs {
  const void* base;
  const void* query;
  const float* query_packed;  // chunked float kernel: operand-order copy (bf_mfma.hip QueryWindow)
  const float* mean;   // [D] shift applied to base and query rows (float32 squared L2), or null
  const float* bnorm;
  const float* qnorm;
  int32_t* part_ids;   // [slices][Nq][KP]
  float* part_dists;   // [slices][Nq][KP]
  uint32_t D, Dh, DP, Nq, N_base, KP, slices, rows_per_slice;
  uint32_t DM;  // floats of the shift vector kept in LDS by the chunked kernel (D rounded up)
  uint32_t* gthr;  // i8 v2 kernel: exchange area of the slices' published set entries
                   // ([Nq][5 ranks][slices padded to 4] ints, 0x7fffffff = none), or null
  uint32_t rank_mask;  // which of the published positions are used (bit i = rank i)
  uint32_t refresh_every;  // stages between exchanges after the doubling phase
  int32_t* seed;       // [Nq] K-th best distance over the head of the base (seeding launch), or null
  uint32_t seeding;    // this launch IS the seeding launch: writes `seed`, no lists
  // float tile kernels, equal_ranges != 0: the (query block, unit) sequence is cut into equal
  // ranges, a unit being 32 rows (single chunk) or one accumulator group of T x 32 rows (chunked)
  uint32_t equal_ranges;
  uint32_t tiles_per_q;      // units per query block
  uint32_t tiles_per_block;  // range of one workgroup
  uint64_t total_tiles;      // query blocks * tiles_per_q
};

// Filter mode of bf_mfma_kernel (template parameter FM).  The filtered instantiations live in
// translation units of their own (bf_mfma_bits.hip, bf_mfma_labels.hip, bf_mfma_pred.hip); the
// unfiltered kernels keep their argument block.
//   kBfBits    a bitset row per query: the call's one bitset for every query, or the row of the
//              filter table that the query's filter id names
//   kBfLabels  an int32 label per base row against one per query
//   kBfPredicate  a predicate on the int32 label of a base row -- a label set, label ranges or label
//              masks per query (LabelSetSpec / LabelRangeSpec / LabelMaskSpec) --, optionally ANDed
//              with the row of the filter table that the query's filter id names
constexpr int kBfNoFilter = 0, kBfBits = 1, kBfLabels = 2, kBfPredicate = 3;
struct BfMfmaFilteredArgs : BfMfmaArgs {
  const uint32_t* filter_bits;  // bitset / filter table / label column (BfLaunch)
  uint32_t filter_bit_offset;   // kBfBits: a multiple of 32
  FilterTable filter_table;
};
// kBfPredicate: one record of kBfPredWords words per query, made by bf_pred_prep_kernel (bf_mfma.hip)
// from the user's spec once per launch -- what the wave constructors of LabelSetFilter,
// LabelRangeFilter and LabelMaskFilter (traversal.hpp) make once per wave:
//   sets    w[0..8) the eight labels (a narrow set padded with its first entry)
//   ranges  w[0..4) lo, w[4..8) span = hi - lo (an empty interval replaced by the first non-empty one)
//   masks   w[0..3) / w[3..6) the two clauses (mask, value, any), a single clause repeated
//   w[8]    kBfPredWildcard: the set holds a -1 (every label passes);  kBfPredClosed: every interval
//           is empty (no row passes)
// The family is uniform over the launch (pred_family).  The filter table is filter_bits /
// filter_table of the base struct (ids null: no table), a multiple of 32 as the bit offset.
constexpr uint32_t kBfPredWords = 9;
constexpr uint32_t kBfPredWildcard = 1u, kBfPredClosed = 2u;
constexpr uint32_t kBfPredSets = 0, kBfPredRanges = 1, kBfPredMasks = 2;
struct BfMfmaPredArgs : BfMfmaFilteredArgs {
  const int32_t* pred_labels;    // the label column at the first global id of this base
  const uint32_t* pred_records;  // [Nq][kBfPredWords]
  uint32_t pred_family;          // kBfPredSets | kBfPredRanges | kBfPredMasks
};
template <int FM>
using BfMfmaArgsOf =
    std::conditional_t<FM == kBfPredicate, BfMfmaPredArgs,
                       std::conditional_t<FM != kBfNoFilter, BfMfmaFilteredArgs, BfMfmaArgs>>;
// LDS words behind the thresholds (single chunk) / the group norms (chunked) of a filtered kernel
//   kBfBits    verdict words of the block's 128 queries: [2][128], chunked [2][T][128]
//   kBfLabels  128 query labels; chunked: + [2][T][32] row labels beside the group norms
//   kBfPredicate  the verdict words of kBfBits, then the 128 predicate records of the block
constexpr uint32_t bf_filter_lds_words(int fm, uint32_t T)
{
  return fm == kBfBits     ? 2u * T * kBfQueriesPerBlock
         : fm == kBfLabels ? kBfQueriesPerBlock + (T > 1 ? 2u * T * kBfTileRows : 0u)
         : fm == kBfPredicate
             ? 2u * T * kBfQueriesPerBlock + kBfPredWords * kBfQueriesPerBlock
             : 0u;
}
// The filtered SINGLE-CHUNK kernels exist with the list length as a compile-time constant only
// (KPC = 18: k <= 10, shorter lists are rounded up -- any list longer than k is exact).  With a
// run-time list length the single-chunk kernels do not hold three waves per SIMD without a private
// segment (the unfiltered ones keep 12 to 52 bytes at NU = 12 / 16, the filtered ones came out at
// 12 to 76; longer constants, 64 and 120, made the compiler unroll the list loops and spill
// hundreds of bytes).  A filtered call with k > 10 and D <= 128 therefore runs the CHUNKED kernel
// with its one chunk of 128 columns (columns past D are zero in the query operand): two waves per
// SIMD, run-time list length, private segment 0.
constexpr uint32_t kBfFilteredSingleChunkKP = 18;
constexpr bool bf_filtered_runs_chunked(uint32_t D, uint32_t k_query)
{
  return D > 128 || k_query + 8 > kBfFilteredSingleChunkKP;
}
// the filtered tile kernel of a launch (defined in the filtered translation units)
const void* bf_mfma_bits_kernel(ggnn_dtype dtype, ggnn_measure measure, int T, int NU, int KPC);
const void* bf_mfma_labels_kernel(ggnn_dtype dtype, ggnn_measure measure, int T, int NU, int KPC);
const void* bf_mfma_pred_kernel(ggnn_dtype dtype, ggnn_measure measure, int T, int NU, int KPC);

// bf_mfma.hip: the shift of float32 squared L2 -- mean[D] = column mean of (a sample of) the base,
// q_shifted = fl(query - mean); partial is kBfMeanBlocks x D floats of scratch
constexpr uint32_t kBfMeanBlocks = 256;
void bf_center_rows(const float* base, uint32_t N_base, uint32_t D, const float* query, uint32_t Nq,
                    float* mean, float* partial, float* q_shifted, hipStream_t stream);

typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
constexpr uint32_t kBfI8RowStride = 144;

// bf_i8.hip: launches bf_i8v2_kernel for KP in {4, 10, 16} (a seeding launch over the first
// seed_rows rows of the base first, when m.seed is set and there are several slices); m.gthr must
// point to bf_i8v2_exchange_ints(Nq, slices) words initialised to 0x7fffffff (or be null: no exchange)
// is_signed: int8 rows (the SIGNED kernels), else uint8
void launch_bf_i8v2(const BfMfmaArgs& m, bool is_signed, uint32_t qblocks, uint32_t slices,
                    uint32_t seed_rows, hipStream_t stream);
size_t bf_i8v2_lds_bytes();
size_t bf_i8v2_exchange_ints(uint32_t Nq, uint32_t slices);
uint32_t bf_i8v2_default_rank_mask(uint32_t KP, uint32_t slices);

// bf_i8_wide.hip: the register-set kernel for uint8 / int8 rows of 128 < D <= 4096 bytes under
// squared L2 (the file's header has the arithmetic contract).  Norms are int32: |x'|^2 <= 2^26.
struct BfI8WideArgs {
  const void* base;
  const uint4* query_packed;  // the query set in operand order (bf_i8_wide_packed_words), flipped, zero past D
  const int32_t* bnorm;       // [N_base] |b'|^2
  const int32_t* qnorm;       // [Nq] |q'|^2
  int32_t* part_ids;          // [slices][Nq][KP]
  float* part_dists;          // [slices][Nq][KP]
  uint32_t D, nch, Nq, N_base, slices, rows_per_slice;  // nch: 128-byte column chunks of a row
  uint32_t* gthr;             // exchange area, as BfMfmaArgs::gthr
  uint32_t rank_mask, refresh_every;
  int32_t* seed;              // [Nq], as BfMfmaArgs::seed
  uint32_t seeding;
};
// (bf_i8_wide_supported / bf_i8_wide_routes: common.hpp)
size_t bf_i8_wide_packed_words(uint32_t qblocks, uint32_t D);  // 32-bit words of the packed query set
// norms[r] = |x'|^2 of N rows (bf_range_i8.hip's norm kernel; scratch_word: any device word, cleared)
void launch_bf_i8_row_norms(const void* rows, uint32_t N, uint32_t D, bool is_signed, int32_t* norms,
                            uint32_t* scratch_word, hipStream_t stream);
void launch_bf_i8_wide_pack(const void* query, uint32_t Nq, uint32_t D, bool is_signed,
                            uint32_t qblocks, uint4* packed, hipStream_t stream);
// the tile kernel for KP in {4, 10, 16} (m.slices x qblocks workgroups of 256 queries), after a seeding
// launch over the first seed_rows rows when m.seed is set and there are several slices
void launch_bf_i8_wide(const BfI8WideArgs& m, uint32_t KP, bool is_signed, uint32_t qblocks,
                       uint32_t seed_rows, hipStream_t stream);
// the 2^24 rule: queries whose K-th reported distance is >= 2^24 are appended to the rescan list
void launch_bf_i8_wide_uncertified(const float* dists, uint32_t Nq, uint32_t K, uint32_t* rescan_list,
                                   uint32_t* rescan_count, hipStream_t stream);

// bf_i8_cos.hip: the register-set kernel for uint8 / int8 rows of 16 <= D <= 4096 bytes under cosine
// (the file's header has the arithmetic contract).  Side data of a row or a query, one 16-byte record:
//   x  float bits of 1 / sqrtf((float)y), 0 for a zero row
//   y  sum x^2 of the row as stored (uint8: 0..255, int8: -128..127), <= 255^2 * 4096 < 2^31
//   z  uint8: 128 * sum (x - 128), the row's term of the true dot product; int8: 0
struct BfI8CosArgs {
  const void* base;
  const uint4* query_packed;  // as BfI8WideArgs::query_packed
  const int4* brec;           // [N_base] records of the base rows
  const int4* qrec;           // [Nq] records of the queries
  int32_t* part_ids;          // [slices][Nq][KP]
  float* part_dists;          // [slices][Nq][KP] the scan's values
  uint32_t D, nch, Nq, N_base, slices, rows_per_slice;
  uint32_t* gthr;             // exchange area, as BfMfmaArgs::gthr (float bits of values)
  uint32_t rank_mask, refresh_every;
  int32_t* seed;              // [Nq], as BfMfmaArgs::seed (float bits)
  uint32_t seeding;
};
// (bf_i8_cos_supported / bf_i8_cos_routes: common.hpp)
// records of N rows; norm_max (device word, cleared by the caller, or null): receives the largest y
void launch_bf_i8_cos_records(const void* rows, uint32_t N, uint32_t D, bool is_signed, int4* rec,
                              uint32_t* norm_max, hipStream_t stream);
// the tile kernel for KP in {4, 10, 16}, after a seeding launch as for launch_bf_i8_wide
void launch_bf_i8_cos(const BfI8CosArgs& m, uint32_t KP, bool is_signed, uint32_t qblocks,
                      uint32_t seed_rows, hipStream_t stream);
// the 2^24 rule under cosine: a query with sum q^2 >= 2^24 is appended to the rescan list, and every
// query when *norm_max >= 2^24
void launch_bf_i8_cos_uncertified(const int4* qrec, const uint32_t* norm_max, uint32_t Nq,
                                  uint32_t* rescan_list, uint32_t* rescan_count, hipStream_t stream);

// bf_i8_filtered.hip: the filtered forms of the two register-set kernels (the file's header has the
// design).  One argument block for both row regimes; norms are int32 as for the wide rows.
//   kI8fBits    the call's one bitset, folded into the staged row norms
//   kI8fTable   a filter table row per query, verdict per (query, row) on the hit path
//   kI8fLabels  an int32 label per base row against one per query, verdict on the hit path
constexpr int kI8fBits = 1, kI8fTable = 2, kI8fLabels = 3;
struct BfI8FilteredArgs {
  const void* base;
  const void* query;          // D <= 128: the query rows (the operand stays in registers)
  const uint4* query_packed;  // D > 128: the query set in operand order (launch_bf_i8_wide_pack)
  const int32_t* bnorm;       // [N_base] |b'|^2
  const int32_t* qnorm;       // [Nq] |q'|^2
  int32_t* part_ids;          // [slices][Nq][KP]
  float* part_dists;          // [slices][Nq][KP]
  uint32_t D, nch, Nq, N_base, slices, rows_per_slice;
  uint32_t flip;              // 0x80808080 for uint8 rows, 0 for int8
  uint32_t* gthr;             // exchange area, as BfMfmaArgs::gthr
  uint32_t rank_mask, refresh_every;
  int32_t* seed;              // [Nq], as BfMfmaArgs::seed
  uint32_t seeding;
  const uint32_t* filter_bits;  // bitset / filter table / label column (BfLaunch)
  uint32_t filter_bit_offset;   // bitsets: a multiple of 32
  FilterTable filter_table;
};
// the kernels of one filter mode live in an object of their own (Makefile: bf_i8_filtered.hip once per
// mode); nm: 32-column blocks of the resident operand (2 | 4), 0 = the streamed regime
const void* bf_i8f_bits_kernel(int nm, uint32_t KP);
const void* bf_i8f_table_kernel(int nm, uint32_t KP);
const void* bf_i8f_labels_kernel(int nm, uint32_t KP);
size_t bf_i8f_lds_bytes(int fm, bool wide);
// the kernel of the launch for KP in {4, 10, 16} (m.slices x qblocks workgroups of 256 queries), after a
// seeding launch over the first seed_rows rows when m.seed is set and there are several slices
void launch_bf_i8_filtered(const BfI8FilteredArgs& m, int fm, uint32_t KP, uint32_t qblocks,
                           uint32_t seed_rows, hipStream_t stream);
// the 2^24 rule under a filter: queries whose K-th reported distance is finite and >= 2^24
void launch_bf_i8_filtered_uncertified(const float* dists, uint32_t Nq, uint32_t K,
                                       uint32_t* rescan_list, uint32_t* rescan_count,
                                       hipStream_t stream);

// ---- the scan kernels' argument block and filter verdicts (bf_query.hip, bf_range.hip) ----------
struct BfArgs {
  const void* base;
  const void* query;
  int32_t* ids;    // [slices x Nq x K] partial results (or final when slices == 1)
  float* dists;
  uint32_t D, Nq, N_base, K, slices, rows_per_slice;
  // optional subset: only the queries qlist[0, *qcount) are scanned (device memory; the grid is
  // sized for all Nq queries and the surplus blocks leave at once)
  const uint32_t* qlist;
  const uint32_t* qcount;
  // filtered scan (FILT kernels): allowed-id bitset, row i is allowed iff bit i + filter_bit_offset
  const uint32_t* filter_bits;
  uint32_t filter_bit_offset;
};

// Arguments of the FILT kernels: per-query filters make filter_bits a table and add the id array
// (FilterTable, common.hpp).  A struct of its own: the unfiltered kernels keep their argument block.
struct BfFilteredArgs : BfArgs {
  FilterTable filter_table;
};
template <bool FILT>
using BfArgsOf = std::conditional_t<FILT, BfFilteredArgs, BfArgs>;

#if defined(__HIPCC__)
// FILT: the bitset of this (query, slice) wave -- the call's, or the table row that the filter id
// of query n names (scalar, once per wave)
template <bool FILT>
GGNN_DEV const uint32_t* bf_wave_filter(const BfArgsOf<FILT>& a, uint32_t n)
{
  if constexpr (FILT)
    return wave_filter_bits(a.filter_bits, a.filter_table, n);
  else
    return nullptr;
}

// FILT: this lane's word of the bitset for the 64 (or fewer) rows of a batch starting at i0 -- one
// coalesced load per batch, issued in front of the rows -- and the verdict for row i0 + lane
template <bool FILT>
GGNN_DEV uint32_t bf_filter_word(const BfArgs& a, const uint32_t* bits, uint32_t i0, uint32_t end)
{
  if constexpr (FILT) {
    const uint32_t row = i0 + threadIdx.x;
    return row < end ? bits[(row + a.filter_bit_offset) >> 5] : 0u;
  }
  return 0u;
}
template <bool FILT>
GGNN_DEV bool bf_row_allowed(const BfArgs& a, uint32_t word, uint32_t i0)
{
  if constexpr (FILT)
    return (word >> ((i0 + threadIdx.x + a.filter_bit_offset) & 31u)) & 1u;
  return true;
}

// LAB (label filters, with FILT): the rows whose int32 label equals the label of query n; label -1
// admits every row.  Kernels of their own (the trailing template argument), so that the bitset
// kernels keep their code: a read parametrised over both forms costs them registers (DESIGN.md
// 4.9).  One coalesced dword per row of the batch, issued in front of the rows like the bit words;
// the shard offset is folded into the wave-uniform pointer and the label addressed as a 32-bit
// byte offset from it (at most 2^30 rows per scan: kMaxLabeledShardRows, traversal.hpp).
//   allowed = (label & vmask) == want      label L: vmask ~0u, want L;  label -1: vmask 0, want 0
struct BfLabelFilter {
  const uint32_t* labels;  // the column at the first global id of this base
  uint32_t vmask, want;
};
template <bool LAB, class Args>
GGNN_DEV BfLabelFilter bf_wave_labels(const Args& a, uint32_t n)
{
  if constexpr (LAB) {
    const int32_t L = __builtin_amdgcn_readfirstlane(a.filter_table.query_labels[n]);
    const uint32_t vmask = (L == -1) ? 0u : ~0u;
    return BfLabelFilter{a.filter_bits + a.filter_bit_offset, vmask, static_cast<uint32_t>(L) & vmask};
  }
  else
    return BfLabelFilter{nullptr, 0u, 0u};
}
GGNN_DEV uint32_t bf_label_word(const BfLabelFilter& f, uint32_t i0, uint32_t end)
{
  const uint32_t row = i0 + threadIdx.x;
  return row < end ? filter_word_at(f.labels, row << 2) : 0u;
}
GGNN_DEV bool bf_label_allowed(const BfLabelFilter& f, uint32_t word)
{
  return (word & f.vmask) == f.want;
}
// the filter word and the verdict of a kernel: the bitset's, or the label's
template <bool FILT, bool LAB>
GGNN_DEV uint32_t bf_word(const BfArgs& a, const uint32_t* bits, const BfLabelFilter& f,
                          uint32_t i0, uint32_t end)
{
  if constexpr (LAB)
    return bf_label_word(f, i0, end);
  else
    return bf_filter_word<FILT>(a, bits, i0, end);
}
template <bool FILT, bool LAB>
GGNN_DEV bool bf_allowed(const BfArgs& a, const BfLabelFilter& f, uint32_t word, uint32_t i0)
{
  if constexpr (LAB)
    return bf_label_allowed(f, word);
  else
    return bf_row_allowed<FILT>(a, word, i0);
}
#endif  // __HIPCC__

// (bf_query.hip; shared with the label-family scans and bf_range.hip)
void bf_slice_rows(uint32_t N_base, uint32_t& slices, uint32_t& rows_per_slice);

// ---- range search (bf_range.hip: the scan; bf_range_mfma.hip: tile pre-selection, exact hits) -----
// dtype / D / filter of a launch suit the tile kernels, and (hook BF_RANGE_PATH = 0) Nq and N_base
// reach their minima; BF_RANGE_PATH = 1 says no to everything, 2 waives the minima
void launch_bf_range_query_mfma(const BfRangeLaunch& a, hipStream_t stream);
// bf_range_i8.hip: uint8 / int8 rows under squared L2 on the integer matrix cores, exact verdicts
// (a launch that bf_range_i8_supported admits)
void launch_bf_range_query_i8(const BfRangeLaunch& a, hipStream_t stream);
// its last pass (bf_range_i8_take_lims_kernel): lims[0, n) = from[0, n) if *flag != 0
void launch_bf_range_i8_take_lims(const uint32_t* flag, const uint64_t* from, uint32_t n, uint64_t* lims,
                                  hipStream_t stream);
// bf_range_i8_cos.hip: uint8 / int8 rows under cosine on the integer matrix cores, exact verdicts
// (a launch that bf_range_i8_cos_supported admits)
void launch_bf_range_query_i8_cos(const BfRangeLaunch& a, hipStream_t stream);
// bf_range_f16.hip: float16 / bfloat16 rows under squared L2 on the 16-bit matrix cores, tile
// pre-selection and exact hits (a launch that bf_range_f16_supported admits)
void launch_bf_range_query_f16(const BfRangeLaunch& a, hipStream_t stream);
// bf_range_mfma.hip's last passes, shared with bf_range_f16.hip.  Compaction: every (query, part) copies
// its hits (candidates with distance <= radius), in candidate order, to ids / dists -- unless the
// candidates overflowed their budget or the total exceeds the capacity.  take_lims: lims[0, n) = from[0, n)
// if *flag != 0 (the scan passes answered the call)
struct BfRangeCompactArgs {
  const float* radii;
  const uint32_t* cand_counts;
  const uint64_t* cand_offsets;
  const uint64_t* cand_lims;
  const int32_t* cand_ids;
  const float* cand_dists;
  const uint64_t* hit_offsets;  // [Nq x parts] exclusive
  const uint64_t* lims;         // [Nq + 1]
  int32_t* ids;
  float* dists;
  uint64_t budget, capacity;
  uint32_t Nq, parts;
};
void launch_bf_range_compact(const BfRangeCompactArgs& cp, hipStream_t stream);
void launch_bf_range_take_lims(const uint32_t* flag, const uint64_t* from, uint32_t n, uint64_t* lims,
                               hipStream_t stream);
// The scan passes (count, prefix, fill) of a validated launch.  gate (device, or null: the plain scan):
// with *gate == 0 every wave of the count and fill passes returns before it touches the base, and
// what the prefix pass then writes to a.lims means nothing -- the caller gives it lims of its own.
void launch_bf_range_scan(const BfRangeLaunch& a, const uint32_t* gate, hipStream_t stream);
// bf_range_prefix_kernel: counts [Nq x slices] -> exclusive offsets [Nq x slices] and lims [Nq + 1]
void launch_bf_range_prefix(const uint32_t* counts, uint32_t Nq, uint32_t slices, uint64_t* offsets,
                            uint64_t* lims, hipStream_t stream);

}  // namespace ggnn_amd
