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
// translation units of their own (bf_mfma_bits.hip, bf_mfma_labels.hip); the unfiltered kernels
// keep their argument block.
//   kBfBits    a bitset row per query: the call's one bitset for every query, or the row of the
//              filter table that the query's filter id names
//   kBfLabels  an int32 label per base row against one per query
constexpr int kBfNoFilter = 0, kBfBits = 1, kBfLabels = 2;
struct BfMfmaFilteredArgs : BfMfmaArgs {
  const uint32_t* filter_bits;  // bitset / filter table / label column (BfLaunch)
  uint32_t filter_bit_offset;   // kBfBits: a multiple of 32
  FilterTable filter_table;
};
template <int FM>
using BfMfmaArgsOf = std::conditional_t<FM != kBfNoFilter, BfMfmaFilteredArgs, BfMfmaArgs>;
// LDS words behind the thresholds (single chunk) / the group norms (chunked) of a filtered kernel
//   kBfBits    verdict words of the block's 128 queries: [2][128], chunked [2][T][128]
//   kBfLabels  128 query labels; chunked: + [2][T][32] row labels beside the group norms
constexpr uint32_t bf_filter_lds_words(int fm, uint32_t T)
{
  return fm == kBfBits     ? 2u * T * kBfQueriesPerBlock
         : fm == kBfLabels ? kBfQueriesPerBlock + (T > 1 ? 2u * T * kBfTileRows : 0u)
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

}  // namespace ggnn_amd
