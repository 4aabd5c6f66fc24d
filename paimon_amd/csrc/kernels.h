// Device structures + kernel launcher declarations shared between
// kernels.hip (device) and plan.cpp (host).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "bits_core.h"
#include "orc_decimal_core.h"
#include "orc_timestamp_core.h"
#include "stream_core.h"

namespace pmh {

// Hard capacity limits (validated host-side at plan creation):
//  - PMH_MAX_RUNS sorted runs per section (the reference's disk-spill path,
//    MergeSorter.java:112-125, stays out of scope while real compaction
//    shapes fit — 32 covers C5's 16->1 with 2x headroom);
//  - rows per run < 2^PMH_ROW_BITS (winner packing run:5 | row:27; a run is
//    the concatenation of its files, the cap applies to the run TOTAL).
constexpr int PMH_MAX_RUNS = 32;
constexpr int PMH_ROW_BITS = 27;
constexpr uint32_t PMH_ROW_MASK = ((uint32_t)1 << PMH_ROW_BITS) - 1;
// 3584-row tiles with 512-thread workgroups (~76 KB LDS, 2 workgroups/CU).
// Measured on MI355X: halving to 1792/256 for 4 WGs/CU made every phase
// SLOWER (fused 6.3 -> 7.8 ms; C3 emit +60%) — the doubled tile count costs
// more in per-tile setup/barriers/lookback than the extra resident tiles
// buy in latency hiding. The partition runs two-level regardless (coarse
// every PMH_COARSE_G-th boundary, windowed refine for the rest).
constexpr int PMH_TILE_THREADS = 512;
constexpr int64_t PMH_TILE_ROWS = 3584;
constexpr int PMH_COARSE_G = 16;
// packed-seq sentinel for rows removed by a deletion vector: the merge
// kernels treat such rows as nonexistent (ApplyDeletionVectorReader
// semantics). Real packed values are >= 0 (sequence numbers are
// non-negative counters).
constexpr int64_t PMH_DEAD = INT64_MIN;
constexpr int PMH_TILE_MAX = PMH_TILE_ROWS + PMH_MAX_RUNS;
constexpr int PMH_TILE_ITER =
    (PMH_TILE_MAX + PMH_TILE_THREADS - 1) / PMH_TILE_THREADS;

// One column of one run, as plan.cpp stages it: ONE contiguous device buffer
// of `esize`-byte elements (the PLAIN page payloads are packed per column at
// H2D time), addressed directly from addr0.
struct DevCol {
    uint64_t addr0;   // element 0 address
    uint64_t valid0;  // byte-per-row validity array; 0 = all valid
    int32_t esize;    // element size in bytes (stored width)
    int32_t pad;
};

// RleChunk, Rlev2Chunk, DeltaChunk, DeltaStream: stream_core.h (the host
// walks that fill them live there).

extern "C" {

// DELTA_BINARY_PACKED decode, three phases batched across all chunks:
// per-block delta sums, per-stream base scan, then unpack + wave scan +
// base add into the output column.
hipError_t pmh_launch_delta_sum(const DeltaChunk *chunks, int64_t n_chunks,
                                int64_t *sums, hipStream_t stream);
hipError_t pmh_launch_delta_scan(const DeltaStream *streams,
                                 int64_t n_streams, const int64_t *sums,
                                 int64_t *bases, hipStream_t stream);
hipError_t pmh_launch_delta_emit(const DeltaChunk *chunks, int64_t n_chunks,
                                 const int64_t *bases, hipStream_t stream);


// Decode ORC RLEv2 / byte-RLE work chunks into a dense typed column
// (int32 or int64 elements per chunk.out_esize). One wave per chunk.

// value-filter term (single-run sections only — MergeFileSplitRead.java:
// 227-239: value filters must not push into overlapping sections).
// op: 0 eq, 1 ne, 2 lt, 3 le, 4 gt, 5 ge, 6 is_null, 7 is_not_null
struct FilterTerm {
    int32_t col;     // index into the plan's column list
    int32_t op;
    int64_t ilit;    // integer/string-id literal
    double dlit;     // float literal
    int32_t is_fp;   // compare as double
    int32_t pad;
};
// mark rows FAILING the conjunction as dead in the tombstone array
hipError_t pmh_launch_filter(const DevCol *cols, int n_cols,
                             const struct FilterTerm *terms, int n_terms,
                             int64_t rows, uint8_t *tomb,
                             hipStream_t stream);

// full-compaction changelog chain (FullChangelogMergeFunctionWrapper):
// finalize compacts the merge pass's provisional per-group entries into
// rows (evaluating row-deduplicate value equality); emit gathers them.
hipError_t pmh_launch_cl_finalize(const DevCol *cols,
                                  const uint8_t *col_dtype, int n_cols,
                                  int first_val, int k,
                                  const uint64_t *cl_entries,
                                  uint64_t *cl_out, int32_t *cl_counts,
                                  int64_t n_tiles, int64_t tile_rows,
                                  hipStream_t stream);
hipError_t pmh_launch_cl_emit(const DevCol *cols, const uint8_t *col_dtype,
                              const uint8_t *col_nullable, int n_cols,
                              int kind_col, const uint64_t *cl_rows,
                              const int32_t *cl_counts,
                              const int64_t *cl_offsets, int64_t n_tiles,
                              int64_t tile_rows, void *const *out_ptrs,
                              uint8_t *const *out_valid, hipStream_t stream);

// The same chain for the folding engines (partial-update / aggregation),
// whose after-type rows are the engine's folded result: merge flags bit
// PMH_FLAG_FOLD_CL selects the changelog walk of the PU k_merge_tiles, whose
// after-type entries name the main-output row tile_offsets[tile] + g
// (changelog_core.h). Both kernels therefore run after the engine's emit
// kernel on the same stream and read out_ptrs / out_valid (the plan's main
// output); emit writes out_ptrs2 / out_valid2. They stage pmh_fold_cl_lds(k,
// n_cols) bytes of per-run column tables in LDS; the launchers return
// hipErrorInvalidValue past PMH_FOLD_CL_LDS_MAX (plan creation refuses such a
// section first).
constexpr int PMH_FLAG_FOLD_CL = 1 << 16;
constexpr int64_t PMH_FOLD_CL_LDS_MAX = 48 * 1024;
constexpr int64_t pmh_fold_cl_lds(int64_t k, int64_t n_cols) {
    return 16 * k * n_cols + 32 * n_cols + ((n_cols + 7) & ~(int64_t)7);
}
hipError_t pmh_launch_cl_finalize_out(
    const DevCol *cols, const uint8_t *col_dtype, const uint8_t *col_nullable,
    int n_cols, int first_val, int k, const uint64_t *cl_entries,
    uint64_t *cl_out, int32_t *cl_counts, const int64_t *tile_offsets,
    int64_t n_tiles, int64_t tile_rows, void *const *out_ptrs,
    uint8_t *const *out_valid, hipStream_t stream);
hipError_t pmh_launch_cl_emit_out(
    const DevCol *cols, const uint8_t *col_dtype, const uint8_t *col_nullable,
    int n_cols, int k, int kind_col, const uint64_t *cl_rows,
    const int32_t *cl_counts, const int64_t *cl_offsets,
    const int64_t *tile_offsets, int64_t n_tiles, int64_t tile_rows,
    void *const *out_ptrs, uint8_t *const *out_valid, void *const *out_ptrs2,
    uint8_t *const *out_valid2, hipStream_t stream);

// on-GPU zstd page decompression (k_zstd_pages): one job per parquet page.
// scratch must hold n_jobs * PZ_SLOT bytes (PZ_SLOT in zstd_core.h);
// status[j] = decompressed bytes or a PZ_ERR_* code.
struct ZstdJob {
    uint64_t src_off, dst_off;  // into the batch src / dst blobs
    uint32_t src_len, dst_len;
};
// on-GPU zstd page COMPRESSION (k_zstd_compress): one job per page;
// scratch holds n * sizeof(PzEnc) bytes; status[j] = compressed size or
// a PZ_ERR_* code.
hipError_t pmh_launch_zstd_compress(const uint8_t *src,
                                    const struct ZstdJob *jobs, int n,
                                    uint8_t *dst, uint8_t *scratch,
                                    int64_t *status, hipStream_t stream);
hipError_t pmh_launch_zstd_pages(const uint8_t *src,
                                 const struct ZstdJob *jobs, int n,
                                 uint8_t *dst, uint8_t *scratch,
                                 int64_t *status, hipStream_t stream);

hipError_t pmh_launch_rlev2(const Rlev2Chunk *chunks, int64_t n_chunks,
                            hipStream_t stream);

// Decode ORC DECIMAL varint work units (VarintUnit, orc_decimal_core.h) into
// a dense int32/int64 column of unscaled values at the column scale. One
// wave per unit. Units that read a scale scratch must be launched after the
// k_rlev2 launch that fills it, on the same stream.
hipError_t pmh_launch_orc_varint(const VarintUnit *units, int64_t n_units,
                                 hipStream_t stream);

// Expand BOOLEAN work units (BitsUnit, bits_core.h: Parquet PLAIN bits or
// ORC boolean byte-RLE runs / literal groups) into 0/1 elements of 1 or 4
// bytes. One wave per unit; a unit may start at any output index.
hipError_t pmh_launch_bits_expand(const BitsUnit *units, int64_t n_units,
                                  hipStream_t stream);

// Combine ORC TIMESTAMP seconds and stored nanos (TsUnit,
// orc_timestamp_core.h) into INT64 milliseconds / microseconds, in place.
// Launched after the k_rlev2 launch that decodes both streams, on the same
// stream. One workgroup per unit.
hipError_t pmh_launch_orc_timestamp(const TsUnit *units, int64_t n_units,
                                    hipStream_t stream);

hipError_t pmh_launch_partition(const DevCol *keys, const int64_t *lens, int k,
                                int64_t tile_rows, int64_t n_bounds,
                                int64_t total_rows, int32_t *cuts,
                                hipStream_t stream);

hipError_t pmh_launch_merge_tiles(const DevCol *keys, const DevCol *seqs,
                                  const DevCol *kinds, const int64_t *lens,
                                  int k, const int32_t *cuts, int64_t n_tiles,
                                  int64_t tile_rows, int flags,
                                  const uint64_t *tombs,
                                  uint32_t *winners, int32_t *tile_counts,
                                  uint16_t *group_start, uint32_t *err_flag,
                                  const uint8_t *run_levels, int max_level,
                                  uint64_t *cl_entries, int32_t *cl_counts,
                                  const uint32_t *probe_words,
                                  const int64_t *probe_off,
                                  hipStream_t stream);

// lookup changelog producer (LookupChangelogMergeFunctionWrapper): merge
// flags bit selecting the lookup walk of k_merge_tiles. keys/seqs/kinds/
// run_levels then hold k + n_levels slots (the lookup levels after the k
// merge runs) and probe_words/probe_off come from pmh_launch_lookup_probe.
constexpr int PMH_FLAG_LOOKUP = 1 << 15;

// k_lookup_probe: for every row of the section's level-0 runs (probe_off[r]
// >= 0: word offset of run r's first row; < 0: run r is not probed), the
// packed (slot, row) of the first lookup level — slots k .. k+n_levels-1,
// lowest level first — that holds the row's key, or 0xFFFFFFFF.
hipError_t pmh_launch_lookup_probe(const DevCol *keys, const int64_t *lens,
                                   const int64_t *probe_off, int k,
                                   int n_levels, int64_t max_run_rows,
                                   uint32_t *words, hipStream_t stream);

hipError_t pmh_launch_scan_tiles(const int32_t *tile_counts, int64_t n_tiles,
                                 int64_t *tile_offsets, int64_t *total_out,
                                 hipStream_t stream);

// FUSED merge + emit (deduplicate / first-row): ticket-ordered persistent
// workgroups, decoupled-lookback output offsets (packed agent-scope atomic
// per tile in `status`, zeroed before launch along with `ticket`), emission
// from LDS-staged columns. Replaces merge_tiles + scan_tiles + emit for
// non-member-list engines. key_col = -1 for composite keys (key columns
// then emit through the generic column path).
hipError_t pmh_launch_merge_emit(const DevCol *keys, const DevCol *seqs,
                                 const DevCol *kinds, const int64_t *lens,
                                 int k, const int32_t *cuts,
                                 int64_t tile_base, int64_t tile_limit,
                                 int64_t n_tiles,
                                 int64_t tile_rows, int flags,
                                 const uint64_t *tombs,
                                 const DevCol *cols, const uint8_t *col_dtype,
                                 const uint8_t *col_nullable, int n_cols,
                                 int key_col, int seq_col, int kind_col,
                                 const int16_t *useq_cols, int n_useq,
                                 uint64_t *status, uint64_t *ticket,
                                 int64_t *total_out, uint32_t *dense_winners,
                                 void *const *out_ptrs,
                                 uint8_t *const *out_valid,
                                 uint32_t *err_flag, hipStream_t stream);

// SPLIT-mode value emission: gathers value columns by the densely-written
// packed winners (k_merge_emit with dense_winners != null emitted key/seq/
// kind and the winner list; this kernel runs at full occupancy, no LDS).
hipError_t pmh_launch_emit_dense(const DevCol *cols,
                                 const uint8_t *col_dtype,
                                 const uint8_t *col_nullable, int n_cols,
                                 int key_col, int seq_col, int kind_col,
                                 const uint32_t *winners,
                                 int64_t t0, int64_t t1,
                                 const uint64_t *status,
                                 void *const *out_ptrs,
                                 uint8_t *const *out_valid,
                                 hipStream_t stream);

// The kernel the last pmh_launch_emit chose.
enum {
    PMH_EMIT_NONE = 0,
    PMH_EMIT_GATHER = 1,  // k_emit
    PMH_EMIT_CONTIG = 2,  // k_emit_contig
    PMH_EMIT_STREAM = 3,  // k_emit_stream
};
int pmh_last_emit_kernel();

// Winner gather. n_desc = run slots of `cols` that a winner word can name
// (the k merge runs plus a lookup plan's level slots). cuts / lens are the
// partition's cuts ((n_tiles + 1) * k) and the k run lengths the winners
// were merged from; any_nullable = some column of the plan has a validity
// output. Plans without lookup slots (n_desc == k) and without nullable
// columns stream their tile slices through LDS (k_emit_stream,
// PMH_EMIT_STREAM=0 turns it off); other plans whose descriptor table fits
// LDS run k_emit_contig; the rest, and PMH_EMIT_LEGACY=1, run k_emit, which
// reads its descriptors from global memory.
hipError_t pmh_launch_emit(const DevCol *cols, const uint8_t *col_dtype,
                           const uint8_t *col_nullable, int any_nullable,
                           int n_cols, int k, int n_desc,
                           const int32_t *cuts, const int64_t *lens,
                           const uint32_t *winners,
                           const int32_t *tile_counts,
                           const int64_t *tile_offsets, int64_t n_tiles,
                           int64_t tile_rows, const int64_t *total_out,
                           void *const *out_ptrs, uint8_t *const *out_valid,
                           hipStream_t stream);

hipError_t pmh_launch_rle_decode(const RleChunk *chunks, int64_t n_chunks,
                                 int32_t *out, hipStream_t stream);

// Decode def-level streams (bit width 1) and position the dense PLAIN
// values: valid[row] = level; out[row] = dense[aux + prefix] for valid rows
// (VectorizedColumnReader null handling, VectorizedColumnReader.java:143-241).
hipError_t pmh_launch_level_scatter(const RleChunk *chunks, int64_t n_chunks,
                                    hipStream_t stream);

// PartialUpdate emit: per owned group, overlay non-null fields in ascending
// (seq, isAdd) order (PartialUpdateMergeFunction.java:188-215 + Reducer
// wrapper bypass). members/group_start written by k_merge_tiles in PU mode.
// run_masks: device array of k per-run packed-validity pointers
// (k_pack_valid), or null for the legacy per-column byte walk (>64 cols).
hipError_t pmh_launch_emit_pu(const DevCol *cols, const uint8_t *col_dtype,
                              const uint8_t *col_nullable, int n_cols, int k,
                              int seq_col, int kind_col, int flags,
                              const uint32_t *members,
                              const uint16_t *group_start,
                              const int64_t *tile_offsets, int64_t n_tiles,
                              int64_t tile_rows, const int64_t *total_out,
                              uint64_t *const *run_masks,
                              void *const *out_ptrs,
                              uint8_t *const *out_valid, hipStream_t stream);

// Pack one run's per-column validity bytes into u64 row masks (bit c =
// column c non-null; columns without staged nulls contribute 1).
hipError_t pmh_launch_pack_valid(const DevCol *cols, int n_cols, int64_t rows,
                                 uint64_t *mask, hipStream_t stream);

// Build one run's order-preserving composite key from <= 8 integer key
// columns whose widths sum to <= 64 bits (spec packed 8 bits per sub-key).
hipError_t pmh_launch_composite(const DevCol *keys, int nk, uint64_t shifts,
                                uint64_t bits, int64_t rows, int64_t *ckey,
                                hipStream_t stream);

// Aggregation emit: per owned group, fold members in ascending (seq, isAdd)
// order through per-column FieldAggregators (AggregateMergeFunction.java:
// 82-125; default last_non_null_value, :201). col_agg holds one PMH_AGG_*
// code per output column. INSERT-only streams in v1 (retracts are detected
// by k_merge_tiles in PU mode and fail the read).
enum {
    PMH_AGG_LAST_NON_NULL = 0,  // FieldLastNonNullValueAgg (the default)
    PMH_AGG_LAST_VALUE = 1,     // FieldLastValueAgg
    PMH_AGG_FIRST_VALUE = 2,    // FieldFirstValueAgg
    PMH_AGG_FIRST_NON_NULL = 3, // FieldFirstNonNullValueAgg
    PMH_AGG_SUM = 4,            // FieldSumAgg
    PMH_AGG_MAX = 5,            // FieldMaxAgg
    PMH_AGG_MIN = 6,            // FieldMinAgg
    PMH_AGG_PRIMARY_KEY = 7,    // FieldPrimaryKeyAgg (agg = retract = input)
};
// col_agg bit 0x80: FieldIgnoreRetractAgg wrapper (fields.<f>.ignore-retract
// = true): retract records leave the accumulator untouched
constexpr uint8_t PMH_AGG_IGNORE_RETRACT = 0x80;
// PartialUpdate with sequence groups (PartialUpdateMergeFunction.java:
// 219-377): per-group last-prefix-max-achiever resolution; retracts null
// their group members. col_group[c] = group id or 0xff; sg_fields packs 4
// sequence-field column indices per group; no per-field aggregators in v1.
hipError_t pmh_launch_emit_pu_sg(
    const DevCol *cols, const uint8_t *col_dtype,
    const uint8_t *col_nullable, int n_cols, int k, int seq_col,
    int kind_col, int flags, const uint8_t *col_group,
    const int16_t *sg_fields, const uint8_t *sg_nseq, int n_groups,
    const uint32_t *members, const uint16_t *group_start,
    const int64_t *tile_offsets, int64_t n_tiles, int64_t tile_rows,
    const int64_t *total_out, uint64_t *const *run_masks,
    void *const *out_ptrs, uint8_t *const *out_valid, hipStream_t stream);

hipError_t pmh_launch_emit_agg(const DevCol *cols, const uint8_t *col_dtype,
                               const uint8_t *col_nullable,
                               const uint8_t *col_agg, int n_cols, int k,
                               int seq_col, int kind_col, int flags,
                               const uint32_t *members,
                               const uint16_t *group_start,
                               const int64_t *tile_offsets, int64_t n_tiles,
                               int64_t tile_rows, const int64_t *total_out,
                               uint64_t *const *run_masks,
                               void *const *out_ptrs,
                               uint8_t *const *out_valid, hipStream_t stream);

hipError_t pmh_launch_dict_gather(const int32_t *ids, const void *dict,
                                  int64_t n, void *out, int esize,
                                  hipStream_t stream);

}  // extern "C"

}  // namespace pmh
