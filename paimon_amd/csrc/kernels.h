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

// ------------------------------------------------------------ merge flag word
// The `flags` argument of the merge and folding-emit launchers. The plan
// builds its engine bits once at creation; the profiling fields are added per
// read from the environment. Every launcher of a read gets the same word: the
// folding emit kernels read only RROD, IGNORE_DELETE and AGG_RETRACT from it.
constexpr int PMH_FLAG_DROP_DELETE = 1 << 0;    // drop groups that end deleted
constexpr int PMH_FLAG_IGNORE_DELETE = 1 << 1;  // skip retract records
constexpr int PMH_FLAG_MEMBERS = 1 << 2;   // member lists (partial-update /
                                           // aggregation) instead of winners
constexpr int PMH_FLAG_FIRST_ROW = 1 << 3;      // first-row engine
constexpr int PMH_FLAG_RROD = 1 << 4;           // remove-record-on-delete
constexpr int PMH_FLAG_SEQ_GROUPS = 1 << 5;     // sequence groups
constexpr int PMH_FLAG_AGG_RETRACT = 1 << 6;    // every aggregator retracts
constexpr int PMH_FLAG_CL_ROW_DEDUP = 1 << 7;   // changelog row-deduplicate
// profiling-only fields, (flags >> SHIFT) & MASK:
constexpr int PMH_FLAG_ABLATE_SHIFT = 8;   // PMH_ABLATE: k_merge_tiles phases
constexpr int PMH_FLAG_ABLATE_MASK = 0xf;
constexpr int PMH_FLAG_FABL_SHIFT = 12;    // PMH_FABL: k_merge_emit phases
constexpr int PMH_FLAG_FABL_MASK = 0x3;
constexpr int PMH_FLAG_FSTAGE_SHIFT = 14;  // PMH_FSTAGE: LDS-staged emission
constexpr int PMH_FLAG_FSTAGE_MASK = 1;
// lookup changelog producer (LookupChangelogMergeFunctionWrapper): the lookup
// walk of k_merge_tiles. The run tables then hold RunSet::n_slots > k slots
// (the lookup levels after the k merge runs) and the probe words come from
// pmh_launch_lookup_probe.
constexpr int PMH_FLAG_LOOKUP = 1 << 15;
// full-compaction changelog of a folding engine: the changelog walk of the
// member-list k_merge_tiles (see pmh_launch_cl_finalize_out)
constexpr int PMH_FLAG_FOLD_CL = 1 << 16;

// ----------------------------------------------------------- device error word
// One uint32 per section (TileSet::err), OR-ed by the kernels and read back
// after every pass. Bits 0-4 are the merge and emit kernels'; the ORC decode bits sit
// above them (ODC_ERR_*, orc_decimal_core.h; OTS_ERR_*, orc_timestamp_core.h).
constexpr uint32_t PMH_ERR_RETRACT = 1u << 0;       // engine rejects retracts
constexpr uint32_t PMH_ERR_FIRST_ROW_RETRACT = 1u << 1;
constexpr uint32_t PMH_ERR_LOOKBACK = 1u << 2;      // fused lookback timed out
constexpr uint32_t PMH_ERR_TOP_LEVEL_DUP = 1u << 3; // two max_level records
// partial-update: a retract reached an aggregate function without retract()
constexpr uint32_t PMH_ERR_PU_AGG_RETRACT = 1u << 4;

// ------------------------------------------------------- launcher arguments
// Plain views of device memory the plan owns. A Section and the plan hold
// them filled; a launcher takes the ones its kernel reads and unpacks them
// into the kernel's argument list.

// A section's sorted runs: [n_slots] tables, the k merge runs first.
struct RunSet {
    const DevCol *keys = nullptr;   // merge comparand (a packed composite
                                    // key column for multi-column keys)
    const DevCol *seqs = nullptr;
    const DevCol *kinds = nullptr;
    const DevCol *cols = nullptr;   // [n_slots * n_cols] run-major
    int64_t *lens = nullptr;
    const uint64_t *tombs = nullptr;   // per-run tombstone bytes, or null
    const uint8_t *levels = nullptr;   // per-run level (changelog plans)
    uint64_t *const *masks = nullptr;  // [k] packed row validity (k_pack_valid;
                                       // folding engines), or null: walk the
                                       // per-column bytes (> 64 columns)
    int k = 0;        // merge runs
    int n_slots = 0;  // k + lookup-level slots a winner word can name
    int n_cols = 0;
    // runs [lo, lo + n) as a set of their own (hierarchical batches)
    RunSet sub(int lo, int n) const {
        RunSet r = *this;
        r.keys += lo;
        r.seqs += lo;
        r.kinds += lo;
        r.cols += (size_t)lo * n_cols;
        r.lens += lo;
        if (tombs) r.tombs += lo;
        if (levels) r.levels += lo;
        if (masks) r.masks += lo;
        r.k = r.n_slots = n;
        return r;
    }
};

// The plan's columns: key..., seq, kind, value...
struct ColumnSet {
    const uint8_t *dtype = nullptr;     // [n_cols] pmh_dtype codes
    const uint8_t *nullable = nullptr;  // [n_cols] 1 = has a validity output
    const uint8_t *agg = nullptr;       // [n_cols] PMH_AGG_* (aggregation)
    const int16_t *useq = nullptr;      // [n_useq] sequence.field columns
    int n_useq = 0;
    int any_nullable = 0;  // some column is nullable
    int n_cols = 0;
    int n_key_cols = 1;
    int seq_col() const { return n_key_cols; }
    int kind_col() const { return n_key_cols + 1; }
    int first_val() const { return n_key_cols + 2; }
    // the single key column, -1 for composite keys (their key columns emit
    // through the generic column path)
    int key_col() const { return n_key_cols > 1 ? -1 : 0; }
};

// partial-update sequence groups: col_group[c] = group id or 0xff; fields
// packs 4 sequence-field column indices per group. With aggregate functions
// on group fields (col_agg != nullptr): grp_cols[grp_off[g] .. grp_off[g + 1])
// lists group g's fields that are no sequence fields, and col_agg[c] is the
// column's PMH_AGG_* code (| PMH_AGG_IGNORE_RETRACT) or 0xff for none.
struct SeqGroupSet {
    const uint8_t *col_group = nullptr;
    const int16_t *fields = nullptr;
    const uint8_t *nseq = nullptr;
    int n_groups = 0;
    const int16_t *grp_cols = nullptr;
    const uint16_t *grp_off = nullptr;
    const uint8_t *col_agg = nullptr;
};

// A section's tile state. Every tile holds PMH_TILE_ROWS merged rows.
struct TileSet {
    int32_t *cuts = nullptr;        // [(n_tiles + 1) * k] partition cuts
    int64_t n_tiles = 0;
    uint32_t *winners = nullptr;    // packed (run, row) winners / members
    int32_t *counts = nullptr;      // [n_tiles] rows out per tile
    int64_t *offsets = nullptr;     // [n_tiles] exclusive scan of counts
    int64_t *total = nullptr;       // rows out
    uint16_t *group_start = nullptr;  // member-list group offsets
    uint32_t *err = nullptr;        // the section's error word (PMH_ERR_*)
    // fused path: per-tile lookback words and the tile ticket (zeroed before
    // every launch), dense winner list of the split mode
    uint64_t *status = nullptr;
    uint64_t *ticket = nullptr;
    uint32_t *dense_winners = nullptr;
    // the first n tiles, counting their rows into total_out
    TileSet first(int64_t n, int64_t *total_out) const {
        TileSet t = *this;
        t.n_tiles = n;
        t.total = total_out;
        return t;
    }
};

// One output batch: [n_cols] device arrays of column pointers
struct OutputSet {
    void *const *ptrs = nullptr;
    uint8_t *const *valid = nullptr;  // null entries: column never null
};

// Changelog chain state of a section (both producers)
struct ChangelogSet {
    uint64_t *entries = nullptr;  // 2 slots per group, provisional
    uint64_t *rows = nullptr;     // compacted rows (k_cl_finalize*)
    int32_t *counts = nullptr;
    int64_t *offsets = nullptr;
    int64_t *total = nullptr;
    int max_level = 0;
};

// Lookup probe words of a section: off[r] >= 0 is the word offset of run r's
// first row, < 0 means run r is not probed (not level 0)
struct ProbeSet {
    const int64_t *off = nullptr;
    uint32_t *words = nullptr;
    int n_levels = 0;
    int64_t max_rows = 0;  // longest probed run
};

// Grid of a grid-stride launch over `want` work items: one block each, at
// least 1 and at most `cap` (4096 unless the kernel says otherwise).
inline int pmh_grid(int64_t want, int cap = 4096) {
    return want < cap ? (int)(want > 0 ? want : 1) : cap;
}

// ------------------------------------------------------------------ launchers
// Internal to the library (the exported C ABI is include/paimon_hip.h). A
// merge / emit / changelog launcher takes the argument structs its kernel
// reads, the flag word where the kernel has one, and the stream.

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
// rows (evaluating row-deduplicate value equality); emit gathers them into
// the changelog batch `out2`.
hipError_t pmh_launch_cl_finalize(const RunSet &runs, const ColumnSet &columns,
                                  const TileSet &tiles, const ChangelogSet &cl,
                                  hipStream_t stream);
hipError_t pmh_launch_cl_emit(const RunSet &runs, const ColumnSet &columns,
                              const TileSet &tiles, const ChangelogSet &cl,
                              const OutputSet &out2, hipStream_t stream);

// The same chain for the folding engines (partial-update / aggregation),
// whose after-type rows are the engine's folded result: PMH_FLAG_FOLD_CL
// selects the changelog walk of the member-list k_merge_tiles, whose
// after-type entries name the main-output row tiles.offsets[tile] + g
// (changelog_core.h). Both kernels therefore run after the engine's emit
// kernel on the same stream and read `out` (the plan's main output); emit
// writes `out2`. They stage pmh_fold_cl_lds(k, n_cols) bytes of per-run column
// tables in LDS; the launchers return hipErrorInvalidValue past
// PMH_FOLD_CL_LDS_MAX (plan creation refuses such a section first).
constexpr int64_t PMH_FOLD_CL_LDS_MAX = 48 * 1024;
constexpr int64_t pmh_fold_cl_lds(int64_t k, int64_t n_cols) {
    return 16 * k * n_cols + 32 * n_cols + ((n_cols + 7) & ~(int64_t)7);
}
hipError_t pmh_launch_cl_finalize_out(const RunSet &runs,
                                      const ColumnSet &columns,
                                      const TileSet &tiles,
                                      const ChangelogSet &cl,
                                      const OutputSet &out,
                                      hipStream_t stream);
hipError_t pmh_launch_cl_emit_out(const RunSet &runs, const ColumnSet &columns,
                                  const TileSet &tiles, const ChangelogSet &cl,
                                  const OutputSet &out, const OutputSet &out2,
                                  hipStream_t stream);

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

// Tile merge: winners (or member lists, PMH_FLAG_MEMBERS) and per-tile
// counts into `tiles`. cl / probe are the section's changelog and lookup
// state; a plan without them passes them empty.
hipError_t pmh_launch_merge_tiles(const RunSet &runs, const TileSet &tiles,
                                  int flags, const ChangelogSet &cl,
                                  const ProbeSet &probe, hipStream_t stream);

// k_lookup_probe: for every row of the section's level-0 runs (ProbeSet::off),
// the packed (slot, row) of the first lookup level — slots k .. n_slots - 1,
// lowest level first — that holds the row's key, or 0xFFFFFFFF.
hipError_t pmh_launch_lookup_probe(const RunSet &runs, const ProbeSet &probe,
                                   hipStream_t stream);

hipError_t pmh_launch_scan_tiles(const int32_t *tile_counts, int64_t n_tiles,
                                 int64_t *tile_offsets, int64_t *total_out,
                                 hipStream_t stream);

// FUSED merge + emit (deduplicate / first-row): ticket-ordered persistent
// workgroups, decoupled-lookback output offsets (packed agent-scope atomic
// per tile in tiles.status, zeroed before launch along with tiles.ticket),
// emission from LDS-staged columns. Replaces merge_tiles + scan_tiles + emit
// for non-member-list engines; one launch covers tiles [0, n_tiles).
hipError_t pmh_launch_merge_emit(const RunSet &runs, const ColumnSet &columns,
                                 const TileSet &tiles, int flags,
                                 const OutputSet &out, hipStream_t stream);

// SPLIT-mode value emission: gathers value columns by the densely-written
// packed winners (k_merge_emit with tiles.dense_winners != null emitted key/
// seq/kind and the winner list; this kernel runs at full occupancy, no LDS).
hipError_t pmh_launch_emit_dense(const RunSet &runs, const ColumnSet &columns,
                                 const TileSet &tiles, const OutputSet &out,
                                 hipStream_t stream);

// The kernel the last pmh_launch_emit chose.
enum {
    PMH_EMIT_NONE = 0,
    PMH_EMIT_GATHER = 1,  // k_emit
    PMH_EMIT_CONTIG = 2,  // k_emit_contig
    PMH_EMIT_STREAM = 3,  // k_emit_stream
};
int pmh_last_emit_kernel();

// Winner gather. A winner word can name any of runs.n_slots run slots (the k
// merge runs plus a lookup plan's level slots). Plans without lookup slots
// (n_slots == k) and without nullable columns stream their tile slices
// through LDS (k_emit_stream, PMH_EMIT_STREAM=0 turns it off); other plans
// whose descriptor table fits LDS run k_emit_contig; the rest, and
// PMH_EMIT_LEGACY=1, run k_emit, which reads its descriptors from global
// memory.
hipError_t pmh_launch_emit(const RunSet &runs, const ColumnSet &columns,
                           const TileSet &tiles, const OutputSet &out,
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
// wrapper bypass). Members / group_start written by k_merge_tiles under
// PMH_FLAG_MEMBERS.
hipError_t pmh_launch_emit_pu(const RunSet &runs, const ColumnSet &columns,
                              const TileSet &tiles, int flags,
                              const OutputSet &out, hipStream_t stream);

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
// 82-125; default last_non_null_value, :201). columns.agg holds one PMH_AGG_*
// code per output column. INSERT-only streams in v1 (retracts are detected
// by k_merge_tiles in member-list mode and fail the read).
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
// their group members (SeqGroupSet). groups.col_agg set: some group field
// carries an aggregate function, and k_emit_pu_sga folds every member
// (pu_agg_core.h); its refused retractions land in tiles.err.
hipError_t pmh_launch_emit_pu_sg(const RunSet &runs, const ColumnSet &columns,
                                 const SeqGroupSet &groups,
                                 const TileSet &tiles, int flags,
                                 const OutputSet &out, hipStream_t stream);

hipError_t pmh_launch_emit_agg(const RunSet &runs, const ColumnSet &columns,
                               const TileSet &tiles, int flags,
                               const OutputSet &out, hipStream_t stream);

// Which partial-update emit kernel the last pmh_launch_emit_pu /
// pmh_launch_emit_pu_sg call chose (tests pin the selection)
enum {
    PMH_PU_EMIT_NONE = 0,
    PMH_PU_EMIT_OVERLAY = 1,  // k_emit_pu
    PMH_PU_EMIT_SG = 2,       // k_emit_pu_sg
    PMH_PU_EMIT_SGA = 3,      // k_emit_pu_sga
};
int pmh_last_pu_emit_kernel();

hipError_t pmh_launch_dict_gather(const int32_t *ids, const void *dict,
                                  int64_t n, void *out, int esize,
                                  hipStream_t stream);

}  // namespace pmh
