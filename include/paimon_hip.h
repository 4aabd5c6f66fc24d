/* paimon_hip.h — C-ABI of libpaimon_hip.so: the MI355X-native drop-in for
 * Apache Paimon's merge-on-read hot path.
 *
 * Replaced reference surfaces (apache/paimon @ 2026-08-21), per entry point:
 *  - pmh_plan_create + pmh_read_next replace
 *      SplitRead<KeyValue>.createReader(Split) -> RecordReader<KeyValue>
 *      (paimon-core/.../operation/SplitRead.java:39-63) as implemented by
 *      MergeFileSplitRead.createReader / createMergeReader
 *      (paimon-core/.../operation/MergeFileSplitRead.java:242-270), i.e. the
 *      IntervalPartition sectioning (mergetree/compact/IntervalPartition.java:
 *      67-125), per-section sort-merge (mergetree/compact/SortMergeReader.java:
 *      41-57 with the default LOSER_TREE engine), merge functions
 *      (DeduplicateMergeFunction.java:48-62, PartialUpdateMergeFunction.java:
 *      148-397) wrapped by ReducerMergeFunctionWrapper.java:53-73, and
 *      DropDeleteReader.java:53-61.
 *  - The batch contract mirrors RecordReader<T>
 *      (paimon-common/.../reader/RecordReader.java:40-72): pmh_read_next
 *      returns one batch per section (the loser-tree engine yields one batch
 *      per section, SortMergeReaderWithLoserTree.java:77-83); returned
 *      buffers stay valid until the next pmh_read_next / pmh_plan_close on
 *      the same plan (releaseBatch reuse contract). One plan = one HIP
 *      stream; concurrent plans are allowed (one per bucket).
 *  - pmh_write_parquet is the encode half of the compaction surface
 *      (CompactRewriter.rewrite, mergetree/compact/CompactRewriter.java:
 *      29-56): the merge half runs through a plan, the rolling write-back
 *      through this writer (driven by paimon_amd/compact.py in-repo).
 *
 * JNI precedent in the reference: the Vortex JNI reader
 * (paimon-vortex/.../dev/vortex/jni/NativeRuntime.java:30-34) — a Java-side
 * binding of exactly this shape is sketched in INTEGRATION.md.
 *
 * Error model: functions returning pointers return NULL on error; functions
 * returning int/int64 return negative on error. pmh_last_error() returns a
 * thread-local message (mirrors IOException propagation of RecordReader).
 */
#ifndef PAIMON_HIP_H
#define PAIMON_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pmh_session_t pmh_session_t;
typedef struct pmh_plan_t pmh_plan_t;

/* Column dtypes (paimon logical types on the hot path; TINYINT is stored as
 * parquet INT32 and returned here as INT8 — KeyValueSerializer.java:58-66
 * row layout: key cols | _SEQUENCE_NUMBER | _VALUE_KIND | value cols). */
enum pmh_dtype {
    PMH_DT_INT8 = 1,
    PMH_DT_INT16 = 2,
    PMH_DT_INT32 = 3,
    PMH_DT_INT64 = 4,
    PMH_DT_FLOAT32 = 5,
    PMH_DT_FLOAT64 = 6,
    /* Dictionary-backed string column (CHAR/VARCHAR -> parquet BYTE_ARRAY,
     * ParquetSchemaConverter.java:120-128): data = int32 ids into the
     * column's dictionary (dict_data/dict_offsets/dict_len) — the same
     * shape the reference's WritableColumnVector dictionary support and
     * parquet's own dictionary encoding use. DECIMAL(p,s) is not a
     * separate dtype: p <= 9 rides INT32, p <= 18 INT64 (unscaled values,
     * ParquetSchemaConverter.java:153-171) with precision/scale set. */
    PMH_DT_STRING = 7,
    /* BOOLEAN (parquet BOOLEAN / ORC BOOLEAN, ParquetSchemaConverter.java:
     * 126-216, OrcTypeUtil.java:67-114): one byte per row, 0 or 1. */
    PMH_DT_BOOL = 8,
};

/* Logical annotation of an INT32/INT64 column (pmh_col.logical). DATE, TIME
 * and TIMESTAMP are not separate dtypes: like DECIMAL they ride the integer
 * the file stores (ParquetSchemaConverter.java:126-216, 306-323;
 * OrcTypeUtil.java:67-114) and the batch carries the annotation:
 *   date                      INT32 days since 1970-01-01
 *                             (parquet INT32 DATE / ORC DATE)
 *   time                      INT32 milliseconds of the day
 *                             (parquet INT32 TIME MILLIS / ORC INT)
 *   timestamp(p <= 3) [_ltz]  INT64 milliseconds since the epoch
 *   timestamp(4..6)   [_ltz]  INT64 microseconds since the epoch
 *                             (parquet INT64 TIMESTAMP MILLIS|MICROS, ORC
 *                             TIMESTAMP / TIMESTAMP_INSTANT for _ltz)
 * A bare "timestamp" is timestamp(6). Values are handed out as the plain
 * integers, filter literals are those integers (0/1 for booleans), and
 * sequence_fields may name such a column. Limits (plan creation or the read
 * fails, by name): key columns of these types and of boolean; precision
 * above 6 (parquet INT96, sub-microsecond ORC); a parquet file whose
 * physical type, annotation or timestamp unit differs from the declared
 * type's; RLE-encoded parquet booleans (data page v2); RLEv1 (DIRECT) ORC
 * timestamps; an ORC TIMESTAMP writer timezone other than UTC / GMT; ORC
 * timestamps before 1970 with a fractional second, with nanos of 10^9 or
 * more, or outside int64 in the column unit; numeric aggregators (sum, ...)
 * over these types. */
enum pmh_logical {
    PMH_LT_NONE = 0,
    PMH_LT_DATE = 1,
    PMH_LT_TIME_MILLIS = 2,
    PMH_LT_TIMESTAMP_MILLIS = 3,
    PMH_LT_TIMESTAMP_MICROS = 4,
    PMH_LT_TIMESTAMP_LTZ_MILLIS = 5,
    PMH_LT_TIMESTAMP_LTZ_MICROS = 6,
};

typedef struct pmh_col {
    const char *name;
    int32_t dtype;         /* enum pmh_dtype */
    const void *data;      /* columnar values (PMH_DT_STRING: int32 ids);
                              device ptr unless host batch */
    const uint8_t *valid;  /* byte-per-row validity (1=non-null); NULL = all
                              valid. (Arrow bitmap export: later round.) */
    /* PMH_DT_STRING: the column dictionary (HOST-resident even for device
     * batches — it is plan-level metadata built at staging). Entry i =
     * dict_data[dict_offsets[i] .. dict_offsets[i+1]). */
    const void *dict_data;
    const int32_t *dict_offsets;  /* dict_len + 1 entries */
    int32_t dict_len;
    /* DECIMAL annotation on INT32/INT64 columns (0 = plain integer). */
    int32_t precision;
    int32_t scale;
    /* enum pmh_logical on INT32/INT64 columns (0 = none). */
    int32_t logical;
} pmh_col;

typedef struct pmh_batch {
    int64_t n_rows;
    int32_t n_cols;        /* key cols, then seq, kind, then value cols */
    int32_t device;        /* HIP device ordinal; -1 = host-resident copy */
    const pmh_col *cols;
} pmh_batch;

typedef struct pmh_stats {
    int64_t rows_in;         /* records fed to the merge */
    int64_t rows_out;        /* records emitted */
    int64_t hbm_bytes_algo;  /* encoded input bytes staged in HBM */
    double decode_ms;        /* device time in decode kernels */
    double partition_ms;     /* device time in merge-path partition */
    double merge_ms;         /* device time in the tile merge kernel */
    double scan_ms;          /* device time in the tile-offset scan */
    double emit_ms;          /* device time in gather/emit kernels */
    double total_device_ms;  /* end-to-end device time of read_next calls */
    double h2d_ms;           /* untimed-region staging cost, informational */
    int64_t path_mode;       /* 0 = 3-kernel chain, 1 = fused in-kernel
                              * emission, 2 = fused + split value emission */
    int64_t gpu_zstd_pages;  /* pages decompressed by k_zstd_pages */
    double lookup_ms;        /* device time in k_lookup_probe (lookup
                              * changelog producer; not part of merge_ms) */
} pmh_stats;

/* Session: owns the device + stream pool. device < 0 opens a host-only
 * session usable for metadata entry points (footer parse, planning). */
pmh_session_t *pmh_open_session(int device);
void pmh_close_session(pmh_session_t *s);

/* plan_json (one bucket's DataSplit, table/source/DataSplit.java:63-75):
 * {
 *   "key_cols":   [{"name": "_KEY_k", "type": "int64"}],
 *   "value_cols": [{"name": "v_k", "type": "int64"}, ...],   // read type
 *       // types: tinyint..bigint, float, double, string, decimal(p,s),
 *       // boolean, date, time, timestamp(p), timestamp_ltz(p) (enum
 *       // pmh_logical says how the last four ride integers)
 *   "merge_engine": "deduplicate" | "partial-update",
 *   "drop_delete": true,         // !forceKeepDelete
 *   "ignore_delete": false,      // CoreOptions.IGNORE_DELETE
 *   "output": "device" | "host",
 *   "files": [{"path": "...", "rowCount": N, "minKey": x, "maxKey": y,
 *              "level": L}, ...]                              // DataFileMeta
 *   // optional changelog stream (served by pmh_changelog_next):
 *   "changelog_producer": "none" | "full-compaction" | "lookup",
 *   "changelog_row_deduplicate": false,
 *   "max_level": N,              // full-compaction only (num-levels - 1)
 *   "lookup_files": [...]        // lookup only; same shape as "files"
 * }
 * changelog_producer = "lookup" (LookupChangelogMergeFunctionWrapper.java:
 * 104-163 over LookupMergeFunction.java:66-135, deduplicate engine): "files"
 * are the compaction's inputs (level 0 plus any upper-level members) and
 * "lookup_files" the data files of the levels ABOVE the compaction's output
 * level (outputLevel+1 .. maxLevel, LookupMergeTreeCompactRewriter.java:
 * 211-219). They group by level into one sorted run per level, are staged
 * once and stay device-resident across sections and pmh_plan_reset; a key
 * group without an upper-level member is looked up in them, lowest level
 * first (LookupUtils.java:35-57). Absent/empty lookup_files = empty upper
 * tree. Limits (plan creation fails otherwise): runs of a section + lookup
 * levels <= 32; each lookup level < 2^27 rows; every lookup level above
 * every level in "files"; files of one lookup level key-disjoint;
 * deduplicate engine only; a single integer key column; no ignore_delete,
 * no sequence fields, no PMH_FUSED=1, no deletionVector on a lookup file.
 * Staging (file read + H2D of encoded column chunks + descriptors) happens
 * here; pmh_read_next launches only device work. */
pmh_plan_t *pmh_plan_create(pmh_session_t *s, const char *plan_json);

/* Returns rows in the batch (one section per call), 0 at end of input,
 * negative on error. Batch buffers valid until next call / plan close. */
int64_t pmh_read_next(pmh_plan_t *p, pmh_batch *out);

int pmh_plan_close(pmh_plan_t *p);

/* Rewind the plan to its first section without restaging: the next
 * pmh_read_next re-runs the full device pipeline on the resident encoded
 * data. Used by benchmarks to repeat the timed region; stats accumulate. */
/* Changelog batch of the LAST pmh_read_next (changelog_producer =
 * "full-compaction" in the plan JSON, with "max_level" and optional
 * "changelog_row_deduplicate"): the FullChangelogMergeFunctionWrapper
 * stream (INSERT / UPDATE_BEFORE / UPDATE_AFTER / DELETE rows in key
 * order, same schema as the main batch) for every merge engine. With
 * partial-update and aggregation an UPDATE_BEFORE / DELETE row carries the
 * max-level record's own key, sequence number and values, an INSERT /
 * UPDATE_AFTER row the folded row exactly as the main batch holds it (key,
 * last member's sequence number, values, validity); rows do not depend on
 * drop_delete; row-deduplicate compares the max-level record with the
 * folded row, validity first, then the stored bits. Those two engines
 * refuse ignore_delete with this producer, and a section whose runs x
 * columns exceed the changelog kernels' 48 KB column table (16 bytes per
 * run and column). changelog_producer = "lookup"
 * serves the LookupChangelogMergeFunctionWrapper stream the same way; a row
 * built from a looked-up record carries that record's key, sequence number
 * and values. Valid until the next read_next. Returns row count or < 0. */
int64_t pmh_changelog_next(pmh_plan_t *plan, pmh_batch *out);

int pmh_plan_reset(pmh_plan_t *p);

int pmh_stats_get(pmh_plan_t *p, pmh_stats *out);

const char *pmh_last_error(void);

/* ---- host-only debug/metadata entry points (no GPU required) ---- */

/* Parse a parquet footer + page headers; returns a malloc'd JSON string
 * (caller frees with pmh_free_string). Used by CPU tests to pin the native
 * thrift parser against pyarrow metadata. */
char *pmh_debug_footer_json(const char *path);
void pmh_free_string(char *s);

/* Check one column of a data file against a declared plan type ("boolean",
 * "date", "time", "timestamp(3)", ...) the way staging does, without a plan
 * or a GPU: Parquet physical type, DATE / TIME / TIMESTAMP annotation and
 * unit, boolean page encodings; ORC type kind and, for TIMESTAMP, each
 * stripe's writer timezone. Returns 0, or -1 with pmh_last_error() set to
 * the text plan creation would fail with. */
int pmh_debug_check_column(const char *path, const char *column,
                           const char *type);

/* Write a Parquet v1 data file (PLAIN pages) from HOST columnar
 * buffers — the compaction write-back half of the CompactRewriter surface
 * (what KeyValueDataFileWriter + the vendored parquet-mr writer do in the
 * reference, io/KeyValueDataFileWriter.java:121-170). cols[i].data/valid
 * are host pointers at the column's output width (TINYINT/SMALLINT widen to
 * the INT32 physical type on write, matching the read path). PMH_DT_BOOL
 * columns (one 0/1 byte per row) are written as BOOLEAN, PLAIN, bit-packed
 * LSB first; cols[i].logical on INT32/INT64 columns writes the DATE /
 * TIME(MILLIS) / TIMESTAMP(MILLIS|MICROS) annotation as both converted_type
 * and logicalType, isAdjustedToUTC set for the _LTZ values. No GPU
 * required. row_group_rows/page_rows <= 0 pick defaults (1M / 64k).
 * compression: NULL or "NONE" for uncompressed, "zstd" for ZSTD pages.
 * Returns 0, or -1 with pmh_last_error() set. */
int pmh_write_parquet(const pmh_col *cols, int32_t n_cols, int64_t n_rows,
                      const char *path, int64_t row_group_rows,
                      int64_t page_rows, const char *compression);

/* Raw snappy block decode (the library's from-scratch decoder, used for
 * SNAPPY parquet pages / ORC chunks). Returns decompressed size or -1 with
 * pmh_last_error() set. Exposed so CPU tests can pin the decoder against an
 * independent compressor. */
int64_t pmh_debug_snappy(const void *src, int64_t n, void *dst, int64_t cap);

/* Decode one zstd frame with the from-scratch scalar core (zstd_core.h,
 * RFC 8878 restatement) on the host — test/validation entry for the GPU
 * page decoder which shares the same core. Returns bytes or < 0. */
int64_t pmh_debug_zstd_cpu(const void *src, int64_t n, void *dst,
                           int64_t cap);

/* Decode one zstd frame ON THE GPU (k_zstd_pages batch of 1); `expected`
 * is the known decompressed size. Returns expected or < 0. */
int64_t pmh_debug_zstd_gpu(const void *src, int64_t n, void *dst,
                           int64_t expected);

/* Compress one frame with the from-scratch encoder (scalar core; the GPU
 * page compressor shares it). Returns compressed bytes or < 0. */
int64_t pmh_debug_zstd_enc_cpu(const void *src, int64_t n, void *dst,
                               int64_t cap);

/* Same, on the GPU (k_zstd_compress batch of 1). */
int64_t pmh_debug_zstd_enc_gpu(const void *src, int64_t n, void *dst,
                               int64_t cap);

/* Decode one ORC integer stream through the product's own decoders, so
 * tests can force every sub-encoding, width and alignment instead of taking
 * what a file writer happens to pick.
 *   kind: 0 = RLEv2 signed, 1 = RLEv2 unsigned, 2 = byte-RLE (tinyint).
 *   mode 0, host twin (no GPU): the host decoder that reads string LENGTH
 *     streams; kind 1 only. n_values < 0 decodes until the stream is
 *     exhausted (the DICTIONARY_V2 LENGTH call). Writes up to out_cap
 *     uint64 values to `out`; returns the number of values decoded.
 *   mode 1, prescan only (no GPU): walks the stream into device work chunks
 *     against a dummy device base; returns the number of chunks. `out` is
 *     unused.
 *   mode 2, device path: uploads the stream as staging does (16-byte tail
 *     pad) at src_shift (0..7) bytes past an 8-byte-aligned device address,
 *     prescans, launches k_rlev2 once over all chunks and copies n_values
 *     elements of out_esize (4 or 8) bytes to `out` (out_cap >= n_values
 *     elements). The device output sits between two 64-element guard zones
 *     and is pre-filled, like them, with the byte 0xA5, so an element the
 *     kernel never wrote reads back as 0xA5A5... Returns n_values. Owns its
 *     device memory; needs no session.
 * Returns -1 with pmh_last_error() set on a malformed or truncated stream,
 * bad arguments or a HIP error, and -2 when the kernel changed a guard
 * zone (the output is still copied out). */
int64_t pmh_debug_orc_ints(const void *stream, int64_t len, int64_t n_values,
                           int kind, int out_esize, int mode,
                           int64_t src_shift, void *out, int64_t out_cap);

/* Decode one ORC DECIMAL DATA stream (zigzag base-128 varints of the
 * unscaled values) through the product's own decoder, so tests can force
 * every value length, alignment and scale instead of taking what a file
 * writer happens to pick.
 *   scales: n_values per-value data scales (what the SECONDARY stream holds
 *     once decoded), or NULL when every value already has the column scale.
 *   precision, scale: the column's. precision 1..18 as a plan may declare,
 *     or 19 = the whole int64 range (10^19 > 2^63), which lets a stream hold
 *     the 10-byte values no decimal(p <= 18) column can.
 *   mode 0, host (no GPU): the staging prescan plus the scalar core the
 *     kernel shares (orc_decimal_core.h).
 *   mode 2, device path: uploads the stream as staging does (16-byte tail
 *     pad) at src_shift (0..7) bytes past an 8-byte-aligned device address,
 *     prescans, launches k_orc_varint once over all units. The device output
 *     sits between two 64-element guard zones and is pre-filled, like them,
 *     with the byte 0xA5. Owns its device memory; needs no session.
 * Writes n_values elements of out_esize (4 or 8) bytes to `out` (out_cap >=
 * n_values elements) and returns n_values. Returns -1 with pmh_last_error()
 * set on a malformed or truncated stream, a value the column cannot hold
 * (data scale above the column scale or negative, magnitude of 10^precision
 * or more, outside int32 at out_esize 4), bad arguments or a HIP error, and
 * -2 when the kernel changed a guard zone (the output is still copied). */
int64_t pmh_debug_orc_decimal(const void *data, int64_t len,
                              const int32_t *scales, int precision,
                              int scale, int64_t n_values, int out_esize,
                              int mode, int64_t src_shift, void *out,
                              int64_t out_cap);

/* Expand one BOOLEAN value stream through the product's own decoder
 * (bits_core.h, k_bits_expand), so tests can force every unit shape and
 * alignment instead of taking what a file writer happens to pick.
 *   format 0: raw literal bits, as a Parquet PLAIN page payload holds them
 *     (bit_order 0 = LSB first is Parquet's; 1 = MSB first is accepted too);
 *     format 1: ORC boolean byte-RLE (runs and literal groups; bit_order 1 =
 *     MSB first is ORC's).
 *   out_esize: 1 (one byte per value) or 4 (the staged column width).
 *   out_shift 0..7: the output starts this many ELEMENTS past an address
 *     aligned to 8 elements, so the unit edges fall on every residue.
 *   mode 0, host (no GPU): the staging prescan plus the scalar core the
 *     kernel shares, over the same group geometry.
 *   mode 2, device path: uploads the stream as staging does (16-byte tail
 *     pad) at src_shift (0..7) bytes past an 8-byte-aligned device address,
 *     prescans, launches k_bits_expand once over all units. The device
 *     output sits between two 64-element guard zones and is pre-filled,
 *     like them, with the byte 0xA5. Owns its device memory; needs no
 *     session.
 * Writes n_values elements of out_esize bytes to `out` (out_cap >= n_values
 * elements) and returns n_values. Returns -1 with pmh_last_error() set on a
 * truncated stream, bad arguments or a HIP error, and -2 when the kernel
 * changed a guard zone (the output is still copied). */
int64_t pmh_debug_bits(const void *stream, int64_t len, int64_t n_values,
                       int bit_order, int format, int out_esize, int mode,
                       int64_t src_shift, int64_t out_shift, void *out,
                       int64_t out_cap);

/* Decode one ORC TIMESTAMP column's stream pair through the product's own
 * decoders: DATA (signed RLEv2 seconds relative to 2015-01-01 UTC) and
 * SECONDARY (unsigned RLEv2 nanoseconds, trailing zeros removed).
 *   unit 0: INT64 milliseconds (timestamp(p <= 3)); 1: microseconds.
 *   mode 0, host (no GPU): the host RLEv2 restatement plus the scalar core
 *     the kernel shares (orc_timestamp_core.h).
 *   mode 2, device path: both streams upload as staging does, decode through
 *     k_rlev2 (the nanos into a scratch) and combine in k_orc_timestamp. The
 *     device output sits between two 64-element guard zones pre-filled with
 *     0xA5. Owns its device memory; needs no session.
 * Writes n_values int64 to `out` (out_cap >= n_values) and returns
 * n_values. Returns -1 with pmh_last_error() set on a malformed stream, bad
 * arguments, a HIP error or a refused value ("ORC timestamp refused: ..."
 * naming a value before 1970 with a fractional second, nanos of 10^9 or
 * more, or a result outside int64), and -2 when a kernel changed a guard
 * zone. */
int64_t pmh_debug_orc_timestamp(const void *data, int64_t data_len,
                                const void *secondary, int64_t secondary_len,
                                int64_t n_values, int unit, int mode,
                                void *out, int64_t out_cap);

/* Parse one deletion vector from a DV index file slice (DeletionFile
 * {path, offset, length}; BitmapDeletionVector.java:98-112 wrapper around
 * the portable Roaring serialization). Writes up to `cap` deleted
 * positions ascending; returns the total count or -1. CPU-only debug
 * entry pinning the parser against independently-serialized fixtures. */
int64_t pmh_debug_parse_dv(const char *path, int64_t offset, int64_t length,
                           int64_t *out, int64_t cap);

/* Point lookup into sorted levels on the host, through the same search core
 * k_lookup_probe runs on the device (lookup_core.h): level_keys[l] holds
 * level_rows[l] ascending unique int64 keys. Per query, out_level gets the
 * index of the FIRST level holding the key (levels are searched in array
 * order, LookupUtils.java:35-57) and out_row the row inside it; both -1
 * when no level holds it. Returns 0, or -1 with pmh_last_error() set. */
int pmh_debug_lookup_probe(int n_levels, const int64_t *const *level_keys,
                           const int64_t *level_rows, const int64_t *queries,
                           int64_t n_queries, int32_t *out_level,
                           int64_t *out_row);

/* The full-compaction changelog decision table on the host, through the same
 * core the partial-update / aggregation walk of k_merge_tiles runs on the
 * device (changelog_core.h, FullChangelogMergeFunctionWrapper.java:96-126).
 * Per key group g: nlive[g] >= 1 live records, n_top[g] of them from a
 * max-level run (0 <= n_top <= nlive), merged_is_add[g] != 0 when the
 * wrapper's result is an add (the lone record itself when nlive == 1).
 * pending != 0 = changelog-producer.row-deduplicate is on. Writes out_n[g] =
 * 0, 1 or 2 changelog rows and their RowKinds to out_kinds[2g], [2g + 1]
 * (0 INSERT, 1 UPDATE_BEFORE, 2 UPDATE_AFTER, 3 DELETE; -1 = no row).
 * Optional (may be NULL): out_after_is_merged[g] = the last row carries the
 * merged result (otherwise every row carries the top-level record);
 * out_pending[g] = the pair still awaits the value-equality check that may
 * drop it. Returns 0, or -1 with pmh_last_error() set. */
int pmh_debug_changelog_decide(int64_t n_groups, const int32_t *nlive,
                               const int32_t *n_top,
                               const uint8_t *merged_is_add, int pending,
                               int32_t *out_n, int8_t *out_kinds,
                               uint8_t *out_after_is_merged,
                               uint8_t *out_pending);

/* The merge-path partition on its own: k runs of ascending unique keys
 * (keys[r] holds lens[r] elements of key_width 4 = int32 or 8 = int64; an
 * empty run may pass a null pointer). cuts_out receives n_bounds * k entries,
 * n_bounds = ceil(total / tile_rows) + 1: cuts_out[b * k + r] is the number
 * of run r's rows among the first min(b * tile_rows, total) rows ordered by
 * (key, run index). mode 0 walks the shared search core (partition_core.h)
 * on the host, bound by bound; mode 1 copies the runs to the device, calls
 * pmh_launch_partition the way pmh_read_next does and copies the cuts back —
 * only the partition kernels run. Returns 0, or -1 with pmh_last_error()
 * set. */
int pmh_debug_partition(int k, const void *const *keys, const int64_t *lens,
                        int key_width, int64_t tile_rows, int mode,
                        int32_t *cuts_out);

/* Which kernel the last winner emit of this process ran: 0 none yet, 1
 * k_emit (gathers, descriptors in global memory), 2 k_emit_contig (gathers,
 * descriptors in LDS), 3 k_emit_stream (tile slices streamed through LDS).
 * Lets a test tell a streamed read from a fallback. */
int pmh_debug_last_emit_kernel(void);

/* Which partial-update emit kernel the last read of this process launched: 0
 * none yet, 1 k_emit_pu (no sequence groups), 2 k_emit_pu_sg (sequence
 * groups, no aggregate functions), 3 k_emit_pu_sga (aggregate functions on
 * group fields). */
int pmh_debug_last_pu_emit_kernel(void);

/* One key group through the partial-update fold with aggregate functions
 * inside sequence groups, on the host, through the same core k_emit_pu_sga
 * runs on the device (pu_agg_core.h; PartialUpdateMergeFunction.java
 * :149-397 and the FieldAggregators). The group has n_members (1..32)
 * records in ascending (sequence number, isAdd) order: kinds[x] is member
 * x's RowKind byte; values[x * n_cols + c] its field c as 64 bits (integers
 * sign-extended, FLOAT32 the raw 32 bits sign-extended, FLOAT64 the raw
 * bits) and valid[x * n_cols + c] != 0 when it is non-null. dtypes[c] is a
 * pmh_dtype code. Sequence groups as in the plan: col_group[c] = group id or
 * 0xff, sg_fields[g * 4 + j] = group g's sequence-field columns, sg_nseq[g]
 * of them (1..4). col_agg[c] = 0 last_non_null_value, 1 last_value, 2
 * first_value, 3 first_non_null_value, 4 sum, 5 max, 6 min, | 0x80 for
 * ignore-retract, or 0xff for no aggregate function. Writes the merged row
 * to out_values / out_valid ([n_cols]), the result RowKind to *out_kind (a
 * single member passes through with its own), the index of the member whose
 * sequence number the result carries to *out_last (-1: none, the number is
 * 0) and to *out_unsupported whether a retract met an aggregate function
 * without retraction. Returns 0, or -1 with pmh_last_error() set. */
int pmh_debug_pu_agg_fold(int n_members, const int8_t *kinds, int n_cols,
                          const uint8_t *dtypes, const int64_t *values,
                          const uint8_t *valid, int n_groups,
                          const uint8_t *col_group, const int16_t *sg_fields,
                          const uint8_t *sg_nseq, const uint8_t *col_agg,
                          int ignore_delete, int64_t *out_values,
                          uint8_t *out_valid, int32_t *out_kind,
                          int32_t *out_last, int32_t *out_unsupported);

/* Parse one JSON number the way the plan descriptor's numbers are parsed
 * (minKey/maxKey, rowCount, integer filter literals): a token without '.',
 * 'e' or 'E' is an exact int64, a fractional token rounds to nearest, an
 * integer outside int64 is an error. Writes the value to *out; returns 0,
 * or -1 with pmh_last_error() set. CPU-only debug entry pinning the parser
 * over the whole int64 range. */
int pmh_debug_json_i64(const char *text, int64_t *out);

/* Restatement of IntervalPartition.partition() for int64 keys
 * (mergetree/compact/IntervalPartition.java:67-125): given n files'
 * (minKey, maxKey), writes section id and run-within-section id per file
 * (by input order). Returns number of sections, or negative on error. */
int pmh_debug_interval_partition(int n, const int64_t *min_keys,
                                 const int64_t *max_keys,
                                 int32_t *out_section, int32_t *out_run);

#ifdef __cplusplus
}
#endif
#endif /* PAIMON_HIP_H */
