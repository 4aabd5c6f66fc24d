// libpaimon_hip host side: session/plan lifecycle, planning
// (IntervalPartition restatement), file staging (footer parse, page tables,
// H2D of encoded column chunks), and the read_next device pipeline.
//
// Replaces, for this path, MergeFileSplitRead.createReader
// (paimon-core/.../operation/MergeFileSplitRead.java:242-270) +
// MergeTreeReaders (mergetree/MergeTreeReaders.java:40-102) +
// KeyValueFileReaderFactory (io/KeyValueFileReaderFactory.java:127-209).
// The KeyValue row layout contract (key cols | _SEQUENCE_NUMBER |
// _VALUE_KIND | value cols) follows KeyValueSerializer.java:34-99.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <fstream>
#include <memory>
#include <queue>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/paimon_hip.h"
#include "changelog_core.h"
#include "codec.h"
#include "column_core.h"
#include "zstd_core.h"
#include <map>
#include "common.h"
#include "json.h"
#include "kernels.h"
#include "lookup_core.h"
#include "orc_meta.h"
#include "parquet_meta.h"
#include "parquet_write.h"
#include "partition_core.h"
#include "pu_agg_core.h"

#include <dlfcn.h>

namespace pmh {

std::string &last_error() {
    thread_local std::string e;
    return e;
}

#define HIP_TRY(expr)                                                     \
    do {                                                                  \
        hipError_t _e = (expr);                                           \
        if (_e != hipSuccess) {                                           \
            set_error("HIP error %s at %s:%d: %s", hipGetErrorString(_e), \
                      __FILE__, __LINE__, #expr);                         \
            return false;                                                 \
        }                                                                 \
    } while (0)

// ---------------------------------------------------------------- codecs

static bool zstd_decompress(const uint8_t *src, size_t src_n, uint8_t *dst,
                            size_t dst_n) {
    std::string err;
    if (!zstd_decompress_exact(src, src_n, dst, dst_n, err)) {
        set_error("%s", err.c_str());
        return false;
    }
    return true;
}



// ------------------------------------------------ on-GPU zstd page batch
//
// Decode all zstd pages of one column chunk on the GPU (k_zstd_pages, one
// wavefront per page frame) and copy the uncompressed image back to the
// host staging buffer. v1 keeps the host round trip so every downstream
// staging path (def-level peeks, dict pages, DELTA prescan) is unchanged;
// the PLAIN fast path staying device-resident is the follow-up. Returns
// false (WITHOUT set_error) to fall back to the host codec.
static bool gpu_zstd_enabled() {
    static int on = -1;
    if (on < 0) {
        const char *e = getenv("PMH_GPU_ZSTD");
        on = !(e && e[0] == '0');
        if (on) {
            int ndev = 0;
            if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) on = 0;
        }
    }
    return on;
}

struct ZstdBatchPage {
    int64_t src_off;  // into src_base
    int64_t src_len;
    int64_t dst_off;  // into the host image
    int64_t dst_len;
};

static bool gpu_zstd_batch_dev(
    const uint8_t *src_base, int64_t src_total,
    const std::vector<ZstdBatchPage> &pages, ::pmh_plan_t *plan,
    uint8_t **dev_out, int64_t out_total,
    const std::vector<std::pair<int64_t, int64_t>> &host_rngs,
    uint8_t *host_out);


static bool gpu_zstd_batch(const uint8_t *src_base, int64_t src_total,
                           const std::vector<ZstdBatchPage> &pages,
                           uint8_t *host_out, int64_t out_total) {
    if (pages.empty()) return true;
    int n = (int)pages.size();
    uint8_t *d_src = nullptr, *d_dst = nullptr, *d_scr = nullptr;
    ZstdJob *d_jobs = nullptr;
    int64_t *d_st = nullptr;
    std::vector<ZstdJob> jobs(n);
    for (int i = 0; i < n; i++) {
        jobs[i] = {(uint64_t)pages[i].src_off, (uint64_t)pages[i].dst_off,
                   (uint32_t)pages[i].src_len, (uint32_t)pages[i].dst_len};
    }
    bool ok = false;
    std::vector<int64_t> st(n);
    do {
        if (hipMalloc(&d_src, src_total) != hipSuccess) break;
        if (hipMalloc(&d_dst, out_total) != hipSuccess) break;
        if (hipMalloc(&d_scr, (size_t)n * PZ_SLOT) != hipSuccess) break;
        if (hipMalloc(&d_jobs, n * sizeof(ZstdJob)) != hipSuccess) break;
        if (hipMalloc(&d_st, n * 8) != hipSuccess) break;
        if (hipMemcpy(d_src, src_base, src_total, hipMemcpyHostToDevice) !=
            hipSuccess)
            break;
        if (hipMemcpy(d_jobs, jobs.data(), n * sizeof(ZstdJob),
                      hipMemcpyHostToDevice) != hipSuccess)
            break;
        if (pmh_launch_zstd_pages(d_src, d_jobs, n, d_dst, d_scr, d_st,
                                  nullptr) != hipSuccess)
            break;
        if (hipMemcpy(st.data(), d_st, n * 8, hipMemcpyDeviceToHost) !=
            hipSuccess)
            break;
        bool all = true;
        for (int i = 0; i < n; i++)
            if (st[i] != pages[i].dst_len) all = false;
        if (!all) break;
        if (hipMemcpy(host_out, d_dst, out_total, hipMemcpyDeviceToHost) !=
            hipSuccess)
            break;
        ok = true;
    } while (0);
    if (d_src) (void)hipFree(d_src);
    if (d_dst) (void)hipFree(d_dst);
    if (d_scr) (void)hipFree(d_scr);
    if (d_jobs) (void)hipFree(d_jobs);
    if (d_st) (void)hipFree(d_st);
    return ok;
}


// GPU batch page compression for the parquet write-back (k_zstd_compress).
// Returns false (no set_error) to fall back to the host codec.
// Opt-in (PMH_GPU_ZSTD_ENC=1): the v0 block compressor is spec-valid and
// wave-parallel, but the measured write-side A/B (profiles/ r02 zenc_ab)
// has host libzstd 4x faster AND ~2.5x smaller (huffman literals + a real
// parser beat predefined-FSE + greedy matching on typical column data) —
// so the HOST codec stays the write-side default. The debug entry and
// tests exercise the GPU path regardless.
bool pw_gpu_zstd_enc_enabled() {
    // read per call (cheap; tests toggle it within one process)
    const char *e = getenv("PMH_GPU_ZSTD_ENC");
    return e && e[0] == '1' && gpu_zstd_enabled();
}

bool pw_gpu_zstd_compress(const std::vector<std::string> &payloads,
                          std::vector<std::vector<uint8_t>> &outs) {
    if (!gpu_zstd_enabled() || payloads.empty()) return false;
    // one job per 128 KB BLOCK (pages can be multi-MB: block jobs keep
    // thousands of waves busy); the host stitches blocks into frames
    struct BlockRef {
        int page;
        int64_t dst_off;
    };
    std::vector<ZstdJob> jobs;
    std::vector<BlockRef> refs;
    int64_t src_total = 0, dst_total = 0;
    for (size_t i = 0; i < payloads.size(); i++) {
        int64_t sz = (int64_t)payloads[i].size();
        int64_t off = 0;
        while (off < sz) {
            int64_t bn = sz - off < PZ_BLOCK_MAX ? sz - off : PZ_BLOCK_MAX;
            int last = off + bn >= sz;
            int64_t cap = bn + (bn >> 8) + 256;
            ZstdJob j{(uint64_t)(src_total + off), (uint64_t)dst_total,
                      (uint32_t)bn,
                      (uint32_t)cap | (last ? 0x80000000u : 0u)};
            jobs.push_back(j);
            refs.push_back({(int)i, dst_total});
            dst_total += cap;
            off += bn;
        }
        src_total += sz;
    }
    int n = (int)jobs.size();
    if (n == 0) {  // all payloads empty: frames assemble host-side below
        n = 0;
    }
    std::vector<uint8_t> src_host(src_total ? src_total : 1);
    {
        int64_t o = 0;
        for (size_t i = 0; i < payloads.size(); i++) {
            memcpy(src_host.data() + o, payloads[i].data(),
                   payloads[i].size());
            o += (int64_t)payloads[i].size();
        }
    }
    uint8_t *d_src = nullptr, *d_dst = nullptr, *d_scr = nullptr;
    ZstdJob *d_jobs = nullptr;
    int64_t *d_st = nullptr;
    bool ok = false;
    std::vector<int64_t> st(n);
    do {
        if (hipMalloc(&d_src, src_host.size()) != hipSuccess) break;
        if (hipMalloc(&d_dst, dst_total ? dst_total : 1) != hipSuccess)
            break;
        if (hipMalloc(&d_scr, (size_t)n * sizeof(PzEnc)) != hipSuccess)
            break;
        if (hipMalloc(&d_jobs, n * sizeof(ZstdJob)) != hipSuccess) break;
        if (hipMalloc(&d_st, n * 8) != hipSuccess) break;
        if (hipMemcpy(d_src, src_host.data(), src_host.size(),
                      hipMemcpyHostToDevice) != hipSuccess)
            break;
        if (hipMemcpy(d_jobs, jobs.data(), n * sizeof(ZstdJob),
                      hipMemcpyHostToDevice) != hipSuccess)
            break;
        if (pmh_launch_zstd_compress(d_src, d_jobs, n, d_dst, d_scr, d_st,
                                     nullptr) != hipSuccess)
            break;
        if (hipMemcpy(st.data(), d_st, n * 8, hipMemcpyDeviceToHost) !=
            hipSuccess)
            break;
        bool all = true;
        for (int i = 0; i < n; i++)
            if (st[i] <= 0) all = false;
        if (!all) break;
        // stitch blocks into frames: header + concatenated block outputs
        std::vector<uint8_t> blob(dst_total ? dst_total : 1);
        if (dst_total &&
            hipMemcpy(blob.data(), d_dst, dst_total,
                      hipMemcpyDeviceToHost) != hipSuccess)
            break;
        outs.assign(payloads.size(), {});
        for (size_t i = 0; i < payloads.size(); i++) {
            uint8_t hdr[16];
            int hn = pz_frame_header(hdr, (int64_t)payloads[i].size());
            outs[i].insert(outs[i].end(), hdr, hdr + hn);
            if (payloads[i].empty()) {
                uint8_t raw0[3] = {1, 0, 0};  // empty raw last block
                outs[i].insert(outs[i].end(), raw0, raw0 + 3);
            }
        }
        for (int j = 0; j < n; j++) {
            auto &o = outs[refs[j].page];
            o.insert(o.end(), blob.data() + refs[j].dst_off,
                     blob.data() + refs[j].dst_off + st[j]);
        }
        ok = true;
    } while (0);
    if (d_src) (void)hipFree(d_src);
    if (d_dst) (void)hipFree(d_dst);
    if (d_scr) (void)hipFree(d_scr);
    if (d_jobs) (void)hipFree(d_jobs);
    if (d_st) (void)hipFree(d_st);
    return ok;
}

// ---------------------------------------------------- deletion vectors
//
// Paimon deletion vectors: per data file, a RoaringBitmap32
// of deleted row positions stored in a DV index file at (offset, length)
// (DeletionFile; deletionvectors/BitmapDeletionVector.java:98-112 wrapper =
// [i32 BE size][i32 BE magic 1581511376][roaring bytes][i32 BE crc];
// DeletionVector.read :101-118). The bitmap itself is the portable Roaring
// serialization (little-endian; cookie 12347 = no run containers, cookie
// low-16 12346 = with runs + bitset of run containers).
static bool parse_roaring32(const uint8_t *p, int64_t len,
                            std::vector<uint32_t> &out, std::string &err) {
    auto rd16 = [&](int64_t o) { return (uint32_t)p[o] | ((uint32_t)p[o + 1] << 8); };
    auto rd32 = [&](int64_t o) {
        return (uint32_t)p[o] | ((uint32_t)p[o + 1] << 8) |
               ((uint32_t)p[o + 2] << 16) | ((uint32_t)p[o + 3] << 24);
    };
    if (len < 8) { err = "roaring: short"; return false; }
    uint32_t cookie = rd32(0);
    int64_t o = 4;
    int32_t n_cont;
    bool has_run = false;
    std::vector<uint8_t> run_flags;
    if ((cookie & 0xFFFF) == 12346) {
        has_run = true;
        n_cont = (int32_t)(cookie >> 16) + 1;
        int64_t rb = (n_cont + 7) / 8;
        run_flags.assign(p + o, p + o + rb);
        o += rb;
    } else if (cookie == 12347) {
        n_cont = (int32_t)rd32(o);
        o += 4;
    } else {
        err = "roaring: bad cookie";
        return false;
    }
    std::vector<uint32_t> keys(n_cont), cards(n_cont);
    for (int i = 0; i < n_cont; i++) {
        keys[i] = rd16(o);
        cards[i] = rd16(o + 2) + 1;
        o += 4;
    }
    const bool has_offsets = !has_run || n_cont >= 4;
    if (has_offsets) o += 4 * (int64_t)n_cont;  // container offsets (unused)
    for (int i = 0; i < n_cont; i++) {
        const uint32_t hi = keys[i] << 16;
        const bool is_run =
            has_run && (run_flags[i / 8] >> (i % 8)) & 1;
        if (is_run) {
            uint32_t n_runs = rd16(o);
            o += 2;
            for (uint32_t r = 0; r < n_runs; r++) {
                uint32_t start = rd16(o), rl = rd16(o + 2);
                o += 4;
                for (uint32_t v = start; v <= start + rl; v++)
                    out.push_back(hi | v);
            }
        } else if (cards[i] > 4096) {  // bitmap container: 8 KB
            for (int w = 0; w < 1024; w++) {
                uint64_t word = 0;
                for (int b = 0; b < 8; b++)
                    word |= (uint64_t)p[o + w * 8 + b] << (8 * b);
                while (word) {
                    int bit = __builtin_ctzll(word);
                    out.push_back(hi | (uint32_t)(w * 64 + bit));
                    word &= word - 1;
                }
            }
            o += 8192;
        } else {  // array container
            for (uint32_t v = 0; v < cards[i]; v++)
                out.push_back(hi | rd16(o + 2 * v));
            o += 2 * (int64_t)cards[i];
        }
        if (o > len) { err = "roaring: overrun"; return false; }
    }
    return true;
}

// Read one file's DV from its index file slice; returns deleted positions.
static bool load_deletion_vector(const std::string &path, int64_t offset,
                                 int64_t length,
                                 std::vector<uint32_t> &out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) {
        set_error("cannot open deletion vector file %s", path.c_str());
        return false;
    }
    if (length <= 0) {  // whole file
        fseek(f, 0, SEEK_END);
        length = ftell(f) - offset;
    }
    std::vector<uint8_t> buf(length);
    fseek(f, offset, SEEK_SET);
    bool ok = fread(buf.data(), 1, length, f) == (size_t)length;
    fclose(f);
    if (!ok || length < 12) {
        set_error("deletion vector read failed (%s @%lld+%lld)",
                  path.c_str(), (long long)offset, (long long)length);
        return false;
    }
    auto be32 = [&](int64_t o) {
        return ((uint32_t)buf[o] << 24) | ((uint32_t)buf[o + 1] << 16) |
               ((uint32_t)buf[o + 2] << 8) | (uint32_t)buf[o + 3];
    };
    uint32_t size = be32(0);
    if (be32(4) != 1581511376u) {
        set_error("deletion vector magic mismatch in %s", path.c_str());
        return false;
    }
    if ((int64_t)size + 8 > length) {
        set_error("deletion vector truncated in %s", path.c_str());
        return false;
    }
    std::string err;
    if (!parse_roaring32(buf.data() + 8, size - 4, out, err)) {
        set_error("%s (%s)", err.c_str(), path.c_str());
        return false;
    }
    return true;
}

// ------------------------------------------- IntervalPartition (restated)

struct FileDesc {
    std::string dv_path;  // deletion vector (DeletionFile); empty = none
    int64_t dv_offset = 0;
    int64_t dv_length = 0;
    std::string path;
    int64_t row_count = 0;
    int64_t min_key = 0;
    int64_t max_key = 0;
    int level = 0;
    int input_index = 0;
};

// Restatement of IntervalPartition (mergetree/compact/IntervalPartition.java
// :40-126) for int64 keys: sort files by (minKey, maxKey); cut sections
// where minKey exceeds the running right bound; within a section, greedily
// pack files into the fewest sorted runs via a min-heap on each run's last
// maxKey.
static std::vector<std::vector<std::vector<FileDesc>>> interval_partition(
    std::vector<FileDesc> files, bool level_pure_runs = false) {
    std::sort(files.begin(), files.end(), [](const FileDesc &a, const FileDesc &b) {
        if (a.min_key != b.min_key) return a.min_key < b.min_key;
        return a.max_key < b.max_key;
    });
    std::vector<std::vector<std::vector<FileDesc>>> result;
    std::vector<FileDesc> section;
    int64_t bound = 0;
    bool has_bound = false;

    auto pack = [level_pure_runs](const std::vector<FileDesc> &metas) {
        // min-heap of runs keyed by last file's maxKey (IntervalPartition.java:93-125)
        auto cmp = [](const std::vector<FileDesc> &a, const std::vector<FileDesc> &b) {
            return a.back().max_key > b.back().max_key;  // min-heap
        };
        std::priority_queue<std::vector<FileDesc>, std::vector<std::vector<FileDesc>>,
                            decltype(cmp)>
            q(cmp);
        q.push({metas[0]});
        for (size_t i = 1; i < metas.size(); i++) {
            auto top = q.top();
            q.pop();
            if (metas[i].min_key > top.back().max_key &&
                (!level_pure_runs ||
                 metas[i].level == top.back().level)) {
                // level_pure_runs (changelog mode): records carry the level
                // of the FILE they were read from (KeyValue.setLevel per
                // file reader), so a run must not chain files of different
                // levels — start a new run instead (same merge semantics)
                top.push_back(metas[i]);
            } else {
                q.push({metas[i]});
            }
            q.push(top);
        }
        std::vector<std::vector<FileDesc>> runs;
        while (!q.empty()) {
            runs.push_back(q.top());
            q.pop();
        }
        return runs;
    };

    for (const auto &meta : files) {
        if (!section.empty() && meta.min_key > bound) {
            result.push_back(pack(section));
            section.clear();
            has_bound = false;
        }
        section.push_back(meta);
        if (!has_bound || meta.max_key > bound) {
            bound = meta.max_key;
            has_bound = true;
        }
    }
    if (!section.empty()) result.push_back(pack(section));
    return result;
}

// ------------------------------------------------------------- data model

struct ColSpec {
    std::string name;
    int dtype;  // pmh_dtype
    int out_esize;
    int stored_esize;  // parquet physical width (TINYINT stored as INT32)
    int precision = 0;  // DECIMAL(p,s) annotation on INT32/INT64
    int scale = 0;
    // date / time / timestamp annotation on INT32/INT64 (enum pmh_logical)
    int logical = 0;
    // BOOLEAN: dtype is PMH_DT_INT8 inside the pipeline, so the column
    // stages at the 4-byte stored width every merge and emit kernel loads
    // and narrows to one 0/1 byte on emit, as TINYINT does; the batch
    // reports PMH_DT_BOOL
    bool is_bool = false;
};

// Plan-level GLOBAL dictionary for one string column: per-file parquet
// dictionaries remap into it at staging (id streams then decode to global
// ids on device and flow through merge/emit as int32), and the output
// batch exposes it — the same dictionary-vector shape the reference's
// columnar batches use (paimon-common heap vectors with setDictionary).
struct StrDict {
    std::vector<uint8_t> bytes;
    std::vector<int32_t> offsets{0};
    std::unordered_map<std::string, int32_t> index;
    int32_t add(const uint8_t *p, uint32_t len) {
        std::string s((const char *)p, len);
        auto it = index.find(s);
        if (it != index.end()) return it->second;
        int32_t id = (int32_t)offsets.size() - 1;
        bytes.insert(bytes.end(), p, p + len);
        offsets.push_back((int32_t)bytes.size());
        index.emplace(std::move(s), id);
        return id;
    }
};

struct DeviceBufs {
    std::vector<void *> bufs;
    void *alloc(size_t n) {
        void *p = nullptr;
        if (hipMalloc(&p, n ? n : 8) != hipSuccess) return nullptr;
        bufs.push_back(p);
        return p;
    }
    ~DeviceBufs() {
        for (void *p : bufs) (void)hipFree(p);
    }
};

// one (run, column), staged as ONE contiguous device column:
//  - PLAIN chunks: page value-payloads packed host-side, H2D straight into
//    `contig` at the chunk's row offset (the encoded PLAIN bytes ARE the
//    column values; packing is layout, not decode);
//  - dictionary chunks: the RLE id streams stay encoded in HBM; at read
//    time k_rle_decode + k_dict_gather materialize the chunk's row range of
//    `contig` (decode_ms, inside the timed region).
struct GatherTask {
    int64_t start = 0;  // run-row offset (or dense offset, to_dense)
    int64_t n = 0;
    void *dict_dev = nullptr;
    bool to_dense = false;  // nullable chunk: gather into the dense buffer,
                            // k_level_scatter positions the rows after
    bool in_place = false;  // ORC dictionary strings: the RLEv2 decode
                            // already wrote LOCAL ids at the target; remap
                            // them to global ids in place
};

struct RunCol {
    void *contig = nullptr;
    bool dict_encoded = false;  // any dictionary-encoded chunk
    std::vector<RleChunk> rle_host;
    RleChunk *rle_dev = nullptr;
    int32_t *ids_dev = nullptr;
    std::vector<GatherTask> gathers;
    int64_t n_rows = 0;
    // nullable columns with actual nulls: dense PLAIN values + def-level
    // streams stay encoded in HBM; k_level_scatter positions them at read
    // time (timed decode) and fills the byte-validity array.
    bool has_nulls = false;
    std::vector<uint8_t> dense_host;   // packed non-null values (staging)
    // (dense_start, nbytes) per dense_host append — PLAIN and dictionary
    // null-chunks can interleave, so host segments land at their own offsets
    std::vector<std::pair<int64_t, int64_t>> dense_segs;
    std::vector<uint8_t> levels_host;  // packed def-level streams (staging)
    std::vector<RleChunk> def_host;    // src = RELATIVE offset until upload
    int64_t dense_before = 0;          // running non-null count
    void *dense_dev = nullptr;
    RleChunk *def_dev = nullptr;
    uint8_t *valid_dev = nullptr;
    // ORC: RLEv2 / byte-RLE work chunks decode on the GPU at read time
    bool orc_encoded = false;
    std::vector<Rlev2Chunk> rlev2_host;
    Rlev2Chunk *rlev2_dev = nullptr;
    // ORC DECIMAL: varint work units (k_orc_varint). scale_dev is the
    // (run, column)'s int32 data-scale scratch: stripes whose SECONDARY
    // stream is not uniformly the column scale append their scales to it
    // (scale_rows so far). Units of such stripes carry 1 + the scratch index
    // of their first value in scale_addr until finalize patches the address
    std::vector<VarintUnit> varint_host;
    int64_t scale_rows = 0;
    int32_t *scale_dev = nullptr;
    // BOOLEAN (parquet PLAIN bits / ORC boolean byte-RLE): k_bits_expand
    // work units; the encoded bytes stay in HBM and expand at read time
    std::vector<BitsUnit> bits_host;
    // ORC TIMESTAMP: the SECONDARY stream's stored nanos decode through
    // k_rlev2 into nanos_dev, the (run, column)'s uint64 scratch
    // (nanos_rows values); k_orc_timestamp then combines them with the
    // seconds k_rlev2 wrote to the column. Units carry scratch INDICES in
    // nanos_start and get their addresses at finalize
    std::vector<TsUnit> ts_host;
    int64_t nanos_rows = 0;
    uint64_t *nanos_dev = nullptr;
    // parquet DELTA_BINARY_PACKED pages (decoded on GPU at read time)
    std::vector<DeltaChunk> delta_host;
    std::vector<DeltaStream> dstreams_host;
};

struct Run {
    int64_t length = 0;
    std::vector<RunCol> cols;
    uint8_t *tomb = nullptr;  // deletion-vector tombstones (1 = deleted)
    int level = 0;            // the SortedRun's level (files of one run
                              // share it; changelog top-level detection)
};

struct Section {
    std::vector<Run> runs;
    int64_t total_rows = 0;
    int64_t n_tiles = 0;
    // device-side state, as the launchers take it (kernels.h). runs_dev
    // describes what the merge chain reads: the section's runs (plus a
    // lookup plan's level slots), or the virtual runs of a hierarchical
    // section
    RunSet runs_dev;
    TileSet tiles;
    ChangelogSet cl;
    // lookup changelog: k_lookup_probe writes one word per row of the
    // level-0 runs
    ProbeSet probe;
    bool any_tomb = false;
    // packed per-row validity (PU/agg emit): one u64 per row per run,
    // bit c = column c non-null; rebuilt every read by k_pack_valid
    // (runs_dev.masks is the device array of these)
    std::vector<uint64_t *> row_masks;
    // hierarchical sections (> PMH_MAX_RUNS runs): the reference spills
    // to disk (MergeSorter.spillMergeSort); here the winner fold is
    // ASSOCIATIVE for deduplicate/first-row (max/min by (seq, isAdd)), so
    // run batches merge on-device into VIRTUAL runs first (keeping delete
    // winners), then the normal chain merges the virtual runs.
    bool hier = false;
    RunSet real_dev;                 // the REAL runs (tombstones included)
    std::vector<int> blo, bhi;       // batch run ranges
    std::vector<int64_t> brows, bntiles;
    std::vector<OutputSet> bout;     // per batch: its virtual run's columns
    std::vector<int64_t *> ckeys;  // per-run composite keys (k_composite)
    // batched decode work (all run-columns in ONE launch each)
    Rlev2Chunk *rlev2_all = nullptr;
    int64_t n_rlev2 = 0;
    VarintUnit *varint_all = nullptr;
    int64_t n_varint = 0;
    BitsUnit *bits_all = nullptr;
    int64_t n_bits = 0;
    TsUnit *ts_all = nullptr;
    int64_t n_ts = 0;
    DeltaChunk *delta_all = nullptr;
    int64_t n_delta = 0;
    DeltaStream *dstreams_all = nullptr;
    int64_t n_dstreams = 0;
    int64_t *delta_sums = nullptr;   // per-chunk block sums
    int64_t *delta_bases = nullptr;  // per-chunk entering values
    RleChunk *def_all = nullptr;
    int64_t n_def = 0;
    bool any_dict = false;
    bool any_decode = false;  // dict or null-scatter work at read time
};

// One output stream of a plan (the main batch or the changelog batch):
// device buffers reused per section, their host copies under
// output = "host", and the pmh_col descriptors handed to the caller.
struct OutBatch {
    std::vector<void *> dev;       // per column
    std::vector<uint8_t *> valid;  // per column; nullptr if never null
    OutputSet set;                 // device arrays of the two above
    std::vector<std::vector<uint8_t>> host, valid_host;
    std::vector<pmh_col> cols;
};

}  // namespace pmh

struct pmh_session_t {
    int device = -1;
};

struct pmh_plan_t {
    pmh_session_t *session = nullptr;
    hipStream_t stream = nullptr;
    pmh::DeviceBufs bufs;
    std::vector<pmh::ColSpec> cols;  // key..., seq, kind, value...
    // device tables over `cols` as the launchers take them (n_key_cols,
    // the sequence.field columns and the aggregator codes included);
    // hier_columns is the batch pass's view (int8/16 -> int32, so virtual
    // runs hold the STORED width)
    pmh::ColumnSet columns, hier_columns;
    // engine bits of the merge flag word (PMH_FLAG_*), built once at the end
    // of plan creation
    int merge_flags = 0;
    bool drop_delete = true;
    bool ignore_delete = false;
    bool host_output = false;
    bool pu = false;         // partial-update merge engine
    bool first_row = false;  // first-row merge engine
    bool fused = false;      // single-pass k_merge_emit (non-member-list
                             // engines; PMH_FUSED=0 falls back for A/B)
    bool fsplit = false;     // split value emission (PMH_FSPLIT=1 A/B)
    bool agg = false;        // aggregation merge engine (uses PU member lists)
    // value filters (conjunction; applied to single-run sections only,
    // MergeFileSplitRead.java:227-239)
    std::vector<pmh::FilterTerm> filters;
    pmh::FilterTerm *filters_dev = nullptr;
    // composite key (>1 key column): order-preserving packed comparand
    bool composite_key = false;
    uint64_t key_shifts = 0, key_bits = 0;  // 8 bits per sub-key
    // partial-update.remove-record-on-delete: a DELETE resets the row
    // (PartialUpdateMergeFunction.java:173-180); v1 accepts INSERT/DELETE
    // streams (UPDATE_BEFORE rejected)
    bool rrod = false;
    // sequence groups (fields.<seq>.sequence-group=members,
    // PartialUpdateMergeFunction.java:219-377): retracts become legal and
    // act on their groups
    bool seqg = false;
    bool agg_retract = false;  // every aggregator retract-capable
    pmh::SeqGroupSet seq_groups;
    // partial-update aggregate functions: [n_cols] PMH_AGG_* code
    // (| PMH_AGG_IGNORE_RETRACT) or PAC_NONE; empty without any
    std::vector<uint8_t> pu_col_agg;
    // changelog-producer = full-compaction (FullChangelogMergeFunction-
    // Wrapper): a second output stream of changelog rows per read_next
    bool changelog = false;
    bool cl_row_dedup = false;
    // full-compaction changelog of a folding engine (partial-update /
    // aggregation): after-type rows come from the main output
    bool cl_fold = false;
    int max_level = 0;
    // changelog-producer = lookup (LookupChangelogMergeFunctionWrapper):
    // the levels above the compaction's output level, one sorted run per
    // level (ascending), staged once and resident for the plan's lifetime;
    // lookup_sec only carries their runs and decode tables
    bool lookup = false;
    pmh::Section lookup_sec;
    int64_t cl_rows_last = 0;
    std::vector<pmh::Section> sections;
    size_t cur_section = 0;
    int64_t rows_in_total = 0;
    int64_t encoded_bytes_total = 0;
    pmh::OutBatch out;   // main batch
    pmh::OutBatch out2;  // changelog batch (changelog plans)
    std::vector<bool> col_nullable;        // any nulls staged for this col
    std::vector<std::string> col_names;
    std::vector<std::unique_ptr<pmh::StrDict>> sdicts;  // per col; string only
    pmh_stats stats{};
    double h2d_ms = 0;
    // the device buffers go with `bufs`, after the stream
    ~pmh_plan_t() {
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace pmh {

static int dtype_from_str(const std::string &s) {
    if (s == "int8" || s == "tinyint") return PMH_DT_INT8;
    if (s == "int16" || s == "smallint") return PMH_DT_INT16;
    if (s == "int32" || s == "int") return PMH_DT_INT32;
    if (s == "int64" || s == "bigint") return PMH_DT_INT64;
    if (s == "float" || s == "float32") return PMH_DT_FLOAT32;
    if (s == "double" || s == "float64") return PMH_DT_FLOAT64;
    if (s == "string" || s == "varchar" || s == "char") return PMH_DT_STRING;
    return -1;
}

// "decimal(p,s)": p <= 9 rides INT32, p <= 18 INT64 (unscaled values) —
// exactly the reference's physical mapping, ParquetSchemaConverter.java:
// 153-171 + is32BitDecimal/is64BitDecimal :334-341. Wider decimals (FLBA)
// are a later round.
static bool parse_decimal(const std::string &s, int *p, int *sc) {
    if (s.rfind("decimal(", 0) != 0 || s.back() != ')') return false;
    return sscanf(s.c_str(), "decimal(%d,%d)", p, sc) == 2;
}

// "boolean", "date", "time", "timestamp[(p)]", "timestamp_ltz[(p)]": the
// reference's physical mapping (ParquetSchemaConverter.java:126-216,
// 306-323; OrcTypeUtil.java:67-114) — boolean is its own column, the others
// ride INT32/INT64 with a pmh_logical annotation; a bare timestamp is
// timestamp(6). Returns 0 = none of these, 1 = parsed into cs, -1 = refused
// (error set): precision above 6 would be parquet INT96 / sub-microsecond ORC.
static int parse_bool_or_temporal(const std::string &s, ColSpec &cs) {
    if (s == "boolean" || s == "bool") {
        cs.dtype = PMH_DT_INT8;
        cs.is_bool = true;
        return 1;
    }
    if (s == "date") {
        cs.dtype = PMH_DT_INT32;
        cs.logical = PMH_LT_DATE;
        return 1;
    }
    if (s == "time") {
        cs.dtype = PMH_DT_INT32;
        cs.logical = PMH_LT_TIME_MILLIS;
        return 1;
    }
    bool ltz = false;
    std::string rest;
    if (s.rfind("timestamp_ltz", 0) == 0) {
        ltz = true;
        rest = s.substr(13);
    } else if (s.rfind("timestamp", 0) == 0) {
        rest = s.substr(9);
    } else {
        return 0;
    }
    int p = 6;
    if (!rest.empty()) {
        int used = 0;
        if (sscanf(rest.c_str(), "(%d)%n", &p, &used) != 1 ||
            used != (int)rest.size())
            return 0;
    }
    if (p < 0 || p > 6) {
        set_error("%s: timestamp precision %d is not supported (0..6: INT64 "
                  "milliseconds / microseconds; parquet INT96 and "
                  "sub-microsecond ORC timestamps are out of scope)",
                  s.c_str(), p);
        return -1;
    }
    cs.dtype = PMH_DT_INT64;
    cs.logical = p <= 3 ? (ltz ? PMH_LT_TIMESTAMP_LTZ_MILLIS
                               : PMH_LT_TIMESTAMP_MILLIS)
                        : (ltz ? PMH_LT_TIMESTAMP_LTZ_MICROS
                               : PMH_LT_TIMESTAMP_MICROS);
    return 1;
}

static bool logical_is_timestamp(int lt) {
    return lt >= PMH_LT_TIMESTAMP_MILLIS && lt <= PMH_LT_TIMESTAMP_LTZ_MICROS;
}
static bool logical_is_ltz(int lt) {
    return lt == PMH_LT_TIMESTAMP_LTZ_MILLIS ||
           lt == PMH_LT_TIMESTAMP_LTZ_MICROS;
}
static bool logical_is_micros(int lt) {
    return lt == PMH_LT_TIMESTAMP_MICROS || lt == PMH_LT_TIMESTAMP_LTZ_MICROS;
}
static const char *logical_name(int lt) {
    switch (lt) {
    case PMH_LT_DATE: return "date";
    case PMH_LT_TIME_MILLIS: return "time";
    case PMH_LT_TIMESTAMP_MILLIS: return "timestamp(3)";
    case PMH_LT_TIMESTAMP_MICROS: return "timestamp(6)";
    case PMH_LT_TIMESTAMP_LTZ_MILLIS: return "timestamp_ltz(3)";
    case PMH_LT_TIMESTAMP_LTZ_MICROS: return "timestamp_ltz(6)";
    }
    return "none";
}

static int expected_phys(int dtype) {
    switch (dtype) {
    case PMH_DT_INT8:
    case PMH_DT_INT16:
    case PMH_DT_INT32: return PHYS_INT32;
    case PMH_DT_INT64: return PHYS_INT64;
    case PMH_DT_FLOAT32: return PHYS_FLOAT;
    case PMH_DT_FLOAT64: return PHYS_DOUBLE;
    case PMH_DT_STRING: return PHYS_BYTE_ARRAY;
    }
    return -1;
}

static const char *pq_unit_name(int u) {
    return u == PQ_UNIT_MILLIS   ? "MILLIS"
           : u == PQ_UNIT_MICROS ? "MICROS"
           : u == PQ_UNIT_NANOS  ? "NANOS"
                                 : "none";
}

// A column declared boolean / date / time / timestamp against the parquet
// file's schema element: the physical type has to be the reference's mapping
// and, for the annotated types, the annotation has to say the same thing.
// The timestamp unit is the one mismatch that would otherwise mis-scale
// every value silently. Each refusal has its own text.
static bool check_parquet_declared(const std::string &path, const ColSpec &cs,
                                   const ParquetFileMeta &m, int leaf) {
    if (!cs.is_bool && !cs.logical) return true;
    const int phys = (int)m.phys_types.size() > leaf ? m.phys_types[leaf] : -1;
    const int want = cs.is_bool ? PHYS_BOOLEAN : expected_phys(cs.dtype);
    const char *decl = cs.is_bool ? "boolean" : logical_name(cs.logical);
    if (phys != want) {
        set_error("%s: column %s declared %s but the file's physical type "
                  "is %d (expect %d)", path.c_str(), cs.name.c_str(), decl,
                  phys, want);
        return false;
    }
    if (cs.is_bool) return true;
    const int conv = m.converted_types[leaf];
    const int lk = m.logical_kinds[leaf];
    if (cs.logical == PMH_LT_DATE) {
        if (lk != LOGICAL_DATE && conv != CONV_DATE) {
            set_error("%s: column %s declared date but the file column "
                      "carries no DATE annotation", path.c_str(),
                      cs.name.c_str());
            return false;
        }
        return true;
    }
    int unit = PQ_UNIT_NONE;
    if (cs.logical == PMH_LT_TIME_MILLIS) {
        if (lk == LOGICAL_TIME) unit = m.logical_units[leaf];
        else if (conv == CONV_TIME_MILLIS) unit = PQ_UNIT_MILLIS;
        else if (conv == CONV_TIME_MICROS) unit = PQ_UNIT_MICROS;
        if (unit == PQ_UNIT_NONE) {
            set_error("%s: column %s declared time but the file column "
                      "carries no TIME annotation", path.c_str(),
                      cs.name.c_str());
            return false;
        }
        if (unit != PQ_UNIT_MILLIS) {
            set_error("%s: column %s declared time (INT32 milliseconds) but "
                      "the file's TIME unit is %s", path.c_str(),
                      cs.name.c_str(), pq_unit_name(unit));
            return false;
        }
        return true;
    }
    if (lk == LOGICAL_TIMESTAMP) unit = m.logical_units[leaf];
    else if (conv == CONV_TIMESTAMP_MILLIS) unit = PQ_UNIT_MILLIS;
    else if (conv == CONV_TIMESTAMP_MICROS) unit = PQ_UNIT_MICROS;
    if (unit == PQ_UNIT_NONE) {
        set_error("%s: column %s declared %s but the file column carries no "
                  "TIMESTAMP annotation", path.c_str(), cs.name.c_str(),
                  decl);
        return false;
    }
    const int want_unit =
        logical_is_micros(cs.logical) ? PQ_UNIT_MICROS : PQ_UNIT_MILLIS;
    if (unit != want_unit) {
        set_error("%s: column %s declared %s (%s) but the file's TIMESTAMP "
                  "unit is %s", path.c_str(), cs.name.c_str(), decl,
                  pq_unit_name(want_unit), pq_unit_name(unit));
        return false;
    }
    return true;
}

// A boolean column's page: PLAIN (bit-packed) v1 data pages only.
static bool check_bool_page(const std::string &path, const ColSpec &cs,
                            const PageMeta &pg) {
    if (pg.page_type == 0 && pg.encoding == ENC_PLAIN) return true;
    const std::string enc = pg.page_type == 2      ? "dictionary"
                            : pg.encoding == ENC_RLE ? "RLE"
                                : std::to_string(pg.encoding);
    set_error("%s col %s: boolean pages in %s encoding are not supported "
              "(PLAIN bit-packed pages only; RLE is what data page v2 "
              "writers emit)", path.c_str(), cs.name.c_str(), enc.c_str());
    return false;
}

struct StagedFile {
    std::vector<uint8_t> data;  // whole file (or decompressed payload view)
    bool orc = false;
    ParquetFileMeta meta;
    OrcFileMeta orc_meta;
};

static bool load_file(const std::string &path, StagedFile &sf) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) {
        set_error("cannot open %s", path.c_str());
        return false;
    }
    int64_t n = f.tellg();
    f.seekg(0);
    sf.data.resize(n);
    f.read((char *)sf.data.data(), n);
    if (is_orc_file(sf.data.data(), n)) {
        sf.orc = true;
        sf.orc_meta = parse_orc_meta(sf.data.data(), n);
        if (!sf.orc_meta.ok()) {
            set_error("%s: %s", path.c_str(), sf.orc_meta.error.c_str());
            return false;
        }
        return true;
    }
    sf.meta = parse_parquet_footer(sf.data.data(), n);
    if (!sf.meta.ok()) {
        set_error("%s: %s", path.c_str(), sf.meta.error.c_str());
        return false;
    }
    std::string err;
    for (auto &rg : sf.meta.row_groups)
        for (auto &cc : rg.columns)
            if (!scan_chunk_pages(sf.data.data(), n, cc, err)) {
                set_error("%s: %s", path.c_str(), err.c_str());
                return false;
            }
    return true;
}

// ------------------------------------------------- ORC staging (RLEv2)

// Message for the ORC decimal bits of a section's device error word
// (k_orc_varint ORs 1 << (ODC_ERR_SHIFT + ODC_ERR_*)).
static std::string orc_decimal_error(uint32_t err_word) {
    std::string m = "ORC decimal rescale failed:";
    const char *sep = " ";
    for (int code = 1; code <= ODC_ERR_WIDTH; code++)
        if (err_word & (1u << (ODC_ERR_SHIFT + code))) {
            m += sep;
            m += odc_err_text(code);
            sep = "; ";
        }
    return m;
}

// The decimal bits of an error word: ODC_ERR_SHIFT + 1 .. + 7 (the
// timestamp bits sit above them, from OTS_ERR_SHIFT on).
static uint32_t orc_decimal_bits(uint32_t err_word) {
    return (err_word >> ODC_ERR_SHIFT) & 0xFFu;
}

// Message for the ORC timestamp bits of a section's device error word
// (k_orc_timestamp ORs 1 << (OTS_ERR_SHIFT + OTS_ERR_*)).
static std::string orc_timestamp_error(uint32_t err_word) {
    std::string m = "ORC timestamp refused:";
    const char *sep = " ";
    for (int code = 1; code <= OTS_ERR_LAST; code++)
        if (err_word & (1u << (OTS_ERR_SHIFT + code))) {
            m += sep;
            m += ots_err_text(code);
            sep = "; ";
        }
    return m;
}

// boolean / date / time / timestamp against one stripe of an ORC file: the
// declared type and the ORC kind have to be the reference's mapping
// (OrcTypeUtil.java:67-114), both ways round, and a TIMESTAMP stripe has to
// be written in UTC.
static bool check_orc_declared(const std::string &path, const ColSpec &cs,
                               int ckind, const OrcStripe &st) {
    const bool k_ts = ckind == ORC_TIMESTAMP || ckind == ORC_TIMESTAMP_INSTANT;
    int want = -1;
    if (cs.is_bool) want = ORC_BOOLEAN;
    else if (cs.logical == PMH_LT_DATE) want = ORC_DATE;
    else if (cs.logical == PMH_LT_TIME_MILLIS) want = ORC_INT;
    else if (logical_is_timestamp(cs.logical))
        want = logical_is_ltz(cs.logical) ? ORC_TIMESTAMP_INSTANT
                                          : ORC_TIMESTAMP;
    if (want >= 0 && ckind != want) {
        set_error("%s col %s: declared %s but ORC kind is %d (expect %d)",
                  path.c_str(), cs.name.c_str(),
                  cs.is_bool ? "boolean" : logical_name(cs.logical), ckind,
                  want);
        return false;
    }
    if (want < 0 && (ckind == ORC_BOOLEAN || ckind == ORC_DATE || k_ts)) {
        set_error("%s col %s: ORC %s column read as another type",
                  path.c_str(), cs.name.c_str(),
                  ckind == ORC_BOOLEAN ? "BOOLEAN"
                  : ckind == ORC_DATE  ? "DATE"
                                       : "TIMESTAMP");
        return false;
    }
    if (ckind == ORC_TIMESTAMP && !orc_timezone_is_utc(st.writer_timezone)) {
        // TIMESTAMP values are relative to 2015-01-01 in the WRITER's zone;
        // TIMESTAMP_INSTANT is always UTC
        set_error("%s col %s: ORC TIMESTAMP written in timezone '%s' is not "
                  "supported (UTC / GMT only)", path.c_str(),
                  cs.name.c_str(), st.writer_timezone.c_str());
        return false;
    }
    return true;
}

// Upload `len` encoded bytes into a plan buffer of len + pad bytes (pad 16:
// the device bit readers load aligned 16-byte windows) and count them as
// staged input. nullptr with the error set on failure.
static void *upload_image(pmh_plan_t *plan, const uint8_t *src, int64_t len,
                          int pad) {
    void *dev = plan->bufs.alloc(len + pad);
    if (!dev) return nullptr;
    if (len && hipMemcpy(dev, src, len, hipMemcpyHostToDevice) != hipSuccess) {
        set_error("H2D failed");
        return nullptr;
    }
    plan->encoded_bytes_total += len;
    return dev;
}

// Upload an ORC side stream whose chunks were prescanned at device base 0
// and point them at the device copy.
static bool upload_rebase(pmh_plan_t *plan, const uint8_t *src, int64_t len,
                          std::vector<Rlev2Chunk> &chunks) {
    void *dev = upload_image(plan, src, len, 16);
    if (!dev) return false;
    for (auto &k : chunks) {
        k.src += (uint64_t)dev;
        if (k.kind == 2) k.patch_src += (uint64_t)dev;
    }
    return true;
}

// The bytes of one ORC stream of a column: the file's own, or, in a
// compressed file, `dec` filled by orc_decompress. `label` names the stream
// in the error (" PRESENT"; "" for DATA).
static bool orc_stream_bytes(const FileDesc &fd, const StagedFile &sf,
                             const ColSpec &cs, const OrcStream *st,
                             const char *label, std::vector<uint8_t> &dec,
                             const uint8_t **ptr, int64_t *len) {
    const OrcFileMeta &om = sf.orc_meta;
    *ptr = sf.data.data() + st->offset;
    *len = st->length;
    if (om.compression == 0) return true;
    std::string cerr;
    if (!orc_decompress(*ptr, *len, om.compression, om.compression_block_size,
                        dec, cerr)) {
        set_error("%s col %s%s: %s", fd.path.c_str(), cs.name.c_str(), label,
                  cerr.c_str());
        return false;
    }
    *ptr = dec.data();
    *len = (int64_t)dec.size();
    return true;
}

// Stage a stripe's PRESENT stream into the column's def chunks. The stripe's
// values then go to the dense buffer: *dense0 = the dense cursor before the
// stripe, *n_dense = its non-null rows.
static bool stage_orc_present(const FileDesc &fd, const ColSpec &cs,
                              const uint8_t *pres, int64_t pres_len,
                              int64_t n_rows, int64_t row0, RunCol &rc,
                              int64_t *dense0, int64_t *n_dense,
                              int *dense_target) {
    const char *why = "";
    rc.has_nulls = true;
    *dense0 = rc.dense_before;
    if (!prescan_present(pres, pres_len, n_rows, row0, rc.levels_host,
                         rc.def_host, &rc.dense_before, &why)) {
        set_error("%s col %s PRESENT: %s", fd.path.c_str(), cs.name.c_str(),
                  why);
        return false;
    }
    *n_dense = rc.dense_before - *dense0;
    *dense_target = 1;
    return true;
}

// Stage one ORC file's stripes for the required columns.
static bool stage_orc_file(pmh_plan_t *plan, const FileDesc &fd,
                           const StagedFile &sf, Run &run, int64_t row_base) {
    const auto &cols = plan->cols;
    const OrcFileMeta &om = sf.orc_meta;
    std::vector<int> col_id(cols.size(), -1);
    for (size_t c = 0; c < cols.size(); c++) {
        for (size_t i = 0; i < om.column_names.size(); i++)
            if (om.column_names[i] == cols[c].name) col_id[c] = (int)i + 1;
        if (col_id[c] < 0) {
            set_error("%s: column %s not found", fd.path.c_str(),
                      cols[c].name.c_str());
            return false;
        }
    }
    int64_t stripe_row = 0;
    for (const auto &st : om.stripes) {
        for (size_t c = 0; c < cols.size(); c++) {
            RunCol &rc = run.cols[c];
            rc.orc_encoded = true;
            int cid = col_id[c];
            int ckind = om.column_kinds[cid - 1];
            if (cols[c].dtype == PMH_DT_STRING && ckind != ORC_STRING) {
                set_error("%s col %s: declared string but ORC kind is %d",
                          fd.path.c_str(), cols[c].name.c_str(), ckind);
                return false;
            }
            if (ckind == ORC_DECIMAL || cols[c].precision > 0) {
                // decimals ride as unscaled INT32/INT64 at the DECLARED
                // (precision, scale): the file must say the same
                const int fp = om.column_precisions[cid - 1];
                const int fs = om.column_scales[cid - 1];
                if (ckind != ORC_DECIMAL) {
                    set_error("%s col %s: declared decimal(%d,%d) but ORC "
                              "kind is %d, not DECIMAL", fd.path.c_str(),
                              cols[c].name.c_str(), cols[c].precision,
                              cols[c].scale, ckind);
                    return false;
                }
                if (cols[c].precision <= 0) {
                    set_error("%s col %s: ORC DECIMAL(%d,%d) column read as "
                              "non-decimal type", fd.path.c_str(),
                              cols[c].name.c_str(), fp, fs);
                    return false;
                }
                if (fp > 18) {
                    set_error("%s col %s: ORC DECIMAL precision %d above 18 "
                              "is not supported (unscaled values ride as "
                              "INT32/INT64)", fd.path.c_str(),
                              cols[c].name.c_str(), fp);
                    return false;
                }
                if (fp != cols[c].precision || fs != cols[c].scale) {
                    set_error("%s col %s: declared decimal(%d,%d) but the "
                              "ORC file holds decimal(%d,%d)",
                              fd.path.c_str(), cols[c].name.c_str(),
                              cols[c].precision, cols[c].scale, fp, fs);
                    return false;
                }
            }
            if (!check_orc_declared(fd.path, cols[c], ckind, st)) return false;
            const int stored = cols[c].stored_esize;
            const OrcStream *data = orc_find_stream(st, cid, ORC_STREAM_DATA);
            const OrcStream *present =
                orc_find_stream(st, cid, ORC_STREAM_PRESENT);
            if (!data) {
                set_error("%s col %s: DATA stream missing", fd.path.c_str(),
                          cols[c].name.c_str());
                return false;
            }
            const int cenc =
                (int)st.encodings.size() > cid ? st.encodings[cid] : 0;
            if (ckind == ORC_STRING
                    ? (cenc != 2 && cenc != 3)
                    : (cenc != 0 && cenc != 2)) {
                set_error("%s col %s: ORC column encoding %d not supported "
                          "(ints: DIRECT/DIRECT_V2; strings: DIRECT_V2 | "
                          "DICTIONARY_V2)",
                          fd.path.c_str(), cols[c].name.c_str(), cenc);
                return false;
            }
            const OrcStream *secondary = nullptr;
            if (ckind == ORC_DECIMAL) {
                if (cenc != 2) {
                    set_error("%s col %s: ORC DECIMAL column encoding %d not "
                              "supported (DIRECT_V2 only; RLEv1 scales are "
                              "out of scope)", fd.path.c_str(),
                              cols[c].name.c_str(), cenc);
                    return false;
                }
                secondary = orc_find_stream(st, cid, ORC_STREAM_SECONDARY);
                if (!secondary) {
                    set_error("%s col %s: SECONDARY stream missing",
                              fd.path.c_str(), cols[c].name.c_str());
                    return false;
                }
            }
            if (ckind == ORC_TIMESTAMP || ckind == ORC_TIMESTAMP_INSTANT) {
                if (cenc != 2) {
                    set_error("%s col %s: ORC TIMESTAMP column encoding %d "
                              "not supported (DIRECT_V2 only; RLEv1 "
                              "timestamps are out of scope)",
                              fd.path.c_str(), cols[c].name.c_str(), cenc);
                    return false;
                }
                secondary = orc_find_stream(st, cid, ORC_STREAM_SECONDARY);
                if (!secondary) {
                    set_error("%s col %s: SECONDARY stream missing",
                              fd.path.c_str(), cols[c].name.c_str());
                    return false;
                }
            }
            // compressed streams decompress on the host at staging, like
            // the parquet zstd path (on-GPU codecs: §8f); the RLEv2/byte-RLE
            // bytes then upload verbatim
            const uint8_t *data_ptr, *pres_ptr = nullptr;
            int64_t data_len, pres_len = 0;
            std::vector<uint8_t> data_dec, pres_dec;
            if (!orc_stream_bytes(fd, sf, cols[c], data, "", data_dec,
                                  &data_ptr, &data_len) ||
                (present &&
                 !orc_stream_bytes(fd, sf, cols[c], present, " PRESENT",
                                   pres_dec, &pres_ptr, &pres_len)))
                return false;
            // where the stripe's values go: its rows of the column, or,
            // under a PRESENT stream, the dense buffer the level scatter
            // consumes
            const int64_t row0 = row_base + stripe_row;
            int64_t n_dense = st.num_rows;
            int64_t dense0 = row0;
            int dense_target = 0;
            if (ckind == ORC_FLOAT || ckind == ORC_DOUBLE) {
                // FLOAT/DOUBLE DATA streams are raw IEEE754 LE values — the
                // stream IS the decoded representation, so staging is a copy
                // (layout, not decode), exactly like parquet PLAIN packing.
                // With PRESENT, the stream holds only the non-null values.
                if (present &&
                    !stage_orc_present(fd, cols[c], pres_ptr, pres_len,
                                       st.num_rows, row0, rc, &dense0,
                                       &n_dense, &dense_target))
                    return false;
                if (data_len < n_dense * stored) {
                    set_error("%s col %s: FLOAT/DOUBLE stream short",
                              fd.path.c_str(), cols[c].name.c_str());
                    return false;
                }
                if (present) {
                    rc.dense_host.insert(rc.dense_host.end(), data_ptr,
                                         data_ptr + n_dense * stored);
                    rc.dense_segs.emplace_back(dense0, n_dense * stored);
                } else {
                    if (hipMemcpy((uint8_t *)rc.contig + row0 * stored,
                                  data_ptr, st.num_rows * stored,
                                  hipMemcpyHostToDevice) != hipSuccess) {
                        set_error("H2D failed");
                        return false;
                    }
                }
                plan->encoded_bytes_total += data_len;
                continue;
            }
            if (ckind == ORC_STRING) {
                // ORC strings (WriterImpl StringTreeWriter):
                //  - DICTIONARY_V2: DICTIONARY_DATA bytes + LENGTH (RLEv2
                //    u) describe the stripe dictionary; DATA = RLEv2 u
                //    local ids -> decode on GPU, then remap IN PLACE to
                //    the column's plan-level GLOBAL dictionary;
                //  - DIRECT_V2: LENGTH + DATA bytes -> each value interns
                //    into the global dictionary at staging (host) and the
                //    int32 ids upload directly (ids ARE the decoded form).
                if (cols[c].dtype != PMH_DT_STRING) {
                    set_error("%s col %s: ORC STRING column read as "
                              "non-string type", fd.path.c_str(),
                              cols[c].name.c_str());
                    return false;
                }
                const OrcStream *lenst =
                    orc_find_stream(st, cid, ORC_STREAM_LENGTH);
                if (!lenst) {
                    set_error("%s col %s: LENGTH stream missing",
                              fd.path.c_str(), cols[c].name.c_str());
                    return false;
                }
                const uint8_t *len_ptr;
                int64_t len_len;
                std::vector<uint8_t> len_dec;
                if (!orc_stream_bytes(fd, sf, cols[c], lenst, " LENGTH",
                                      len_dec, &len_ptr, &len_len))
                    return false;
                if (!plan->sdicts[c])
                    plan->sdicts[c].reset(new StrDict());
                StrDict *sd = plan->sdicts[c].get();
                if (present &&
                    !stage_orc_present(fd, cols[c], pres_ptr, pres_len,
                                       st.num_rows, row0, rc, &dense0,
                                       &n_dense, &dense_target))
                    return false;
                const char *why = "";
                std::vector<uint64_t> lens;
                if (cenc == 3) {  // DICTIONARY_V2
                    const OrcStream *dct =
                        orc_find_stream(st, cid, ORC_STREAM_DICTIONARY);
                    if (!dct) {
                        set_error("%s col %s: DICTIONARY_DATA missing",
                                  fd.path.c_str(), cols[c].name.c_str());
                        return false;
                    }
                    const uint8_t *dp;
                    int64_t dl;
                    std::vector<uint8_t> dict_dec;
                    if (!orc_stream_bytes(fd, sf, cols[c], dct, " DICTIONARY",
                                          dict_dec, &dp, &dl))
                        return false;
                    if (!host_rlev2(len_ptr, len_len, -1, false, lens,
                                    &why)) {
                        set_error("%s col %s: LENGTH stream decode failed "
                                  "(%s)", fd.path.c_str(),
                                  cols[c].name.c_str(), why);
                        return false;
                    }
                    std::vector<int32_t> remap(lens.size());
                    int64_t off = 0;
                    for (size_t i = 0; i < lens.size(); i++) {
                        if (off + (int64_t)lens[i] > dl) {
                            set_error("%s col %s: dictionary bytes short",
                                      fd.path.c_str(), cols[c].name.c_str());
                            return false;
                        }
                        remap[i] = sd->add(dp + off, (uint32_t)lens[i]);
                        off += (int64_t)lens[i];
                    }
                    void *rdev = plan->bufs.alloc(
                        (lens.empty() ? 1 : lens.size()) * 4);
                    if (!rdev) return false;
                    if (!lens.empty() &&
                        hipMemcpy(rdev, remap.data(), lens.size() * 4,
                                  hipMemcpyHostToDevice) != hipSuccess) {
                        set_error("H2D ORC string remap failed");
                        return false;
                    }
                    void *dev = upload_image(plan, data_ptr, data_len, 16);
                    if (!dev) return false;
                    plan->encoded_bytes_total += len_len + dl;
                    if (!prescan_rlev2(data_ptr, data_len, n_dense, 0, 4,
                                       dense_target, (uint64_t)dev, dense0,
                                       rc.rlev2_host, &why)) {
                        set_error("%s col %s: %s", fd.path.c_str(),
                                  cols[c].name.c_str(), why);
                        return false;
                    }
                    GatherTask gt;
                    gt.start = dense0;
                    gt.n = n_dense;
                    gt.dict_dev = rdev;
                    gt.to_dense = dense_target != 0;
                    gt.in_place = true;
                    rc.gathers.push_back(gt);
                } else {  // DIRECT_V2: host id-ification
                    if (!host_rlev2(len_ptr, len_len, n_dense, false, lens,
                                    &why)) {
                        set_error("%s col %s: LENGTH stream decode failed "
                                  "(%s)", fd.path.c_str(),
                                  cols[c].name.c_str(), why);
                        return false;
                    }
                    std::vector<int32_t> ids(n_dense);
                    int64_t off = 0;
                    for (int64_t i = 0; i < n_dense; i++) {
                        if (off + (int64_t)lens[i] > data_len) {
                            set_error("%s col %s: string bytes short",
                                      fd.path.c_str(), cols[c].name.c_str());
                            return false;
                        }
                        ids[i] = sd->add(data_ptr + off,
                                         (uint32_t)lens[i]);
                        off += (int64_t)lens[i];
                    }
                    plan->encoded_bytes_total += data_len + len_len;
                    if (present) {
                        const uint8_t *ib = (const uint8_t *)ids.data();
                        rc.dense_host.insert(rc.dense_host.end(), ib,
                                             ib + n_dense * 4);
                        rc.dense_segs.emplace_back(dense0, n_dense * 4);
                    } else if (n_dense &&
                               hipMemcpy((uint8_t *)rc.contig + row0 * 4,
                                         ids.data(), n_dense * 4,
                                         hipMemcpyHostToDevice) !=
                                   hipSuccess) {
                        set_error("H2D failed");
                        return false;
                    }
                }
                continue;
            }
            // upload the encoded DATA stream (+16 B pad: the RLEv2
            // bit reader uses an aligned 16-byte window)
            void *dev = upload_image(plan, data_ptr, data_len, 16);
            if (!dev) return false;
            if (present &&
                !stage_orc_present(fd, cols[c], pres_ptr, pres_len,
                                   st.num_rows, row0, rc, &dense0, &n_dense,
                                   &dense_target))
                return false;
            // DECIMAL and TIMESTAMP: the SECONDARY stream's chunks, based
            // at 0 until the stream is uploaded
            const uint8_t *sec_ptr = nullptr;
            int64_t sec_len = 0;
            std::vector<uint8_t> sec_dec;
            std::vector<Rlev2Chunk> sch;
            const char *why = "";
            if (secondary) {
                const bool dec = ckind == ORC_DECIMAL;
                if (!orc_stream_bytes(fd, sf, cols[c], secondary,
                                      " SECONDARY", sec_dec, &sec_ptr,
                                      &sec_len))
                    return false;
                // decimal: signed data scales to the (run, column) scale
                // scratch; timestamp: unsigned stored nanos to its nanos
                // scratch
                if (!prescan_rlev2(sec_ptr, sec_len, n_dense, dec, dec ? 4 : 8,
                                   dec ? 2 : 3, 0,
                                   dec ? rc.scale_rows : rc.nanos_rows, sch,
                                   &why)) {
                    set_error("%s col %s SECONDARY: %s", fd.path.c_str(),
                              cols[c].name.c_str(), why);
                    return false;
                }
            }
            bool ok;
            if (ckind == ORC_DECIMAL) {
                // Constant scale runs equal to the column scale (what the
                // common writers emit) need no device work at all; anything
                // else decodes through k_rlev2
                const int64_t sc0 = rc.scale_rows;
                bool uniform = true;
                int64_t sc_end = sc0;
                for (const auto &k : sch) {
                    const bool constant =
                        k.kind == 0 ||
                        (k.kind == 3 && k.width == 0 && k.delta == 0);
                    if (!constant || k.base != cols[c].scale) uniform = false;
                    sc_end = k.out_start + k.count;
                }
                if (!uniform) {
                    // the scratch is sized by the value count: a stream
                    // whose last run decodes past it is refused
                    if (sc_end != sc0 + n_dense) {
                        set_error("%s col %s: SECONDARY stream holds %lld "
                                  "scales for %lld values", fd.path.c_str(),
                                  cols[c].name.c_str(),
                                  (long long)(sc_end - sc0),
                                  (long long)n_dense);
                        return false;
                    }
                    if (!upload_rebase(plan, sec_ptr, sec_len, sch))
                        return false;
                    rc.rlev2_host.insert(rc.rlev2_host.end(), sch.begin(),
                                         sch.end());
                    rc.scale_rows += n_dense;
                }
                const size_t u0 = rc.varint_host.size();
                ok = prescan_varint(data_ptr, data_len, n_dense, stored,
                                    cols[c].precision, cols[c].scale,
                                    dense_target, (uint64_t)dev, dense0,
                                    rc.varint_host, &why);
                if (ok && !uniform)
                    for (size_t i = u0; i < rc.varint_host.size(); i++) {
                        VarintUnit &vu = rc.varint_host[i];
                        vu.scale_addr =
                            (uint64_t)(1 + sc0 + (vu.out_start - dense0));
                    }
            } else if (ckind == ORC_TIMESTAMP ||
                       ckind == ORC_TIMESTAMP_INSTANT) {
                const int64_t n0 = rc.nanos_rows;
                int64_t n_end = n0;
                for (const auto &k : sch) n_end = k.out_start + k.count;
                // the scratch is sized by the value count: a stream whose
                // last run decodes past it is refused
                if (n_end != n0 + n_dense) {
                    set_error("%s col %s: SECONDARY stream holds %lld nanos "
                              "for %lld values", fd.path.c_str(),
                              cols[c].name.c_str(), (long long)(n_end - n0),
                              (long long)n_dense);
                    return false;
                }
                if (!upload_rebase(plan, sec_ptr, sec_len, sch)) return false;
                // DATA: signed RLEv2 seconds relative to 2015-01-01, to the
                // column (or its dense buffer) as int64
                const size_t v0 = rc.rlev2_host.size();
                ok = prescan_rlev2(data_ptr, data_len, n_dense, 1, 8,
                                   dense_target, (uint64_t)dev, dense0,
                                   rc.rlev2_host, &why);
                if (ok) {
                    int64_t d_end = dense0;
                    for (size_t i = v0; i < rc.rlev2_host.size(); i++)
                        d_end = rc.rlev2_host[i].out_start +
                                rc.rlev2_host[i].count;
                    if (d_end != dense0 + n_dense) {
                        set_error("%s col %s: DATA stream holds %lld seconds "
                                  "for %lld values", fd.path.c_str(),
                                  cols[c].name.c_str(),
                                  (long long)(d_end - dense0),
                                  (long long)n_dense);
                        return false;
                    }
                    rc.rlev2_host.insert(rc.rlev2_host.end(), sch.begin(),
                                         sch.end());
                    rc.nanos_rows += n_dense;
                    for (int64_t d = 0; d < n_dense; d += OTS_UNIT_VALUES) {
                        TsUnit tu{};
                        tu.out_start = dense0 + d;
                        tu.nanos_start = n0 + d;
                        tu.count = (int32_t)std::min<int64_t>(
                            OTS_UNIT_VALUES, n_dense - d);
                        tu.unit = logical_is_micros(cols[c].logical)
                                      ? OTS_UNIT_MICROS
                                      : OTS_UNIT_MILLIS;
                        tu.dense_target = (uint8_t)dense_target;
                        rc.ts_host.push_back(tu);
                    }
                }
            } else if (ckind == ORC_BOOLEAN) {
                // DATA: byte-RLE over MSB-first bytes; one unit per run or
                // literal group, expanded by k_bits_expand at read time
                ok = prescan_boolrle(data_ptr, data_len, n_dense, stored,
                                     dense_target, (uint64_t)dev, dense0,
                                     rc.bits_host, &why);
            } else if (ckind == ORC_BYTE) {
                ok = prescan_byterle(data_ptr, data_len, n_dense, stored,
                                     dense_target, (uint64_t)dev, dense0,
                                     rc.rlev2_host, &why);
            } else if (ckind == ORC_SHORT || ckind == ORC_INT ||
                       ckind == ORC_LONG || ckind == ORC_DATE) {
                ok = prescan_rlev2(data_ptr, data_len, n_dense, 1, stored,
                                   dense_target, (uint64_t)dev, dense0,
                                   rc.rlev2_host, &why);
            } else {
                set_error("%s col %s: ORC type kind %d not supported yet",
                          fd.path.c_str(), cols[c].name.c_str(), ckind);
                return false;
            }
            if (!ok) {
                set_error("%s col %s: %s", fd.path.c_str(),
                          cols[c].name.c_str(), why);
                return false;
            }
        }
        stripe_row += st.num_rows;
    }
    if (stripe_row != fd.row_count) {
        set_error("%s: rowCount %lld != file rows %lld", fd.path.c_str(),
                  (long long)fd.row_count, (long long)stripe_row);
        return false;
    }
    return true;
}

// Stage one run (list of files) for the required columns onto the device.
// Upload one chunk's dictionary for k_dict_gather. Numeric columns upload
// the raw fixed-width values; STRING columns remap the chunk's byte-array
// entries into the column's plan-level GLOBAL dictionary and upload the
// int32 remap table instead (ids then decode straight to global ids).
static bool upload_chunk_dict(pmh_plan_t *plan, int c,
                              const uint8_t *dict_host, int64_t dict_count,
                              int stored, void **out) {
    if (plan->cols[c].dtype == PMH_DT_STRING) {
        if (!plan->sdicts[c]) plan->sdicts[c].reset(new StrDict());
        StrDict *sd = plan->sdicts[c].get();
        std::vector<int32_t> remap((size_t)dict_count);
        const uint8_t *p = dict_host;
        for (int64_t i = 0; i < dict_count; i++) {
            uint32_t len;
            memcpy(&len, p, 4);
            p += 4;
            remap[i] = sd->add(p, len);
            p += len;
        }
        void *dev = plan->bufs.alloc((dict_count ? dict_count : 1) * 4);
        if (!dev) return false;
        if (dict_count &&
            hipMemcpy(dev, remap.data(), dict_count * 4,
                      hipMemcpyHostToDevice) != hipSuccess) {
            set_error("H2D string remap failed");
            return false;
        }
        *out = dev;
        return true;
    }
    void *dev = plan->bufs.alloc(dict_count * stored);
    if (!dev) return false;
    if (hipMemcpy(dev, dict_host, dict_count * stored,
                  hipMemcpyHostToDevice) != hipSuccess) {
        set_error("H2D dict failed");
        return false;
    }
    *out = dev;
    return true;
}

// Byte length of a page's payload in its chunk's uncompressed image.
static int64_t page_len(const ColumnChunkMeta &cc, const PageMeta &pg) {
    return cc.codec != CODEC_UNCOMPRESSED ? pg.uncompressed_size
                                          : pg.compressed_size;
}

// Upload a chunk's payload image (everything up to its longest page end;
// ppo = the pages' offsets in it) for the device decoders.
static void *upload_chunk_image(pmh_plan_t *plan, const ColumnChunkMeta &cc,
                                const std::vector<int64_t> &ppo,
                                const uint8_t *payload_base, int pad) {
    int64_t payload_len = 0;
    for (size_t pi = 0; pi < cc.pages.size(); pi++)
        payload_len =
            std::max(payload_len, ppo[pi] + page_len(cc, cc.pages[pi]));
    return upload_image(plan, payload_base, payload_len, pad);
}

// Stage a v1 data page's def levels (pp = the page, vpos = where its values
// begin: 4 length bytes + the level stream, checked against the page) into
// the column's levels buffer and def chunks. *before = the dense cursor
// before the page, *nvalid = the page's non-null values.
static bool stage_page_def(const FileDesc &fd, const ColSpec &cs,
                           const uint8_t *pp, int64_t vpos, int64_t n_values,
                           int64_t out_row0, RunCol &rc, int64_t *before,
                           int64_t *nvalid) {
    const int64_t rel = (int64_t)rc.levels_host.size();
    rc.levels_host.insert(rc.levels_host.end(), pp + 4, pp + vpos);
    *before = rc.dense_before;
    const char *why = "";
    if (!prescan_def(pp + 4, vpos - 4, n_values, out_row0, rel,
                     &rc.dense_before, rc.def_host, &why)) {
        set_error("%s col %s: %s", fd.path.c_str(), cs.name.c_str(), why);
        return false;
    }
    *nvalid = rc.dense_before - *before;
    return true;
}

// Prescan a dictionary-encoded page's id stream (at vpos of page pp: the bit
// width byte, then hybrid RLE) into the column's RLE chunks. page_dev = the
// page's device address.
static bool stage_page_ids(const FileDesc &fd, const ColSpec &cs,
                           const uint8_t *pp, int64_t plen, int64_t vpos,
                           int64_t n_values, int64_t out_base,
                           uint64_t page_dev, RunCol &rc) {
    const char *why = "dictionary id stream lacks its bit-width byte";
    if (vpos >= plen ||
        !prescan_rle(pp + vpos + 1, plen - vpos - 1, pp[vpos], n_values,
                     out_base, page_dev, vpos + 1, rc.rle_host, &why)) {
        set_error("%s col %s: %s", fd.path.c_str(), cs.name.c_str(), why);
        return false;
    }
    return true;
}

static bool stage_run(pmh_plan_t *plan, const std::vector<FileDesc> &files,
                      Run &run) {
    const auto &cols = plan->cols;
    run.cols.resize(cols.size());
    int64_t total_rows = 0;
    for (const auto &fd : files) total_rows += fd.row_count;
    run.level = files.empty() ? 0 : files[0].level;
    if (total_rows >= ((int64_t)1 << PMH_ROW_BITS)) {
        // a run is the CONCATENATION of non-overlapping files; the winner
        // packing (run | row) indexes into the whole run, so the cap applies
        // to the run total, not per file (a >=2^row-bits run would silently
        // overflow into the run bits and merge wrong)
        set_error("run totals %lld rows >= 2^%d per-run limit (%zu files)",
                  (long long)total_rows, PMH_ROW_BITS, files.size());
        return false;
    }
    for (size_t c = 0; c < cols.size(); c++) {
        RunCol &rc = run.cols[c];
        rc.contig = plan->bufs.alloc(total_rows * cols[c].stored_esize);
        if (!rc.contig) {
            set_error("hipMalloc failed (%lld rows col %s)",
                      (long long)total_rows, cols[c].name.c_str());
            return false;
        }
        plan->encoded_bytes_total += total_rows * cols[c].stored_esize;
    }
    std::vector<uint8_t> tomb_host;
    {
        int64_t rb = 0;
        for (const auto &fd : files) {
            if (!fd.dv_path.empty()) {
                // ApplyDeletionVectorReader semantics (io/
                // KeyValueFileReaderFactory.java:139-143): deleted positions
                // never reach the merge — staged as per-run tombstones the
                // merge kernels treat as nonexistent rows
                std::vector<uint32_t> pos;
                if (!load_deletion_vector(fd.dv_path, fd.dv_offset,
                                          fd.dv_length, pos))
                    return false;
                if (tomb_host.empty()) tomb_host.assign(total_rows, 0);
                for (uint32_t pp : pos) {
                    if ((int64_t)pp < fd.row_count)
                        tomb_host[rb + pp] = 1;
                }
            }
            rb += fd.row_count;
        }
    }
    if (!tomb_host.empty()) {
        run.tomb = (uint8_t *)plan->bufs.alloc(total_rows);
        if (!run.tomb ||
            hipMemcpy(run.tomb, tomb_host.data(), total_rows,
                      hipMemcpyHostToDevice) != hipSuccess) {
            set_error("H2D tombstones failed");
            return false;
        }
    }
    int64_t row_base = 0;
    for (const auto &fd : files) {
        StagedFile sf;
        if (!load_file(fd.path, sf)) return false;
        if (sf.orc) {
            if (!stage_orc_file(plan, fd, sf, run, row_base)) return false;
            row_base += fd.row_count;
            continue;
        }
        std::vector<int> leaf(cols.size(), -1);
        for (size_t c = 0; c < cols.size(); c++) {
            for (size_t i = 0; i < sf.meta.schema_names.size(); i++)
                if (sf.meta.schema_names[i] == cols[c].name) leaf[c] = (int)i;
            if (leaf[c] < 0) {
                set_error("%s: column %s not found", fd.path.c_str(),
                          cols[c].name.c_str());
                return false;
            }
            if (cols[c].is_bool || cols[c].logical) {
                if (!check_parquet_declared(fd.path, cols[c], sf.meta,
                                            leaf[c]))
                    return false;
                continue;
            }
            if ((int)sf.meta.phys_types.size() > leaf[c] &&
                sf.meta.phys_types[leaf[c]] != expected_phys(cols[c].dtype)) {
                set_error("%s: column %s physical type %d does not match "
                          "declared type (expect %d; decimals ride "
                          "INT32/INT64 per ParquetSchemaConverter.java:"
                          "153-171, strings BYTE_ARRAY)",
                          fd.path.c_str(), cols[c].name.c_str(),
                          sf.meta.phys_types[leaf[c]],
                          expected_phys(cols[c].dtype));
                return false;
            }
        }
        // file-level GPU zstd pre-pass: decode EVERY
        // selected zstd chunk's pages in ONE k_zstd_pages batch — thousands
        // of wavefronts in flight hide the per-page serial decode latency
        // that per-chunk batches cannot. Failure falls back to the host
        // codec per chunk.
        std::vector<uint8_t> file_unc;
        std::map<const void *, int64_t> zchunk_base;
        // chunks whose decoded image can stay DEVICE-RESIDENT (simple
        // PLAIN, no def levels, no dictionary page): their uncompressed
        // bytes never cross PCIe — the PLAIN staging copies D2D
        std::map<const void *, uint8_t *> zchunk_dev;
        if (gpu_zstd_enabled()) {
            std::vector<ZstdBatchPage> zp;
            std::vector<std::pair<int64_t, int64_t>> host_rngs;
            int64_t lo = INT64_MAX, hi = 0, out = 0;
            // chunk classes: HOST (dict pages / non-PLAIN / strings:
            // full D2H), PREFIX (PLAIN under a nullable schema: D2H only
            // each page's def-level prefix; values stay on device unless
            // the prefix shows REAL nulls), DEV (required PLAIN: nothing
            // copies back)
            struct PfxChunk {
                const void *cc;
                int64_t base;
                int leafc;
            };
            std::vector<PfxChunk> pfx_chunks;
            const int64_t PFX = 16384;
            for (auto &rg : sf.meta.row_groups)
                for (size_t c = 0; c < cols.size(); c++) {
                    auto &cc = rg.columns[leaf[c]];
                    if (cc.codec != CODEC_ZSTD || cc.pages.empty()) continue;
                    if (zchunk_base.count(&cc)) continue;
                    zchunk_base[&cc] = out;
                    // boolean pages are bit-packed: staging walks them on
                    // the host, they never stage as PLAIN column bytes
                    bool needs_host =
                        cols[c].dtype == PMH_DT_STRING || cols[c].is_bool;
                    const bool has_def =
                        sf.meta.max_def_levels[leaf[c]] > 0;
                    int64_t c0 = out;
                    for (auto &pg : cc.pages) {
                        if (pg.page_type == 2 ||
                            (pg.page_type == 0 &&
                             pg.encoding != ENC_PLAIN))
                            needs_host = true;
                        if (pg.data_off < lo) lo = pg.data_off;
                        if (pg.data_off + pg.compressed_size > hi)
                            hi = pg.data_off + pg.compressed_size;
                        zp.push_back({pg.data_off, pg.compressed_size, out,
                                      pg.uncompressed_size});
                        out += pg.uncompressed_size;
                    }
                    if (needs_host)
                        host_rngs.push_back({c0, out});
                    else if (has_def)
                        pfx_chunks.push_back({&cc, c0, leaf[c]});
                    else
                        zchunk_dev[&cc] = nullptr;  // patched below
                }
            if (!zp.empty()) {
                for (auto &p : zp) p.src_off -= lo;
                file_unc.resize(out);
                uint8_t *dev_blob = nullptr;
                // page-prefix ranges for PREFIX chunks (def levels live
                // at page start)
                for (const auto &pc : pfx_chunks) {
                    const auto &cc =
                        *(const ColumnChunkMeta *)pc.cc;
                    int64_t o = pc.base;
                    for (auto &pg : cc.pages) {
                        int64_t take = pg.uncompressed_size < PFX
                                           ? pg.uncompressed_size
                                           : PFX;
                        host_rngs.push_back({o, o + take});
                        o += pg.uncompressed_size;
                    }
                }
                if (gpu_zstd_batch_dev(sf.data.data() + lo, hi - lo, zp,
                                       plan, &dev_blob, out, host_rngs,
                                       file_unc.data())) {
                    plan->stats.gpu_zstd_pages += (int64_t)zp.size();
                    // PREFIX chunks: stay on device unless a page's def
                    // stream shows real nulls (or overflows the prefix) —
                    // then the chunk needs its full host image
                    for (const auto &pc : pfx_chunks) {
                        const auto &cc =
                            *(const ColumnChunkMeta *)pc.cc;
                        bool full = false;
                        int64_t o = pc.base, cend = pc.base;
                        for (auto &pg : cc.pages)
                            cend += pg.uncompressed_size;
                        for (auto &pg : cc.pages) {
                            if (pg.page_type == 0) {
                                // a length that does not fit the page takes
                                // the host path, which refuses it
                                const int64_t have =
                                    std::min<int64_t>(pg.uncompressed_size,
                                                      PFX);
                                uint32_t dl = 0;
                                if (have >= 4)
                                    memcpy(&dl, file_unc.data() + o, 4);
                                if (4 + (int64_t)dl > have ||
                                    def_levels_have_nulls(
                                        file_unc.data() + o + 4, dl,
                                        pg.num_values))
                                    full = true;
                            }
                            o += pg.uncompressed_size;
                            if (full) break;
                        }
                        if (full) {
                            if (hipMemcpy(file_unc.data() + pc.base,
                                          dev_blob + pc.base,
                                          cend - pc.base,
                                          hipMemcpyDeviceToHost) !=
                                hipSuccess) {
                                set_error("zstd prefix D2H failed");
                                return false;
                            }
                        } else {
                            zchunk_dev[pc.cc] = nullptr;
                        }
                    }
                    for (auto &kv : zchunk_dev)
                        kv.second = dev_blob + zchunk_base[kv.first];
                    if (getenv("PMH_DEBUG_ZSTD"))
                        fprintf(stderr,
                                "[zstd] file chunks=%zu dev-resident=%zu "
                                "host-rngs=%zu\n",
                                zchunk_base.size(), zchunk_dev.size(),
                                host_rngs.size());
                } else {
                    file_unc.clear();
                    zchunk_base.clear();
                    zchunk_dev.clear();
                }
            }
        }
        int64_t rg_row = 0;
        for (auto &rg : sf.meta.row_groups) {
            for (size_t c = 0; c < cols.size(); c++) {
                auto &cc = rg.columns[leaf[c]];
                RunCol &rc = run.cols[c];
                const int stored = cols[c].stored_esize;
                const int max_def = sf.meta.max_def_levels[leaf[c]];
                const int64_t chunk_row0 = row_base + rg_row;
                // uncompressed payload image of this chunk
                int64_t chunk_start = cc.dictionary_page_offset
                                          ? cc.dictionary_page_offset
                                          : cc.data_page_offset;
                std::vector<uint8_t> packed;  // compressed codecs
                std::vector<int64_t> ppo(cc.pages.size());
                const uint8_t *payload_base = sf.data.data() + chunk_start;
                const uint8_t *zdev_base = nullptr;
                auto zit = zchunk_base.find((const void *)&cc);
                if (zit != zchunk_base.end()) {
                    // pages already decoded by the file-level k_zstd_pages
                    // batch; the chunk's image starts at zit->second.
                    // Device-resident chunks (zchunk_dev) never copied
                    // back — the PLAIN staging below goes D2D.
                    int64_t o = 0;
                    for (size_t pi = 0; pi < cc.pages.size(); pi++) {
                        ppo[pi] = o;
                        o += cc.pages[pi].uncompressed_size;
                    }
                    payload_base = file_unc.data() + zit->second;
                    auto zdv = zchunk_dev.find((const void *)&cc);
                    if (zdv != zchunk_dev.end()) zdev_base = zdv->second;
                } else if (cc.codec == CODEC_ZSTD || cc.codec == CODEC_GZIP ||
                    cc.codec == CODEC_SNAPPY) {
                    int64_t total_unc = 0;
                    for (auto &pg : cc.pages) total_unc += pg.uncompressed_size;
                    packed.resize(total_unc);
                    int64_t off = 0;
                    for (size_t pi = 0; pi < cc.pages.size(); pi++) {
                        auto &pg = cc.pages[pi];
                        std::string cerr;
                        size_t got = 0;
                        bool ok;
                        if (cc.codec == CODEC_ZSTD)
                            ok = zstd_decompress(
                                sf.data.data() + pg.data_off,
                                pg.compressed_size, packed.data() + off,
                                pg.uncompressed_size);
                        else if (cc.codec == CODEC_GZIP)
                            ok = gzip_decompress_exact(
                                sf.data.data() + pg.data_off,
                                pg.compressed_size, packed.data() + off,
                                pg.uncompressed_size, cerr);
                        else
                            ok = snappy_decompress(
                                     sf.data.data() + pg.data_off,
                                     pg.compressed_size, packed.data() + off,
                                     pg.uncompressed_size, got, cerr) &&
                                 got == (size_t)pg.uncompressed_size;
                        if (!ok) {
                            if (!cerr.empty()) set_error("%s", cerr.c_str());
                            else if (cc.codec == CODEC_SNAPPY)
                                set_error("snappy page size mismatch");
                            return false;
                        }
                        ppo[pi] = off;
                        off += pg.uncompressed_size;
                    }
                    payload_base = packed.data();
                } else if (cc.codec == CODEC_UNCOMPRESSED) {
                    for (size_t pi = 0; pi < cc.pages.size(); pi++)
                        ppo[pi] = cc.pages[pi].data_off - chunk_start;
                } else {
                    set_error("%s: unsupported codec %d", fd.path.c_str(),
                              cc.codec);
                    return false;
                }
                // classify data pages
                bool has_plain = false, has_dict = false, has_delta = false,
                     has_dba = false;
                const uint8_t *dict_host = nullptr;
                int64_t dict_count = 0;
                for (size_t pi = 0; pi < cc.pages.size(); pi++) {
                    auto &pg = cc.pages[pi];
                    if (cols[c].is_bool &&
                        !check_bool_page(fd.path, cols[c], pg))
                        return false;
                    if (pg.page_type == 2) {
                        dict_host = payload_base + ppo[pi];
                        dict_count = pg.num_values;
                    } else if (pg.encoding == ENC_PLAIN) {
                        has_plain = true;
                    } else if (pg.encoding == ENC_RLE_DICTIONARY ||
                               pg.encoding == ENC_PLAIN_DICTIONARY) {
                        has_dict = true;
                    } else if (pg.encoding == ENC_DELTA_BINARY_PACKED) {
                        has_delta = true;
                    } else if ((pg.encoding == ENC_DELTA_BYTE_ARRAY ||
                                pg.encoding ==
                                    ENC_DELTA_LENGTH_BYTE_ARRAY) &&
                               cols[c].dtype == PMH_DT_STRING) {
                        // DELTA_LENGTH_BYTE_ARRAY = DELTA_BYTE_ARRAY with
                        // no prefix stream (lengths + bytes)
                        has_dba = true;
                    } else {
                        set_error("%s: unsupported encoding %d",
                                  fd.path.c_str(), pg.encoding);
                        return false;
                    }
                }
                if (has_plain && has_dict) {
                    set_error("%s col %s: mixed PLAIN/dictionary pages in one "
                              "chunk not supported yet",
                              fd.path.c_str(), cols[c].name.c_str());
                    return false;
                }
                if ((has_delta || has_dba) &&
                    (has_plain || has_dict || (has_delta && has_dba))) {
                    set_error("%s col %s: mixed DELTA/other pages in one "
                              "chunk not supported", fd.path.c_str(),
                              cols[c].name.c_str());
                    return false;
                }
                if (cols[c].dtype == PMH_DT_STRING && has_plain) {
                    set_error("%s col %s: PLAIN byte-array pages are not on "
                              "the GPU path yet — string columns must be "
                              "dictionary-encoded (the parquet writer "
                              "default; C5's dictionary strings are)",
                              fd.path.c_str(), cols[c].name.c_str());
                    return false;
                }
                // per-page value offsets past def levels (+ null detection)
                std::vector<int64_t> vpos(cc.pages.size(), 0);
                bool chunk_nulls = false;
                for (size_t pi = 0; pi < cc.pages.size(); pi++) {
                    auto &pg = cc.pages[pi];
                    if (pg.page_type != 0) continue;
                    const uint8_t *pp = payload_base + ppo[pi];
                    if (max_def == 0) continue;
                    uint32_t dl_len = 0;
                    if (page_len(cc, pg) >= 4) memcpy(&dl_len, pp, 4);
                    if (4 + (int64_t)dl_len > page_len(cc, pg)) {
                        set_error("%s col %s: def-level stream of %lld bytes "
                                  "does not fit its %lld-byte page",
                                  fd.path.c_str(), cols[c].name.c_str(),
                                  (long long)dl_len,
                                  (long long)page_len(cc, pg));
                        return false;
                    }
                    chunk_nulls |= def_levels_have_nulls(pp + 4, dl_len,
                                                         pg.num_values);
                    vpos[pi] = 4 + dl_len;
                }
                if (cols[c].is_bool) {
                    // PLAIN booleans: 1 bit per value, LSB first, every page
                    // restarting on a byte boundary. The payload image
                    // uploads verbatim (+16 B pad, the staging convention);
                    // k_bits_expand materialises the column at read time,
                    // into the dense buffer where the chunk has nulls
                    // (k_level_scatter positions them, as for DELTA)
                    void *dev =
                        upload_chunk_image(plan, cc, ppo, payload_base, 16);
                    if (!dev) return false;
                    if (chunk_nulls) rc.has_nulls = true;
                    for (size_t pi = 0; pi < cc.pages.size(); pi++) {
                        auto &pg = cc.pages[pi];
                        if (pg.page_type != 0) continue;
                        const uint8_t *pp = payload_base + ppo[pi];
                        const int64_t pos = vpos[pi];
                        const int64_t plen = page_len(cc, pg);
                        int64_t n_vals = pg.num_values;
                        int64_t out0 = chunk_row0 + pg.first_row;
                        int target = 0;
                        if (chunk_nulls && max_def > 0) {
                            if (!stage_page_def(fd, cols[c], pp, pos,
                                                pg.num_values, out0, rc,
                                                &out0, &n_vals))
                                return false;
                            target = 1;
                        }
                        const char *why = "";
                        if (!prescan_bits_plain(
                                pp + pos, plen - pos, n_vals, stored, target,
                                (uint64_t)dev + (uint64_t)(ppo[pi] + pos),
                                out0, rc.bits_host, &why)) {
                            set_error("%s col %s: %s", fd.path.c_str(),
                                      cols[c].name.c_str(), why);
                            return false;
                        }
                    }
                } else if (has_dba) {
                    // DELTA_BYTE_ARRAY strings (VectorizedDeltaByteArray-
                    // Reader.java): per page, prefix lengths (DELTA) +
                    // suffix lengths (DELTA) + suffix bytes; values share
                    // prefixes with their predecessor. They intern into
                    // the plan-level GLOBAL dictionary at staging (the ids
                    // are the device representation, like ORC DIRECT_V2).
                    if (!plan->sdicts[c])
                        plan->sdicts[c].reset(new StrDict());
                    StrDict *sd = plan->sdicts[c].get();
                    for (size_t pi = 0; pi < cc.pages.size(); pi++) {
                        auto &pg = cc.pages[pi];
                        if (pg.page_type != 0) continue;
                        const uint8_t *pp = payload_base + ppo[pi];
                        int64_t plen2 = page_len(cc, pg);
                        int64_t row0 = chunk_row0 + pg.first_row;
                        int64_t n_dense = pg.num_values;
                        int64_t dense0 = row0;
                        const bool to_dense = max_def > 0 && chunk_nulls;
                        if (to_dense) {
                            rc.has_nulls = true;
                            if (!stage_page_def(fd, cols[c], pp, vpos[pi],
                                                pg.num_values, row0, rc,
                                                &dense0, &n_dense))
                                return false;
                        }
                        int64_t pos = vpos[pi];
                        std::vector<int64_t> pre, suf;
                        const bool dlba =
                            pg.encoding == ENC_DELTA_LENGTH_BYTE_ARRAY;
                        const char *why = "short of the page's values";
                        int64_t used;
                        if (dlba) {
                            pre.assign((size_t)n_dense, 0);  // no prefixes
                        } else {
                            used = host_delta_i64(pp + pos, plen2 - pos, pre,
                                                  &why);
                            if (used < 0 ||
                                (int64_t)pre.size() < n_dense) {
                                set_error("%s col %s: DELTA_BYTE_ARRAY "
                                          "prefix stream bad (%s)",
                                          fd.path.c_str(),
                                          cols[c].name.c_str(), why);
                                return false;
                            }
                            pos += used;
                        }
                        used = host_delta_i64(pp + pos, plen2 - pos, suf,
                                              &why);
                        if (used < 0 ||
                            (int64_t)suf.size() < n_dense) {
                            set_error("%s col %s: DELTA_BYTE_ARRAY suffix "
                                      "stream bad (%s)", fd.path.c_str(),
                                      cols[c].name.c_str(), why);
                            return false;
                        }
                        pos += used;
                        std::string prev;
                        std::vector<int32_t> ids(n_dense);
                        for (int64_t i = 0; i < n_dense; i++) {
                            int64_t pl = pre[i], sl = suf[i];
                            if (pl < 0 || sl < 0 ||
                                pl > (int64_t)prev.size() ||
                                pos + sl > plen2) {
                                set_error("%s col %s: DELTA_BYTE_ARRAY "
                                          "lengths bad", fd.path.c_str(),
                                          cols[c].name.c_str());
                                return false;
                            }
                            std::string v = prev.substr(0, pl);
                            v.append((const char *)pp + pos, (size_t)sl);
                            pos += sl;
                            ids[i] = sd->add((const uint8_t *)v.data(),
                                             (uint32_t)v.size());
                            prev = std::move(v);
                        }
                        plan->encoded_bytes_total += plen2;
                        if (to_dense) {
                            const uint8_t *ib = (const uint8_t *)ids.data();
                            rc.dense_host.insert(rc.dense_host.end(), ib,
                                                 ib + n_dense * 4);
                            rc.dense_segs.emplace_back(dense0, n_dense * 4);
                        } else if (n_dense &&
                                   hipMemcpy((uint8_t *)rc.contig +
                                                 row0 * 4,
                                             ids.data(), n_dense * 4,
                                             hipMemcpyHostToDevice) !=
                                       hipSuccess) {
                            set_error("H2D failed");
                            return false;
                        }
                    }
                } else if (has_delta) {
                    if (cols[c].dtype == PMH_DT_STRING) {
                        set_error("%s col %s: DELTA byte arrays are a later "
                                  "round", fd.path.c_str(),
                                  cols[c].name.c_str());
                        return false;
                    }
                    // upload the encoded payload image (+16 B pad for the
                    // device bit-window loads); blocks decode on GPU at
                    // read time (k_delta_sum/scan/emit)
                    void *dev =
                        upload_chunk_image(plan, cc, ppo, payload_base, 16);
                    if (!dev) return false;
                    if (chunk_nulls) rc.has_nulls = true;
                    for (size_t pi = 0; pi < cc.pages.size(); pi++) {
                        auto &pg = cc.pages[pi];
                        if (pg.page_type != 0) continue;
                        const uint8_t *pp = payload_base + ppo[pi];
                        int64_t pos = vpos[pi];
                        int64_t n_vals = pg.num_values;
                        int64_t out0 = chunk_row0 + pg.first_row;
                        uint64_t out_addr = (uint64_t)rc.contig;
                        if (chunk_nulls && max_def > 0) {
                            // nullable DELTA: the stream encodes only the
                            // NON-NULL values — decode them to the dense
                            // buffer (out_addr 0 patched to dense_dev at
                            // finalize) and let k_level_scatter position
                            // them like dense PLAIN/dictionary values
                            if (!stage_page_def(fd, cols[c], pp, pos,
                                                pg.num_values, out0, rc,
                                                &out0, &n_vals))
                                return false;
                            out_addr = 0;
                        }
                        const char *why = "";
                        if (!prescan_delta(pp + pos, page_len(cc, pg) - pos,
                                           n_vals, out0, (uint64_t)dev,
                                           ppo[pi] + pos, out_addr, stored,
                                           rc.delta_host, rc.dstreams_host,
                                           &why)) {
                            set_error("%s col %s: %s", fd.path.c_str(),
                                      cols[c].name.c_str(), why);
                            return false;
                        }
                    }
                } else if (chunk_nulls && has_dict) {
                    // dictionary chunk with nulls: def-level streams stay
                    // encoded; the id stream decodes to DENSE positions on
                    // the GPU (k_rle_decode), k_dict_gather fills the dense
                    // buffer, and k_level_scatter positions the rows
                    rc.has_nulls = true;
                    if (!dict_host) {
                        set_error("%s: dictionary page missing",
                                  fd.path.c_str());
                        return false;
                    }
                    rc.dict_encoded = true;
                    void *dev =
                        upload_chunk_image(plan, cc, ppo, payload_base, 0);
                    if (!dev) return false;
                    int64_t dense_start = rc.dense_before;
                    for (size_t pi = 0; pi < cc.pages.size(); pi++) {
                        auto &pg = cc.pages[pi];
                        if (pg.page_type != 0) continue;
                        const uint8_t *pp = payload_base + ppo[pi];
                        int64_t before, nvalid;
                        if (!stage_page_def(fd, cols[c], pp, vpos[pi],
                                            pg.num_values,
                                            chunk_row0 + pg.first_row, rc,
                                            &before, &nvalid) ||
                            !stage_page_ids(fd, cols[c], pp, page_len(cc, pg),
                                            vpos[pi], nvalid, before,
                                            (uint64_t)dev + ppo[pi], rc))
                            return false;
                    }
                    void *dict_dev = nullptr;
                    if (!upload_chunk_dict(plan, (int)c, dict_host,
                                           dict_count, stored, &dict_dev))
                        return false;
                    GatherTask gt;
                    gt.start = dense_start;
                    gt.n = rc.dense_before - dense_start;
                    gt.dict_dev = dict_dev;
                    gt.to_dense = true;
                    rc.gathers.push_back(gt);
                } else if (chunk_nulls) {
                    // dense PLAIN values + def-level streams stay encoded;
                    // k_level_scatter positions them at read time
                    rc.has_nulls = true;
                    for (size_t pi = 0; pi < cc.pages.size(); pi++) {
                        auto &pg = cc.pages[pi];
                        if (pg.page_type != 0) continue;
                        const uint8_t *pp = payload_base + ppo[pi];
                        int64_t before, nvalid;
                        if (!stage_page_def(fd, cols[c], pp, vpos[pi],
                                            pg.num_values,
                                            chunk_row0 + pg.first_row, rc,
                                            &before, &nvalid))
                            return false;
                        rc.dense_host.insert(
                            rc.dense_host.end(), pp + vpos[pi],
                            pp + vpos[pi] + nvalid * stored);
                        rc.dense_segs.emplace_back(before,
                                                   nvalid * stored);
                    }
                } else if ((has_plain || (!has_dict && cc.num_values > 0))
                           && zdev_base) {
                    // PLAIN pages already decoded on DEVICE: stage D2D
                    int64_t row_at = chunk_row0;
                    for (size_t pi = 0; pi < cc.pages.size(); pi++) {
                        auto &pg = cc.pages[pi];
                        if (pg.page_type != 0) continue;
                        int64_t nbytes = (int64_t)pg.num_values * stored;
                        if (nbytes &&
                            hipMemcpy((uint8_t *)rc.contig +
                                          row_at * stored,
                                      zdev_base + ppo[pi] + vpos[pi],
                                      nbytes,
                                      hipMemcpyDeviceToDevice) !=
                                hipSuccess) {
                            set_error("D2D staging failed");
                            return false;
                        }
                        row_at += pg.num_values;
                    }
                } else if (has_plain || (!has_dict && cc.num_values > 0)) {
                    // pack PLAIN value payloads and copy into contig
                    std::vector<uint8_t> pack(cc.num_values * stored);
                    int64_t off = 0;
                    for (size_t pi = 0; pi < cc.pages.size(); pi++) {
                        auto &pg = cc.pages[pi];
                        if (pg.page_type != 0) continue;
                        int64_t nbytes = (int64_t)pg.num_values * stored;
                        memcpy(pack.data() + off,
                               payload_base + ppo[pi] + vpos[pi], nbytes);
                        off += nbytes;
                    }
                    if (off != (int64_t)pack.size()) {
                        set_error("%s: page value counts disagree with chunk",
                                  fd.path.c_str());
                        return false;
                    }
                    if (hipMemcpy((uint8_t *)rc.contig + chunk_row0 * stored,
                                  pack.data(), off,
                                  hipMemcpyHostToDevice) != hipSuccess) {
                        set_error("H2D failed");
                        return false;
                    }
                } else if (has_dict) {
                    if (!dict_host) {
                        set_error("%s: dictionary page missing",
                                  fd.path.c_str());
                        return false;
                    }
                    rc.dict_encoded = true;
                    // upload the id-stream payload image
                    void *dev =
                        upload_chunk_image(plan, cc, ppo, payload_base, 0);
                    if (!dev) return false;
                    for (size_t pi = 0; pi < cc.pages.size(); pi++) {
                        auto &pg = cc.pages[pi];
                        if (pg.page_type != 0) continue;
                        if (!stage_page_ids(fd, cols[c],
                                            payload_base + ppo[pi],
                                            page_len(cc, pg), vpos[pi],
                                            pg.num_values,
                                            chunk_row0 + pg.first_row,
                                            (uint64_t)dev + ppo[pi], rc))
                            return false;
                    }
                    void *dict_dev = nullptr;
                    if (!upload_chunk_dict(plan, (int)c, dict_host,
                                           dict_count, stored, &dict_dev))
                        return false;
                    GatherTask gt;
                    gt.start = chunk_row0;
                    gt.n = cc.num_values;
                    gt.dict_dev = dict_dev;
                    rc.gathers.push_back(gt);
                }
            }
            rg_row += rg.num_rows;
        }
        if (rg_row != fd.row_count) {
            set_error("%s: rowCount %lld != file rows %lld", fd.path.c_str(),
                      (long long)fd.row_count, (long long)rg_row);
            return false;
        }
        row_base += rg_row;
    }
    run.length = row_base;
    for (size_t c = 0; c < run.cols.size(); c++) {
        RunCol &rc = run.cols[c];
        rc.n_rows = run.length;
        if (rc.dict_encoded) {
            rc.ids_dev = (int32_t *)plan->bufs.alloc(run.length * 4);
            rc.rle_dev = (RleChunk *)plan->bufs.alloc(rc.rle_host.size() *
                                                      sizeof(RleChunk));
            if (!rc.ids_dev || !rc.rle_dev) return false;
            if (hipMemcpy(rc.rle_dev, rc.rle_host.data(),
                          rc.rle_host.size() * sizeof(RleChunk),
                          hipMemcpyHostToDevice) != hipSuccess)
                return false;
        }
        if (rc.has_nulls) {
            // parquet PLAIN: dense values packed host-side (dense_host);
            // parquet dictionary / ORC: dense values are produced on-device
            // (k_dict_gather / k_rlev2) — size by the global dense count
            size_t dense_bytes =
                (size_t)rc.dense_before * plan->cols[c].stored_esize;
            rc.valid_dev = (uint8_t *)plan->bufs.alloc(run.length);
            rc.dense_dev = plan->bufs.alloc(dense_bytes);
            void *levels_dev = plan->bufs.alloc(rc.levels_host.size());
            if (!rc.valid_dev || !rc.dense_dev || !levels_dev)
                return false;
            // rows in non-null chunks of this column keep validity 1
            if (hipMemset(rc.valid_dev, 1, run.length) != hipSuccess)
                return false;
            size_t ho = 0;
            for (const auto &sg : rc.dense_segs) {
                if (sg.second > 0 &&
                    hipMemcpy((uint8_t *)rc.dense_dev +
                                  sg.first * plan->cols[c].stored_esize,
                              rc.dense_host.data() + ho, sg.second,
                              hipMemcpyHostToDevice) != hipSuccess)
                    return false;
                ho += sg.second;
            }
            if (hipMemcpy(levels_dev, rc.levels_host.data(),
                          rc.levels_host.size(),
                          hipMemcpyHostToDevice) != hipSuccess)
                return false;
            for (auto &dc : rc.def_host) {
                if (dc.kind == 1) dc.src += (uint64_t)levels_dev;
                dc.out_addr = (uint64_t)rc.contig;
                dc.valid_addr = (uint64_t)rc.valid_dev;
                dc.dense_addr = (uint64_t)rc.dense_dev;
                dc.esize = plan->cols[c].stored_esize;
            }
            // nullable DELTA pages decode into the dense buffer
            // (k_delta_emit runs before k_level_scatter)
            for (auto &ch : rc.delta_host)
                if (!ch.out_addr) ch.out_addr = (uint64_t)rc.dense_dev;
            for (auto &ds : rc.dstreams_host)
                if (!ds.out_addr) ds.out_addr = (uint64_t)rc.dense_dev;
            plan->encoded_bytes_total += rc.levels_host.size();
            rc.dense_host.clear();
            rc.dense_host.shrink_to_fit();
            rc.levels_host.clear();
            rc.levels_host.shrink_to_fit();
        }
        if (rc.scale_rows) {
            rc.scale_dev =
                (int32_t *)plan->bufs.alloc((size_t)rc.scale_rows * 4);
            if (!rc.scale_dev) return false;
        }
        if (rc.nanos_rows) {
            rc.nanos_dev =
                (uint64_t *)plan->bufs.alloc((size_t)rc.nanos_rows * 8);
            if (!rc.nanos_dev) return false;
        }
        for (auto &vc : rc.rlev2_host)
            vc.out_addr = vc.dense_target == 3   ? (uint64_t)rc.nanos_dev
                          : vc.dense_target == 2 ? (uint64_t)rc.scale_dev
                          : vc.dense_target      ? (uint64_t)rc.dense_dev
                                                 : (uint64_t)rc.contig;
        for (auto &bu : rc.bits_host)
            bu.out_addr =
                bu.dense_target ? (uint64_t)rc.dense_dev : (uint64_t)rc.contig;
        for (auto &tu : rc.ts_host) {
            tu.out_addr =
                tu.dense_target ? (uint64_t)rc.dense_dev : (uint64_t)rc.contig;
            tu.nanos_addr = (uint64_t)rc.nanos_dev;
        }
        for (auto &vu : rc.varint_host) {
            vu.out_addr =
                vu.dense_target ? (uint64_t)rc.dense_dev : (uint64_t)rc.contig;
            if (vu.scale_addr)
                vu.scale_addr =
                    (uint64_t)(rc.scale_dev + (vu.scale_addr - 1));
        }
    }
    return true;
}

// Like gpu_zstd_batch, but the decoded blob STAYS on device (allocated
// from the plan arena; *dev_out) and only `host_rngs` (chunks whose
// staging needs host peeks) copy back. Simple PLAIN chunks then stage
// with D2D copies — no PCIe round trip for their bytes.
static bool gpu_zstd_batch_dev(
    const uint8_t *src_base, int64_t src_total,
    const std::vector<ZstdBatchPage> &pages, pmh_plan_t *plan,
    uint8_t **dev_out, int64_t out_total,
    const std::vector<std::pair<int64_t, int64_t>> &host_rngs,
    uint8_t *host_out) {
    if (pages.empty()) return true;
    int n = (int)pages.size();
    uint8_t *d_src = nullptr, *d_scr = nullptr;
    ZstdJob *d_jobs = nullptr;
    int64_t *d_st = nullptr;
    uint8_t *d_dst = (uint8_t *)plan->bufs.alloc(out_total ? out_total : 1);
    if (!d_dst) return false;
    std::vector<ZstdJob> jobs(n);
    for (int i = 0; i < n; i++)
        jobs[i] = {(uint64_t)pages[i].src_off, (uint64_t)pages[i].dst_off,
                   (uint32_t)pages[i].src_len, (uint32_t)pages[i].dst_len};
    bool ok = false;
    std::vector<int64_t> st(n);
    do {
        if (hipMalloc(&d_src, src_total) != hipSuccess) break;
        if (hipMalloc(&d_scr, (size_t)n * PZ_SLOT) != hipSuccess) break;
        if (hipMalloc(&d_jobs, n * sizeof(ZstdJob)) != hipSuccess) break;
        if (hipMalloc(&d_st, n * 8) != hipSuccess) break;
        if (hipMemcpy(d_src, src_base, src_total, hipMemcpyHostToDevice) !=
            hipSuccess)
            break;
        if (hipMemcpy(d_jobs, jobs.data(), n * sizeof(ZstdJob),
                      hipMemcpyHostToDevice) != hipSuccess)
            break;
        if (pmh_launch_zstd_pages(d_src, d_jobs, n, d_dst, d_scr, d_st,
                                  nullptr) != hipSuccess)
            break;
        if (hipMemcpy(st.data(), d_st, n * 8, hipMemcpyDeviceToHost) !=
            hipSuccess)
            break;
        bool all = true;
        for (int i = 0; i < n; i++)
            if (st[i] != pages[i].dst_len) all = false;
        if (!all) break;
        ok = true;
        for (auto &r : host_rngs) {
            if (r.second > r.first &&
                hipMemcpy(host_out + r.first, d_dst + r.first,
                          r.second - r.first,
                          hipMemcpyDeviceToHost) != hipSuccess) {
                ok = false;
                break;
            }
        }
    } while (0);
    if (d_src) (void)hipFree(d_src);
    if (d_scr) (void)hipFree(d_scr);
    if (d_jobs) (void)hipFree(d_jobs);
    if (d_st) (void)hipFree(d_st);
    if (ok) *dev_out = d_dst;
    return ok;
}

// Hierarchical section setup: group real runs into batches (<= PMH_MAX_RUNS
// runs AND < 2^PMH_ROW_BITS input rows each, so every virtual run respects
// the winner row packing), allocate the virtual runs' columns, and swap the
// section's chain descriptors to point at them. The batch pass runs in
// pmh_read_next (it needs decoded columns).
static bool build_hier_section(pmh_plan_t *plan, Section &sec);

static bool build_hier_section(pmh_plan_t *plan, Section &sec) {
    const int n_real = (int)sec.runs.size();
    const int n_cols = (int)plan->cols.size();
    // keep the real-run descriptors for the batch pass, which also consumes
    // the tombstones
    sec.real_dev = sec.runs_dev;
    // batches: <= PMH_MAX_RUNS runs and < 2^PMH_ROW_BITS input rows each
    {
        int lo = 0;
        while (lo < n_real) {
            int hi = lo;
            int64_t rows = 0;
            while (hi < n_real && hi - lo < PMH_MAX_RUNS &&
                   rows + sec.runs[hi].length < ((int64_t)1 << PMH_ROW_BITS))
                rows += sec.runs[hi++].length;
            if (hi == lo) {
                set_error("run of %lld rows cannot batch under the 2^%d "
                          "winner row limit",
                          (long long)sec.runs[lo].length, PMH_ROW_BITS);
                return false;
            }
            sec.blo.push_back(lo);
            sec.bhi.push_back(hi);
            sec.brows.push_back(rows);
            sec.bntiles.push_back((rows + PMH_TILE_ROWS - 1) / PMH_TILE_ROWS);
            lo = hi;
        }
        if ((int)sec.blo.size() > PMH_MAX_RUNS) {
            set_error("section needs %zu virtual runs > %d (two-level "
                      "hierarchy is a later round)",
                      sec.blo.size(), PMH_MAX_RUNS);
            return false;
        }
    }
    const int nb = (int)sec.blo.size();
    // batch-pass dtype map: int8/int16 emit as int32 so the virtual runs
    // hold the STORED width the second merge/emit pass reads
    if (!plan->hier_columns.dtype) {
        std::vector<uint8_t> hd(n_cols);
        for (int c = 0; c < n_cols; c++) {
            uint8_t d = (uint8_t)plan->cols[c].dtype;
            hd[c] = (d == 1 || d == 2) ? 3 : d;
        }
        uint8_t *hd_dev = (uint8_t *)plan->bufs.alloc(n_cols);
        if (!hd_dev || hipMemcpy(hd_dev, hd.data(), n_cols,
                                 hipMemcpyHostToDevice) != hipSuccess) {
            set_error("H2D hier dtype map failed");
            return false;
        }
        plan->hier_columns.dtype = hd_dev;
    }
    // virtual runs: one per batch; columns at stored width
    std::vector<DevCol> vkeys(nb), vseqs(nb), vkinds(nb), vall(nb * n_cols);
    const int seq_idx = plan->columns.seq_col();
    const int kind_idx = plan->columns.kind_col();
    for (int b = 0; b < nb; b++) {
        std::vector<void *> outs(n_cols);
        std::vector<uint8_t *> valids(n_cols, nullptr);
        for (int c = 0; c < n_cols; c++) {
            int es = plan->cols[c].stored_esize;
            outs[c] = plan->bufs.alloc((size_t)sec.brows[b] * es);
            if (!outs[c]) return false;
            // nullability decided per plan at create end; allocate byte
            // validity for every value column that CAN be null in any run
            bool nullable = false;
            for (auto &run : sec.runs)
                if (run.cols[c].has_nulls) nullable = true;
            if (nullable) {
                valids[c] = (uint8_t *)plan->bufs.alloc(sec.brows[b]);
                if (!valids[c]) return false;
            }
            DevCol dc{(uint64_t)outs[c], (uint64_t)valids[c], es, 0};
            vall[b * n_cols + c] = dc;
            if (c == 0) vkeys[b] = dc;
            if (c == seq_idx) vseqs[b] = dc;
            if (c == kind_idx) vkinds[b] = dc;
        }
        void **op = (void **)plan->bufs.alloc(n_cols * sizeof(void *));
        uint8_t **vp =
            (uint8_t **)plan->bufs.alloc(n_cols * sizeof(void *));
        if (!op || !vp ||
            hipMemcpy(op, outs.data(), n_cols * sizeof(void *),
                      hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(vp, valids.data(), n_cols * sizeof(void *),
                      hipMemcpyHostToDevice) != hipSuccess) {
            set_error("H2D hier batch outputs failed");
            return false;
        }
        sec.bout.push_back(OutputSet{op, vp});
    }
    auto up = [&](const void *host, size_t n) -> void * {
        void *d = plan->bufs.alloc(n);
        if (d && host &&
            hipMemcpy(d, host, n, hipMemcpyHostToDevice) != hipSuccess)
            return nullptr;
        return d;
    };
    // the chain's runs: the nb virtual runs, their lengths written by the
    // batch pass
    RunSet &vr = sec.runs_dev;
    vr = RunSet{};
    vr.k = vr.n_slots = nb;
    vr.n_cols = n_cols;
    vr.keys = (DevCol *)up(vkeys.data(), nb * sizeof(DevCol));
    vr.seqs = (DevCol *)up(vseqs.data(), nb * sizeof(DevCol));
    vr.kinds = (DevCol *)up(vkinds.data(), nb * sizeof(DevCol));
    vr.cols = (DevCol *)up(vall.data(), vall.size() * sizeof(DevCol));
    vr.lens = (int64_t *)plan->bufs.alloc(nb * 8);
    if (!vr.keys || !vr.seqs || !vr.kinds || !vr.cols || !vr.lens) {
        set_error("hier descriptor allocation failed");
        return false;
    }
    return true;
}

static bool build_decode_tables(pmh_plan_t *plan, Section &sec);

static bool build_section_descriptors(pmh_plan_t *plan, Section &sec) {
    int k = (int)sec.runs.size();
    int n_cols = (int)plan->cols.size();
    // lookup changelog: every lookup level takes one more slot after the k
    // merge runs in the key/seq/kind/all-column/level tables, so a packed
    // (run, row) word can address a lookup-level record; the slots take no
    // part in partition or merge
    std::vector<Run> &lk_runs = plan->lookup_sec.runs;
    const int kt = k + (plan->lookup ? (int)lk_runs.size() : 0);
    std::vector<DevCol> keyv(kt), seqv(kt), kindv(kt), allv(kt * n_cols);
    std::vector<int64_t> lens(kt);
    const int seq_idx = plan->columns.seq_col();
    const int kind_idx = plan->columns.kind_col();
    if (plan->composite_key) sec.ckeys.assign(k, nullptr);
    for (int r = 0; r < kt; r++) {
        Run &run = r < k ? sec.runs[r] : lk_runs[r - k];
        lens[r] = run.length;
        if (r < k) sec.total_rows += run.length;
        for (int c = 0; c < n_cols; c++) {
            DevCol dc{(uint64_t)run.cols[c].contig,
                      (uint64_t)run.cols[c].valid_dev,
                      plan->cols[c].stored_esize, 0};
            allv[r * n_cols + c] = dc;
            if (c == 0) keyv[r] = dc;  // single-column key: the column itself
            if (c == seq_idx) seqv[r] = dc;
            if (c == kind_idx) kindv[r] = dc;
        }
        if (plan->composite_key) {
            // the partition/merge comparand is the packed composite key,
            // built per pass by k_composite
            int64_t n = run.length > 0 ? run.length : 1;
            sec.ckeys[r] = (int64_t *)plan->bufs.alloc(n * 8);
            if (!sec.ckeys[r]) return false;
            keyv[r] = DevCol{(uint64_t)sec.ckeys[r], 0, 8, 0};
        }
    }
    sec.n_tiles = (sec.total_rows + PMH_TILE_ROWS - 1) / PMH_TILE_ROWS;
    if (sec.n_tiles == 0) sec.n_tiles = 1;
    auto up = [&](const void *host, size_t n) -> void * {
        void *d = plan->bufs.alloc(n);
        if (d && host) (void)hipMemcpy(d, host, n, hipMemcpyHostToDevice);
        return d;
    };
    RunSet &rs = sec.runs_dev;
    TileSet &ts = sec.tiles;
    rs.k = k;
    rs.n_slots = kt;
    rs.n_cols = n_cols;
    rs.keys = (DevCol *)up(keyv.data(), kt * sizeof(DevCol));
    rs.seqs = (DevCol *)up(seqv.data(), kt * sizeof(DevCol));
    rs.kinds = (DevCol *)up(kindv.data(), kt * sizeof(DevCol));
    rs.cols = (DevCol *)up(allv.data(), allv.size() * sizeof(DevCol));
    rs.lens = (int64_t *)up(lens.data(), kt * sizeof(int64_t));
    ts.n_tiles = sec.n_tiles;
    ts.cuts = (int32_t *)plan->bufs.alloc((sec.n_tiles + 1) * k * 4);
    if (plan->fused) {
        // single-pass path: no winners round-trip, no scan arrays — just
        // the per-tile lookback words and the tile ticket
        ts.status = (uint64_t *)plan->bufs.alloc(sec.n_tiles * 8);
        ts.ticket = (uint64_t *)plan->bufs.alloc(8);
        if (!ts.status || !ts.ticket) return false;
        if (plan->fsplit) {
            ts.dense_winners =
                (uint32_t *)plan->bufs.alloc(sec.total_rows * 4);
            if (!ts.dense_winners) return false;
        }
    } else {
        ts.winners = (uint32_t *)plan->bufs.alloc(
            sec.n_tiles * (PMH_TILE_ROWS + PMH_MAX_RUNS) * 4);
        ts.counts = (int32_t *)plan->bufs.alloc(sec.n_tiles * 4);
        ts.offsets = (int64_t *)plan->bufs.alloc(sec.n_tiles * 8);
        if (!ts.winners || !ts.counts || !ts.offsets) return false;
    }
    if (plan->changelog) {
        std::vector<uint8_t> lv(kt);
        for (int r = 0; r < kt; r++)
            lv[r] = (uint8_t)(r < k ? sec.runs[r] : lk_runs[r - k]).level;
        rs.levels = (uint8_t *)up(lv.data(), kt);
        ChangelogSet &cl = sec.cl;
        int64_t slots2 = sec.n_tiles * 2 * (PMH_TILE_ROWS + PMH_MAX_RUNS);
        cl.entries = (uint64_t *)plan->bufs.alloc(slots2 * 8);
        cl.rows = (uint64_t *)plan->bufs.alloc(slots2 * 8);
        cl.counts = (int32_t *)plan->bufs.alloc(sec.n_tiles * 4);
        cl.offsets = (int64_t *)plan->bufs.alloc(sec.n_tiles * 8);
        cl.total = (int64_t *)plan->bufs.alloc(8);
        cl.max_level = plan->max_level;
        if (!rs.levels || !cl.entries || !cl.rows || !cl.counts ||
            !cl.offsets || !cl.total)
            return false;
    }
    if (plan->lookup) {
        // probe words: one per row of the section's level-0 runs
        ProbeSet &pr = sec.probe;
        pr.n_levels = kt - k;
        std::vector<int64_t> po(k, -1);
        int64_t words = 0;
        for (int r = 0; r < k; r++) {
            if (sec.runs[r].level != 0) continue;
            po[r] = words;
            words += sec.runs[r].length;
            pr.max_rows = std::max(pr.max_rows, sec.runs[r].length);
        }
        pr.off = (int64_t *)up(po.data(), k * sizeof(int64_t));
        pr.words = (uint32_t *)plan->bufs.alloc(words * 4);
        if (!pr.off || !pr.words) return false;
    }
    ts.total = (int64_t *)plan->bufs.alloc(8);
    ts.err = (uint32_t *)plan->bufs.alloc(4);
    if (ts.err) (void)hipMemset(ts.err, 0, 4);
    {
        std::vector<uint64_t> th(k, 0);
        for (int r = 0; r < k; r++) {
            th[r] = (uint64_t)sec.runs[r].tomb;
            sec.any_tomb |= sec.runs[r].tomb != nullptr;
        }
        if (sec.any_tomb) {
            rs.tombs = (uint64_t *)up(th.data(), k * 8);
            if (!rs.tombs) return false;
        }
    }
    if (plan->pu) {
        ts.group_start = (uint16_t *)plan->bufs.alloc(
            sec.n_tiles * (PMH_TILE_ROWS + 1) * 2);
        if (!ts.group_start) return false;
        bool any_valid = false;
        for (auto &run : sec.runs)
            for (auto &rc : run.cols)
                if (rc.valid_dev) any_valid = true;
        if (any_valid && n_cols <= 64) {
            sec.row_masks.assign(k, nullptr);
            for (int r = 0; r < k; r++) {
                int64_t n = sec.runs[r].length > 0 ? sec.runs[r].length : 1;
                sec.row_masks[r] = (uint64_t *)plan->bufs.alloc(n * 8);
                if (!sec.row_masks[r]) return false;
            }
            rs.masks =
                (uint64_t **)up(sec.row_masks.data(), k * sizeof(void *));
            if (!rs.masks) return false;
        }
    }
    if (!build_decode_tables(plan, sec)) return false;
    return rs.keys && rs.seqs && rs.kinds && rs.cols && rs.lens && ts.cuts &&
           ts.total && ts.err;
}

// Batched read-time decode work of a section's runs (one launch each
// across every run-column): also serves the plan's lookup levels, which
// decode once at plan creation.
static bool build_decode_tables(pmh_plan_t *plan, Section &sec) {
    auto up = [&](const void *host, size_t n) -> void * {
        void *d = plan->bufs.alloc(n);
        if (d && host) (void)hipMemcpy(d, host, n, hipMemcpyHostToDevice);
        return d;
    };
    std::vector<Rlev2Chunk> all_v;
    std::vector<VarintUnit> all_u;
    std::vector<BitsUnit> all_b;
    std::vector<TsUnit> all_t;
    std::vector<RleChunk> all_d;
    std::vector<DeltaChunk> all_dc;
    std::vector<DeltaStream> all_ds;
    for (auto &run : sec.runs)
        for (auto &rc : run.cols) {
            sec.any_dict |= rc.dict_encoded;
            sec.any_decode |= rc.dict_encoded || rc.has_nulls ||
                              !rc.rlev2_host.empty() ||
                              !rc.varint_host.empty() ||
                              !rc.bits_host.empty() ||
                              !rc.delta_host.empty() ||
                              !rc.gathers.empty();
            all_b.insert(all_b.end(), rc.bits_host.begin(),
                         rc.bits_host.end());
            all_t.insert(all_t.end(), rc.ts_host.begin(), rc.ts_host.end());
            all_v.insert(all_v.end(), rc.rlev2_host.begin(),
                         rc.rlev2_host.end());
            all_u.insert(all_u.end(), rc.varint_host.begin(),
                         rc.varint_host.end());
            all_d.insert(all_d.end(), rc.def_host.begin(), rc.def_host.end());
            const int64_t cbase = (int64_t)all_dc.size();
            all_dc.insert(all_dc.end(), rc.delta_host.begin(),
                          rc.delta_host.end());
            for (DeltaStream st : rc.dstreams_host) {
                st.chunk_lo += cbase;  // indices into the BATCHED arrays
                st.chunk_hi += cbase;
                all_ds.push_back(st);
            }
        }
    sec.n_rlev2 = (int64_t)all_v.size();
    sec.n_def = (int64_t)all_d.size();
    if (sec.n_rlev2) {
        sec.rlev2_all =
            (Rlev2Chunk *)up(all_v.data(), all_v.size() * sizeof(Rlev2Chunk));
        if (!sec.rlev2_all) return false;
    }
    sec.n_bits = (int64_t)all_b.size();
    if (sec.n_bits) {
        sec.bits_all =
            (BitsUnit *)up(all_b.data(), all_b.size() * sizeof(BitsUnit));
        if (!sec.bits_all) return false;
    }
    sec.n_ts = (int64_t)all_t.size();
    if (sec.n_ts) {
        // timestamp refusals land in the section's error word, like the
        // decimal ones below
        if (!sec.tiles.err) {
            sec.tiles.err = (uint32_t *)plan->bufs.alloc(4);
            if (!sec.tiles.err || hipMemset(sec.tiles.err, 0, 4) != hipSuccess)
                return false;
        }
        for (auto &tu : all_t) tu.err_addr = (uint64_t)sec.tiles.err;
        sec.ts_all = (TsUnit *)up(all_t.data(), all_t.size() * sizeof(TsUnit));
        if (!sec.ts_all) return false;
    }
    sec.n_varint = (int64_t)all_u.size();
    if (sec.n_varint) {
        // decimal range / scale violations land in the section's error word
        // (the lookup section owns none yet)
        if (!sec.tiles.err) {
            sec.tiles.err = (uint32_t *)plan->bufs.alloc(4);
            if (!sec.tiles.err || hipMemset(sec.tiles.err, 0, 4) != hipSuccess)
                return false;
        }
        for (auto &vu : all_u) vu.err_addr = (uint64_t)sec.tiles.err;
        sec.varint_all =
            (VarintUnit *)up(all_u.data(), all_u.size() * sizeof(VarintUnit));
        if (!sec.varint_all) return false;
    }
    if (sec.n_def) {
        sec.def_all =
            (RleChunk *)up(all_d.data(), all_d.size() * sizeof(RleChunk));
        if (!sec.def_all) return false;
    }
    sec.n_delta = (int64_t)all_dc.size();
    sec.n_dstreams = (int64_t)all_ds.size();
    if (sec.n_delta) {
        sec.delta_all = (DeltaChunk *)up(all_dc.data(),
                                         all_dc.size() * sizeof(DeltaChunk));
        sec.dstreams_all = (DeltaStream *)up(
            all_ds.data(), all_ds.size() * sizeof(DeltaStream));
        sec.delta_sums = (int64_t *)plan->bufs.alloc(sec.n_delta * 8);
        sec.delta_bases = (int64_t *)plan->bufs.alloc(sec.n_delta * 8);
        if (!sec.delta_all || !sec.dstreams_all || !sec.delta_sums ||
            !sec.delta_bases)
            return false;
    }
    return true;
}

// Read-time decode of a section's runs: batched RLEv2/byte-RLE +
// PRESENT/def-level scatter, plus parquet dictionary materialization per
// chunk. On failure *what names the failing stage.
static hipError_t launch_section_decode(pmh_plan_t *p, Section &sec,
                                        hipStream_t st, const char **what) {
    if (sec.any_decode) {
        if (sec.n_rlev2) {
            hipError_t e = pmh_launch_rlev2(sec.rlev2_all, sec.n_rlev2, st);
            if (e != hipSuccess) {
                *what = "rlev2";
                return e;
            }
        }
        if (sec.n_varint) {
            // after k_rlev2 on the same stream: units with per-value scales
            // read the scratch it fills
            hipError_t e =
                pmh_launch_orc_varint(sec.varint_all, sec.n_varint, st);
            if (e != hipSuccess) {
                *what = "orc_varint";
                return e;
            }
        }
        if (sec.n_ts) {
            // after k_rlev2 on the same stream: it decodes the seconds to
            // the column and the stored nanos to the scratch
            hipError_t e =
                pmh_launch_orc_timestamp(sec.ts_all, sec.n_ts, st);
            if (e != hipSuccess) {
                *what = "orc_timestamp";
                return e;
            }
        }
        if (sec.n_bits) {
            hipError_t e = pmh_launch_bits_expand(sec.bits_all, sec.n_bits, st);
            if (e != hipSuccess) {
                *what = "bits_expand";
                return e;
            }
        }
        if (sec.n_delta) {
            hipError_t e = pmh_launch_delta_sum(sec.delta_all, sec.n_delta,
                                                sec.delta_sums, st);
            if (e == hipSuccess)
                e = pmh_launch_delta_scan(sec.dstreams_all, sec.n_dstreams,
                                          sec.delta_sums, sec.delta_bases,
                                          st);
            if (e == hipSuccess)
                e = pmh_launch_delta_emit(sec.delta_all, sec.n_delta,
                                          sec.delta_bases, st);
            if (e != hipSuccess) {
                *what = "delta";
                return e;
            }
        }
        for (auto &run : sec.runs) {
            for (size_t c = 0; c < run.cols.size(); c++) {
                RunCol &rc = run.cols[c];
                int es = p->cols[c].stored_esize;
                if (!rc.dict_encoded && rc.gathers.empty()) continue;
                if (rc.dict_encoded) {
                    hipError_t e = pmh_launch_rle_decode(
                        rc.rle_dev, (int64_t)rc.rle_host.size(), rc.ids_dev,
                        st);
                    if (e != hipSuccess) {
                        *what = "rle_decode";
                        return e;
                    }
                }
                for (const GatherTask &gt : rc.gathers) {
                    if (!gt.n) continue;
                    uint8_t *dst = gt.to_dense
                                       ? (uint8_t *)rc.dense_dev
                                       : (uint8_t *)rc.contig;
                    // in_place: ORC dictionary-string LOCAL ids were
                    // RLEv2-decoded at the target already; remap to global
                    const int32_t *ids =
                        gt.in_place
                            ? (const int32_t *)(dst + gt.start * es)
                            : rc.ids_dev + gt.start;
                    hipError_t e = pmh_launch_dict_gather(
                        ids, gt.dict_dev, gt.n, dst + gt.start * es, es,
                        st);
                    if (e != hipSuccess) {
                        *what = "dict_gather";
                        return e;
                    }
                }
            }
        }
        if (sec.n_def) {
            hipError_t e =
                pmh_launch_level_scatter(sec.def_all, sec.n_def, st);
            if (e != hipSuccess) {
                *what = "level_scatter";
                return e;
            }
        }
    }
    return hipSuccess;
}

// ------------------------------------------------------------------ one read

// Profiling fields of the merge flag word. Read per read: tests and the
// profiling scripts vary them within a process.
static int profile_flags() {
    auto field = [](const char *name, int shift, int mask) {
        const char *e = getenv(name);
        return e ? (atoi(e) & mask) << shift : 0;
    };
    return field("PMH_ABLATE", PMH_FLAG_ABLATE_SHIFT, PMH_FLAG_ABLATE_MASK) |
           field("PMH_FABL", PMH_FLAG_FABL_SHIFT, PMH_FLAG_FABL_MASK) |
           field("PMH_FSTAGE", PMH_FLAG_FSTAGE_SHIFT, PMH_FLAG_FSTAGE_MASK);
}

// aggregate function names <-> PMH_AGG_* codes
static int agg_code_of(const std::string &s) {
    if (s == "last_non_null_value") return PMH_AGG_LAST_NON_NULL;
    if (s == "last_value") return PMH_AGG_LAST_VALUE;
    if (s == "first_value") return PMH_AGG_FIRST_VALUE;
    if (s == "first_non_null_value" || s == "first_not_null_value")
        return PMH_AGG_FIRST_NON_NULL;
    if (s == "sum") return PMH_AGG_SUM;
    if (s == "max") return PMH_AGG_MAX;
    if (s == "min") return PMH_AGG_MIN;
    if (s == "primary_key") return PMH_AGG_PRIMARY_KEY;
    return -1;
}

static const char *agg_name_of(int code) {
    switch (code & 0x7f) {
    case PMH_AGG_LAST_NON_NULL: return "last_non_null_value";
    case PMH_AGG_LAST_VALUE: return "last_value";
    case PMH_AGG_FIRST_VALUE: return "first_value";
    case PMH_AGG_FIRST_NON_NULL: return "first_non_null_value";
    case PMH_AGG_SUM: return "sum";
    case PMH_AGG_MAX: return "max";
    case PMH_AGG_MIN: return "min";
    default: return "primary_key";
    }
}

// What a set device error word refuses the read with; empty for a clean one.
static std::string error_word_message(const pmh_plan_t *p, uint32_t w) {
    if (w & PMH_ERR_RETRACT) {
        if (p->rrod)
            return "remove-record-on-delete accepts INSERT/DELETE "
                   "streams in v1; UPDATE_BEFORE records are not "
                   "supported yet";
        return std::string(p->agg ? "aggregation" : "partial-update") +
               " with retract records is not supported "
               "(the reference default also rejects them, "
               "PartialUpdateMergeFunction.java:170-186); configure "
               "'partial-update.remove-record-on-delete', or wait "
               "for the sequence-group/retract-aggregator rounds";
    }
    if (w & PMH_ERR_PU_AGG_RETRACT) {
        // FieldAggregator.retract throws; the candidates are the plan's
        // group fields whose function has no retract and no ignore-retract
        std::string cols;
        for (size_t c = 0; c < p->pu_col_agg.size(); c++) {
            const uint8_t a = p->pu_col_agg[c];
            if (a == PAC_NONE || (a & PMH_AGG_IGNORE_RETRACT)) continue;
            if (a != PMH_AGG_MAX && a != PMH_AGG_MIN &&
                a != PMH_AGG_FIRST_VALUE && a != PMH_AGG_FIRST_NON_NULL)
                continue;
            cols += std::string(cols.empty() ? "" : ", ") + "'" +
                    agg_name_of(a) + "' on column '" + p->cols[c].name + "'";
        }
        return "partial-update: a retract record (UPDATE_BEFORE / DELETE) "
               "with a non-empty sequence group reached an aggregate "
               "function that does not support retraction (" + cols +
               "); list the column in ignore_retract "
               "('fields.<field>.ignore-retract' = 'true') to let the "
               "function ignore retraction messages "
               "(FieldAggregator.retract)";
    }
    if (w & PMH_ERR_FIRST_ROW_RETRACT)
        return "first-row merge engine cannot accept DELETE/UPDATE_BEFORE "
               "records; configure 'ignore-delete' to skip them "
               "(FirstRowMergeFunction.java:49-59)";
    if (w & PMH_ERR_LOOKBACK)
        return "internal: fused merge lookback timed out waiting for a "
               "predecessor tile";
    if (w >> OTS_ERR_SHIFT) return orc_timestamp_error(w);
    if (orc_decimal_bits(w)) return orc_decimal_error(w);
    if (w & PMH_ERR_TOP_LEVEL_DUP)
        return "Top level key-value already exists (two runs at "
               "max_level hold the same key; "
               "FullChangelogMergeFunctionWrapper.java:76-78 checkState)";
    return "";
}

static bool hip_ok(const char *what, hipError_t e) {
    if (e == hipSuccess) return true;
    set_error("%s: %s", what, hipGetErrorString(e));
    return false;
}

// Timing events of one read, destroyed on every way out of it. The stage
// intervals are contiguous on the plan's stream:
//   START decode DECODED partition PARTITIONED [lookup PROBED] merge MERGED
//   scan SCANNED emit EMITTED
struct StageEvents {
    enum { START, DECODED, PARTITIONED, MERGED, SCANNED, EMITTED, N };
    hipEvent_t ev[N] = {};
    hipEvent_t probed = nullptr;  // lookup plans only
    StageEvents() {
        for (auto &e : ev) (void)hipEventCreate(&e);
    }
    ~StageEvents() {
        for (auto e : ev)
            if (e) (void)hipEventDestroy(e);
        if (probed) (void)hipEventDestroy(probed);
    }
    StageEvents(const StageEvents &) = delete;
    StageEvents &operator=(const StageEvents &) = delete;
    void record(int which, hipStream_t st) {
        (void)hipEventRecord(ev[which], st);
    }
    void record_probed(hipStream_t st) {
        (void)hipEventCreate(&probed);
        (void)hipEventRecord(probed, st);
    }
    // after the stream synchronized
    void add_to(pmh_stats &s) const {
        auto ms = [](hipEvent_t a, hipEvent_t b) {
            float v = 0;
            (void)hipEventElapsedTime(&v, a, b);
            return v;
        };
        s.decode_ms += ms(ev[START], ev[DECODED]);
        s.partition_ms += ms(ev[DECODED], ev[PARTITIONED]);
        if (probed) s.lookup_ms += ms(ev[PARTITIONED], probed);
        s.merge_ms += ms(probed ? probed : ev[PARTITIONED], ev[MERGED]);
        s.scan_ms += ms(ev[MERGED], ev[SCANNED]);
        s.emit_ms += ms(ev[SCANNED], ev[EMITTED]);
        s.total_device_ms += ms(ev[START], ev[EMITTED]);
    }
};

// What one pmh_read_next carries from step to step.
struct ReadPass {
    pmh_plan_t *p;
    Section &sec;
    hipStream_t st;
    int flags;      // plan flags + this read's profiling fields
    RunSet runs;    // what the chain merges
    TileSet tiles;  // ... in these tiles (a hierarchical batch pass leaves
    int64_t rows;   // fewer rows, so fewer tiles, than the section staged)
    StageEvents ev;
};

// Decode and the columns derived from it: batched RLEv2/byte-RLE +
// PRESENT/def-level scatter (one launch each across every run-column — the
// per-run-column launches serialized ~350 small kernels per step on C3),
// parquet dictionary materialization per chunk, composite keys, packed
// validity. The value filter runs after them, inside the partition interval.
static bool read_decode(ReadPass &rp) {
    pmh_plan_t *p = rp.p;
    Section &sec = rp.sec;
    const int k = (int)sec.runs.size();
    const int n_cols = rp.runs.n_cols;
    rp.ev.record(StageEvents::START, rp.st);
    const char *dwhat = "decode";
    // the call first: it names the launch that failed through dwhat
    const hipError_t de = launch_section_decode(p, sec, rp.st, &dwhat);
    if (!hip_ok(dwhat, de)) return false;
    if (p->composite_key) {
        // rebuilt per pass (decode-derived, like the validity masks)
        for (int r = 0; r < k; r++) {
            if (sec.runs[r].length <= 0) continue;
            if (!hip_ok("composite",
                        pmh_launch_composite(
                            rp.runs.cols + (size_t)r * n_cols,
                            p->columns.n_key_cols, p->key_shifts, p->key_bits,
                            sec.runs[r].length, sec.ckeys[r], rp.st)))
                return false;
        }
    }
    if (rp.runs.masks) {
        // rebuilt every pass: masks derive from the per-step level decode,
        // so caching them across steps would skip timed work
        for (int r = 0; r < k; r++) {
            if (sec.runs[r].length <= 0) continue;
            if (!hip_ok("pack_valid",
                        pmh_launch_pack_valid(
                            rp.runs.cols + (size_t)r * n_cols, n_cols,
                            sec.runs[r].length, sec.row_masks[r], rp.st)))
                return false;
        }
    }
    rp.ev.record(StageEvents::DECODED, rp.st);
    if (p->filters_dev && k == 1 && !sec.hier && sec.runs[0].tomb &&
        sec.runs[0].length > 0) {
        // value-filter pushdown: single-run sections only (overlapping
        // sections would lose newer records — MergeFileSplitRead.java:
        // 227-239); idempotent across repeats (OR into the tombstones)
        if (!hip_ok("filter",
                    pmh_launch_filter(rp.runs.cols, n_cols, p->filters_dev,
                                      (int)p->filters.size(),
                                      sec.runs[0].length, sec.runs[0].tomb,
                                      rp.st)))
            return false;
    }
    return true;
}

// Hierarchical batch pass: merge run batches into the virtual runs
// (winner-of-winners — the dedup/first-row fold is associative; deletes are
// KEPT here and drop only in the final chain). Leaves the chain the rows and
// tiles of what the batches kept.
static bool read_hier_batches(ReadPass &rp) {
    pmh_plan_t *p = rp.p;
    Section &sec = rp.sec;
    const int nb = (int)sec.blo.size();
    // no drop, no ignore
    const int bflags = rp.flags & PMH_FLAG_FIRST_ROW;
    for (int b = 0; b < nb; b++) {
        const RunSet batch =
            sec.real_dev.sub(sec.blo[b], sec.bhi[b] - sec.blo[b]);
        // the batch's row count is its virtual run's length
        const TileSet bt = sec.tiles.first(sec.bntiles[b], rp.runs.lens + b);
        if (!hip_ok("hier partition",
                    pmh_launch_partition(batch.keys, batch.lens, batch.k,
                                         PMH_TILE_ROWS, bt.n_tiles + 1,
                                         sec.brows[b], bt.cuts, rp.st)) ||
            !hip_ok("hier merge",
                    // never a changelog or lookup walk in the batch pass
                    pmh_launch_merge_tiles(batch, bt, bflags, ChangelogSet{},
                                           ProbeSet{}, rp.st)) ||
            !hip_ok("hier scan",
                    pmh_launch_scan_tiles(bt.counts, bt.n_tiles, bt.offsets,
                                          bt.total, rp.st)) ||
            !hip_ok("hier emit",
                    pmh_launch_emit(batch, p->hier_columns, bt, sec.bout[b],
                                    rp.st)))
            return false;
    }
    std::vector<int64_t> vl(nb);
    if (hipMemcpy(vl.data(), rp.runs.lens, nb * 8, hipMemcpyDeviceToHost) !=
        hipSuccess)
        return hip_ok("hier lens D2H", hipErrorUnknown);
    rp.rows = 0;
    for (int b = 0; b < nb; b++) rp.rows += vl[b];
    rp.tiles.n_tiles = (rp.rows + PMH_TILE_ROWS - 1) / PMH_TILE_ROWS;
    if (rp.tiles.n_tiles == 0) rp.tiles.n_tiles = 1;
    return true;
}

static bool read_partition(ReadPass &rp) {
    if (!hip_ok("partition",
                pmh_launch_partition(rp.runs.keys, rp.runs.lens, rp.runs.k,
                                     PMH_TILE_ROWS, rp.tiles.n_tiles + 1,
                                     rp.rows, rp.tiles.cuts, rp.st)))
        return false;
    rp.ev.record(StageEvents::PARTITIONED, rp.st);
    return true;
}

// Single-pass merge + emit: zero the lookback words + ticket, then one kernel
// does merge, offsets and emission (scan/emit launches and the winners
// round-trip disappear). Split mode (the default; PMH_FSPLIT=0 keeps in-kernel
// emission): that kernel emits key/seq/kind and a dense winner list, and
// k_emit_dense gathers the value columns after it. No scan: the scan interval
// is empty.
static bool read_fused(ReadPass &rp) {
    pmh_plan_t *p = rp.p;
    const TileSet &t = rp.tiles;
    if (!hip_ok("status memset",
                hipMemsetAsync(t.status, 0, t.n_tiles * 8, rp.st)) ||
        !hip_ok("ticket memset", hipMemsetAsync(t.ticket, 0, 8, rp.st)) ||
        !hip_ok("merge_emit",
                pmh_launch_merge_emit(rp.runs, p->columns, t, rp.flags,
                                      p->out.set, rp.st)))
        return false;
    rp.ev.record(StageEvents::MERGED, rp.st);
    rp.ev.record(StageEvents::SCANNED, rp.st);
    return !t.dense_winners ||
           hip_ok("emit_dense", pmh_launch_emit_dense(rp.runs, p->columns, t,
                                                      p->out.set, rp.st));
}

// The chain: lookup probe, tile merge, scan, the engine's emit.
static bool read_chain(ReadPass &rp) {
    pmh_plan_t *p = rp.p;
    Section &sec = rp.sec;
    const TileSet &t = rp.tiles;
    if (p->cl_fold &&
        ((rp.flags >> PMH_FLAG_ABLATE_SHIFT) & PMH_FLAG_ABLATE_MASK)) {
        // an ablated merge leaves the changelog counts unwritten
        set_error("PMH_ABLATE cannot be combined with a partial-update / "
                  "aggregation changelog plan");
        return false;
    }
    if (p->lookup) {
        // point lookup into the upper levels for every level-0 row, before
        // the merge walk consumes the probe words (timed as lookup_ms)
        if (!hip_ok("lookup_probe",
                    pmh_launch_lookup_probe(rp.runs, sec.probe, rp.st)))
            return false;
        rp.ev.record_probed(rp.st);
    }
    if (!hip_ok("merge_tiles",
                pmh_launch_merge_tiles(rp.runs, t, rp.flags, sec.cl,
                                       sec.probe, rp.st)))
        return false;
    rp.ev.record(StageEvents::MERGED, rp.st);
    if (!hip_ok("scan_tiles",
                pmh_launch_scan_tiles(t.counts, t.n_tiles, t.offsets, t.total,
                                      rp.st)))
        return false;
    rp.ev.record(StageEvents::SCANNED, rp.st);
    hipError_t e;
    if (p->agg)
        e = pmh_launch_emit_agg(rp.runs, p->columns, t, rp.flags, p->out.set,
                                rp.st);
    else if (p->pu && p->seqg)
        e = pmh_launch_emit_pu_sg(rp.runs, p->columns, p->seq_groups, t,
                                  rp.flags, p->out.set, rp.st);
    else if (p->pu)
        e = pmh_launch_emit_pu(rp.runs, p->columns, t, rp.flags, p->out.set,
                               rp.st);
    else
        // a lookup winner may name a lookup-level slot past the k merge
        // runs (runs.n_slots); a hierarchical chain reads its (contiguous)
        // virtual runs
        e = pmh_launch_emit(rp.runs, p->columns, t, p->out.set, rp.st);
    return hip_ok("emit", e);
}

// Changelog rows of the section, inside the emit interval: compact the merge
// pass's entries, scan the per-tile counts, gather into the changelog batch.
// The folding engines' chain reads the merged rows from the main output.
static bool read_changelog_tail(ReadPass &rp) {
    pmh_plan_t *p = rp.p;
    const ChangelogSet &cl = rp.sec.cl;
    const TileSet &t = rp.tiles;
    if (!p->changelog) return true;
    const bool fold = p->cl_fold;
    return hip_ok(fold ? "cl_finalize_out" : "cl_finalize",
                  fold ? pmh_launch_cl_finalize_out(rp.runs, p->columns, t, cl,
                                                    p->out.set, rp.st)
                       : pmh_launch_cl_finalize(rp.runs, p->columns, t, cl,
                                                rp.st)) &&
           hip_ok("cl_scan",
                  pmh_launch_scan_tiles(cl.counts, t.n_tiles, cl.offsets,
                                        cl.total, rp.st)) &&
           hip_ok(fold ? "cl_emit_out" : "cl_emit",
                  fold ? pmh_launch_cl_emit_out(rp.runs, p->columns, t, cl,
                                                p->out.set, p->out2.set,
                                                rp.st)
                       : pmh_launch_cl_emit(rp.runs, p->columns, t, cl,
                                            p->out2.set, rp.st));
}

// The pmh_col descriptors of `rows` rows of one output stream, after their
// D2H copies under output = "host".
static bool assemble_batch(pmh_plan_t *p, OutBatch &ob, int64_t rows,
                           const char *d2h_error,
                           const char *d2h_valid_error) {
    const int n_cols = (int)p->cols.size();
    ob.cols.resize(n_cols);
    if (p->host_output) {
        ob.host.resize(n_cols);
        ob.valid_host.resize(n_cols);
        for (int c = 0; c < n_cols; c++) {
            const size_t bytes = (size_t)rows * p->cols[c].out_esize;
            ob.host[c].resize(bytes);
            if (rows > 0 && hipMemcpy(ob.host[c].data(), ob.dev[c], bytes,
                                      hipMemcpyDeviceToHost) != hipSuccess) {
                set_error("%s", d2h_error);
                return false;
            }
            if (!ob.valid[c]) continue;
            ob.valid_host[c].resize(rows);
            if (rows > 0 &&
                hipMemcpy(ob.valid_host[c].data(), ob.valid[c], rows,
                          hipMemcpyDeviceToHost) != hipSuccess) {
                set_error("%s", d2h_valid_error);
                return false;
            }
        }
    }
    for (int c = 0; c < n_cols; c++) {
        pmh_col &pc = ob.cols[c];
        pc.name = p->col_names[c].c_str();
        pc.dtype = p->cols[c].is_bool ? PMH_DT_BOOL : p->cols[c].dtype;
        pc.logical = p->cols[c].logical;
        pc.data = p->host_output ? (const void *)ob.host[c].data()
                                 : (const void *)ob.dev[c];
        pc.valid = nullptr;
        if (ob.valid[c])
            pc.valid = p->host_output
                           ? (const uint8_t *)ob.valid_host[c].data()
                           : (const uint8_t *)ob.valid[c];
        pc.dict_data = nullptr;
        pc.dict_offsets = nullptr;
        pc.dict_len = 0;
        pc.precision = p->cols[c].precision;
        pc.scale = p->cols[c].scale;
        if (p->cols[c].dtype == PMH_DT_STRING && p->sdicts[c]) {
            StrDict *sd = p->sdicts[c].get();
            pc.dict_data = sd->bytes.data();
            pc.dict_offsets = sd->offsets.data();
            pc.dict_len = (int32_t)sd->offsets.size() - 1;
        }
    }
    return true;
}

// Wait for the pass, refuse on a set error word, account the stage times and
// hand out the batches. Returns the main batch's rows, -1 on error.
static int64_t read_collect(ReadPass &rp, pmh_batch *out) {
    pmh_plan_t *p = rp.p;
    Section &sec = rp.sec;
    int64_t total = 0;
    int64_t cl_total = 0;
    uint32_t err_word = 0;
    if (!hip_ok("total D2H",
                hipMemcpyAsync(&total, rp.tiles.total, 8,
                               hipMemcpyDeviceToHost, rp.st)) ||
        (p->changelog && sec.cl.total &&
         !hip_ok("cl total D2H",
                 hipMemcpyAsync(&cl_total, sec.cl.total, 8,
                                hipMemcpyDeviceToHost, rp.st))) ||
        !hip_ok("err D2H", hipMemcpyAsync(&err_word, rp.tiles.err, 4,
                                          hipMemcpyDeviceToHost, rp.st)) ||
        !hip_ok("stream sync", hipStreamSynchronize(rp.st)))
        return -1;
    const std::string refusal = error_word_message(p, err_word);
    if (!refusal.empty()) {
        set_error("%s", refusal.c_str());
        return -1;
    }
    rp.ev.add_to(p->stats);
    p->stats.rows_in += sec.total_rows;
    p->stats.rows_out += total;

    if (!assemble_batch(p, p->out, total, "D2H output failed",
                        "D2H validity failed"))
        return -1;
    if (p->changelog) {
        p->cl_rows_last = cl_total;
        if (!assemble_batch(p, p->out2, cl_total, "D2H changelog failed",
                            "D2H changelog validity failed"))
            return -1;
    }
    if (out) {
        out->n_rows = total;
        out->n_cols = (int32_t)p->cols.size();
        out->device = p->host_output ? -1 : p->session->device;
        out->cols = p->out.cols.data();
    }
    return total;
}

}  // namespace pmh

// ==================================================================== C ABI

using namespace pmh;

extern "C" {

const char *pmh_last_error(void) { return last_error().c_str(); }

pmh_session_t *pmh_open_session(int device) {
    auto *s = new pmh_session_t();
    s->device = device;
    if (device >= 0) {
        if (hipSetDevice(device) != hipSuccess) {
            set_error("hipSetDevice(%d) failed", device);
            delete s;
            return nullptr;
        }
    }
    return s;
}

void pmh_close_session(pmh_session_t *s) { delete s; }

// The per-column aggregator table of both folding engines, from the plan's
// "aggregations": {"col": "sum", ...} and "ignore_retract": ["col", ...]
// ("first_not_null_value" is the legacy alias,
// FieldFirstNonNullValueAggLegacyFactory.java:29). ca arrives filled with
// each column's default and leaves with one PMH_AGG_* code per column
// (| PMH_AGG_IGNORE_RETRACT).
//
// Aggregation engine (pu = false): unnamed value columns keep the
// last_non_null_value they arrive with (AggregateMergeFunction.java:197-203).
//
// Partial-update (pu = true; getAggFuncName, PartialUpdateMergeFunction
// .java:698-728): ca arrives PAC_NONE everywhere. "default_aggregation"
// (fields.default-aggregate-function) fills every value column that is
// neither a sequence field nor named; an entry that names a sequence field
// gives it no aggregator; every function but last_non_null_value needs the
// column to be a group_fields member of a sequence group (col_group /
// is_seq_field: the plan's sequence-group tables, empty without groups).
static bool parse_agg_table(pmh_plan_t *plan, const Json &j, bool pu,
                            const std::vector<uint8_t> &col_group,
                            const std::vector<uint8_t> &is_seq_field,
                            std::vector<uint8_t> &ca) {
    const int n_cols = (int)plan->cols.size();
    const int first_val = plan->columns.first_val();
    // one function on one column: the type rules, and under partial-update
    // the sequence-group rule
    auto check = [&](int idx, const std::string &fn, int code) -> bool {
        if (code < 0) {
            set_error("aggregate function '%s' not on the GPU path "
                      "(v1: sum, max, min, last_value, first_value, "
                      "last_non_null_value, first_non_null_value)",
                      fn.c_str());
            return false;
        }
        if (pu && code == PMH_AGG_PRIMARY_KEY) {
            set_error("aggregate function 'primary_key' on column '%s': "
                      "partial-update keys are key columns, not value "
                      "columns, and take no aggregate function",
                      plan->cols[idx].name.c_str());
            return false;
        }
        if (plan->cols[idx].dtype == PMH_DT_STRING &&
            (code == PMH_AGG_SUM || code == PMH_AGG_MAX ||
             code == PMH_AGG_MIN)) {
            set_error("aggregate '%s' on a string column is not on "
                      "the GPU path (ids are not ordered by value)",
                      fn.c_str());
            return false;
        }
        if ((plan->cols[idx].is_bool || plan->cols[idx].logical) &&
            code == PMH_AGG_SUM) {
            set_error("aggregate 'sum' on %s column '%s' is not "
                      "supported (boolean / date / time / timestamp "
                      "columns take last_value, first_value, "
                      "last_non_null_value, first_non_null_value, "
                      "max, min)",
                      plan->cols[idx].is_bool
                          ? "boolean"
                          : logical_name(plan->cols[idx].logical),
                      plan->cols[idx].name.c_str());
            return false;
        }
        if (!pu && plan->rrod && (code == PMH_AGG_FIRST_VALUE ||
                                  code == PMH_AGG_FIRST_NON_NULL)) {
            set_error("aggregate function '%s' is not supported "
                      "with remove-record-on-delete in v1 (its "
                      "initialized-state does not reset on DELETE "
                      "in the reference; later round)",
                      fn.c_str());
            return false;
        }
        if (pu && code != PMH_AGG_LAST_NON_NULL &&
            (col_group.empty() || col_group[idx] == 0xff)) {
            set_error("Must use sequence group for aggregation functions "
                      "but not found for field %s.",
                      plan->cols[idx].name.c_str());
            return false;
        }
        return true;
    };
    auto seq_field = [&](int c) {
        return !is_seq_field.empty() && is_seq_field[c];
    };
    std::vector<uint8_t> named(n_cols, 0);
    for (const auto &kv : j["aggregations"].obj) {
        int idx = -1;
        for (int c = first_val; c < n_cols; c++)
            if (plan->cols[c].name == kv.first) idx = c;
        if (idx < 0) {
            set_error("aggregations: '%s' is not a value column",
                      kv.first.c_str());
            return false;
        }
        named[idx] = 1;
        // no aggregate function for sequence fields (getAggFuncName)
        if (pu && seq_field(idx)) continue;
        const std::string fn = kv.second.as_str();
        const int code = agg_code_of(fn);
        if (!check(idx, fn, code)) return false;
        ca[idx] = (uint8_t)code;
    }
    if (pu) {
        const std::string dfl = j["default_aggregation"].as_str("");
        if (!dfl.empty()) {
            const int code = agg_code_of(dfl);
            for (int c = first_val; c < n_cols; c++) {
                if (named[c] || seq_field(c)) continue;
                if (!check(c, dfl, code)) return false;
                ca[c] = (uint8_t)code;
            }
        }
    }
    // fields.<f>.ignore-retract = true (FieldIgnoreRetractAgg):
    // retract records leave that field's accumulator untouched
    for (const auto &irj : j["ignore_retract"].arr) {
        int idx = -1;
        for (int c = first_val; c < n_cols; c++)
            if (plan->cols[c].name == irj.as_str()) idx = c;
        if (idx < 0) {
            set_error("ignore_retract: '%s' is not a value column",
                      irj.as_str().c_str());
            return false;
        }
        if (pu && ca[idx] == PAC_NONE) {
            // stricter than the reference, which drops the option silently
            set_error("ignore_retract: column '%s' has no aggregate "
                      "function under partial-update (name one in "
                      "aggregations or default_aggregation)",
                      irj.as_str().c_str());
            return false;
        }
        ca[idx] |= PMH_AGG_IGNORE_RETRACT;
    }
    return true;
}

pmh_plan_t *pmh_plan_create(pmh_session_t *s, const char *plan_json) {
    if (!s) {
        set_error("null session");
        return nullptr;
    }
    if (s->device < 0) {
        set_error("pmh_plan_create requires a GPU session (device >= 0)");
        return nullptr;
    }
    (void)hipSetDevice(s->device);
    std::unique_ptr<pmh_plan_t> plan(new pmh_plan_t());
    plan->session = s;
    try {
        Json j = JsonParser(plan_json).parse();
        // columns: key cols, then seq, kind, then value cols
        auto add_col = [&](const Json &cj) -> bool {
            ColSpec cs;
            cs.name = cj["name"].as_str();
            const std::string ts = cj["type"].as_str();
            int dp = 0, ds = 0;
            if (parse_decimal(ts, &dp, &ds)) {
                if (dp <= 0 || dp > 18 || ds < 0 || ds > dp) {
                    set_error("decimal(%d,%d): v1 supports precision 1..18 "
                              "(INT32/INT64 physical per the reference; "
                              "FLBA decimals are a later round)", dp, ds);
                    return false;
                }
                cs.dtype = dp <= 9 ? PMH_DT_INT32 : PMH_DT_INT64;
                cs.precision = dp;
                cs.scale = ds;
            } else {
                const int bt = parse_bool_or_temporal(ts, cs);
                if (bt < 0) return false;
                if (bt == 0) cs.dtype = dtype_from_str(ts);
            }
            if (cs.dtype < 0 || cs.name.empty()) {
                set_error("bad column spec");
                return false;
            }
            cs.out_esize = pmh_out_width(cs.dtype);
            cs.stored_esize = pmh_stored_width(cs.dtype);
            plan->cols.push_back(cs);
            return true;
        };
        const Json &kc = j["key_cols"];
        if (kc.arr.empty() || kc.arr.size() > 8) {
            set_error("v1 supports 1..8 integer key columns (got %zu)",
                      kc.arr.size());
            return nullptr;
        }
        int key_total_bits = 0;
        {
            int shift = 64;
            for (size_t i = 0; i < kc.arr.size(); i++) {
                {
                    ColSpec probe;
                    const std::string kts = kc.arr[i]["type"].as_str();
                    const int bt = parse_bool_or_temporal(kts, probe);
                    if (bt < 0) return nullptr;
                    if (bt > 0) {
                        set_error("key column '%s': a %s key column is a "
                                  "later round (boolean / date / time / "
                                  "timestamp are value-column and "
                                  "sequence-field types in v1)",
                                  kc.arr[i]["name"].as_str().c_str(),
                                  kts.c_str());
                        return nullptr;
                    }
                }
                int dt = dtype_from_str(kc.arr[i]["type"].as_str());
                if (dt < PMH_DT_INT8 || dt > PMH_DT_INT64) {
                    set_error("key column %zu: integer types only "
                              "(TINYINT..BIGINT) in v1",
                              i);
                    return nullptr;
                }
                int bits = 8 << (dt - PMH_DT_INT8);
                key_total_bits += bits;
                shift -= bits;
                if (key_total_bits > 64) {
                    set_error("composite key widths sum to %d bits > 64 "
                              "(the order-preserving packed comparand is one "
                              "int64; wider keys are a later round)",
                              key_total_bits);
                    return nullptr;
                }
                plan->key_shifts |= (uint64_t)(uint8_t)shift << (8 * i);
                plan->key_bits |= (uint64_t)(uint8_t)bits << (8 * i);
            }
        }
        plan->columns.n_key_cols = (int)kc.arr.size();
        plan->composite_key = plan->columns.n_key_cols > 1;
        for (const auto &c : kc.arr)
            if (!add_col(c)) return nullptr;
        {  // _SEQUENCE_NUMBER, _VALUE_KIND (SpecialFields.java:79-83)
            ColSpec seq{"_SEQUENCE_NUMBER", PMH_DT_INT64, 8, 8};
            ColSpec kind{"_VALUE_KIND", PMH_DT_INT8, 1, 4};
            plan->cols.push_back(seq);
            plan->cols.push_back(kind);
        }
        for (const auto &c : j["value_cols"].arr)
            if (!add_col(c)) return nullptr;
        plan->columns.n_cols = (int)plan->cols.size();
        plan->sdicts.resize(plan->cols.size());  // before staging touches it
        std::string engine = j["merge_engine"].as_str("deduplicate");
        if (engine == "partial-update") {
            plan->pu = true;  // INSERT-only unless remove-record-on-delete
                              // or sequence groups
                              // (PartialUpdateMergeFunction rejects retracts
                              // by default, :170-186)
            plan->rrod = j["remove_record_on_delete"].as_bool(false);
            const Json &sgs = j["sequence_groups"];
            // host copies for the aggregator table below
            std::vector<uint8_t> sg_col_group, sg_is_seq_field;
            if (!sgs.arr.empty()) {
                plan->seqg = true;
                if (sgs.arr.size() > 16) {
                    set_error("at most 16 sequence groups in v1");
                    return nullptr;
                }
                const int first_val = plan->columns.first_val();
                const int n_cols = (int)plan->cols.size();
                std::vector<uint8_t> cg(n_cols, 0xff);
                std::vector<int16_t> sf(sgs.arr.size() * 4, -1);
                std::vector<uint8_t> ns(sgs.arr.size(), 0);
                auto col_idx = [&](const std::string &nm) -> int {
                    for (int c = first_val; c < n_cols; c++)
                        if (plan->cols[c].name == nm) return c;
                    return -1;
                };
                for (size_t g = 0; g < sgs.arr.size(); g++) {
                    const Json &sg = sgs.arr[g];
                    const auto &sfj = sg["sequence_fields"].arr;
                    if (sfj.empty() || sfj.size() > 4) {
                        set_error("sequence group %zu: 1..4 sequence "
                                  "fields in v1", g);
                        return nullptr;
                    }
                    for (size_t i2 = 0; i2 < sfj.size(); i2++) {
                        int c = col_idx(sfj[i2].as_str());
                        if (c < 0 || plan->cols[c].dtype > PMH_DT_INT64) {
                            set_error("sequence field '%s': integer value "
                                      "columns only in v1",
                                      sfj[i2].as_str().c_str());
                            return nullptr;
                        }
                        if (cg[c] != 0xff) {
                            set_error("column '%s' is in two sequence "
                                      "groups", sfj[i2].as_str().c_str());
                            return nullptr;
                        }
                        cg[c] = (uint8_t)g;
                        sf[g * 4 + i2] = (int16_t)c;
                    }
                    ns[g] = (uint8_t)sfj.size();
                    for (const auto &mf : sg["group_fields"].arr) {
                        int c = col_idx(mf.as_str());
                        if (c < 0) {
                            set_error("sequence-group member '%s' is not a "
                                      "value column", mf.as_str().c_str());
                            return nullptr;
                        }
                        if (cg[c] != 0xff) {
                            set_error("column '%s' is in two sequence "
                                      "groups", mf.as_str().c_str());
                            return nullptr;
                        }
                        cg[c] = (uint8_t)g;
                    }
                }
                uint8_t *cg_dev = (uint8_t *)plan->bufs.alloc(n_cols);
                int16_t *sf_dev = (int16_t *)plan->bufs.alloc(sf.size() * 2);
                uint8_t *ns_dev = (uint8_t *)plan->bufs.alloc(ns.size());
                if (!cg_dev || !sf_dev || !ns_dev ||
                    hipMemcpy(cg_dev, cg.data(), n_cols,
                              hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(sf_dev, sf.data(), sf.size() * 2,
                              hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(ns_dev, ns.data(), ns.size(),
                              hipMemcpyHostToDevice) != hipSuccess) {
                    set_error("H2D of sequence-group tables failed");
                    return nullptr;
                }
                plan->seq_groups =
                    SeqGroupSet{cg_dev, sf_dev, ns_dev, (int)sgs.arr.size()};
                sg_col_group = cg;
                sg_is_seq_field.assign(n_cols, 0);
                for (int16_t c : sf)
                    if (c >= 0) sg_is_seq_field[c] = 1;
            }
            {
                // fields.<f>.aggregate-function inside sequence groups: a
                // group field with an aggregator sends the plan's emit to
                // k_emit_pu_sga. last_non_null_value on a field in no group
                // equals the overlay and needs nothing.
                const int n_cols = (int)plan->cols.size();
                std::vector<uint8_t> ca(n_cols, PAC_NONE);
                if (!parse_agg_table(plan.get(), j, true, sg_col_group,
                                     sg_is_seq_field, ca))
                    return nullptr;
                bool any = false;
                for (int c = 0; c < n_cols; c++)
                    any |= ca[c] != PAC_NONE && !sg_col_group.empty() &&
                           sg_col_group[c] != 0xff;
                if (any) {
                    // per-group column lists: a group's fields that are no
                    // sequence fields, next to col_group
                    const int ng = plan->seq_groups.n_groups;
                    std::vector<int16_t> gc;
                    std::vector<uint16_t> go(ng + 1, 0);
                    for (int g = 0; g < ng; g++) {
                        for (int c = 0; c < n_cols; c++)
                            if (sg_col_group[c] == g && !sg_is_seq_field[c])
                                gc.push_back((int16_t)c);
                        go[g + 1] = (uint16_t)gc.size();
                    }
                    int16_t *gc_dev = (int16_t *)plan->bufs.alloc(
                        std::max<size_t>(gc.size(), 1) * 2);
                    uint16_t *go_dev =
                        (uint16_t *)plan->bufs.alloc(go.size() * 2);
                    uint8_t *ca_dev = (uint8_t *)plan->bufs.alloc(n_cols);
                    if (!gc_dev || !go_dev || !ca_dev ||
                        hipMemcpy(gc_dev, gc.data(), gc.size() * 2,
                                  hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(go_dev, go.data(), go.size() * 2,
                                  hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(ca_dev, ca.data(), n_cols,
                                  hipMemcpyHostToDevice) != hipSuccess) {
                        set_error("H2D of partial-update aggregator tables "
                                  "failed");
                        return nullptr;
                    }
                    plan->seq_groups.grp_cols = gc_dev;
                    plan->seq_groups.grp_off = go_dev;
                    plan->seq_groups.col_agg = ca_dev;
                    plan->pu_col_agg = ca;
                }
            }
        } else if (engine == "first-row") {
            plan->first_row = true;  // FirstRowMergeFunction.java:32-77
        } else if (engine == "aggregation") {
            // AggregateMergeFunction.java:50-125 — per-field aggregators
            // over the same grouped stream as partial-update
            plan->pu = true;
            plan->agg = true;
            plan->rrod = j["remove_record_on_delete"].as_bool(false);
        } else if (engine != "deduplicate") {
            set_error("merge engine '%s' not on the GPU path (deduplicate | "
                      "partial-update | aggregation | first-row)",
                      engine.c_str());
            return nullptr;
        }
        // sort-engine (CoreOptions.java:733-736, default LOSER_TREE):
        // both engines share one output contract (SortMergeReader.java:41-57
        // — identical merged stream), so either value maps to the same GPU
        // merge; accepted for drop-in config compatibility.
        {
            std::string se = j["sort_engine"].as_str("loser-tree");
            if (se != "loser-tree" && se != "min-heap") {
                set_error("unknown sort-engine '%s'", se.c_str());
                return nullptr;
            }
        }
        {
            const Json &uf = j["sequence_fields"];
            if (!uf.arr.empty()) {
                if (plan->pu) {
                    set_error("sequence.field with partial-update/"
                              "aggregation engines is a later round (v1: "
                              "deduplicate / first-row)");
                    return nullptr;
                }
                if (uf.arr.size() > 4) {
                    set_error("at most 4 sequence fields in v1");
                    return nullptr;
                }
                const int first_val = plan->columns.first_val();
                const int n_cols = (int)plan->cols.size();
                std::vector<int16_t> uc;
                for (const auto &fj : uf.arr) {
                    int idx = -1;
                    for (int c = first_val; c < n_cols; c++)
                        if (plan->cols[c].name == fj.as_str()) idx = c;
                    if (idx < 0 ||
                        plan->cols[idx].dtype > PMH_DT_INT64) {
                        set_error("sequence field '%s': integer value "
                                  "columns only in v1",
                                  fj.as_str().c_str());
                        return nullptr;
                    }
                    uc.push_back((int16_t)idx);
                }
                // sequence.field (user-defined sequence comparator): the
                // listed value columns compare before the sequence number
                int16_t *uc_dev = (int16_t *)plan->bufs.alloc(uc.size() * 2);
                if (!uc_dev ||
                    hipMemcpy(uc_dev, uc.data(), uc.size() * 2,
                              hipMemcpyHostToDevice) != hipSuccess) {
                    set_error("H2D of sequence fields failed");
                    return nullptr;
                }
                plan->columns.useq = uc_dev;
                plan->columns.n_useq = (int)uc.size();
            }
        }
        plan->drop_delete = j["drop_delete"].as_bool(true);
        plan->ignore_delete = j["ignore_delete"].as_bool(false);
        {
            std::string cp = j["changelog_producer"].as_str("none");
            if (cp == "full-compaction") {
                plan->changelog = true;
                plan->cl_row_dedup =
                    j["changelog_row_deduplicate"].as_bool(false);
                plan->max_level = (int)j["max_level"].as_i64(-1);
                if (plan->max_level < 0) {
                    set_error("changelog_producer=full-compaction needs "
                              "max_level (the table's num-levels - 1; "
                              "FullChangelogMergeFunctionWrapper maxLevel)");
                    return nullptr;
                }
                // partial-update / aggregation: the folded changelog chain
                // (k_cl_finalize_out / k_cl_emit_out read the merged row
                // from the main output)
                plan->cl_fold = plan->pu;
                if (plan->cl_fold && plan->ignore_delete) {
                    set_error("changelog_producer=full-compaction with the "
                              "%s engine cannot be combined with "
                              "ignore_delete",
                              plan->agg ? "aggregation" : "partial-update");
                    return nullptr;
                }
            } else if (cp == "lookup") {
                // LookupChangelogMergeFunctionWrapper: changelog at every
                // level-0 compaction; the upper levels come as lookup_files
                plan->changelog = true;
                plan->lookup = true;
                plan->cl_row_dedup =
                    j["changelog_row_deduplicate"].as_bool(false);
                if (engine != "deduplicate") {
                    set_error("changelog_producer=lookup is supported for "
                              "the deduplicate engine in v1 (first-row uses "
                              "FirstRowMergeFunctionWrapper; partial-update/"
                              "aggregation changelog is a later round)");
                    return nullptr;
                }
                if (plan->ignore_delete) {
                    set_error("changelog_producer=lookup cannot be combined "
                              "with ignore_delete in v1");
                    return nullptr;
                }
                if (plan->composite_key) {
                    set_error("changelog_producer=lookup needs a single "
                              "integer key column in v1 (composite keys are "
                              "a later round)");
                    return nullptr;
                }
            } else if (cp != "none") {
                set_error("changelog_producer '%s' not supported (none | "
                          "full-compaction | lookup)", cp.c_str());
                return nullptr;
            }
        }
        {
            // Same-box A/B (DESIGN.md §7 experiment log): the classic
            // partition->merge->scan->emit chain with the two-level
            // partition is the fastest winner-engine configuration
            // (C2 6.4ms vs 7.1ms split-fused; 16x20M 31.6 vs 36.4ms), so
            // the chain is the product default. The fused single-pass path
            // stays as the path for user-defined sequence fields (its
            // comparator lives there) and behind PMH_FUSED=1 for A/B.
            const char *pf = getenv("PMH_FUSED");
            bool want_fused = pf ? pf[0] != '0' : (plan->columns.n_useq > 0);
            plan->fused = !plan->pu && want_fused;
            if (plan->changelog && plan->fused) {
                if (plan->columns.n_useq > 0 || (pf && pf[0] != '0')) {
                    set_error("changelog_producer=%s runs on "
                              "the classic merge chain (no sequence.field / "
                              "PMH_FUSED=1 combination in v1)",
                              plan->lookup ? "lookup" : "full-compaction");
                    return nullptr;
                }
                plan->fused = false;
            }
            if (plan->columns.n_useq > 0 && !plan->pu && !plan->fused) {
                set_error("sequence.field needs the fused merge path "
                          "(unset PMH_FUSED=0)");
                return nullptr;
            }
            // within the fused path, split value emission (merge_emit +
            // emit_dense) is the faster variant; PMH_FSPLIT=0 keeps
            // in-kernel emission for A/B
            const char *fs = getenv("PMH_FSPLIT");
            plan->fsplit = plan->fused && !(fs && fs[0] == '0');
        }
        if (plan->rrod && plan->ignore_delete) {
            set_error("remove-record-on-delete cannot be used with "
                      "ignore-delete (PartialUpdateMergeFunction.java:"
                      "491-495)");
            return nullptr;
        }
        plan->host_output = j["output"].as_str("device") == "host";
        {
            // "filters": [{"field": "...", "op": "eq|ne|lt|le|gt|ge|
            // is_null|is_not_null", "literal": x}] — a conjunction; the
            // reference pushes VALUE filters only into single-run
            // sections (overlapping runs would lose newer records,
            // MergeFileSplitRead.java:227-239). Key filters prune by file
            // stats before planning (caller side, as DataSplit already
            // carries the pruned file list).
            const Json &fj = j["filters"];
            for (const auto &f : fj.arr) {
                std::string field = f["field"].as_str("");
                std::string op = f["op"].as_str("");
                int idx = -1;
                for (size_t c = 0; c < plan->cols.size(); c++)
                    if (plan->cols[c].name == field) idx = (int)c;
                if (idx < 0) {
                    set_error("filters: unknown field '%s'", field.c_str());
                    return nullptr;
                }
                static const char *ops[] = {"eq", "ne", "lt", "le",
                                            "gt", "ge", "is_null",
                                            "is_not_null"};
                int opc = -1;
                for (int o = 0; o < 8; o++)
                    if (op == ops[o]) opc = o;
                if (opc < 0) {
                    set_error("filters: unknown op '%s'", op.c_str());
                    return nullptr;
                }
                FilterTerm ft{};
                ft.col = idx;
                ft.op = opc;
                int dt = plan->cols[idx].dtype;
                if (dt == PMH_DT_STRING && opc < 6 && opc > 1) {
                    set_error("filters: order comparisons on string "
                              "columns are not supported (dictionary ids "
                              "are unordered); eq/ne/is_null only");
                    return nullptr;
                }
                ft.is_fp = (dt == PMH_DT_FLOAT32 || dt == PMH_DT_FLOAT64);
                if (opc < 6) {
                    if (ft.is_fp)
                        ft.dlit = f["literal"].type == Json::NUM
                                      ? f["literal"].num
                                      : 0.0;
                    else ft.ilit = f["literal"].as_i64(0);
                }
                plan->filters.push_back(ft);
            }
            if (!plan->filters.empty()) {
                plan->filters_dev = (FilterTerm *)plan->bufs.alloc(
                    plan->filters.size() * sizeof(FilterTerm));
                if (!plan->filters_dev ||
                    hipMemcpy(plan->filters_dev, plan->filters.data(),
                              plan->filters.size() * sizeof(FilterTerm),
                              hipMemcpyHostToDevice) != hipSuccess) {
                    set_error("H2D filters failed");
                    return nullptr;
                }
            }
        }

        std::vector<FileDesc> files;
        int idx = 0;
        for (const auto &fj : j["files"].arr) {
            FileDesc fd;
            fd.path = fj["path"].as_str();
            fd.row_count = fj["rowCount"].as_i64();
            fd.min_key = fj["minKey"].as_i64();
            fd.max_key = fj["maxKey"].as_i64();
            fd.level = (int)fj["level"].as_i64();
            fd.input_index = idx++;
            const Json &dv = fj["deletionVector"];
            if (!dv.obj.empty()) {
                fd.dv_path = dv["file"].as_str();
                fd.dv_offset = dv["offset"].as_i64();
                fd.dv_length = dv["length"].as_i64();
            }
            if (fd.row_count >= ((int64_t)1 << PMH_ROW_BITS)) {
                set_error("file %s exceeds 2^%d rows-per-run limit",
                          fd.path.c_str(), PMH_ROW_BITS);
                return nullptr;
            }
            files.push_back(fd);
        }
        if (files.empty()) {
            set_error("no files in plan");
            return nullptr;
        }

        if (hipStreamCreate(&plan->stream) != hipSuccess) {
            set_error("hipStreamCreate failed");
            return nullptr;
        }

        auto sections = interval_partition(files, plan->changelog);
        auto t0 = std::chrono::steady_clock::now();
        if (plan->lookup) {
            // lookup levels (LookupMergeTreeCompactRewriter.java:211-219:
            // the lookup starts at outputLevel + 1): group lookup_files by
            // level into one sorted run per level, files of a level
            // concatenated in key order — staged ONCE here, before the
            // sections, whose descriptor tables reference them
            std::map<int, std::vector<FileDesc>> by_level;
            int max_merge_level = 0;
            for (const auto &fd : files)
                max_merge_level = std::max(max_merge_level, fd.level);
            for (const auto &fj : j["lookup_files"].arr) {
                FileDesc fd;
                fd.path = fj["path"].as_str();
                fd.row_count = fj["rowCount"].as_i64();
                fd.min_key = fj["minKey"].as_i64();
                fd.max_key = fj["maxKey"].as_i64();
                fd.level = (int)fj["level"].as_i64();
                if (!fj["deletionVector"].obj.empty()) {
                    set_error("lookup file %s carries a deletionVector: the "
                              "deletion-vector lookup strategy is not "
                              "supported in v1", fd.path.c_str());
                    return nullptr;
                }
                if (fd.level <= max_merge_level || fd.level > 255) {
                    set_error("lookup file %s: level %d must be above every "
                              "level in files (max %d) — lookup levels are "
                              "outputLevel+1 .. maxLevel", fd.path.c_str(),
                              fd.level, max_merge_level);
                    return nullptr;
                }
                by_level[fd.level].push_back(fd);
            }
            size_t max_k = 0;
            for (auto &sf : sections) max_k = std::max(max_k, sf.size());
            if (max_k + by_level.size() > (size_t)PMH_MAX_RUNS) {
                set_error("%zu merge runs + %zu lookup levels exceed the %d "
                          "run slots of a section", max_k, by_level.size(),
                          PMH_MAX_RUNS);
                return nullptr;
            }
            for (auto &kv : by_level) {
                auto &lf = kv.second;
                std::sort(lf.begin(), lf.end(),
                          [](const FileDesc &a, const FileDesc &b) {
                              return a.min_key < b.min_key;
                          });
                int64_t rows = 0;
                for (size_t i = 0; i < lf.size(); i++) {
                    rows += lf[i].row_count;
                    if (i > 0 && lf[i].min_key <= lf[i - 1].max_key) {
                        set_error("lookup level %d: files %s and %s overlap "
                                  "in key range (a level above 0 is one "
                                  "sorted run)", kv.first,
                                  lf[i - 1].path.c_str(), lf[i].path.c_str());
                        return nullptr;
                    }
                }
                if (rows >= ((int64_t)1 << PMH_ROW_BITS)) {
                    set_error("lookup level %d totals %lld rows >= 2^%d "
                              "rows-per-run limit", kv.first,
                              (long long)rows, PMH_ROW_BITS);
                    return nullptr;
                }
            }
            Section &ls = plan->lookup_sec;
            ls.runs.resize(by_level.size());
            size_t li = 0;
            for (auto &kv : by_level)  // std::map: ascending level
                if (!stage_run(plan.get(), kv.second, ls.runs[li++]))
                    return nullptr;
            if (!build_decode_tables(plan.get(), ls)) {
                set_error("device allocation failed for lookup levels");
                return nullptr;
            }
            // decode once: the levels stay resident (and decoded) across
            // sections and pmh_plan_reset
            const char *dwhat = "decode";
            hipError_t de = launch_section_decode(plan.get(), ls,
                                                  plan->stream, &dwhat);
            if (de == hipSuccess) de = hipStreamSynchronize(plan->stream);
            if (de != hipSuccess) {
                set_error("lookup levels %s: %s", dwhat,
                          hipGetErrorString(de));
                return nullptr;
            }
            if (ls.n_varint || ls.n_ts) {
                uint32_t ew = 0;
                if (hipMemcpy(&ew, ls.tiles.err, 4, hipMemcpyDeviceToHost) !=
                    hipSuccess) {
                    set_error("lookup levels: err D2H failed");
                    return nullptr;
                }
                const std::string msg = error_word_message(plan.get(), ew);
                if (!msg.empty()) {
                    set_error("lookup levels: %s", msg.c_str());
                    return nullptr;
                }
            }
        }
        for (auto &sec_files : sections) {
            Section sec;
            if ((int)sec_files.size() > PMH_MAX_RUNS) {
                if (plan->pu || plan->agg || plan->ignore_delete ||
                    plan->changelog || plan->fused || plan->composite_key) {
                    set_error(
                        "section has %zu runs > %d: the hierarchical "
                        "winner merge serves deduplicate/first-row without "
                        "ignore-delete / changelog / sequence-fields / "
                        "composite keys in v1 (the reference spills to "
                        "disk here, MergeSorter.java:112-125)",
                        sec_files.size(), PMH_MAX_RUNS);
                    return nullptr;
                }
                sec.hier = true;
            }
            sec.runs.resize(sec_files.size());
            int64_t run_rows = 0;
            for (size_t r = 0; r < sec_files.size(); r++) {
                if (!stage_run(plan.get(), sec_files[r], sec.runs[r]))
                    return nullptr;
                run_rows += sec.runs[r].length;
            }
            if (!plan->filters.empty() && sec.runs.size() == 1 &&
                !sec.runs[0].tomb && sec.runs[0].length > 0) {
                // single-run section: value filters apply via the
                // tombstone mechanism (k_filter marks failing rows)
                sec.runs[0].tomb =
                    (uint8_t *)plan->bufs.alloc(sec.runs[0].length);
                if (!sec.runs[0].tomb ||
                    hipMemset(sec.runs[0].tomb, 0,
                              sec.runs[0].length) != hipSuccess) {
                    set_error("filter tombstone allocation failed");
                    return nullptr;
                }
            }
            if (!build_section_descriptors(plan.get(), sec)) {
                set_error("device allocation failed for section");
                return nullptr;
            }
            if (sec.hier && !build_hier_section(plan.get(), sec))
                return nullptr;
            if (plan->cl_fold) {
                // the folded changelog kernels keep per-run column tables in
                // LDS
                const int64_t lds = pmh_fold_cl_lds(
                    (int64_t)sec.runs.size(), (int64_t)plan->cols.size());
                if (lds > PMH_FOLD_CL_LDS_MAX) {
                    set_error("changelog_producer=full-compaction with the "
                              "%s engine: a section of %zu runs x %zu columns "
                              "needs %lld bytes of column tables (limit %lld)",
                              plan->agg ? "aggregation" : "partial-update",
                              sec.runs.size(), plan->cols.size(),
                              (long long)lds,
                              (long long)PMH_FOLD_CL_LDS_MAX);
                    return nullptr;
                }
            }
            plan->rows_in_total += run_rows;
            plan->sections.push_back(std::move(sec));
        }
        auto t1 = std::chrono::steady_clock::now();
        plan->h2d_ms =
            std::chrono::duration<double, std::milli>(t1 - t0).count();

        // output buffers: sized for the largest section
        int64_t max_rows = 0;
        for (auto &sec : plan->sections)
            max_rows = std::max(max_rows, sec.total_rows);
        int n_cols = (int)plan->cols.size();
        std::vector<void *> outs(n_cols);
        std::vector<uint8_t> dts(n_cols);
        for (int c = 0; c < n_cols; c++) {
            outs[c] = plan->bufs.alloc(max_rows * plan->cols[c].out_esize);
            if (!outs[c]) {
                set_error("output allocation failed");
                return nullptr;
            }
            dts[c] = (uint8_t)plan->cols[c].dtype;
        }
        plan->out.dev = outs;
        void **out_ptrs_dev =
            (void **)plan->bufs.alloc(n_cols * sizeof(void *));
        uint8_t *col_dtype_dev = (uint8_t *)plan->bufs.alloc(n_cols);
        if (hipMemcpy(out_ptrs_dev, outs.data(), n_cols * sizeof(void *),
                      hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(col_dtype_dev, dts.data(), n_cols,
                      hipMemcpyHostToDevice) != hipSuccess) {
            set_error("H2D of output descriptors failed");
            return nullptr;
        }
        // per-column nullability (any staged nulls in any section/run) +
        // output validity buffers
        plan->col_nullable.assign(n_cols, false);
        for (auto &sec : plan->sections)
            for (auto &run : sec.runs)
                for (int c = 0; c < n_cols; c++)
                    if (run.cols[c].has_nulls) plan->col_nullable[c] = true;
        for (auto &run : plan->lookup_sec.runs)
            for (int c = 0; c < n_cols; c++)
                if (run.cols[c].has_nulls) plan->col_nullable[c] = true;
        plan->out.valid.assign(n_cols, nullptr);
        std::vector<uint8_t> nul(n_cols, 0);
        for (int c = 0; c < n_cols; c++) {
            nul[c] = plan->col_nullable[c] ? 1 : 0;
            if (plan->col_nullable[c]) {
                // validity outputs keep emit off the streamed kernel
                plan->columns.any_nullable = 1;
                plan->out.valid[c] = (uint8_t *)plan->bufs.alloc(max_rows);
                if (!plan->out.valid[c]) {
                    set_error("validity allocation failed");
                    return nullptr;
                }
            }
        }
        uint8_t *col_nullable_dev = (uint8_t *)plan->bufs.alloc(n_cols);
        uint8_t **out_valid_dev =
            (uint8_t **)plan->bufs.alloc(n_cols * sizeof(void *));
        if (hipMemcpy(col_nullable_dev, nul.data(), n_cols,
                      hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(out_valid_dev, plan->out.valid.data(),
                      n_cols * sizeof(void *),
                      hipMemcpyHostToDevice) != hipSuccess) {
            set_error("H2D of validity descriptors failed");
            return nullptr;
        }
        plan->out.set = OutputSet{out_ptrs_dev, out_valid_dev};
        plan->columns.dtype = col_dtype_dev;
        plan->columns.nullable = col_nullable_dev;
        if (plan->changelog) {
            // changelog outputs: up to 2 rows per key group <= 2 * inputs
            int64_t cap2 = 2 * max_rows;
            OutBatch &o2 = plan->out2;
            o2.dev.resize(n_cols);
            o2.valid.assign(n_cols, nullptr);
            for (int c = 0; c < n_cols; c++) {
                o2.dev[c] = plan->bufs.alloc(cap2 * plan->cols[c].out_esize);
                if (!o2.dev[c]) {
                    set_error("changelog output allocation failed");
                    return nullptr;
                }
                if (plan->col_nullable[c]) {
                    o2.valid[c] = (uint8_t *)plan->bufs.alloc(cap2);
                    if (!o2.valid[c]) {
                        set_error("changelog validity allocation failed");
                        return nullptr;
                    }
                }
            }
            void **ptrs2 = (void **)plan->bufs.alloc(n_cols * sizeof(void *));
            uint8_t **valid2 =
                (uint8_t **)plan->bufs.alloc(n_cols * sizeof(void *));
            if (!ptrs2 || !valid2 ||
                hipMemcpy(ptrs2, o2.dev.data(), n_cols * sizeof(void *),
                          hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(valid2, o2.valid.data(), n_cols * sizeof(void *),
                          hipMemcpyHostToDevice) != hipSuccess) {
                set_error("H2D of changelog descriptors failed");
                return nullptr;
            }
            o2.set = OutputSet{ptrs2, valid2};
        }
        for (auto &cs : plan->cols) plan->col_names.push_back(cs.name);
        if (plan->agg) {
            // unnamed value columns get last_non_null_value
            // (AggregateMergeFunction.java:197-203)
            std::vector<uint8_t> ca(n_cols, PMH_AGG_LAST_NON_NULL);
            const int first_val = plan->columns.first_val();
            if (!parse_agg_table(plan.get(), j, false, {}, {}, ca))
                return nullptr;
            // retract records are accepted iff EVERY value column's
            // aggregator supports retraction (FieldSumAgg.retract,
            // FieldPrimaryKeyAgg) or ignores it (ignore-retract wrapper) —
            // otherwise the reference throws on the first retract
            // (FieldAggregator.retract :47-53) and so do we, at merge time
            {
                bool all_rt = true;
                for (int c = first_val; c < n_cols; c++) {
                    uint8_t a = ca[c];
                    if (a & PMH_AGG_IGNORE_RETRACT) continue;
                    if (a == PMH_AGG_SUM || a == PMH_AGG_PRIMARY_KEY)
                        continue;
                    all_rt = false;
                }
                plan->agg_retract = all_rt && !plan->rrod;
            }
            uint8_t *ca_dev = (uint8_t *)plan->bufs.alloc(n_cols);
            if (!ca_dev || hipMemcpy(ca_dev, ca.data(), n_cols,
                                     hipMemcpyHostToDevice) != hipSuccess) {
                set_error("H2D of aggregator codes failed");
                return nullptr;
            }
            plan->columns.agg = ca_dev;
        }
        // the batch pass of hierarchical sections reads the same columns at
        // their stored width (build_hier_section made its dtype map)
        {
            const uint8_t *hd = plan->hier_columns.dtype;
            plan->hier_columns = plan->columns;
            plan->hier_columns.dtype = hd;
        }
        plan->merge_flags =
            (plan->drop_delete ? PMH_FLAG_DROP_DELETE : 0) |
            (plan->ignore_delete ? PMH_FLAG_IGNORE_DELETE : 0) |
            (plan->pu ? PMH_FLAG_MEMBERS : 0) |
            (plan->first_row ? PMH_FLAG_FIRST_ROW : 0) |
            (plan->rrod ? PMH_FLAG_RROD : 0) |
            (plan->seqg ? PMH_FLAG_SEQ_GROUPS : 0) |
            (plan->agg_retract ? PMH_FLAG_AGG_RETRACT : 0) |
            (plan->cl_row_dedup ? PMH_FLAG_CL_ROW_DEDUP : 0) |
            (plan->lookup ? PMH_FLAG_LOOKUP : 0) |
            (plan->cl_fold ? PMH_FLAG_FOLD_CL : 0);
    } catch (const std::exception &e) {
        set_error("plan parse: %s", e.what());
        return nullptr;
    }
    plan->stats.h2d_ms = plan->h2d_ms;
    return plan.release();
}

int64_t pmh_read_next(pmh_plan_t *p, pmh_batch *out) {
    if (!p) {
        set_error("null plan");
        return -1;
    }
    if (p->cur_section >= p->sections.size()) return 0;
    (void)hipSetDevice(p->session->device);
    Section &sec = p->sections[p->cur_section++];
    ReadPass rp{p,         sec,          p->stream,
                p->merge_flags | profile_flags(),
                sec.runs_dev,  sec.tiles, sec.total_rows, {}};
    if (!read_decode(rp)) return -1;
    if (sec.hier && !read_hier_batches(rp)) return -1;
    if (!read_partition(rp)) return -1;
    if (p->fused) {
        if (!read_fused(rp)) return -1;
    } else if (!read_chain(rp) || !read_changelog_tail(rp)) {
        return -1;
    }
    rp.ev.record(StageEvents::EMITTED, rp.st);
    return read_collect(rp, out);
}

// Changelog batch of the LAST pmh_read_next call (changelog_producer =
// full-compaction). Valid until the next read_next, like the main batch.
int64_t pmh_changelog_next(pmh_plan_t *p, pmh_batch *out) {
    if (!p) return -1;
    if (!p->changelog) {
        set_error("plan has no changelog_producer configured");
        return -1;
    }
    if (out) {
        out->n_rows = p->cl_rows_last;
        out->n_cols = (int32_t)p->cols.size();
        out->device = p->host_output ? -1 : p->session->device;
        out->cols = p->out2.cols.data();
    }
    return p->cl_rows_last;
}

int pmh_plan_reset(pmh_plan_t *p) {
    if (!p) return -1;
    p->cur_section = 0;
    return 0;
}

int pmh_plan_close(pmh_plan_t *p) {
    if (!p) return 0;
    delete p;  // its destructor releases the stream and the buffers
    return 0;
}

int pmh_stats_get(pmh_plan_t *p, pmh_stats *out) {
    if (p) p->stats.path_mode = !p->fused ? 0 : (p->fsplit ? 2 : 1);
    if (!p || !out) return -1;
    p->stats.hbm_bytes_algo = 0;  // filled by bench from encoded+output sizes
    *out = p->stats;
    out->hbm_bytes_algo = p->encoded_bytes_total;
    return 0;
}

void pmh_free_string(char *s) { free(s); }

int64_t pmh_debug_parse_dv(const char *path, int64_t offset, int64_t length,
                           int64_t *out, int64_t cap) {
    std::vector<uint32_t> pos;
    if (!load_deletion_vector(path, offset, length, pos)) return -1;
    int64_t n = (int64_t)pos.size() < cap ? (int64_t)pos.size() : cap;
    for (int64_t i = 0; i < n; i++) out[i] = pos[i];
    return (int64_t)pos.size();
}

// CPU-side entry to the scalar zstd restatement (zstd_core.h): decode one
// frame; the CPU tests fuzz this against libzstd before the GPU kernel
// (which shares the same core) ever runs.
int64_t pmh_debug_zstd_cpu(const void *src, int64_t n, void *dst,
                           int64_t cap) {
    std::vector<uint8_t> lit(PZ_BLOCK_MAX);
    std::vector<PzCtx> cx(1);
    int64_t r = pz_decode_frame((const uint8_t *)src, n, (uint8_t *)dst, cap,
                                lit.data(), cx.data());
    if (r < 0) set_error("pz_decode_frame: error %lld", (long long)r);
    return r;
}

// GPU round trip of the zstd page kernel: decode one frame whose
// decompressed size the caller knows (parity tests vs libzstd on the box).
int64_t pmh_debug_zstd_gpu(const void *src, int64_t n, void *dst,
                           int64_t expected) {
    std::vector<ZstdBatchPage> zp(1);
    zp[0] = {0, n, 0, expected};
    if (!gpu_zstd_batch((const uint8_t *)src, n, zp, (uint8_t *)dst,
                        expected)) {
        set_error("gpu zstd decode failed (batch of 1)");
        return -1;
    }
    return expected;
}

// CPU-side entry to the from-scratch zstd ENCODER (zstd_core.h): compress
// one frame; tests round-trip it through libzstd/pyarrow to prove the
// frames are spec-valid (the GPU kernel shares the same core).
int64_t pmh_debug_zstd_enc_cpu(const void *src, int64_t n, void *dst,
                               int64_t cap) {
    std::vector<PzEnc> e(1);
    std::vector<int32_t> ht(1 << PZ_ENC_HLOG);
    e[0].htab = ht.data();
    int64_t r = pz_encode_frame((const uint8_t *)src, n, (uint8_t *)dst,
                                cap, e.data());
    if (r < 0) set_error("pz_encode_frame: error %lld", (long long)r);
    return r;
}

// GPU round trip of the zstd COMPRESS kernel (batch of 1).
int64_t pmh_debug_zstd_enc_gpu(const void *src, int64_t n, void *dst,
                               int64_t cap) {
    std::vector<std::string> in(1);
    in[0].assign((const char *)src, (size_t)n);
    std::vector<std::vector<uint8_t>> outs;
    if (!pw_gpu_zstd_compress(in, outs)) {
        set_error("gpu zstd compress failed (batch of 1)");
        return -1;
    }
    if ((int64_t)outs[0].size() > cap) return PZ_ERR_DST_SMALL;
    memcpy(dst, outs[0].data(), outs[0].size());
    return (int64_t)outs[0].size();
}

// Stream-level entry to the three ORC integer decoders (host_rlev2_u, the
// prescan walk, k_rlev2): see paimon_hip.h. Calls the very functions the
// plan calls.
int64_t pmh_debug_orc_ints(const void *stream, int64_t len, int64_t n_values,
                           int kind, int out_esize, int mode,
                           int64_t src_shift, void *out, int64_t out_cap) {
    const uint8_t *s = (const uint8_t *)stream;
    if ((!s && len > 0) || len < 0 || kind < 0 || kind > 2 || mode < 0 ||
        mode > 2 || (out_cap > 0 && !out)) {
        set_error("pmh_debug_orc_ints: bad arguments");
        return -1;
    }
    if (mode == 0) {  // host twin
        if (kind != 1) {
            set_error("pmh_debug_orc_ints: the host decoder is unsigned "
                      "RLEv2 only (kind 1)");
            return -1;
        }
        std::vector<uint64_t> v;
        const char *why = "";
        if (!host_rlev2(s, len, n_values, false, v, &why)) {
            set_error("pmh_debug_orc_ints: host RLEv2 decode failed (%s)",
                      why);
            return -1;
        }
        int64_t n = std::min<int64_t>((int64_t)v.size(), out_cap);
        if (n > 0) memcpy(out, v.data(), (size_t)n * 8);
        return (int64_t)v.size();
    }
    if (n_values < 0 || (out_esize != 4 && out_esize != 8) ||
        src_shift < 0 || src_shift > 7) {
        set_error("pmh_debug_orc_ints: bad arguments (n_values >= 0, "
                  "out_esize 4|8, src_shift 0..7)");
        return -1;
    }
    auto prescan = [&](uint64_t dev_base, std::vector<Rlev2Chunk> &ch) {
        const char *why = "";
        const bool ok =
            kind == 2 ? prescan_byterle(s, len, n_values, out_esize, 0,
                                        dev_base, 0, ch, &why)
                      : prescan_rlev2(s, len, n_values, kind == 0, out_esize,
                                      0, dev_base, 0, ch, &why);
        if (!ok) set_error("%s", why);
        return ok;
    };
    std::vector<Rlev2Chunk> chunks;
    if (mode == 1) {  // prescan only: dummy device base
        if (!prescan(0x1000, chunks)) return -1;
        return (int64_t)chunks.size();
    }
    if (out_cap < n_values) {
        set_error("pmh_debug_orc_ints: out_cap < n_values");
        return -1;
    }
    if (n_values == 0) return 0;
    // device path: stream at an 8-byte-aligned address + src_shift with the
    // 16-byte tail pad staging gives it; output between two guard zones
    const int64_t GUARD = 64;  // elements, each side
    const uint8_t FILL = 0xA5;
    uint8_t *d_src = nullptr, *d_out = nullptr;
    Rlev2Chunk *d_chunks = nullptr;
    const size_t out_bytes = (size_t)(n_values + 2 * GUARD) * out_esize;
    std::vector<uint8_t> back(out_bytes);
    int64_t rc = -1;
    do {
        if (hipMalloc(&d_src, (size_t)len + 8 + 16) != hipSuccess ||
            hipMalloc(&d_out, out_bytes) != hipSuccess) {
            set_error("pmh_debug_orc_ints: hipMalloc failed");
            break;
        }
        if (((uint64_t)d_src & 7) != 0) {
            set_error("pmh_debug_orc_ints: device allocation not 8-aligned");
            break;
        }
        if (hipMemset(d_src, 0, (size_t)len + 8 + 16) != hipSuccess ||
            hipMemset(d_out, FILL, out_bytes) != hipSuccess ||
            (len && hipMemcpy(d_src + src_shift, s, (size_t)len,
                              hipMemcpyHostToDevice) != hipSuccess)) {
            set_error("pmh_debug_orc_ints: H2D failed");
            break;
        }
        if (!prescan((uint64_t)(d_src + src_shift), chunks)) break;
        // the prescan may overshoot n_values only in an RLEv2 stream's last
        // run; the plan sizes its buffers from the file's row count, so a
        // stream that decodes past n_values is refused here, not run
        int64_t total = 0;
        for (auto &c : chunks) {
            c.out_addr = (uint64_t)(d_out + GUARD * out_esize);
            total = std::max<int64_t>(total, c.out_start + c.count);
        }
        if (total > n_values) {
            set_error("pmh_debug_orc_ints: stream holds %lld values, more "
                      "than n_values %lld", (long long)total,
                      (long long)n_values);
            break;
        }
        if (hipMalloc(&d_chunks, chunks.size() * sizeof(Rlev2Chunk)) !=
                hipSuccess ||
            hipMemcpy(d_chunks, chunks.data(),
                      chunks.size() * sizeof(Rlev2Chunk),
                      hipMemcpyHostToDevice) != hipSuccess) {
            set_error("pmh_debug_orc_ints: chunk upload failed");
            break;
        }
        hipError_t e =
            pmh_launch_rlev2(d_chunks, (int64_t)chunks.size(), nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess)
            e = hipMemcpy(back.data(), d_out, out_bytes,
                          hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            set_error("pmh_debug_orc_ints: k_rlev2: %s",
                      hipGetErrorString(e));
            break;
        }
        rc = n_values;
        const size_t g = (size_t)GUARD * out_esize;
        for (size_t i = 0; i < g; i++)
            if (back[i] != FILL || back[out_bytes - 1 - i] != FILL) {
                set_error("pmh_debug_orc_ints: k_rlev2 wrote outside its "
                          "output (guard zone changed)");
                rc = -2;
                break;
            }
        memcpy(out, back.data() + g, (size_t)n_values * out_esize);
    } while (0);
    if (d_src) (void)hipFree(d_src);
    if (d_out) (void)hipFree(d_out);
    if (d_chunks) (void)hipFree(d_chunks);
    return rc;
}

// Stream-level entry to the ORC DECIMAL decode (prescan_varint, the shared
// scalar core, k_orc_varint): see paimon_hip.h. Calls the very functions the
// plan calls.
int64_t pmh_debug_orc_decimal(const void *data, int64_t len,
                              const int32_t *scales, int precision,
                              int scale, int64_t n_values, int out_esize,
                              int mode, int64_t src_shift, void *out,
                              int64_t out_cap) {
    const uint8_t *s = (const uint8_t *)data;
    if ((!s && len > 0) || len < 0 || n_values < 0 ||
        (mode != 0 && mode != 2) || (out_esize != 4 && out_esize != 8) ||
        precision < 1 || precision > ODC_MAX_PRECISION || scale < 0 ||
        scale > 18 || src_shift < 0 || src_shift > 7 || out_cap < n_values ||
        (n_values > 0 && !out)) {
        set_error("pmh_debug_orc_decimal: bad arguments (mode 0|2, out_esize "
                  "4|8, precision 1..19, scale 0..18, src_shift 0..7, "
                  "out_cap >= n_values >= 0)");
        return -1;
    }
    if (n_values == 0) return 0;
    std::vector<VarintUnit> units;
    const char *why = "";
    if (mode == 0) {  // host twin
        if (!prescan_varint(s, len, n_values, out_esize, precision, scale, 0,
                            0, 0, units, &why)) {
            set_error("pmh_debug_orc_decimal: %s", why);
            return -1;
        }
        for (const auto &u : units) {
            int bad = 0;
            int err = odc_decode_unit_host(
                s + u.src, u, scales ? scales + u.out_start : nullptr, out,
                &bad);
            if (err) {
                set_error("pmh_debug_orc_decimal: ORC decimal rescale "
                          "failed at value %lld: %s",
                          (long long)(u.out_start + bad), odc_err_text(err));
                return -1;
            }
        }
        return n_values;
    }
    // device path: stream at an 8-byte-aligned address + src_shift with the
    // 16-byte tail pad staging gives it; output between two guard zones
    const int64_t GUARD = 64;  // elements, each side
    const uint8_t FILL = 0xA5;
    uint8_t *d_src = nullptr, *d_out = nullptr;
    int32_t *d_scales = nullptr;
    uint32_t *d_err = nullptr;
    VarintUnit *d_units = nullptr;
    const size_t out_bytes = (size_t)(n_values + 2 * GUARD) * out_esize;
    std::vector<uint8_t> back(out_bytes);
    int64_t rc = -1;
    do {
        if (hipMalloc(&d_src, (size_t)len + 8 + 16) != hipSuccess ||
            hipMalloc(&d_out, out_bytes) != hipSuccess ||
            hipMalloc(&d_err, 4) != hipSuccess ||
            (scales &&
             hipMalloc(&d_scales, (size_t)n_values * 4) != hipSuccess)) {
            set_error("pmh_debug_orc_decimal: hipMalloc failed");
            break;
        }
        if (((uint64_t)d_src & 7) != 0) {
            set_error("pmh_debug_orc_decimal: device allocation not "
                      "8-aligned");
            break;
        }
        if (hipMemset(d_src, 0, (size_t)len + 8 + 16) != hipSuccess ||
            hipMemset(d_out, FILL, out_bytes) != hipSuccess ||
            hipMemset(d_err, 0, 4) != hipSuccess ||
            (len && hipMemcpy(d_src + src_shift, s, (size_t)len,
                              hipMemcpyHostToDevice) != hipSuccess) ||
            (scales && hipMemcpy(d_scales, scales, (size_t)n_values * 4,
                                 hipMemcpyHostToDevice) != hipSuccess)) {
            set_error("pmh_debug_orc_decimal: H2D failed");
            break;
        }
        if (!prescan_varint(s, len, n_values, out_esize, precision, scale, 0,
                            (uint64_t)(d_src + src_shift), 0, units, &why)) {
            set_error("pmh_debug_orc_decimal: %s", why);
            break;
        }
        for (auto &u : units) {
            u.out_addr = (uint64_t)(d_out + GUARD * out_esize);
            u.scale_addr =
                d_scales ? (uint64_t)(d_scales + u.out_start) : 0;
            u.err_addr = (uint64_t)d_err;
        }
        if (hipMalloc(&d_units, units.size() * sizeof(VarintUnit)) !=
                hipSuccess ||
            hipMemcpy(d_units, units.data(),
                      units.size() * sizeof(VarintUnit),
                      hipMemcpyHostToDevice) != hipSuccess) {
            set_error("pmh_debug_orc_decimal: unit upload failed");
            break;
        }
        uint32_t err_word = 0;
        hipError_t e =
            pmh_launch_orc_varint(d_units, (int64_t)units.size(), nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess)
            e = hipMemcpy(back.data(), d_out, out_bytes,
                          hipMemcpyDeviceToHost);
        if (e == hipSuccess)
            e = hipMemcpy(&err_word, d_err, 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            set_error("pmh_debug_orc_decimal: k_orc_varint: %s",
                      hipGetErrorString(e));
            break;
        }
        rc = n_values;
        const size_t g = (size_t)GUARD * out_esize;
        for (size_t i = 0; i < g; i++)
            if (back[i] != FILL || back[out_bytes - 1 - i] != FILL) {
                set_error("pmh_debug_orc_decimal: k_orc_varint wrote "
                          "outside its output (guard zone changed)");
                rc = -2;
                break;
            }
        memcpy(out, back.data() + g, (size_t)n_values * out_esize);
        if (rc >= 0 && orc_decimal_bits(err_word)) {
            set_error("pmh_debug_orc_decimal: %s",
                      orc_decimal_error(err_word).c_str());
            rc = -1;
        }
    } while (0);
    if (d_src) (void)hipFree(d_src);
    if (d_out) (void)hipFree(d_out);
    if (d_scales) (void)hipFree(d_scales);
    if (d_err) (void)hipFree(d_err);
    if (d_units) (void)hipFree(d_units);
    return rc;
}

// Stream-level entry to the BOOLEAN decode (the two prescans, the shared
// scalar core, k_bits_expand): see paimon_hip.h. Calls the very functions
// the plan calls.
int64_t pmh_debug_bits(const void *stream, int64_t len, int64_t n_values,
                       int bit_order, int format, int out_esize, int mode,
                       int64_t src_shift, int64_t out_shift, void *out,
                       int64_t out_cap) {
    const uint8_t *s = (const uint8_t *)stream;
    if ((!s && len > 0) || len < 0 || n_values < 0 ||
        (bit_order != BITS_LSB && bit_order != BITS_MSB) ||
        (format != 0 && format != 1) || (out_esize != 1 && out_esize != 4) ||
        (mode != 0 && mode != 2) || src_shift < 0 || src_shift > 7 ||
        out_shift < 0 || out_shift > 7 || out_cap < n_values ||
        (n_values > 0 && !out)) {
        set_error("pmh_debug_bits: bad arguments (bit_order 0|1, format 0|1, "
                  "out_esize 1|4, mode 0|2, src_shift 0..7, out_shift 0..7, "
                  "out_cap >= n_values >= 0)");
        return -1;
    }
    if (n_values == 0) return 0;
    std::vector<BitsUnit> units;
    auto prescan = [&](uint64_t dev_base) {
        const char *why = "";
        units.clear();
        const bool ok =
            format == 0 ? prescan_bits_plain(s, len, n_values, out_esize, 0,
                                             dev_base, 0, units, &why)
                        : prescan_boolrle(s, len, n_values, out_esize, 0,
                                          dev_base, 0, units, &why);
        if (!ok) set_error("pmh_debug_bits: %s", why);
        for (auto &u : units) u.msb = (uint8_t)bit_order;
        return ok;
    };
    if (mode == 0) {  // host twin: src offsets relative to the stream
        if (!prescan(0)) return -1;
        for (auto &u : units) {
            // pose the requested alignment: element 0 sits out_shift
            // elements past an address aligned to 8 elements
            u.out_addr = (uint64_t)out_shift * (uint64_t)out_esize;
            bits_decode_unit_host(s + u.src, u, out);
        }
        return n_values;
    }
    // device path: stream at an 8-byte-aligned address + src_shift with the
    // 16-byte tail pad staging gives it; output out_shift elements past an
    // address aligned to 8 elements, between two guard zones
    const int64_t GUARD = 64;  // elements, each side (a multiple of 8)
    const uint8_t FILL = 0xA5;
    uint8_t *d_src = nullptr, *d_out = nullptr;
    BitsUnit *d_units = nullptr;
    const size_t lead = (size_t)(GUARD + out_shift) * out_esize;
    const size_t body = (size_t)n_values * out_esize;
    const size_t out_bytes = lead + body + (size_t)GUARD * out_esize;
    std::vector<uint8_t> back(out_bytes);
    int64_t rc = -1;
    do {
        if (hipMalloc(&d_src, (size_t)len + 8 + 16) != hipSuccess ||
            hipMalloc(&d_out, out_bytes) != hipSuccess) {
            set_error("pmh_debug_bits: hipMalloc failed");
            break;
        }
        if (((uint64_t)d_src & 7) != 0 || ((uint64_t)d_out & 31) != 0) {
            set_error("pmh_debug_bits: device allocation not aligned");
            break;
        }
        if (hipMemset(d_src, 0, (size_t)len + 8 + 16) != hipSuccess ||
            hipMemset(d_out, FILL, out_bytes) != hipSuccess ||
            (len && hipMemcpy(d_src + src_shift, s, (size_t)len,
                              hipMemcpyHostToDevice) != hipSuccess)) {
            set_error("pmh_debug_bits: H2D failed");
            break;
        }
        if (!prescan((uint64_t)(d_src + src_shift))) break;
        for (auto &u : units) u.out_addr = (uint64_t)(d_out + lead);
        if (hipMalloc(&d_units, units.size() * sizeof(BitsUnit)) !=
                hipSuccess ||
            hipMemcpy(d_units, units.data(), units.size() * sizeof(BitsUnit),
                      hipMemcpyHostToDevice) != hipSuccess) {
            set_error("pmh_debug_bits: unit upload failed");
            break;
        }
        hipError_t e =
            pmh_launch_bits_expand(d_units, (int64_t)units.size(), nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess)
            e = hipMemcpy(back.data(), d_out, out_bytes,
                          hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            set_error("pmh_debug_bits: k_bits_expand: %s",
                      hipGetErrorString(e));
            break;
        }
        rc = n_values;
        for (size_t i = 0; i < out_bytes; i++) {
            if (i >= lead && i < lead + body) continue;
            if (back[i] != FILL) {
                set_error("pmh_debug_bits: k_bits_expand wrote outside its "
                          "output (guard zone changed)");
                rc = -2;
                break;
            }
        }
        memcpy(out, back.data() + lead, body);
    } while (0);
    if (d_src) (void)hipFree(d_src);
    if (d_out) (void)hipFree(d_out);
    if (d_units) (void)hipFree(d_units);
    return rc;
}

// Stream-level entry to the ORC TIMESTAMP decode (prescan_rlev2 + k_rlev2
// for both streams, the shared scalar core, k_orc_timestamp): see
// paimon_hip.h.
int64_t pmh_debug_orc_timestamp(const void *data, int64_t data_len,
                                const void *secondary, int64_t secondary_len,
                                int64_t n_values, int unit, int mode,
                                void *out, int64_t out_cap) {
    const uint8_t *ds = (const uint8_t *)data;
    const uint8_t *ss = (const uint8_t *)secondary;
    if ((!ds && data_len > 0) || (!ss && secondary_len > 0) || data_len < 0 ||
        secondary_len < 0 || n_values < 0 ||
        (unit != OTS_UNIT_MILLIS && unit != OTS_UNIT_MICROS) ||
        (mode != 0 && mode != 2) || out_cap < n_values ||
        (n_values > 0 && !out)) {
        set_error("pmh_debug_orc_timestamp: bad arguments (unit 0|1, mode "
                  "0|2, out_cap >= n_values >= 0)");
        return -1;
    }
    if (n_values == 0) return 0;
    // both streams have to hold exactly n_values: the plan sizes the column
    // and the nanos scratch by the row count
    std::vector<Rlev2Chunk> dch, sch;
    auto prescan = [&](uint64_t d_base, uint64_t s_base) {
        dch.clear();
        sch.clear();
        const char *why = "";
        if (!prescan_rlev2(ds, data_len, n_values, 1, 8, 0, d_base, 0, dch,
                           &why) ||
            !prescan_rlev2(ss, secondary_len, n_values, 0, 8, 3, s_base, 0,
                           sch, &why)) {
            set_error("pmh_debug_orc_timestamp: %s", why);
            return false;
        }
        int64_t d_end = 0, s_end = 0;
        for (const auto &k : dch) d_end = k.out_start + k.count;
        for (const auto &k : sch) s_end = k.out_start + k.count;
        if (d_end != n_values || s_end != n_values) {
            set_error("pmh_debug_orc_timestamp: streams hold %lld seconds "
                      "and %lld nanos for %lld values", (long long)d_end,
                      (long long)s_end, (long long)n_values);
            return false;
        }
        return true;
    };
    if (mode == 0) {  // host: the oracle-independent host RLEv2 + the core
        if (!prescan(0x1000, 0x1000)) return -1;
        std::vector<uint64_t> secs_zz, nanos;
        const char *why = "";
        if (!host_rlev2(ds, data_len, n_values, true, secs_zz, &why) ||
            !host_rlev2(ss, secondary_len, n_values, false, nanos, &why) ||
            (int64_t)secs_zz.size() < n_values ||
            (int64_t)nanos.size() < n_values) {
            set_error("pmh_debug_orc_timestamp: host RLEv2 decode failed");
            return -1;
        }
        for (int64_t i = 0; i < n_values; i++) {
            int64_t v;
            const int err =
                ots_value((int64_t)secs_zz[i], nanos[i], unit, &v);
            if (err) {
                set_error("pmh_debug_orc_timestamp: ORC timestamp refused "
                          "at value %lld: %s", (long long)i,
                          ots_err_text(err));
                return -1;
            }
            ((int64_t *)out)[i] = v;
        }
        return n_values;
    }
    const int64_t GUARD = 64;  // elements, each side
    const uint8_t FILL = 0xA5;
    uint8_t *d_data = nullptr, *d_sec = nullptr, *d_out = nullptr;
    uint64_t *d_nanos = nullptr;
    uint32_t *d_err = nullptr;
    Rlev2Chunk *d_chunks = nullptr;
    TsUnit *d_units = nullptr;
    const size_t out_bytes = (size_t)(n_values + 2 * GUARD) * 8;
    std::vector<uint8_t> back(out_bytes);
    int64_t rc = -1;
    do {
        if (hipMalloc(&d_data, (size_t)data_len + 16) != hipSuccess ||
            hipMalloc(&d_sec, (size_t)secondary_len + 16) != hipSuccess ||
            hipMalloc(&d_out, out_bytes) != hipSuccess ||
            hipMalloc(&d_nanos, (size_t)n_values * 8) != hipSuccess ||
            hipMalloc(&d_err, 4) != hipSuccess) {
            set_error("pmh_debug_orc_timestamp: hipMalloc failed");
            break;
        }
        if (hipMemset(d_data, 0, (size_t)data_len + 16) != hipSuccess ||
            hipMemset(d_sec, 0, (size_t)secondary_len + 16) != hipSuccess ||
            hipMemset(d_out, FILL, out_bytes) != hipSuccess ||
            hipMemset(d_nanos, FILL, (size_t)n_values * 8) != hipSuccess ||
            hipMemset(d_err, 0, 4) != hipSuccess ||
            (data_len && hipMemcpy(d_data, ds, (size_t)data_len,
                                   hipMemcpyHostToDevice) != hipSuccess) ||
            (secondary_len &&
             hipMemcpy(d_sec, ss, (size_t)secondary_len,
                       hipMemcpyHostToDevice) != hipSuccess)) {
            set_error("pmh_debug_orc_timestamp: H2D failed");
            break;
        }
        if (!prescan((uint64_t)d_data, (uint64_t)d_sec)) break;
        for (auto &k : dch) k.out_addr = (uint64_t)(d_out + GUARD * 8);
        for (auto &k : sch) k.out_addr = (uint64_t)d_nanos;
        dch.insert(dch.end(), sch.begin(), sch.end());
        std::vector<TsUnit> units;
        for (int64_t d = 0; d < n_values; d += OTS_UNIT_VALUES) {
            TsUnit tu{};
            tu.out_addr = (uint64_t)(d_out + GUARD * 8);
            tu.nanos_addr = (uint64_t)d_nanos;
            tu.err_addr = (uint64_t)d_err;
            tu.out_start = d;
            tu.nanos_start = d;
            tu.count =
                (int32_t)std::min<int64_t>(OTS_UNIT_VALUES, n_values - d);
            tu.unit = (uint8_t)unit;
            units.push_back(tu);
        }
        if (hipMalloc(&d_chunks, dch.size() * sizeof(Rlev2Chunk)) !=
                hipSuccess ||
            hipMalloc(&d_units, units.size() * sizeof(TsUnit)) != hipSuccess ||
            hipMemcpy(d_chunks, dch.data(), dch.size() * sizeof(Rlev2Chunk),
                      hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_units, units.data(), units.size() * sizeof(TsUnit),
                      hipMemcpyHostToDevice) != hipSuccess) {
            set_error("pmh_debug_orc_timestamp: work upload failed");
            break;
        }
        uint32_t err_word = 0;
        hipError_t e = pmh_launch_rlev2(d_chunks, (int64_t)dch.size(), nullptr);
        if (e == hipSuccess)
            e = pmh_launch_orc_timestamp(d_units, (int64_t)units.size(),
                                         nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess)
            e = hipMemcpy(back.data(), d_out, out_bytes,
                          hipMemcpyDeviceToHost);
        if (e == hipSuccess)
            e = hipMemcpy(&err_word, d_err, 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            set_error("pmh_debug_orc_timestamp: k_rlev2 / k_orc_timestamp: "
                      "%s", hipGetErrorString(e));
            break;
        }
        rc = n_values;
        const size_t g = (size_t)GUARD * 8;
        for (size_t i = 0; i < g; i++)
            if (back[i] != FILL || back[out_bytes - 1 - i] != FILL) {
                set_error("pmh_debug_orc_timestamp: a kernel wrote outside "
                          "its output (guard zone changed)");
                rc = -2;
                break;
            }
        memcpy(out, back.data() + g, (size_t)n_values * 8);
        if (rc >= 0 && (err_word >> OTS_ERR_SHIFT)) {
            set_error("pmh_debug_orc_timestamp: %s",
                      orc_timestamp_error(err_word).c_str());
            rc = -1;
        }
    } while (0);
    if (d_data) (void)hipFree(d_data);
    if (d_sec) (void)hipFree(d_sec);
    if (d_out) (void)hipFree(d_out);
    if (d_nanos) (void)hipFree(d_nanos);
    if (d_err) (void)hipFree(d_err);
    if (d_chunks) (void)hipFree(d_chunks);
    if (d_units) (void)hipFree(d_units);
    return rc;
}

int64_t pmh_debug_snappy(const void *src, int64_t n, void *dst, int64_t cap) {
    size_t got = 0;
    std::string err;
    if (!snappy_decompress((const uint8_t *)src, (size_t)n, (uint8_t *)dst,
                           (size_t)cap, got, err)) {
        set_error("%s", err.c_str());
        return -1;
    }
    return (int64_t)got;
}

int pmh_write_parquet(const pmh_col *cols, int32_t n_cols, int64_t n_rows,
                      const char *path, int64_t row_group_rows,
                      int64_t page_rows, const char *compression) {
    int codec = CODEC_UNCOMPRESSED;
    if (compression && *compression) {
        std::string cs(compression);
        if (cs == "zstd" || cs == "ZSTD") codec = CODEC_ZSTD;
        else if (cs != "NONE" && cs != "none" && cs != "UNCOMPRESSED") {
            set_error("write compression '%s' not supported (NONE | zstd)",
                      compression);
            return -1;
        }
    }
    if (!cols || n_cols <= 0 || !path) {
        set_error("pmh_write_parquet: bad arguments");
        return -1;
    }
    std::vector<PwCol> pc(n_cols);
    for (int32_t i = 0; i < n_cols; i++) {
        pc[i].name = cols[i].name ? cols[i].name : "";
        pc[i].dtype = cols[i].dtype;
        pc[i].data = cols[i].data;
        pc[i].valid = cols[i].valid;
        pc[i].dict_data = (const uint8_t *)cols[i].dict_data;
        pc[i].dict_offsets = cols[i].dict_offsets;
        pc[i].dict_len = cols[i].dict_len;
        pc[i].precision = cols[i].precision;
        pc[i].scale = cols[i].scale;
        pc[i].logical = cols[i].logical;
        if (pc[i].name.empty() || (!pc[i].data && n_rows > 0)) {
            set_error("pmh_write_parquet: column %d missing name/data", i);
            return -1;
        }
    }
    std::string err;
    if (!write_parquet(pc, n_rows, path, row_group_rows, page_rows, codec,
                       err)) {
        set_error("%s", err.c_str());
        return -1;
    }
    return 0;
}

char *pmh_debug_footer_json(const char *path) {
    StagedFile sf;
    if (!load_file(path, sf)) return nullptr;
    std::string out = "{\"num_rows\": " + std::to_string(sf.meta.num_rows) +
                      ", \"columns\": [";
    for (size_t i = 0; i < sf.meta.schema_names.size(); i++) {
        if (i) out += ",";
        out += "{\"name\": \"" + json_escape(sf.meta.schema_names[i]) +
               "\", \"max_def\": " + std::to_string(sf.meta.max_def_levels[i]) +
               ", \"phys\": " + std::to_string(sf.meta.phys_types[i]) +
               ", \"converted\": " +
               std::to_string(sf.meta.converted_types[i]) +
               ", \"logical\": " + std::to_string(sf.meta.logical_kinds[i]) +
               ", \"unit\": \"" + pq_unit_name(sf.meta.logical_units[i]) +
               "\", \"utc\": " + (sf.meta.logical_utc[i] ? "true" : "false") +
               "}";
    }
    out += "], \"row_groups\": [";
    for (size_t g = 0; g < sf.meta.row_groups.size(); g++) {
        auto &rg = sf.meta.row_groups[g];
        if (g) out += ",";
        out += "{\"num_rows\": " + std::to_string(rg.num_rows) + ", \"chunks\": [";
        for (size_t c = 0; c < rg.columns.size(); c++) {
            auto &cc = rg.columns[c];
            if (c) out += ",";
            int64_t n_data_pages = 0;
            for (auto &pg : cc.pages)
                if (pg.page_type == 0) n_data_pages++;
            out += "{\"name\": \"" + json_escape(cc.name) +
                   "\", \"num_values\": " + std::to_string(cc.num_values) +
                   ", \"codec\": " + std::to_string(cc.codec) +
                   ", \"data_page_offset\": " +
                   std::to_string(cc.data_page_offset) +
                   ", \"dict_page_offset\": " +
                   std::to_string(cc.dictionary_page_offset) +
                   ", \"n_data_pages\": " + std::to_string(n_data_pages) + "}";
        }
        out += "]}";
    }
    out += "]}";
    return strdup(out.c_str());
}

// The file-against-declared-type checks of staging, without a plan or a GPU:
// see paimon_hip.h. Calls the very functions staging calls.
int pmh_debug_check_column(const char *path, const char *column,
                           const char *type) {
    if (!path || !column || !type) {
        set_error("pmh_debug_check_column: bad arguments");
        return -1;
    }
    ColSpec cs;
    cs.name = column;
    cs.dtype = -1;
    int dp = 0, ds = 0;
    const std::string ts = type;
    if (parse_decimal(ts, &dp, &ds)) {
        cs.dtype = dp <= 9 ? PMH_DT_INT32 : PMH_DT_INT64;
        cs.precision = dp;
        cs.scale = ds;
    } else {
        const int bt = parse_bool_or_temporal(ts, cs);
        if (bt < 0) return -1;
        if (bt == 0) cs.dtype = dtype_from_str(ts);
    }
    if (cs.dtype < 0) {
        set_error("pmh_debug_check_column: unknown type '%s'", type);
        return -1;
    }
    StagedFile sf;
    if (!load_file(path, sf)) return -1;
    if (sf.orc) {
        const OrcFileMeta &om = sf.orc_meta;
        int cid = -1;
        for (size_t i = 0; i < om.column_names.size(); i++)
            if (om.column_names[i] == cs.name) cid = (int)i + 1;
        if (cid < 0) {
            set_error("%s: column %s not found", path, column);
            return -1;
        }
        for (const auto &st : om.stripes)
            if (!check_orc_declared(path, cs, om.column_kinds[cid - 1], st))
                return -1;
        return 0;
    }
    int leaf = -1;
    for (size_t i = 0; i < sf.meta.schema_names.size(); i++)
        if (sf.meta.schema_names[i] == cs.name) leaf = (int)i;
    if (leaf < 0) {
        set_error("%s: column %s not found", path, column);
        return -1;
    }
    if (!check_parquet_declared(path, cs, sf.meta, leaf)) return -1;
    if (cs.is_bool)
        for (const auto &rg : sf.meta.row_groups)
            for (const auto &pg : rg.columns[leaf].pages)
                if (!check_bool_page(path, cs, pg)) return -1;
    return 0;
}

// Host entry to the lookup search core (lookup_core.h) shared with
// k_lookup_probe: queries are walked in chunks of PLK_CHUNK like the
// kernel's workgroups — one window per level from the chunk's smallest and
// largest key, then a windowed bisection per query.
int pmh_debug_lookup_probe(int n_levels, const int64_t *const *level_keys,
                           const int64_t *level_rows, const int64_t *queries,
                           int64_t n_queries, int32_t *out_level,
                           int64_t *out_row) {
    if (n_levels < 0 || n_levels > PMH_MAX_RUNS || n_queries < 0 ||
        (n_levels > 0 && (!level_keys || !level_rows)) ||
        (n_queries > 0 && (!queries || !out_level || !out_row))) {
        set_error("pmh_debug_lookup_probe: bad arguments (0..%d levels)",
                  PMH_MAX_RUNS);
        return -1;
    }
    std::vector<PlkLevel> lv(n_levels);
    for (int l = 0; l < n_levels; l++) {
        if (level_rows[l] < 0 || (level_rows[l] > 0 && !level_keys[l])) {
            set_error("pmh_debug_lookup_probe: level %d is malformed", l);
            return -1;
        }
        lv[l] = PlkLevel{(uint64_t)(uintptr_t)level_keys[l], level_rows[l],
                         8, 0};
    }
    std::vector<int64_t> wlo(n_levels), whi(n_levels);
    for (int64_t base = 0; base < n_queries; base += PLK_CHUNK) {
        const int64_t cnt = std::min<int64_t>(PLK_CHUNK, n_queries - base);
        const auto mm =
            std::minmax_element(queries + base, queries + base + cnt);
        for (int l = 0; l < n_levels; l++)
            plk_window(lv[l], *mm.first, *mm.second, &wlo[l], &whi[l]);
        for (int64_t i = base; i < base + cnt; i++) {
            int64_t row = -1;
            int l = plk_probe(lv.data(), n_levels, wlo.data(), whi.data(),
                              queries[i], &row);
            out_level[i] = l;
            out_row[i] = l < 0 ? -1 : row;
        }
    }
    return 0;
}

int pmh_debug_changelog_decide(int64_t n_groups, const int32_t *nlive,
                               const int32_t *n_top,
                               const uint8_t *merged_is_add, int pending,
                               int32_t *out_n, int8_t *out_kinds,
                               uint8_t *out_after_is_merged,
                               uint8_t *out_pending) {
    if (n_groups < 0 ||
        (n_groups > 0 && (!nlive || !n_top || !merged_is_add || !out_n ||
                          !out_kinds))) {
        set_error("pmh_debug_changelog_decide: bad arguments");
        return -1;
    }
    for (int64_t g = 0; g < n_groups; g++) {
        if (nlive[g] < 1 || n_top[g] < 0 || n_top[g] > nlive[g]) {
            set_error("pmh_debug_changelog_decide: group %lld is malformed "
                      "(nlive >= 1, 0 <= n_top <= nlive)", (long long)g);
            return -1;
        }
        const ClcDecision d = clc_decide(nlive[g], n_top[g],
                                         merged_is_add[g] != 0, pending != 0);
        out_n[g] = d.n;
        out_kinds[2 * g] = (int8_t)(d.n >= 1 ? d.kind0 : -1);
        out_kinds[2 * g + 1] = (int8_t)(d.n == 2 ? d.kind1 : -1);
        if (out_after_is_merged) out_after_is_merged[g] = d.after_is_merged;
        if (out_pending) out_pending[g] = d.pending;
    }
    return 0;
}

int pmh_debug_last_emit_kernel(void) { return pmh_last_emit_kernel(); }
int pmh_debug_last_pu_emit_kernel(void) { return pmh_last_pu_emit_kernel(); }

// CPU-side entry to the partial-update aggregate fold (pu_agg_core.h): one
// key group through the code k_emit_pu_sga runs per output row.
int pmh_debug_pu_agg_fold(int n_members, const int8_t *kinds, int n_cols,
                          const uint8_t *dtypes, const int64_t *values,
                          const uint8_t *valid, int n_groups,
                          const uint8_t *col_group, const int16_t *sg_fields,
                          const uint8_t *sg_nseq, const uint8_t *col_agg,
                          int ignore_delete, int64_t *out_values,
                          uint8_t *out_valid, int32_t *out_kind,
                          int32_t *out_last, int32_t *out_unsupported) {
    if (!kinds || !dtypes || !values || !valid || !col_group || !col_agg ||
        (n_groups > 0 && (!sg_fields || !sg_nseq)) || !out_values ||
        !out_valid || !out_kind || !out_last || !out_unsupported) {
        set_error("pmh_debug_pu_agg_fold: null argument");
        return -1;
    }
    const char *what = pac_host_check(n_members, n_cols, n_groups, col_group,
                                      sg_fields, sg_nseq);
    if (what) {
        set_error("pmh_debug_pu_agg_fold: %s", what);
        return -1;
    }
    pac_host_fold(n_members, kinds, n_cols, dtypes, values, valid, n_groups,
                  col_group, sg_fields, sg_nseq, col_agg, ignore_delete != 0,
                  out_values, out_valid, out_kind, out_last, out_unsupported);
    return 0;
}

int pmh_debug_partition(int k, const void *const *keys, const int64_t *lens,
                        int key_width, int64_t tile_rows, int mode,
                        int32_t *cuts_out) {
    if (k < 1 || k > PMH_MAX_RUNS || !keys || !lens || !cuts_out ||
        (key_width != 4 && key_width != 8) || tile_rows < 1 ||
        (mode != 0 && mode != 1)) {
        set_error("pmh_debug_partition: bad arguments (1..%d runs, key_width "
                  "4|8, tile_rows >= 1, mode 0|1)", PMH_MAX_RUNS);
        return -1;
    }
    int64_t total = 0;
    for (int r = 0; r < k; r++) {
        if (lens[r] < 0 || lens[r] >= ((int64_t)1 << PMH_ROW_BITS) ||
            (lens[r] > 0 && !keys[r])) {
            set_error("pmh_debug_partition: run %d is malformed", r);
            return -1;
        }
        total += lens[r];
    }
    const int64_t n_bounds = (total + tile_rows - 1) / tile_rows + 1;
    if (mode == 0) {
        // the launcher's level rule (pmh_launch_partition)
        const int64_t G = k <= 8 ? (n_bounds > PMH_COARSE_G + 1 ? PMH_COARSE_G
                                                                 : 1)
                                 : (n_bounds > 1 ? n_bounds - 1 : 1);
        static_assert(PPC_MAX_RUNS == PMH_MAX_RUNS, "widest instantiation");
        ppc_host_partition(k, keys, lens, key_width, tile_rows, n_bounds,
                           total, G, cuts_out);
        return 0;
    }
    // device: the runs as staged columns, then exactly pmh_read_next's call
    constexpr int GUARD = 64;  // sentinel words behind the cuts
    const size_t n_cuts = (size_t)n_bounds * k;
    std::vector<void *> bufs;
    auto dalloc = [&](size_t n) -> void * {
        void *p = nullptr;
        if (hipMalloc(&p, n ? n : 8) != hipSuccess) return nullptr;
        bufs.push_back(p);
        return p;
    };
    int rc = -1;
    do {
        std::vector<DevCol> cols(k);
        bool ok = true;
        for (int r = 0; r < k && ok; r++) {
            DevCol c{0, 0, key_width, 0};
            if (lens[r] > 0) {  // an empty run keeps a null address
                const size_t nb = (size_t)lens[r] * key_width;
                void *d = dalloc(nb);
                ok = d && hipMemcpy(d, keys[r], nb, hipMemcpyHostToDevice) ==
                              hipSuccess;
                c.addr0 = (uint64_t)(uintptr_t)d;
            }
            cols[r] = c;
        }
        DevCol *d_cols = (DevCol *)dalloc(k * sizeof(DevCol));
        int64_t *d_lens = (int64_t *)dalloc(k * 8);
        int32_t *d_cuts = (int32_t *)dalloc((n_cuts + GUARD) * 4);
        if (!ok || !d_cols || !d_lens || !d_cuts ||
            hipMemcpy(d_cols, cols.data(), k * sizeof(DevCol),
                      hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_lens, lens, k * 8, hipMemcpyHostToDevice) !=
                hipSuccess ||
            hipMemset(d_cuts, 0x5a, (n_cuts + GUARD) * 4) != hipSuccess) {
            set_error("pmh_debug_partition: device staging failed");
            break;
        }
        hipError_t e = pmh_launch_partition(d_cols, d_lens, k, tile_rows,
                                            n_bounds, total, d_cuts, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) {
            set_error("pmh_debug_partition: partition kernels: %s",
                      hipGetErrorString(e));
            break;
        }
        std::vector<int32_t> host(n_cuts + GUARD);
        if (hipMemcpy(host.data(), d_cuts, host.size() * 4,
                      hipMemcpyDeviceToHost) != hipSuccess) {
            set_error("pmh_debug_partition: D2H failed");
            break;
        }
        bool clean = true;
        for (int i = 0; i < GUARD; i++)
            clean &= host[n_cuts + i] == 0x5a5a5a5a;
        if (!clean) {
            set_error("pmh_debug_partition: a kernel wrote outside its cuts");
            break;
        }
        memcpy(cuts_out, host.data(), n_cuts * 4);
        rc = 0;
    } while (false);
    for (void *p : bufs) (void)hipFree(p);
    return rc;
}

// The plan descriptor's number rule, exposed on its own: `text` goes through
// the same JsonParser and as_i64() that read minKey/maxKey and the integer
// filter literals.
int pmh_debug_json_i64(const char *text, int64_t *out) {
    if (!text || !out) {
        set_error("pmh_debug_json_i64: null argument");
        return -1;
    }
    try {
        Json j = JsonParser(text).parse();
        if (j.type != Json::NUM) {
            set_error("pmh_debug_json_i64: not a JSON number");
            return -1;
        }
        *out = j.as_i64();
    } catch (const std::exception &e) {
        set_error("pmh_debug_json_i64: %s", e.what());
        return -1;
    }
    return 0;
}

int pmh_debug_interval_partition(int n, const int64_t *min_keys,
                                 const int64_t *max_keys, int32_t *out_section,
                                 int32_t *out_run) {
    std::vector<FileDesc> files(n);
    for (int i = 0; i < n; i++) {
        files[i].min_key = min_keys[i];
        files[i].max_key = max_keys[i];
        files[i].input_index = i;
    }
    auto sections = interval_partition(files);
    for (size_t s = 0; s < sections.size(); s++)
        for (size_t r = 0; r < sections[s].size(); r++)
            for (const auto &fd : sections[s][r]) {
                out_section[fd.input_index] = (int32_t)s;
                out_run[fd.input_index] = (int32_t)r;
            }
    return (int)sections.size();
}

}  // extern "C"
