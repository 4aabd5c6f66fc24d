// Host walks over the encoded integer streams of both file formats, and the
// device work units they cut the streams into:
//  - Parquet hybrid RLE / bit-packed runs (parquet-format Encodings.md,
//    "Run Length Encoding / Bit-Packing Hybrid"): definition levels and
//    dictionary ids -> RleChunk;
//  - Parquet DELTA_BINARY_PACKED pages -> DeltaChunk / DeltaStream, and a
//    host decode of the same pages (DELTA_BYTE_ARRAY length streams);
//  - ORC RLEv2 (ORC v1 spec, "Integer Run Length Encoding, version 2") ->
//    Rlev2Chunk, and a host decode of the same runs (LENGTH streams);
//  - ORC byte-RLE -> Rlev2Chunk, and the PRESENT stream (boolean RLE) ->
//    RleChunk over bit-reversed level bytes.
// Host only, no HIP: every format has ONE header parse (a "step"), checked
// against the stream length before any byte is read, and the walkers are
// thin loops over it. A walker reports failure through *why, like
// prescan_bits_plain (bits_core.h); the caller names the file and column.
// stream_hostcheck.cpp runs all of it under ASan + UBSan.
#ifndef PMH_STREAM_CORE_H
#define PMH_STREAM_CORE_H

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace pmh {

// Host-prescanned RLE/bit-packed work unit (split at group boundaries).
struct RleChunk {
    uint64_t src;       // device pointer to first packed group (kind 1)
    int64_t out_start;  // output element index
    int32_t count;
    int32_t kind;       // 0 = RLE run, 1 = bit-packed groups
    uint32_t value;     // RLE literal (kind 0)
    int32_t bit_width;  // per-page bit width (dict-id streams vary per page)
    int64_t aux;        // def-level streams: dense (non-null) values before
                        // this chunk within its (run, column)
    // absolute device addresses (patched at staging finalize) so decode
    // chunks from every (run, column) batch into ONE launch:
    uint64_t out_addr;    // positioned column values
    uint64_t valid_addr;  // byte validity
    uint64_t dense_addr;  // dense (non-null) values
    int32_t esize;
    int32_t _pad2;
};

// Host-prescanned ORC RLEv2 / byte-RLE work unit (one run per chunk; runs
// are <= 512 values and byte-aligned). Restates the ORC v1 spec RLEv2 as
// consumed by the reference through orc-core 1.9.8.
struct Rlev2Chunk {
    uint64_t src;        // packed values (byte-aligned within DATA stream)
    int64_t out_start;   // dense output element index
    int32_t count;
    uint8_t kind;        // 0 SHORT_REPEAT, 1 DIRECT, 2 PATCHED_BASE,
                         // 3 DELTA, 4 BYTE_RUN, 5 BYTE_LITERAL
    uint8_t width;       // packed bit width (0 = fixed-delta / none)
    uint8_t is_signed;   // zigzag-decode DIRECT/SHORT_REPEAT values
    uint8_t out_esize;   // 4 or 8
    int64_t base;        // SR/BYTE_RUN: value; DELTA/PATCHED: base
    int64_t delta;       // DELTA: delta base (sign = direction)
    uint64_t patch_src;  // PATCHED: packed patch entries
    uint16_t patch_pl;   // PATCHED: number of patch entries
    uint8_t patch_pw;    // PATCHED: patch value bits (decoded)
    uint8_t patch_pgw;   // PATCHED: gap bits
    uint8_t patch_cfb;   // PATCHED: packed entry bits
    uint8_t dense_target;  // 0: contig (positioned); 1: dense buffer
                           // (PRESENT scatter follows); 2: the (run,
                           // column)'s int32 decimal-scale scratch
                           // (out_start = scratch index); 3: its uint64
                           // timestamp-nanos scratch (likewise)
    uint8_t _pad[2];
    uint64_t out_addr;     // absolute output base (patched at finalize)
};

// Host-prescanned DELTA_BINARY_PACKED work unit: one parquet delta BLOCK
// (VectorizedDeltaBinaryPackedReader.java; parquet-format encodings.md):
// per block, <= 8 miniblocks of vpm values each, bit widths packed into
// `widths` (8 bits each), LSB-first bit packing. Blocks chain: the value
// base entering block b = page first_value + sum of all prior blocks'
// delta sums — computed on device (k_delta_sum + per-stream scan).
struct DeltaChunk {
    uint64_t src;       // packed miniblock data (byte-aligned)
    uint64_t out_addr;  // absolute output base (patched at finalize)
    int64_t out_start;  // output index of this block's FIRST delta value
    int64_t min_delta;
    int32_t count;      // real delta values in this block
    int32_t stream;     // delta-stream index (for base resolution)
    uint64_t widths;    // miniblock bit widths, 8 bits each
    int16_t vpm;        // values per miniblock
    int16_t n_mini;
    int32_t out_esize;  // 4 or 8
};

// One DELTA stream (= one PAGE: pages are self-contained): chunk range + the
// page's first value and where it lands in the output.
struct DeltaStream {
    int64_t chunk_lo;
    int64_t chunk_hi;
    int64_t first;       // header first value = output element out0
    int64_t out0;        // output index of the first value
    uint64_t out_addr;   // absolute output base (patched at finalize)
    int32_t out_esize;
    int32_t _pad;
};

// ------------------------------------------------------------- varints

// ULEB128 at s[*p]: at most 10 bytes and 64 bits, none of them past len.
inline bool uleb64(const uint8_t *s, int64_t len, int64_t *p, uint64_t *v) {
    uint64_t r = 0;
    for (int i = 0; i < 10; i++) {
        if (*p >= len) return false;
        const uint8_t b = s[(*p)++];
        if (i == 9 && b > 1) return false;  // bit 64 and up, or an 11th byte
        r |= (uint64_t)(b & 0x7F) << (7 * i);
        if (!(b & 0x80)) {
            *v = r;
            return true;
        }
    }
    return false;
}

inline int64_t unzigzag(uint64_t v) {
    return (int64_t)(v >> 1) ^ -(int64_t)(v & 1);
}

// ------------------------------------- Parquet hybrid RLE / bit-packed

struct HybridRun {
    bool packed;     // false: `count` copies of `value`; true: bit-packed
    int64_t count;   // values of the run, clipped to the values still wanted
    uint32_t value;  // RLE run value
    int64_t off;     // bit-packed: stream offset of the first group
    int64_t nbytes;  // bit-packed: bytes the `count` values occupy
};

// One run at s[*p], `left` values still wanted. The header, the run value
// and the bytes of the `count` values are all inside len; *p moves past the
// whole run (a last bit-packed run that its writer cut short of whole
// groups, which parquet-mr tolerates, ends the stream).
inline bool hybrid_step(const uint8_t *s, int64_t len, int bit_width,
                        int64_t left, int64_t *p, HybridRun *r,
                        const char **why) {
    if (bit_width < 0 || bit_width > 32) {
        *why = "RLE bit width above 32";
        return false;
    }
    uint64_t header;
    if (!uleb64(s, len, p, &header)) {
        *why = "RLE run header truncated";
        return false;
    }
    const int64_t n = (int64_t)(header >> 1);
    r->packed = header & 1;
    r->value = 0;
    r->off = *p;
    r->nbytes = 0;
    if (!r->packed) {
        const int byte_width = (bit_width + 7) / 8;
        if (byte_width > len - *p) {
            *why = "RLE run value truncated";
            return false;
        }
        for (int i = 0; i < byte_width; i++)
            r->value |= (uint32_t)s[*p + i] << (8 * i);
        *p += byte_width;
        r->count = std::min(n, left);
        return true;
    }
    r->count = n >= (left + 7) / 8 ? left : n * 8;
    r->nbytes = (r->count * bit_width + 7) / 8;
    const int64_t room = len - *p;
    if (r->nbytes > room) {
        *why = "RLE bit-packed groups truncated";
        return false;
    }
    *p += bit_width && n > room / bit_width ? room : n * bit_width;
    return true;
}

// Walk a def-level stream (bit width 1): emit device work chunks with
// running dense offsets (aux) and report the number of non-null values.
// src offsets are RELATIVE to the (run,col) levels buffer (rel_base =
// offset of this stream within it); patched to device addresses at upload.
inline bool prescan_def(const uint8_t *s, int64_t len, int64_t n,
                        int64_t out_row0, int64_t rel_base,
                        int64_t *dense_before, std::vector<RleChunk> &out,
                        const char **why) {
    // one wave per chunk in k_level_scatter: chunk size bounds the serial
    // 64-value passes per wave
    const int64_t MAX_CHUNK = 512;
    int64_t p = 0, cnt = 0;
    HybridRun r;
    while (cnt < n) {
        if (p >= len) {
            *why = "def-level stream overrun";
            return false;
        }
        if (!hybrid_step(s, len, 1, n - cnt, &p, &r, why)) return false;
        const uint32_t v = r.value & 1;
        for (int64_t off = 0; off < r.count; off += MAX_CHUNK) {
            const int64_t take = std::min(MAX_CHUNK, r.count - off);
            RleChunk c{};
            c.kind = r.packed;
            c.value = v;
            if (r.packed) c.src = (uint64_t)(rel_base + r.off + off / 8);
            c.out_start = out_row0 + cnt + off;
            c.count = (int32_t)take;
            c.bit_width = 1;
            c.aux = *dense_before + (!r.packed && v ? off : 0);
            out.push_back(c);
            // advance the dense count by the set bits of a packed chunk
            for (int64_t i = 0; r.packed && i < take; i += 8) {
                const int64_t rem = take - i;
                const uint8_t mask =
                    rem >= 8 ? 0xFF : (uint8_t)((1u << rem) - 1);
                *dense_before +=
                    __builtin_popcount(s[r.off + (off + i) / 8] & mask);
            }
        }
        if (!r.packed && v) *dense_before += r.count;
        cnt += r.count;
    }
    return true;
}

// Walk a def-level stream (bit width 1) and report whether any zero (null)
// occurs among the first n values. A malformed stream answers true.
inline bool def_levels_have_nulls(const uint8_t *s, int64_t len, int64_t n) {
    int64_t p = 0, cnt = 0;
    HybridRun r;
    const char *why;
    while (cnt < n) {
        if (!hybrid_step(s, len, 1, n - cnt, &p, &r, &why)) return true;
        if (!r.packed && r.value == 0 && r.count > 0) return true;
        for (int64_t i = 0; r.packed && i < r.count; i += 8) {
            const int64_t rem = r.count - i;
            const uint8_t mask = rem >= 8 ? 0xFF : (uint8_t)((1u << rem) - 1);
            if ((s[r.off + i / 8] & mask) != mask) return true;
        }
        cnt += r.count;
    }
    return false;
}

// Prescan an RLE stream into device work chunks (splitting long runs).
inline bool prescan_rle(const uint8_t *s, int64_t len, int bit_width,
                        int64_t n, int64_t out_base, uint64_t dev_base,
                        int64_t host_off, std::vector<RleChunk> &out,
                        const char **why) {
    const int64_t MAX_CHUNK = 16384;
    int64_t p = 0, cnt = 0;
    HybridRun r;
    while (cnt < n) {
        if (p >= len) {
            *why = "RLE stream overrun";
            return false;
        }
        if (!hybrid_step(s, len, bit_width, n - cnt, &p, &r, why))
            return false;
        // packed runs split at group boundaries
        for (int64_t off = 0; off < r.count; off += MAX_CHUNK) {
            RleChunk c{};
            c.kind = r.packed;
            c.value = r.value;
            if (r.packed)
                c.src = dev_base + (uint64_t)(host_off + r.off) +
                        (uint64_t)((off / 8) * bit_width);
            c.out_start = out_base + cnt + off;
            c.count = (int32_t)std::min(MAX_CHUNK, r.count - off);
            c.bit_width = bit_width;
            out.push_back(c);
        }
        cnt += r.count;
    }
    return true;
}

// ------------------------------------------ Parquet DELTA_BINARY_PACKED
// (parquet-format Encodings.md; VectorizedDeltaBinaryPackedReader.java):
// page header <block_size><miniblocks_per_block><total_count><first zigzag>,
// then blocks of [min_delta zigzag][miniblock widths][packed miniblocks].

struct DeltaHeader {
    int64_t block_size, n_mini, total;
    int64_t first;
};

inline bool delta_header(const uint8_t *s, int64_t len, int64_t *p,
                         DeltaHeader *h, const char **why) {
    uint64_t bs, mpb, total, zfirst;
    if (!uleb64(s, len, p, &bs) || !uleb64(s, len, p, &mpb) ||
        !uleb64(s, len, p, &total) || !uleb64(s, len, p, &zfirst)) {
        *why = "delta: truncated header";
        return false;
    }
    if (mpb == 0 || bs % mpb != 0) {
        *why = "delta: unsupported miniblock layout (v1: <= 8 per block)";
        return false;
    }
    if (bs > INT32_MAX || total > INT32_MAX) {
        *why = "delta: block size or value count above 2^31";
        return false;
    }
    h->block_size = (int64_t)bs;
    h->n_mini = (int64_t)mpb;
    h->total = (int64_t)total;
    h->first = unzigzag(zfirst);
    return true;
}

// A block's min_delta and its n_mini width bytes; *p moves to the first
// miniblock.
inline bool delta_block(const uint8_t *s, int64_t len, int64_t n_mini,
                        int64_t *p, int64_t *min_delta,
                        const uint8_t **widths, const char **why) {
    uint64_t zmd;
    if (!uleb64(s, len, p, &zmd) || n_mini > len - *p) {
        *why = "delta: truncated block";
        return false;
    }
    *min_delta = unzigzag(zmd);
    *widths = s + *p;
    *p += n_mini;
    return true;
}

// Host decode of one complete stream (the GPU path decodes these on device;
// this serves DELTA_BYTE_ARRAY string staging, where values intern into the
// global dictionary anyway). Values wrap in 64 bits, as the format says.
// Returns bytes consumed or -1.
inline int64_t host_delta_i64(const uint8_t *s, int64_t len,
                              std::vector<int64_t> &out, const char **why) {
    int64_t pos = 0;
    DeltaHeader h;
    if (!delta_header(s, len, &pos, &h, why)) return -1;
    const int64_t vpm = h.block_size / h.n_mini;
    out.clear();
    out.reserve((size_t)std::min(h.total, len * 8 + 1));
    if (h.total == 0) return pos;
    uint64_t cur = (uint64_t)h.first;
    out.push_back((int64_t)cur);
    int64_t remaining = h.total - 1;
    while (remaining > 0) {
        int64_t mind;
        const uint8_t *widths;
        if (!delta_block(s, len, h.n_mini, &pos, &mind, &widths, why))
            return -1;
        for (int64_t m = 0; m < h.n_mini && remaining > 0; m++) {
            const int w = widths[m];
            if (w > 64) {
                *why = "delta: miniblock width > 64";
                return -1;
            }
            const int64_t take = std::min(remaining, vpm);
            const int64_t nbytes = (vpm * w + 7) / 8;  // stored in full
            if (nbytes > len - pos) {
                *why = "delta: truncated miniblocks";
                return -1;
            }
            for (int64_t j = 0; j < take; j++) {
                uint64_t d = 0;  // LSB-first bit-packed
                for (int b = 0; b < w; b++) {
                    const int64_t bit = j * w + b;
                    d |= (uint64_t)((s[pos + (bit >> 3)] >> (bit & 7)) & 1)
                         << b;
                }
                cur += (uint64_t)mind + d;
                out.push_back((int64_t)cur);
            }
            pos += nbytes;
            remaining -= take;
        }
    }
    return pos;
}

// Prescan one page. Each PAGE is self-contained (its own first value), so it
// forms one DeltaStream; each block becomes one DeltaChunk. Miniblocks
// holding no real values carry a width byte but no data (their widths zero
// out in the packed u64 so device byte offsets skip nothing); partially-
// filled miniblocks are stored in full. The kernel handles <= 8 miniblocks
// per block, and the page's value count has to be the header's.
inline bool prescan_delta(const uint8_t *s, int64_t len, int64_t n_values,
                          int64_t out_row0, uint64_t dev_base,
                          int64_t rel_off, uint64_t out_addr, int out_esize,
                          std::vector<DeltaChunk> &chunks,
                          std::vector<DeltaStream> &streams,
                          const char **why) {
    int64_t pos = 0;
    DeltaHeader h;
    if (!delta_header(s, len, &pos, &h, why)) return false;
    if (h.n_mini > 8) {
        *why = "delta: unsupported miniblock layout (v1: <= 8 per block)";
        return false;
    }
    if (h.total != n_values) {
        *why = "delta: header count disagrees with page";
        return false;
    }
    const int64_t vpm = h.block_size / h.n_mini;
    if (n_values == 0) return true;
    DeltaStream st{};
    st.chunk_lo = (int64_t)chunks.size();
    st.first = h.first;
    st.out0 = out_row0;
    st.out_addr = out_addr;
    st.out_esize = out_esize;
    int64_t remaining = n_values - 1;
    int64_t out_i = out_row0 + 1;
    while (remaining > 0) {
        DeltaChunk ch{};
        const uint8_t *widths;
        if (!delta_block(s, len, h.n_mini, &pos, &ch.min_delta, &widths, why))
            return false;
        ch.vpm = (int16_t)vpm;
        ch.n_mini = (int16_t)h.n_mini;
        ch.out_addr = out_addr;
        ch.out_start = out_i;
        ch.out_esize = out_esize;
        ch.count = (int32_t)std::min(remaining, h.block_size);
        int64_t data = 0;
        for (int64_t j = 0; j < h.n_mini; j++) {
            const int w = widths[j];
            if (w > 64) {
                *why = "delta: miniblock width > 64";
                return false;
            }
            if (remaining - j * vpm > 0) {
                ch.widths |= (uint64_t)w << (8 * j);
                data += vpm * w / 8;
            }
        }
        ch.src = dev_base + (uint64_t)(rel_off + pos);
        if (data > len - pos) {
            *why = "delta: truncated miniblocks";
            return false;
        }
        pos += data;
        chunks.push_back(ch);
        out_i += ch.count;
        remaining -= ch.count;
    }
    st.chunk_hi = (int64_t)chunks.size();
    streams.push_back(st);
    return true;
}

// ------------------------------------------------------------ ORC RLEv2

// The spec's 5-bit width code -> bit width table ("fixed bit sizes").
static const int RLEV2_FBS[32] = {1,  2,  3,  4,  5,  6,  7,  8,
                                  9,  10, 11, 12, 13, 14, 15, 16,
                                  17, 18, 19, 20, 21, 22, 23, 24,
                                  26, 28, 30, 32, 40, 48, 56, 64};

inline int rlev2_width(int enc) { return RLEV2_FBS[enc & 31]; }

// Smallest encodable width >= n: PATCHED_BASE packs each (gap, patch) entry
// at closest_fixed_bits(pgw + pw) bits.
inline int rlev2_closest_fixed_bits(int n) {
    for (int i = 0; i < 32; i++)
        if (RLEV2_FBS[i] >= n) return RLEV2_FBS[i];
    return 64;
}

// One run header. The packed payloads are MSB-first and byte-aligned.
struct Rlev2Run {
    int kind;       // 0 SHORT_REPEAT, 1 DIRECT, 2 PATCHED_BASE, 3 DELTA
    int width;      // packed bit width (0: SHORT_REPEAT, fixed-delta DELTA)
    int count;      // values of the run
    int64_t base;   // SHORT_REPEAT: the value; PATCHED_BASE / DELTA: the base
    int64_t delta;  // DELTA: first delta (its sign is the run's direction)
    int patch_pl, patch_pw, patch_pgw, patch_cfb;  // PATCHED_BASE
    int64_t off, nbytes;              // packed values / DELTA's later deltas
    int64_t patch_off, patch_nbytes;  // PATCHED_BASE: packed patch entries
};

// Parse the run at s[*p]; header, payload and patch list all lie inside len
// and *p moves past them. is_signed: SHORT_REPEAT values and the DELTA base
// are zigzag (DIRECT values too: the consumer's business).
inline bool rlev2_run(const uint8_t *s, int64_t len, bool is_signed,
                      int64_t *p, Rlev2Run *r, const char **why) {
    if (*p >= len) {
        *why = "RLEv2 stream overrun";
        return false;
    }
    auto need = [&](int64_t nbytes) {
        if (nbytes <= len - *p) return true;
        *why = "RLEv2 run header truncated";
        return false;
    };
    const uint8_t first = s[(*p)++];
    *r = Rlev2Run{};
    r->kind = first >> 6;
    if (r->kind == 0) {
        const int w = ((first >> 3) & 7) + 1;
        if (!need(w)) return false;
        uint64_t raw = 0;
        for (int i = 0; i < w; i++) raw = (raw << 8) | s[(*p)++];
        r->count = (first & 7) + 3;
        r->base = is_signed ? unzigzag(raw) : (int64_t)raw;
        r->off = *p;
        return true;
    }
    if (!need(1)) return false;
    const int wcode = (first >> 1) & 31;
    r->width = r->kind == 3 && wcode == 0 ? 0 : rlev2_width(wcode);
    r->count = (((int)(first & 1) << 8) | s[(*p)++]) + 1;
    r->nbytes = ((int64_t)r->count * r->width + 7) / 8;
    if (r->kind == 2) {
        if (!need(2)) return false;
        const uint8_t third = s[(*p)++], fourth = s[(*p)++];
        const int bw = ((third >> 5) & 7) + 1;
        r->patch_pw = rlev2_width(third & 31);
        r->patch_pgw = ((fourth >> 5) & 7) + 1;
        r->patch_pl = fourth & 31;
        if (!need(bw)) return false;
        if (r->patch_pw + r->patch_pgw > 64) {
            *why = "RLEv2 patch entry wider than 64 bits";
            return false;
        }
        uint64_t braw = 0;
        for (int i = 0; i < bw; i++) braw = (braw << 8) | s[(*p)++];
        const uint64_t smask = 1ull << (bw * 8 - 1);  // sign-magnitude
        r->base = (braw & smask) ? -(int64_t)(braw & ~smask) : (int64_t)braw;
        r->patch_cfb = rlev2_closest_fixed_bits(r->patch_pw + r->patch_pgw);
        r->patch_nbytes = ((int64_t)r->patch_pl * r->patch_cfb + 7) / 8;
    } else if (r->kind == 3) {
        uint64_t braw, draw;
        if (!uleb64(s, len, p, &braw) || !uleb64(s, len, p, &draw)) {
            *why = "RLEv2 delta varint overrun";
            return false;
        }
        r->base = is_signed ? unzigzag(braw) : (int64_t)braw;
        r->delta = unzigzag(draw);
        // the first two values come from base and delta alone
        r->nbytes = r->count > 2
                        ? ((int64_t)(r->count - 2) * r->width + 7) / 8
                        : 0;
    }
    r->off = *p;
    r->patch_off = r->off + r->nbytes;
    if (r->nbytes + r->patch_nbytes > len - *p) {
        *why = "RLEv2 stream overran its length";
        return false;
    }
    *p += r->nbytes + r->patch_nbytes;
    return true;
}

// Host RLEv2 decode: the ORC LENGTH / side streams that staging needs on the
// host (string id-ification), same arithmetic as k_rlev2
// (orc/impl/RunLengthIntegerReaderV2.java is the reference consumer).
// is_signed streams come back as the int64 bit patterns. n < 0: decode until
// the stream is exhausted (dictionary LENGTH streams: the entry count comes
// from the stream itself).
inline bool host_rlev2(const uint8_t *s, int64_t len, int64_t n,
                       bool is_signed, std::vector<uint64_t> &out,
                       const char **why) {
    auto bits_be = [&](int64_t q, int64_t bitpos, int w) -> uint64_t {
        uint64_t v = 0;
        for (int i = 0; i < w; i++) {
            const int64_t b = bitpos + i;
            v = (v << 1) | ((s[q + (b >> 3)] >> (7 - (b & 7))) & 1);
        }
        return v;
    };
    out.clear();
    if (n > 0) out.reserve((size_t)std::min(n, len * 512));
    int64_t p = 0;
    Rlev2Run r;
    std::vector<uint64_t> vals;
    while (n < 0 ? p < len : (int64_t)out.size() < n) {
        if (!rlev2_run(s, len, is_signed, &p, &r, why)) return false;
        const int w = r.width;
        if (r.kind == 0) {
            out.insert(out.end(), (size_t)r.count, (uint64_t)r.base);
        } else if (r.kind == 1) {
            for (int i = 0; i < r.count; i++) {
                const uint64_t v = bits_be(r.off, (int64_t)i * w, w);
                out.push_back(is_signed ? (uint64_t)unzigzag(v) : v);
            }
        } else if (r.kind == 2) {
            vals.resize((size_t)r.count);
            for (int i = 0; i < r.count; i++)
                vals[i] = bits_be(r.off, (int64_t)i * w, w);
            const int pw = r.patch_pw;  // <= 63: pw + pgw <= 64, pgw >= 1
            int64_t gap = 0;
            for (int i = 0; i < r.patch_pl; i++) {
                const uint64_t e = bits_be(
                    r.patch_off, (int64_t)i * r.patch_cfb, r.patch_cfb);
                const uint64_t patch = e & ((1ull << pw) - 1);
                gap += (int64_t)(e >> pw);
                if (gap >= r.count) {
                    *why = "RLEv2 patch position past the run";
                    return false;
                }
                if (w < 64) vals[gap] |= patch << w;
            }
            for (int i = 0; i < r.count; i++)
                out.push_back((uint64_t)r.base + vals[i]);
        } else {
            uint64_t cur = (uint64_t)r.base;
            out.push_back(cur);
            for (int i = 1; i < r.count; i++) {
                uint64_t d = (uint64_t)r.delta;
                if (i >= 2 && w > 0) {
                    d = bits_be(r.off, (int64_t)(i - 2) * w, w);
                    if (r.delta < 0) d = 0 - d;
                }
                cur += d;
                out.push_back(cur);
            }
        }
    }
    return true;
}

// Walk an RLEv2 stream and emit one device work chunk per run. dev_base =
// device address of the uploaded stream bytes; dense0 = dense output offset
// of this stream's first value.
inline bool prescan_rlev2(const uint8_t *s, int64_t len, int64_t n_values,
                          int is_signed, int out_esize, int dense_target,
                          uint64_t dev_base, int64_t dense0,
                          std::vector<Rlev2Chunk> &out, const char **why) {
    int64_t p = 0, cnt = 0;
    Rlev2Run r;
    while (cnt < n_values) {
        if (!rlev2_run(s, len, is_signed != 0, &p, &r, why)) return false;
        Rlev2Chunk c{};
        c.is_signed = (uint8_t)is_signed;
        c.out_esize = (uint8_t)out_esize;
        c.dense_target = (uint8_t)dense_target;
        c.out_start = dense0 + cnt;
        c.kind = (uint8_t)r.kind;
        c.width = (uint8_t)r.width;
        c.count = r.count;
        c.base = r.base;
        c.delta = r.delta;
        if (r.kind != 0) c.src = dev_base + (uint64_t)r.off;
        if (r.kind == 2) {
            c.patch_src = dev_base + (uint64_t)r.patch_off;
            c.patch_pl = (uint16_t)r.patch_pl;
            c.patch_pw = (uint8_t)r.patch_pw;
            c.patch_pgw = (uint8_t)r.patch_pgw;
            c.patch_cfb = (uint8_t)r.patch_cfb;
        }
        cnt += r.count;
        out.push_back(c);
    }
    return true;
}

// ------------------------------------------------- ORC byte-RLE, PRESENT

struct ByteRun {
    bool run;       // true: n copies of `value`; false: n literal bytes
    int n;          // 3..130 (run), 1..128 (literal)
    uint8_t value;  // run byte
    int64_t off;    // literal: stream offset of the first byte
};

// One header at s[*p] (h >= 0: h + 3 copies of the next byte; h < 0: -h
// literal bytes), `left` bytes still wanted: the run byte, or the wanted
// ones of the literal bytes, are inside len; *p moves past the whole run.
inline bool byterle_step(const uint8_t *s, int64_t len, int64_t left,
                         int64_t *p, ByteRun *r, const char **why) {
    if (*p >= len) {
        *why = "byte-RLE stream overrun";
        return false;
    }
    const int8_t h = (int8_t)s[(*p)++];
    r->run = h >= 0;
    r->value = 0;
    r->off = *p;
    if (r->run) {
        if (*p >= len) {
            *why = "byte-RLE run truncated";
            return false;
        }
        r->n = h + 3;
        r->value = s[(*p)++];
        return true;
    }
    r->n = -(int)h;
    if (std::min<int64_t>(r->n, left) > len - *p) {
        *why = "byte-RLE literal truncated";
        return false;
    }
    *p += r->n;
    return true;
}

// ORC byte-RLE (tinyint columns, e.g. _VALUE_KIND): one chunk per run or
// literal group, the last one cut at n_values.
inline bool prescan_byterle(const uint8_t *s, int64_t len, int64_t n_values,
                            int out_esize, int dense_target,
                            uint64_t dev_base, int64_t dense0,
                            std::vector<Rlev2Chunk> &out, const char **why) {
    int64_t p = 0, cnt = 0;
    ByteRun r;
    while (cnt < n_values) {
        if (!byterle_step(s, len, n_values - cnt, &p, &r, why)) return false;
        Rlev2Chunk c{};
        c.out_esize = (uint8_t)out_esize;
        c.dense_target = (uint8_t)dense_target;
        c.out_start = dense0 + cnt;
        c.kind = r.run ? 4 : 5;
        if (r.run) c.base = (int8_t)r.value;
        else c.src = dev_base + (uint64_t)r.off;
        c.count = (int32_t)std::min<int64_t>(r.n, n_values - cnt);
        cnt += c.count;
        out.push_back(c);
    }
    return true;
}

static const uint8_t BITREV[256] = {
#define R2(n) n, n + 2 * 64, n + 1 * 64, n + 3 * 64
#define R4(n) R2(n), R2(n + 2 * 16), R2(n + 1 * 16), R2(n + 3 * 16)
#define R6(n) R4(n), R4(n + 2 * 4), R4(n + 1 * 4), R4(n + 3 * 4)
    R6(0), R6(2), R6(1), R6(3)
#undef R2
#undef R4
#undef R6
};

// ORC PRESENT stream (boolean RLE = byte-RLE over MSB-first bit-packed
// bytes) -> the parquet-style def-level RleChunks consumed by
// k_level_scatter (which reads LSB-first: bytes are bit-reversed into the
// (run,col) levels buffer `levels`, every byte of a literal group). Tracks
// the dense (non-null) cursor. Runs of 0x00 / 0xFF need no level bytes.
inline bool prescan_present(const uint8_t *s, int64_t len, int64_t n_rows,
                            int64_t out_row0, std::vector<uint8_t> &levels,
                            std::vector<RleChunk> &out, int64_t *dense_before,
                            const char **why) {
    int64_t p = 0, cnt = 0;
    ByteRun r;
    while (cnt < n_rows) {
        if (p >= len) {
            *why = "PRESENT stream overrun";
            return false;
        }
        if (!byterle_step(s, len, 128, &p, &r, why)) return false;
        const int64_t vals = std::min<int64_t>((int64_t)r.n * 8, n_rows - cnt);
        const bool constant = r.run && (r.value == 0x00 || r.value == 0xFF);
        RleChunk c{};
        c.kind = constant ? 0 : 1;
        c.value = constant && r.value ? 1 : 0;
        c.out_start = out_row0 + cnt;
        c.count = (int32_t)vals;
        c.bit_width = 1;
        c.aux = *dense_before;
        if (constant) {
            if (r.value) *dense_before += vals;
        } else {
            c.src = (uint64_t)levels.size();
            for (int i = 0; i < r.n; i++)
                levels.push_back(BITREV[r.run ? r.value : s[r.off + i]]);
            const uint8_t *lv = levels.data() + c.src;
            for (int64_t i = 0; i < vals; i++)
                *dense_before += (lv[i >> 3] >> (i & 7)) & 1;
        }
        out.push_back(c);
        cnt += vals;
    }
    return true;
}

}  // namespace pmh

#endif  // PMH_STREAM_CORE_H
