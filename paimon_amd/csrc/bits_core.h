// Bit-packed BOOLEAN value decode, one core for both file formats:
//  - Parquet PLAIN booleans (parquet-format encodings.md, "Plain: BOOLEAN"):
//    1 bit per value, LSB first, every data page restarting on a byte
//    boundary;
//  - ORC boolean columns (ORC v1 spec, "Boolean Run Length Encoding"): a
//    byte-RLE stream whose bytes hold 8 values each, MSB first, the last
//    byte of a stripe padded.
// A work unit is either literal source bytes or one repeated byte; its
// values land as 0/1 elements (1 or 4 bytes wide) from out_start on.
//
// Shared scalar core, like orc_decimal_core.h: k_bits_expand (kernels.hip)
// and the host mode of pmh_debug_bits (plan.cpp) run exactly bits_norm /
// bits_group / bits_spread over the same group geometry, so the CPU tests
// pin the arithmetic the kernel executes. The prescans (host only) are the
// staging walks that cut a page or a stream into units.
//
// Group geometry: the output is handled in groups of 8 elements aligned to
// 8 elements in ABSOLUTE address terms (8 bytes at width 1, 32 bytes at
// width 4), because a unit's first element sits anywhere: pages and stripes
// end at any row and dense counts under nulls are arbitrary. With r = the
// first element's index modulo 8, group g of a unit covers the unit's
// values 8g - r .. 8g - r + 7: the top r bits of source byte g-1 and the low
// 8 - r bits of source byte g. A group wholly inside the unit is written
// with wide stores, the (at most two) edge groups element by element.
#ifndef PMH_BITS_CORE_H
#define PMH_BITS_CORE_H

#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define BITS_HD __host__ __device__ inline
#else
#define BITS_HD inline
#endif

enum { BITS_LITERAL = 0, BITS_RUN = 1 };  // BitsUnit.kind
enum { BITS_LSB = 0, BITS_MSB = 1 };      // BitsUnit.msb (bit order)

// bytes per unit the Parquet prescan cuts a page into (ORC units follow the
// byte-RLE headers: <= 130 bytes per run, <= 128 per literal group)
constexpr int BITS_PLAIN_UNIT_BYTES = 256;

// One work unit of k_bits_expand.
struct BitsUnit {
    uint64_t src;        // BITS_LITERAL: device address of the first byte
    uint64_t out_addr;   // absolute output base (patched at finalize)
    int64_t out_start;   // output element index of the unit's first value
    int32_t count;       // values in the unit (>= 1)
    uint8_t kind;        // BITS_LITERAL | BITS_RUN
    uint8_t msb;         // BITS_LSB | BITS_MSB
    uint8_t value;       // BITS_RUN: the repeated byte
    uint8_t out_esize;   // 1 or 4
    uint8_t dense_target;  // 0: contig (positioned); 1: dense buffer
    uint8_t _pad[7];
};

// A source byte in LSB-first value order (bit k = the byte's k-th value).
BITS_HD uint32_t bits_norm(uint32_t b, int msb) {
    if (msb) {
        b = ((b & 0xF0u) >> 4) | ((b & 0x0Fu) << 4);
        b = ((b & 0xCCu) >> 2) | ((b & 0x33u) << 2);
        b = ((b & 0xAAu) >> 1) | ((b & 0x55u) << 1);
    }
    return b & 0xFFu;
}

// The 8 values of one output group: prev/cur = normalised source bytes g-1
// and g (0 where the unit has none), r = 0..7 as above.
BITS_HD uint32_t bits_group(uint32_t prev, uint32_t cur, int r) {
    return ((prev | (cur << 8)) >> (8 - r)) & 0xFFu;
}

// 8 bits -> 8 bytes of 0/1, bit k in byte k (little-endian: element k).
BITS_HD uint64_t bits_spread(uint32_t bits) {
    const uint64_t x =
        ((uint64_t)bits * 0x0101010101010101ull) & 0x8040201008040201ull;
    return ((x + 0x7F7F7F7F7F7F7F7Full) >> 7) & 0x0101010101010101ull;
}

// r of a unit: absolute element index of its first value, modulo 8
BITS_HD int bits_unit_r(uint64_t out_addr, int64_t out_start, int out_esize) {
    const uint64_t e0 = (out_esize == 4 ? out_addr >> 2 : out_addr);
    return (int)((e0 + (uint64_t)out_start) & 7);
}

BITS_HD int bits_unit_groups(int r, int count) { return (r + count + 7) >> 3; }

// The value bits of group g of a unit. `src` = the unit's literal bytes
// (unused for a run). Reads source bytes g-1 and g only where the unit owns
// them.
BITS_HD uint32_t bits_unit_group(const BitsUnit &u, const uint8_t *src, int r,
                                 int g) {
    uint32_t prev = 0, cur = 0;
    if (u.kind == BITS_RUN) {
        prev = cur = bits_norm(u.value, u.msb);
    } else {
        const int nbytes = (u.count + 7) >> 3;
        if (r && g >= 1) prev = bits_norm(src[g - 1], u.msb);
        if (g < nbytes) cur = bits_norm(src[g], u.msb);
    }
    return bits_group(prev, cur, r);
}

// ---- host side (staging walks + host twin of the kernel's group loop)

// Parquet PLAIN boolean page payload: n_values bits from s on, cut every
// BITS_PLAIN_UNIT_BYTES bytes. Fails when the payload is shorter than the
// values need.
inline bool prescan_bits_plain(const uint8_t *s, int64_t len, int64_t n_values,
                               int out_esize, int dense_target,
                               uint64_t dev_base, int64_t out0,
                               std::vector<BitsUnit> &out, const char **why) {
    (void)s;
    if (n_values < 0 || (n_values + 7) / 8 > len) {
        *why = "PLAIN boolean page holds fewer bits than it has values";
        return false;
    }
    const int64_t per = (int64_t)BITS_PLAIN_UNIT_BYTES * 8;
    for (int64_t done = 0; done < n_values; done += per) {
        BitsUnit u{};
        u.src = dev_base + (uint64_t)(done >> 3);
        u.out_start = out0 + done;
        u.count = (int32_t)(n_values - done < per ? n_values - done : per);
        u.kind = BITS_LITERAL;
        u.msb = BITS_LSB;
        u.out_esize = (uint8_t)out_esize;
        u.dense_target = (uint8_t)dense_target;
        out.push_back(u);
    }
    return true;
}

// ORC boolean DATA stream: byte-RLE (header h >= 0: h + 3 copies of the next
// byte; h < 0: -h literal bytes) over MSB-first bytes. One unit per run or
// literal group; the last one is cut at n_values (the stripe's padding).
// Fails on a stream that ends before n_values values.
inline bool prescan_boolrle(const uint8_t *s, int64_t len, int64_t n_values,
                            int out_esize, int dense_target,
                            uint64_t dev_base, int64_t out0,
                            std::vector<BitsUnit> &out, const char **why) {
    int64_t p = 0, cnt = 0;
    while (cnt < n_values) {
        if (p >= len) {
            *why = "boolean byte-RLE stream holds fewer values than the "
                   "column has non-null rows";
            return false;
        }
        const int8_t h = (int8_t)s[p++];
        BitsUnit u{};
        u.out_start = out0 + cnt;
        u.msb = BITS_MSB;
        u.out_esize = (uint8_t)out_esize;
        u.dense_target = (uint8_t)dense_target;
        const int64_t left = n_values - cnt;
        if (h >= 0) {
            if (p >= len) {
                *why = "boolean byte-RLE run truncated";
                return false;
            }
            u.kind = BITS_RUN;
            u.value = s[p++];
            const int64_t vals = ((int64_t)h + 3) * 8;
            u.count = (int32_t)(vals < left ? vals : left);
        } else {
            const int64_t lit = -(int64_t)h;
            const int64_t vals = lit * 8;
            u.kind = BITS_LITERAL;
            u.src = dev_base + (uint64_t)p;
            u.count = (int32_t)(vals < left ? vals : left);
            // the kernel reads ceil(count / 8) literal bytes: they must be
            // there
            if (p + ((int64_t)u.count + 7) / 8 > len) {
                *why = "boolean byte-RLE literal truncated";
                return false;
            }
            p += lit;
        }
        cnt += u.count;
        out.push_back(u);
    }
    return true;
}

// Host decode of one prescanned unit through the shared core, group by
// group as the kernel does. `src` = the unit's literal bytes on the host
// (ignored for a run); out_base = host address standing for u.out_addr (r
// still comes from u.out_addr, so a test can pose any device alignment).
inline void bits_decode_unit_host(const uint8_t *src, const BitsUnit &u,
                                  void *out_base) {
    const int r = bits_unit_r(u.out_addr, u.out_start, u.out_esize);
    const int n_groups = bits_unit_groups(r, u.count);
    for (int g = 0; g < n_groups; g++) {
        const uint64_t bytes = bits_spread(bits_unit_group(u, src, r, g));
        for (int t = 0; t < 8; t++) {
            const int64_t e = (int64_t)8 * g - r + t;  // value of the unit
            if (e < 0 || e >= u.count) continue;
            const uint8_t v = (uint8_t)(bytes >> (8 * t));
            if (u.out_esize == 4)
                ((int32_t *)out_base)[u.out_start + e] = v;
            else
                ((uint8_t *)out_base)[u.out_start + e] = v;
        }
    }
}

#endif  // PMH_BITS_CORE_H
