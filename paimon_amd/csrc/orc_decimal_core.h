// ORC DECIMAL value decode (ORC v1 spec, "Decimal Columns"): the DATA stream
// holds one zigzag base-128 varint per non-null row — the unscaled value,
// least-significant 7-bit group first, the high bit of a byte meaning "more
// follows" — and the SECONDARY stream each value's own scale. The reader
// brings every value to the column's scale.
//
// Shared scalar core, like lookup_core.h and zstd_core.h: k_orc_varint
// (kernels.hip) and the host mode of pmh_debug_orc_decimal (plan.cpp) run
// exactly odc_compact / odc_zigzag / odc_rescale, so the CPU tests pin the
// arithmetic the kernel executes. prescan_varint (host only) is the staging
// walk that cuts a DATA stream into the kernel's work units.
#ifndef PMH_ORC_DECIMAL_CORE_H
#define PMH_ORC_DECIMAL_CORE_H

#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define ODC_HD __host__ __device__ inline
#else
#define ODC_HD inline
#endif

// values per work unit: the granularity of k_rlev2 and k_level_scatter
constexpr int ODC_UNIT_VALUES = 512;
// a varint longer than this cannot fit 64 bits
constexpr int ODC_MAX_VARINT = 10;
// precision 19 is the whole int64 range (10^19 > 2^63): no column declares
// it, the stream-level debug entry uses it to reach 10-byte values
constexpr int ODC_MAX_PRECISION = 19;

// error codes of odc_rescale (0 = ok); the kernel ORs
// 1 << (ODC_ERR_SHIFT + code) into the section's error word (the low bits
// belong to the merge kernels), the host mode reports the first
constexpr int ODC_ERR_SHIFT = 8;
enum {
    ODC_OK = 0,
    ODC_ERR_SCALE_HIGH = 1,   // data scale above the column scale
    ODC_ERR_SCALE_NEG = 2,    // negative data scale
    ODC_ERR_PRECISION = 3,    // |rescaled value| >= 10^precision
    ODC_ERR_INT32 = 4,        // 4-byte output and a value outside int32
    ODC_ERR_WIDTH = 5,        // varint carries more than 64 bits
};

ODC_HD const char *odc_err_text(int code) {
    switch (code) {
    case ODC_ERR_SCALE_HIGH: return "data scale above the column scale";
    case ODC_ERR_SCALE_NEG: return "negative data scale";
    case ODC_ERR_PRECISION: return "rescaled value needs more digits than "
                                   "the column precision";
    case ODC_ERR_INT32: return "value outside int32 in a precision <= 9 "
                               "column";
    case ODC_ERR_WIDTH: return "varint carries more than 64 bits";
    default: return "ok";
    }
}

// 10^e for e = 0..18 (a switch, so host and device share it without a
// device-side constant table)
ODC_HD int64_t odc_pow10(int e) {
    switch (e) {
    case 0: return 1LL;
    case 1: return 10LL;
    case 2: return 100LL;
    case 3: return 1000LL;
    case 4: return 10000LL;
    case 5: return 100000LL;
    case 6: return 1000000LL;
    case 7: return 10000000LL;
    case 8: return 100000000LL;
    case 9: return 1000000000LL;
    case 10: return 10000000000LL;
    case 11: return 100000000000LL;
    case 12: return 1000000000000LL;
    case 13: return 10000000000000LL;
    case 14: return 100000000000000LL;
    case 15: return 1000000000000000LL;
    case 16: return 10000000000000000LL;
    case 17: return 100000000000000000LL;
    default: return 1000000000000000000LL;
    }
}

// One varint of `len` (1..10) bytes, handed over little-endian: b0 = bytes
// 0..7, b1 = bytes 8..9 (bytes at or past len are ignored). Drops the
// continuation bits and packs the 7-bit groups LSB-first. *err is set when
// the 10th byte holds more than the one bit that still fits.
ODC_HD uint64_t odc_compact(uint64_t b0, uint64_t b1, int len, int *err) {
    if (len < 8) b0 &= (1ull << (len * 8)) - 1;
    uint64_t x = b0 & 0x7F7F7F7F7F7F7F7Full;
    x = ((x & 0x7F007F007F007F00ull) >> 1) | (x & 0x007F007F007F007Full);
    x = ((x & 0x3FFF00003FFF0000ull) >> 2) | (x & 0x00003FFF00003FFFull);
    x = ((x & 0x0FFFFFFF00000000ull) >> 4) | (x & 0x000000000FFFFFFFull);
    if (len > 8) {
        x |= (b1 & 0x7F) << 56;
        if (len > 9) {
            uint64_t top = (b1 >> 8) & 0x7F;
            if (top > 1) *err = ODC_ERR_WIDTH;
            x |= top << 63;
        }
    }
    return x;
}

ODC_HD int64_t odc_zigzag(uint64_t v) {
    return (int64_t)(v >> 1) ^ -(int64_t)(v & 1);
}

// Bring unscaled value v from data_scale to the column's (precision,
// col_scale) and check it against the column: returns ODC_OK and *out, or
// an ODC_ERR_* code (then *out is 0). The product never divides: a data
// scale above the column scale is refused, not rounded.
ODC_HD int odc_rescale(int64_t v, int data_scale, int precision,
                       int col_scale, int out_esize, int64_t *out) {
    *out = 0;
    if (data_scale < 0) return ODC_ERR_SCALE_NEG;
    if (data_scale > col_scale) return ODC_ERR_SCALE_HIGH;
    const int up = col_scale - data_scale;  // 0..18
    const int64_t mult = odc_pow10(up);
    // largest magnitude the column holds, before the multiply
    int64_t lim;
    if (precision >= ODC_MAX_PRECISION) {
        if (up == 0) {  // nothing to check: every int64 is in range
            if (out_esize == 4 && (v < INT32_MIN || v > INT32_MAX))
                return ODC_ERR_INT32;
            *out = v;
            return ODC_OK;
        }
        lim = INT64_MAX / mult;
    } else {
        lim = (odc_pow10(precision) - 1) / mult;
    }
    if (v > lim || v < -lim) return ODC_ERR_PRECISION;
    const int64_t r = v * mult;
    if (out_esize == 4 && (r < INT32_MIN || r > INT32_MAX))
        return ODC_ERR_INT32;
    *out = r;
    return ODC_OK;
}

// One work unit of k_orc_varint: <= ODC_UNIT_VALUES consecutive varints.
struct VarintUnit {
    uint64_t src;         // device address of the unit's first byte
    uint64_t out_addr;    // absolute output base (patched at finalize)
    uint64_t scale_addr;  // int32 data scale per value of the unit; 0 =
                          // every value at the column scale
    uint64_t err_addr;    // uint32 error word (see ODC_ERR_SHIFT)
    int64_t out_start;    // dense output element index
    int32_t nbytes;       // bytes of the unit (<= 10 per value)
    int32_t count;        // values in the unit
    uint8_t out_esize;    // 4 or 8
    uint8_t precision;    // column precision (1..19)
    uint8_t scale;        // column scale
    uint8_t dense_target; // 0: contig (positioned); 1: dense buffer
    uint8_t _pad[4];
};

// ---- host side (staging walk + host twin of the kernel's value loop)

// Walk a DATA stream of n_values varints once and cut it into work units.
// Fails (returns false, *why set) when the stream ends inside a value, holds
// fewer than n_values values, or holds a value longer than 10 bytes or wider
// than 64 bits. Bytes past the n_values-th value are left alone.
inline bool prescan_varint(const uint8_t *s, int64_t len, int64_t n_values,
                           int out_esize, int precision, int scale,
                           int dense_target, uint64_t dev_base,
                           int64_t dense0, std::vector<VarintUnit> &out,
                           const char **why) {
    int64_t p = 0, done = 0;
    while (done < n_values) {
        VarintUnit u{};
        u.src = dev_base + (uint64_t)p;
        u.out_start = dense0 + done;
        u.out_esize = (uint8_t)out_esize;
        u.precision = (uint8_t)precision;
        u.scale = (uint8_t)scale;
        u.dense_target = (uint8_t)dense_target;
        const int64_t p0 = p;
        int cnt = 0;
        while (cnt < ODC_UNIT_VALUES && done + cnt < n_values) {
            if (p >= len) {
                *why = "varint stream holds fewer values than the column "
                       "has non-null rows";
                return false;
            }
            int vl = 0;
            for (;;) {
                if (p >= len) {
                    *why = "varint stream ends inside a value";
                    return false;
                }
                const uint8_t b = s[p++];
                if (++vl > ODC_MAX_VARINT) {
                    *why = "varint longer than 10 bytes (does not fit 64 "
                           "bits)";
                    return false;
                }
                if (!(b & 0x80)) {
                    if (vl == ODC_MAX_VARINT && b > 1) {
                        *why = "varint carries more than 64 bits";
                        return false;
                    }
                    break;
                }
            }
            cnt++;
        }
        u.nbytes = (int32_t)(p - p0);
        u.count = cnt;
        done += cnt;
        out.push_back(u);
    }
    return true;
}

// Host decode of one prescanned unit through the shared core. `s` is the
// unit's first byte on the host; scales = the unit's per-value data scales,
// or null for the uniform (column-scale) path. Returns ODC_OK or the
// first ODC_ERR_* met; *bad gets that value's index in the unit.
inline int odc_decode_unit_host(const uint8_t *s, const VarintUnit &u,
                                const int32_t *scales, void *out,
                                int *bad) {
    int64_t p = 0;
    for (int j = 0; j < u.count; j++) {
        uint64_t b0 = 0, b1 = 0;
        int vl = 0;
        for (;; vl++) {
            const uint8_t b = s[p + vl];
            if (vl < 8)
                b0 |= (uint64_t)b << (8 * vl);
            else
                b1 |= (uint64_t)b << (8 * (vl - 8));
            if (!(b & 0x80)) break;
        }
        vl++;
        p += vl;
        int err = ODC_OK;
        const int64_t v = odc_zigzag(odc_compact(b0, b1, vl, &err));
        int64_t r = 0;
        if (!err)
            err = odc_rescale(v, scales ? scales[j] : u.scale,
                              u.precision, u.scale, u.out_esize, &r);
        if (err) {
            *bad = j;
            return err;
        }
        if (u.out_esize == 4)
            ((int32_t *)out)[u.out_start + j] = (int32_t)r;
        else
            ((int64_t *)out)[u.out_start + j] = r;
    }
    return ODC_OK;
}

#endif  // PMH_ORC_DECIMAL_CORE_H
