// ORC TIMESTAMP / TIMESTAMP_INSTANT value arithmetic (ORC v1 spec,
// "Timestamp Columns", DIRECT_V2): the DATA stream holds signed RLEv2 seconds
// relative to 2015-01-01T00:00:00 UTC, the SECONDARY stream unsigned RLEv2
// nanoseconds with their trailing decimal zeros removed: for a stored v,
// z = v & 7 and r = v >> 3; nanos = r when z == 0, else r * 10^(z + 1).
// The reader's column is INT64 milliseconds (precision <= 3) or microseconds
// (precision 4..6) since the Unix epoch, digits below the unit truncated.
//
// Shared scalar core, like orc_decimal_core.h: k_orc_timestamp (kernels.hip)
// and the host mode of pmh_debug_orc_timestamp (plan.cpp) run exactly
// ots_nanos / ots_combine.
//
// Refused, never guessed at:
//  - a value before 1970 with a non-zero fraction: writers disagree on how
//    they store it (truncated seconds plus negative nanos wrapped into the
//    unsigned stream, or positive nanos with the second shifted on read);
//  - decoded nanos of 10^9 or more (this also catches wrapped negatives);
//  - a result outside int64.
// As negative fractional values are refused, truncation equals floor.
#ifndef PMH_ORC_TIMESTAMP_CORE_H
#define PMH_ORC_TIMESTAMP_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define OTS_HD __host__ __device__ inline
#else
#define OTS_HD inline
#endif

// seconds from 1970-01-01 to the ORC timestamp base 2015-01-01, both UTC
constexpr int64_t OTS_BASE_SECONDS = 1420070400LL;

enum { OTS_UNIT_MILLIS = 0, OTS_UNIT_MICROS = 1 };

// values per work unit of k_orc_timestamp (one workgroup per unit)
constexpr int OTS_UNIT_VALUES = 4096;

// error codes (0 = ok); the kernel ORs 1 << (OTS_ERR_SHIFT + code) into the
// section's error word, above the decimal bits (ODC_ERR_SHIFT + 1..5)
constexpr int OTS_ERR_SHIFT = 16;
enum {
    OTS_OK = 0,
    OTS_ERR_NEG_FRACTION = 1,  // before 1970 with non-zero nanos
    OTS_ERR_NANOS = 2,         // nanos >= 10^9
    OTS_ERR_RANGE = 3,         // result outside int64
    OTS_ERR_LAST = 3,
};

OTS_HD const char *ots_err_text(int code) {
    switch (code) {
    case OTS_ERR_NEG_FRACTION:
        return "value before 1970 with a fractional second (writers "
               "disagree on its encoding)";
    case OTS_ERR_NANOS:
        return "nanoseconds of 10^9 or more (or negative nanos wrapped into "
               "the unsigned stream)";
    case OTS_ERR_RANGE: return "value outside the int64 range of the column "
                               "unit";
    default: return "ok";
    }
}

// Stored SECONDARY value -> nanoseconds. OTS_ERR_NANOS when they reach 10^9.
OTS_HD int ots_nanos(uint64_t v, int64_t *nanos) {
    *nanos = 0;
    const int z = (int)(v & 7);
    uint64_t r = v >> 3;
    if (r >= 1000000000ull) return OTS_ERR_NANOS;
    if (z) {
        uint64_t m = 100;  // 10^(z + 1), z = 1..7
        for (int i = 1; i < z; i++) m *= 10;
        r *= m;  // < 10^9 * 10^8: fits
        if (r >= 1000000000ull) return OTS_ERR_NANOS;
    }
    *nanos = (int64_t)r;
    return OTS_OK;
}

// (seconds relative to 2015, nanos) -> the column value in `unit`.
OTS_HD int ots_combine(int64_t secs, int64_t nanos, int unit, int64_t *out) {
    *out = 0;
    int64_t s;
    if (__builtin_add_overflow(secs, OTS_BASE_SECONDS, &s))
        return OTS_ERR_RANGE;
    if (s < 0 && nanos != 0) return OTS_ERR_NEG_FRACTION;
    const int64_t per = unit == OTS_UNIT_MICROS ? 1000000LL : 1000LL;
    const int64_t frac =
        unit == OTS_UNIT_MICROS ? nanos / 1000 : nanos / 1000000;
    int64_t v;
    if (__builtin_mul_overflow(s, per, &v) ||
        __builtin_add_overflow(v, frac, &v))
        return OTS_ERR_RANGE;
    *out = v;
    return OTS_OK;
}

// One stored (DATA, SECONDARY) pair -> the column value.
OTS_HD int ots_value(int64_t secs, uint64_t stored_nanos, int unit,
                     int64_t *out) {
    int64_t nanos;
    *out = 0;
    const int err = ots_nanos(stored_nanos, &nanos);
    if (err) return err;
    return ots_combine(secs, nanos, unit, out);
}

// One work unit of k_orc_timestamp: values [start, start + count) of a
// column's int64 seconds (decoded in place by k_rlev2) and of the (run,
// column)'s uint64 nanos scratch.
struct TsUnit {
    uint64_t out_addr;    // int64 seconds in, column values out
    uint64_t nanos_addr;  // uint64 stored SECONDARY values
    uint64_t err_addr;    // uint32 error word (see OTS_ERR_SHIFT)
    int64_t out_start;    // element index into out_addr
    int64_t nanos_start;  // element index into nanos_addr
    int32_t count;
    uint8_t unit;         // OTS_UNIT_*
    uint8_t dense_target; // 0: contig (positioned); 1: dense buffer
    uint8_t _pad[2];
};

#endif  // PMH_ORC_TIMESTAMP_CORE_H
