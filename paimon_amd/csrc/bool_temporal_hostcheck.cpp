// Stand-alone host check of the BOOLEAN and ORC TIMESTAMP staging code, meant
// to be built with -fsanitize=address,undefined (make hostcheck): the two
// boolean prescans and the shared bit-expansion core over well-formed,
// truncated and malformed streams held in exactly-sized heap blocks (so one
// byte read past a stream is an ASan report), the timestamp core over its
// value edges and refusals, and the ORC metadata parser's writer-timezone
// field over the ORC files given on the command line. No GPU, no HIP.
#include "bits_core.h"
#include "orc_meta.h"
#include "orc_timestamp_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int failures = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__,         \
                    __LINE__, #cond);                                      \
            failures++;                                                    \
        }                                                                  \
    } while (0)

// reference expansion, bit by bit
static int bit_of(const std::vector<uint8_t> &bytes, int64_t i, int msb) {
    const uint8_t b = bytes[(size_t)(i >> 3)];
    return msb ? (b >> (7 - (i & 7))) & 1 : (b >> (i & 7)) & 1;
}

// prescan + host decode over an exactly-sized heap copy of `s`; the output
// is an exactly-sized heap block too, posed at every alignment
static bool decode(const std::vector<uint8_t> &s, int64_t n, int format,
                   int msb, int esize, int out_shift,
                   std::vector<int> &out, std::string &why) {
    uint8_t *heap = (uint8_t *)malloc(s.size() ? s.size() : 1);
    if (!s.empty()) memcpy(heap, s.data(), s.size());
    std::vector<BitsUnit> units;
    const char *w = "";
    bool ok = format == 0 ? prescan_bits_plain(heap, (int64_t)s.size(), n,
                                               esize, 0, 0, 0, units, &w)
                          : prescan_boolrle(heap, (int64_t)s.size(), n, esize,
                                            0, 0, 0, units, &w);
    if (!ok) why = w;
    void *dst = malloc((size_t)(n > 0 ? n : 1) * esize);
    memset(dst, 0xA5, (size_t)(n > 0 ? n : 1) * esize);
    for (size_t i = 0; ok && i < units.size(); i++) {
        units[i].msb = (uint8_t)msb;
        units[i].out_addr = (uint64_t)out_shift * (uint64_t)esize;
        bits_decode_unit_host(heap + units[i].src, units[i], dst);
    }
    out.clear();
    for (int64_t i = 0; ok && i < n; i++)
        out.push_back(esize == 4 ? ((int32_t *)dst)[i] : ((uint8_t *)dst)[i]);
    free(dst);
    free(heap);
    return ok;
}

static void check_bits() {
    std::vector<uint8_t> raw;
    for (int i = 0; i < 600; i++) raw.push_back((uint8_t)(i * 73 + 11));
    std::vector<int> out;
    std::string why;
    const int64_t counts[] = {1, 7, 8, 9, 63, 64, 65, 511, 512, 513,
                              1039, 1040, 1041, 4099};
    for (int64_t n : counts)
        for (int msb = 0; msb < 2; msb++)
            for (int esize : {1, 4})
                for (int sh = 0; sh < 8; sh++) {
                    // exactly ceil(n / 8) bytes: no slack behind the values
                    std::vector<uint8_t> s(raw.begin(),
                                           raw.begin() + (n + 7) / 8);
                    CHECK(decode(s, n, 0, msb, esize, sh, out, why));
                    for (int64_t i = 0; i < n; i++)
                        CHECK(out[(size_t)i] == bit_of(raw, i, msb));
                }
    // one byte short
    {
        std::vector<uint8_t> s(raw.begin(), raw.begin() + 2);
        CHECK(!decode(s, 17, 0, 0, 1, 0, out, why));
        CHECK(why.find("fewer bits") != std::string::npos);
    }
    // ORC byte-RLE: run of 3, literals of 2, run of 130, literal of 128
    std::vector<uint8_t> s, bytes;
    auto run = [&](int k, uint8_t v) {
        s.push_back((uint8_t)(k - 3));
        s.push_back(v);
        bytes.insert(bytes.end(), (size_t)k, v);
    };
    auto lit = [&](int k, int seed) {
        s.push_back((uint8_t)(256 - k));
        for (int i = 0; i < k; i++) {
            s.push_back((uint8_t)(seed + i * 37));
            bytes.push_back((uint8_t)(seed + i * 37));
        }
    };
    run(3, 0xB1);
    lit(2, 5);
    run(130, 0x00);
    lit(128, 9);
    run(130, 0xFF);
    lit(1, 200);
    const int64_t total = (int64_t)bytes.size() * 8;
    for (int64_t n : {(int64_t)1, (int64_t)24, (int64_t)25, (int64_t)40,
                      (int64_t)41, total - 9, total - 7, total})
        for (int msb = 0; msb < 2; msb++)
            for (int sh = 0; sh < 8; sh += 3) {
                CHECK(decode(s, n, 1, msb, 1, sh, out, why));
                for (int64_t i = 0; i < n; i++)
                    CHECK(out[(size_t)i] == bit_of(bytes, i, msb));
            }
    // every truncation point: either the values still fit what is left, or
    // the prescan refuses; it never reads past the block
    for (size_t cut = 0; cut < s.size(); cut++) {
        std::vector<uint8_t> t(s.begin(), s.begin() + cut);
        const bool ok = decode(t, total, 1, 1, 1, 0, out, why);
        CHECK(!ok);
        CHECK(!why.empty());
    }
    // a value count that ends inside a literal group needs only the bytes
    // its values occupy
    {
        std::vector<uint8_t> t = {0xFD, 0x80, 0x01};  // 3 literals, 2 present
        CHECK(decode(t, 16, 1, 1, 1, 0, out, why));
        CHECK(out[0] == 1 && out[15] == 1);
        CHECK(!decode(t, 17, 1, 1, 1, 0, out, why));
    }
    // spread and group arithmetic
    CHECK(bits_spread(0xFF) == 0x0101010101010101ull);
    CHECK(bits_spread(0x81) == 0x0100000000000001ull);
    CHECK(bits_norm(0x80, 1) == 0x01 && bits_norm(0x80, 0) == 0x80);
    CHECK(bits_group(0xF0, 0x0F, 4) == 0xFF);
    CHECK(bits_group(0xAB, 0xCD, 0) == 0xCD);
}

static void check_timestamps() {
    int64_t v = 0, nanos = 0;
    CHECK(ots_nanos(0, &nanos) == OTS_OK && nanos == 0);
    CHECK(ots_nanos((5 << 3) | 7, &nanos) == OTS_OK && nanos == 500000000);
    CHECK(ots_nanos((uint64_t)999999999 << 3, &nanos) == OTS_OK &&
          nanos == 999999999);
    CHECK(ots_nanos((uint64_t)1000000000 << 3, &nanos) == OTS_ERR_NANOS);
    CHECK(ots_nanos((10 << 3) | 7, &nanos) == OTS_ERR_NANOS);
    CHECK(ots_nanos(~0ull, &nanos) == OTS_ERR_NANOS);
    CHECK(ots_nanos((uint64_t)(int64_t)((-5 * 8) | 7), &nanos) ==
          OTS_ERR_NANOS);
    // 2015-01-01 itself, the epoch, one second before it
    CHECK(ots_value(0, 0, OTS_UNIT_MICROS, &v) == OTS_OK &&
          v == OTS_BASE_SECONDS * 1000000);
    CHECK(ots_value(-OTS_BASE_SECONDS, 0, OTS_UNIT_MILLIS, &v) == OTS_OK &&
          v == 0);
    CHECK(ots_value(-OTS_BASE_SECONDS - 1, 0, OTS_UNIT_MILLIS, &v) == OTS_OK &&
          v == -1000);
    CHECK(ots_value(-OTS_BASE_SECONDS - 1, (5 << 3) | 7, OTS_UNIT_MILLIS,
                    &v) == OTS_ERR_NEG_FRACTION);
    // truncation below the unit
    CHECK(ots_value(-OTS_BASE_SECONDS + 1, (uint64_t)1999999 << 3,
                    OTS_UNIT_MICROS, &v) == OTS_OK && v == 1001999);
    CHECK(ots_value(-OTS_BASE_SECONDS + 1, (uint64_t)1999999 << 3,
                    OTS_UNIT_MILLIS, &v) == OTS_OK && v == 1001);
    // both int64 limits of both units, and one step past them (UBSan
    // watches the arithmetic)
    for (int unit : {OTS_UNIT_MILLIS, OTS_UNIT_MICROS}) {
        const int64_t per = unit == OTS_UNIT_MICROS ? 1000000 : 1000;
        const int64_t s_max = INT64_MAX / per, s_min = INT64_MIN / per;
        const int64_t frac = INT64_MAX - s_max * per;  // in units
        const uint64_t stored = (uint64_t)(frac * (1000000000 / per)) << 3;
        CHECK(ots_value(s_max - OTS_BASE_SECONDS, stored, unit, &v) ==
                  OTS_OK && v == INT64_MAX);
        CHECK(ots_value(s_min - OTS_BASE_SECONDS, 0, unit, &v) == OTS_OK &&
              v == s_min * per);
        CHECK(ots_value(s_max + 1 - OTS_BASE_SECONDS, 0, unit, &v) ==
              OTS_ERR_RANGE);
        CHECK(ots_value(s_min - 1 - OTS_BASE_SECONDS, 0, unit, &v) ==
              OTS_ERR_RANGE);
        CHECK(ots_value(s_max - OTS_BASE_SECONDS,
                        (uint64_t)((frac + 1) * (1000000000 / per)) << 3,
                        unit, &v) == OTS_ERR_RANGE);
        CHECK(ots_value(INT64_MAX, 0, unit, &v) == OTS_ERR_RANGE);
        CHECK(ots_value(INT64_MIN, 0, unit, &v) == OTS_ERR_RANGE);
    }
    for (int code = 1; code <= OTS_ERR_LAST; code++)
        CHECK(strcmp(ots_err_text(code), "ok") != 0);
}

static void check_timezones() {
    CHECK(pmh::orc_timezone_is_utc(""));
    CHECK(pmh::orc_timezone_is_utc("UTC"));
    CHECK(pmh::orc_timezone_is_utc("GMT"));
    CHECK(!pmh::orc_timezone_is_utc("PST"));
    CHECK(!pmh::orc_timezone_is_utc("America/Los_Angeles"));
    CHECK(!pmh::orc_timezone_is_utc("utc "));
}

// The ORC files of the command line: parse the metadata from an exactly-sized
// heap block and print each stripe's writer timezone; then parse every
// truncation of the file tail, which must fail cleanly or succeed, never
// read outside the block.
static void check_file(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        failures++;
        return;
    }
    std::vector<uint8_t> buf;
    uint8_t tmp[65536];
    size_t got;
    while ((got = fread(tmp, 1, sizeof tmp, f)) > 0)
        buf.insert(buf.end(), tmp, tmp + got);
    fclose(f);
    uint8_t *heap = (uint8_t *)malloc(buf.size() ? buf.size() : 1);
    memcpy(heap, buf.data(), buf.size());
    pmh::OrcFileMeta om = pmh::parse_orc_meta(heap, (int64_t)buf.size());
    CHECK(om.ok());
    for (size_t i = 0; i < om.stripes.size(); i++)
        printf("%s stripe %zu: writerTimezone '%s' utc=%d\n", path, i,
               om.stripes[i].writer_timezone.c_str(),
               (int)pmh::orc_timezone_is_utc(om.stripes[i].writer_timezone));
    free(heap);
    for (size_t cut = 1; cut <= 64 && cut < buf.size(); cut++) {
        const size_t n = buf.size() - cut;
        uint8_t *h2 = (uint8_t *)malloc(n ? n : 1);
        memcpy(h2, buf.data(), n);
        pmh::OrcFileMeta t = pmh::parse_orc_meta(h2, (int64_t)n);
        (void)t;
        free(h2);
    }
}

int main(int argc, char **argv) {
    check_bits();
    check_timestamps();
    check_timezones();
    for (int i = 1; i < argc; i++) check_file(argv[i]);
    if (failures) {
        fprintf(stderr, "bool_temporal_hostcheck: %d failure(s)\n", failures);
        return 1;
    }
    printf("bool_temporal_hostcheck OK\n");
    return 0;
}
