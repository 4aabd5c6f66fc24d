// Stand-alone host check of the ORC DECIMAL staging code, meant to be built
// with -fsanitize=address,undefined (make hostcheck): prescan_varint and the
// shared scalar core over well-formed, truncated and malformed streams held
// in exactly-sized heap blocks (so one byte read past a stream is an ASan
// report), plus the ORC metadata parser over the ORC files given on the
// command line (decimal precision / scale / SECONDARY streams). No GPU, no
// HIP.
#include "orc_decimal_core.h"
#include "orc_meta.h"

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

static void put_varint(std::vector<uint8_t> &s, int64_t v) {
    uint64_t u = ((uint64_t)v << 1) ^ (uint64_t)(v >> 63);
    while (u >= 0x80) {
        s.push_back((uint8_t)(0x80 | (u & 0x7F)));
        u >>= 7;
    }
    s.push_back((uint8_t)u);
}

// prescan + host decode over an exactly-sized copy of `s`
static bool decode(const std::vector<uint8_t> &s, int64_t n, int precision,
                   int scale, const int32_t *scales, int esize,
                   std::vector<int64_t> &out, std::string &why, int *err) {
    uint8_t *heap = (uint8_t *)malloc(s.size() ? s.size() : 1);
    if (!s.empty()) memcpy(heap, s.data(), s.size());
    std::vector<VarintUnit> units;
    const char *w = "";
    *err = ODC_OK;
    bool ok = prescan_varint(heap, (int64_t)s.size(), n, esize, precision,
                             scale, 0, 0, 0, units, &w);
    if (!ok) why = w;
    out.assign((size_t)(n > 0 ? n : 1), 0);
    std::vector<int32_t> out32((size_t)(n > 0 ? n : 1), 0);
    for (size_t i = 0; ok && i < units.size(); i++) {
        int bad = 0;
        int e = odc_decode_unit_host(
            heap + units[i].src, units[i],
            scales ? scales + units[i].out_start : nullptr,
            esize == 4 ? (void *)out32.data() : (void *)out.data(), &bad);
        if (e) {
            *err = e;
            why = odc_err_text(e);
            ok = false;
        }
    }
    if (ok && esize == 4)
        for (int64_t i = 0; i < n; i++) out[i] = out32[i];
    free(heap);
    return ok;
}

static void check_streams() {
    std::vector<int64_t> vals;
    for (int sh = 0; sh < 63; sh++) {
        vals.push_back((int64_t)1 << sh);
        vals.push_back(-((int64_t)1 << sh));
        vals.push_back(((int64_t)1 << sh) - 1);
    }
    vals.push_back(INT64_MIN);
    vals.push_back(INT64_MAX);
    vals.push_back(0);
    while (vals.size() < 1025) vals.push_back((int64_t)vals.size() * -7919);
    std::vector<uint8_t> s;
    for (int64_t v : vals) put_varint(s, v);
    std::vector<int64_t> out;
    std::string why;
    int err;
    for (int64_t n : {(int64_t)1, (int64_t)511, (int64_t)512, (int64_t)513,
                      (int64_t)1025}) {
        CHECK(decode(s, n, ODC_MAX_PRECISION, 0, nullptr, 8, out, why, &err));
        for (int64_t i = 0; i < n; i++) CHECK(out[i] == vals[i]);
    }
    // every truncation point of a short stream: ends inside a value, or
    // holds fewer values
    std::vector<uint8_t> t;
    std::vector<int64_t> tv = {5, (int64_t)1 << 40, -3, INT64_MIN, 77};
    for (int64_t v : tv) put_varint(t, v);
    for (size_t cut = 0; cut < t.size(); cut++) {
        std::vector<uint8_t> c(t.begin(), t.begin() + cut);
        CHECK(!decode(c, (int64_t)tv.size(), ODC_MAX_PRECISION, 0, nullptr, 8,
                      out, why, &err));
        CHECK(why.find("ends inside a value") != std::string::npos ||
              why.find("fewer values") != std::string::npos);
    }
    // an 11-byte value, and a 10-byte value wider than 64 bits
    std::vector<uint8_t> e11(10, 0x80);
    e11.push_back(0x00);
    CHECK(!decode(e11, 1, ODC_MAX_PRECISION, 0, nullptr, 8, out, why, &err));
    CHECK(why.find("longer than 10 bytes") != std::string::npos);
    std::vector<uint8_t> wide(9, 0xFF);
    wide.push_back(0x02);
    CHECK(!decode(wide, 1, ODC_MAX_PRECISION, 0, nullptr, 8, out, why, &err));
    CHECK(why.find("more than 64 bits") != std::string::npos);
    // continuation bytes to the very end of the block
    std::vector<uint8_t> open(7, 0xFF);
    CHECK(!decode(open, 1, 18, 2, nullptr, 8, out, why, &err));
    // empty stream
    CHECK(!decode({}, 1, 18, 2, nullptr, 8, out, why, &err));
    CHECK(decode({}, 0, 18, 2, nullptr, 8, out, why, &err));
    // rescale: errors and the edges of the range
    std::vector<uint8_t> r;
    put_varint(r, 100);
    put_varint(r, 200);
    int32_t high[2] = {2, 3}, neg[2] = {-1, 2}, low[2] = {0, 1};
    CHECK(!decode(r, 2, 18, 2, high, 8, out, why, &err) &&
          err == ODC_ERR_SCALE_HIGH);
    CHECK(!decode(r, 2, 18, 2, neg, 8, out, why, &err) &&
          err == ODC_ERR_SCALE_NEG);
    CHECK(decode(r, 2, 18, 2, low, 8, out, why, &err) && out[0] == 10000 &&
          out[1] == 2000);
    std::vector<uint8_t> big;
    put_varint(big, 999999999999999999LL);
    put_varint(big, -999999999999999999LL);
    CHECK(decode(big, 2, 18, 2, nullptr, 8, out, why, &err));
    int32_t one_less[2] = {1, 1};
    CHECK(!decode(big, 2, 18, 2, one_less, 8, out, why, &err) &&
          err == ODC_ERR_PRECISION);
    std::vector<uint8_t> over;
    put_varint(over, 1000000000000000000LL);
    CHECK(!decode(over, 1, 18, 2, nullptr, 8, out, why, &err) &&
          err == ODC_ERR_PRECISION);
    // full-range multiply guard: INT64_MAX / 10 + 1 at one scale step
    std::vector<uint8_t> edge;
    put_varint(edge, INT64_MAX / 10);
    put_varint(edge, INT64_MAX / 10 + 1);
    int32_t step[2] = {0, 0};
    CHECK(!decode(edge, 2, ODC_MAX_PRECISION, 1, step, 8, out, why, &err) &&
          err == ODC_ERR_PRECISION);
    CHECK(decode(edge, 1, ODC_MAX_PRECISION, 1, step, 8, out, why, &err) &&
          out[0] == INT64_MAX / 10 * 10);
    // int32 output
    std::vector<uint8_t> i32;
    put_varint(i32, 999999999);
    put_varint(i32, -999999999);
    CHECK(decode(i32, 2, 9, 3, nullptr, 4, out, why, &err) &&
          out[0] == 999999999 && out[1] == -999999999);
    std::vector<uint8_t> o32;
    put_varint(o32, (int64_t)1 << 31);
    CHECK(!decode(o32, 1, ODC_MAX_PRECISION, 0, nullptr, 4, out, why, &err) &&
          err == ODC_ERR_INT32);
}

static void check_meta(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        failures++;
        return;
    }
    std::vector<uint8_t> buf;
    uint8_t tmp[65536];
    size_t got;
    while ((got = fread(tmp, 1, sizeof(tmp), f)) > 0)
        buf.insert(buf.end(), tmp, tmp + got);
    fclose(f);
    {
        uint8_t *heap = (uint8_t *)malloc(buf.size());
        memcpy(heap, buf.data(), buf.size());
        pmh::OrcFileMeta m = pmh::parse_orc_meta(heap, (int64_t)buf.size());
        CHECK(m.ok());
        CHECK(m.column_kinds.size() == m.column_precisions.size());
        CHECK(m.column_kinds.size() == m.column_scales.size());
        int decimals = 0;
        for (size_t i = 0; i < m.column_kinds.size(); i++) {
            if (m.column_kinds[i] == pmh::ORC_DECIMAL) {
                decimals++;
                printf("column %s: decimal(%d,%d)\n",
                       m.column_names[i].c_str(), m.column_precisions[i],
                       m.column_scales[i]);
                for (const auto &st : m.stripes)
                    CHECK(pmh::orc_find_stream(
                              st, (int)i + 1, pmh::ORC_STREAM_SECONDARY) !=
                          nullptr);
            } else {
                CHECK(m.column_precisions[i] == 0);
            }
        }
        CHECK(decimals > 0);
        free(heap);
    }
}

int main(int argc, char **argv) {
    check_streams();
    for (int i = 1; i < argc; i++) check_meta(argv[i]);
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("orc decimal host check: ok\n");
    return 0;
}
