// Stand-alone host check of the partial-update aggregate fold
// (pu_agg_core.h), meant to be built with -fsanitize=address,undefined
// (make hostcheck). What k_emit_pu_sga runs per output row runs here over
// exactly-sized heap blocks: a read past a member list, a column table or a
// group table is an ASan report, a signed overflow in a sum or a shift by
// the mask width a UBSan report. Checked:
//  - two vectors of the reference's PartialUpdateMergeFunctionTest
//    (testFirstValue; testPartialUpdateWithAggregation with its retracts);
//  - random key groups of 2..32 members (bit 31 of the masks live) with
//    nulls, empty tuples, retracts and values at the ends of every integer
//    range, for every aggregator x dtype x {plain, ignore-retract}: the
//    fold's invariants (below) hold.
// No GPU, no HIP.
#include "pu_agg_core.h"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
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

static const int64_t NUL = INT64_MIN;  // a null field in the tables below

struct Group {
    int n_cols;
    std::vector<int8_t> kinds;
    std::vector<int64_t> values;  // [n * n_cols]
    std::vector<uint8_t> valid;
    void add(int kind, const std::vector<int64_t> &row) {
        kinds.push_back((int8_t)kind);
        for (int64_t v : row) {
            values.push_back(v == NUL ? 0 : v);
            valid.push_back(v == NUL ? 0 : 1);
        }
    }
};

struct Tables {
    std::vector<uint8_t> dtypes, col_group, sg_nseq, col_agg;
    std::vector<int16_t> sg_fields;
};

struct Result {
    std::vector<int64_t> values;
    std::vector<uint8_t> valid;
    int32_t kind, last, unsupported;
};

// every buffer the fold sees is a heap block of exactly its size
static Result fold(const Group &g, const Tables &t, bool ignore_delete) {
    const int n = (int)g.kinds.size();
    const int ng = (int)t.sg_nseq.size();
    Result r;
    r.values.assign(g.n_cols, 0);
    r.valid.assign(g.n_cols, 0);
    const char *what = pac_host_check(n, g.n_cols, ng, t.col_group.data(),
                                      t.sg_fields.data(), t.sg_nseq.data());
    CHECK(what == nullptr);
    if (what) exit(1);
    pac_host_fold(n, g.kinds.data(), g.n_cols, t.dtypes.data(),
                  g.values.data(), g.valid.data(), ng, t.col_group.data(),
                  t.sg_fields.data(), t.sg_nseq.data(), t.col_agg.data(),
                  ignore_delete, r.values.data(), r.valid.data(), &r.kind,
                  &r.last, &r.unsupported);
    return r;
}

static void expect_row(const Result &r, const std::vector<int64_t> &want) {
    CHECK(r.values.size() == want.size());
    for (size_t c = 0; c < want.size(); c++) {
        CHECK((want[c] != NUL) == (r.valid[c] != 0));
        if (want[c] != NUL) CHECK(r.values[c] == want[c]);
    }
}

static void check_vectors() {
    {  // testFirstValue: f1 | f2 first_value, f3 last_value
        Tables t;
        t.dtypes.assign(4, PAC_DT_INT32);
        t.col_group = {0xff, 0, 0, 0};
        t.sg_fields = {1, -1, -1, -1};
        t.sg_nseq = {1};
        t.col_agg = {PAC_NONE, PAC_NONE, PAC_FIRST_VALUE, PAC_LAST_VALUE};
        Group g{4, {}, {}, {}};
        g.add(0, {1, 1, 1, 1});
        g.add(0, {1, 2, 2, 2});
        expect_row(fold(g, t, false), {1, 2, 1, 2});
        g.add(0, {1, 0, 3, 3});  // older: first_value's reversed form
        expect_row(fold(g, t, false), {1, 2, 3, 2});
    }
    {  // testPartialUpdateWithAggregation
        Tables t;
        t.dtypes.assign(8, PAC_DT_INT32);
        t.col_group = {0xff, 0, 0, 0, 0, 0xff, 1, 1};
        t.sg_fields = {1, -1, -1, -1, 7, -1, -1, -1};
        t.sg_nseq = {1, 1};
        t.col_agg = {PAC_NONE,
                     PAC_NONE,
                     PAC_SUM,
                     PAC_NONE,
                     PAC_LAST_VALUE | PAC_IGNORE_RETRACT,
                     PAC_NONE,
                     PAC_LAST_NON_NULL | PAC_IGNORE_RETRACT,
                     PAC_NONE};
        Group g{8, {}, {}, {}};
        g.add(0, {1, 1, 1, 1, 1, 1, 1, 1});
        g.add(0, {1, 2, 1, 2, 2, 2, 2, 0});
        expect_row(fold(g, t, false), {1, 2, 2, 2, 2, 2, 1, 1});
        g.add(0, {1, 1, 1, 1, 1, 1, 2, 0});
        expect_row(fold(g, t, false), {1, 2, 3, 2, 2, 1, 1, 1});
        g.add(0, {1, 1, -1, 1, 1, 2, 2, 0});
        g.add(0, {1, 3, NUL, NUL, NUL, NUL, NUL, 2});
        expect_row(fold(g, t, false), {1, 3, 2, NUL, NUL, 2, 1, 2});
        g.add(0, {1, 3, 1, 1, 1, 1, 1, 3});
        expect_row(fold(g, t, false), {1, 3, 3, 1, 1, 1, 1, 3});
        g.add(1, {1, 3, 2, 1, 1, 1, 1, 3});
        expect_row(fold(g, t, false), {1, 3, 1, NUL, 1, 1, 1, 3});
        g.add(3, {1, 3, 2, 1, 1, 1, 1, 3});
        expect_row(fold(g, t, false), {1, 3, -1, NUL, 1, 1, 1, 3});
        g.add(3, {1, 2, 2, 1, 1, 1, 1, 3});  // retract for old sequence
        const Result r = fold(g, t, false);
        expect_row(r, {1, 3, -3, NUL, 1, 1, 1, 3});
        CHECK(r.kind == 0 && r.last == 8 && r.unsupported == 0);
    }
}

static int64_t range_min(int dt) {
    switch (dt) {
    case PAC_DT_INT8: return INT8_MIN;
    case PAC_DT_INT16: return INT16_MIN;
    case PAC_DT_INT32: return INT32_MIN;
    default: return INT64_MIN + 1;  // INT64_MIN is NUL in these tables
    }
}
static int64_t range_max(int dt) {
    switch (dt) {
    case PAC_DT_INT8: return INT8_MAX;
    case PAC_DT_INT16: return INT16_MAX;
    case PAC_DT_INT32: return INT32_MAX;
    default: return INT64_MAX;
    }
}

// columns: 0 group A sequence field; 1, 2 group B sequence fields; 3 group A
// aggregated; 4 group A without aggregator; 5 group B aggregated; 6 plain
static void check_random(std::mt19937_64 &rng) {
    const int aggs[] = {PAC_LAST_NON_NULL, PAC_LAST_VALUE, PAC_FIRST_VALUE,
                        PAC_FIRST_NON_NULL, PAC_SUM, PAC_MAX, PAC_MIN};
    const int dts[] = {PAC_DT_INT8,  PAC_DT_INT16,   PAC_DT_INT32,
                       PAC_DT_INT64, PAC_DT_FLOAT32, PAC_DT_FLOAT64};
    for (int agg : aggs)
        for (int dt : dts)
            for (int ign = 0; ign < 2; ign++)
                for (int trial = 0; trial < 24; trial++) {
                    const int n =
                        trial == 0 ? 32 : trial == 1 ? 2 : 2 + (int)(rng() % 31);
                    const bool ignore_delete = trial % 4 == 3;
                    const int code = agg | (ign ? PAC_IGNORE_RETRACT : 0);
                    Tables t;
                    t.dtypes = {PAC_DT_INT32, PAC_DT_INT32, PAC_DT_INT32,
                                (uint8_t)dt,  PAC_DT_INT32, (uint8_t)dt,
                                PAC_DT_INT32};
                    t.col_group = {0, 1, 1, 0, 0, 1, 0xff};
                    t.sg_fields = {0, -1, -1, -1, 1, 2, -1, -1};
                    t.sg_nseq = {1, 2};
                    t.col_agg = {PAC_NONE,      PAC_NONE, PAC_NONE,
                                 (uint8_t)code, PAC_NONE, (uint8_t)code,
                                 PAC_NONE};
                    Group g{7, {}, {}, {}};
                    bool any_retract_acts = false;
                    for (int x = 0; x < n; x++) {
                        std::vector<int64_t> row(7);
                        for (int c = 0; c < 7; c++) {
                            if (rng() % 100 < 35) {
                                row[c] = NUL;
                            } else if (c == 3 || c == 5) {
                                if (dt == PAC_DT_FLOAT32)
                                    row[c] = pac_f32_bits(
                                        (float)(rng() % 2000) / 7.f - 100.f);
                                else if (dt == PAC_DT_FLOAT64)
                                    row[c] = pac_f64_bits(
                                        (double)(rng() % 2000) / 7. - 100.);
                                else if (rng() % 3 == 0)
                                    row[c] = rng() % 2 ? range_min(dt)
                                                       : range_max(dt);
                                else
                                    row[c] = (int64_t)(rng() % 120) - 60;
                            } else {
                                row[c] = (int64_t)(rng() % 4);
                            }
                        }
                        const int kind = (int)(rng() % 4);
                        if ((kind & 1) && !ignore_delete &&
                            (row[0] != NUL || row[1] != NUL || row[2] != NUL))
                            any_retract_acts = true;
                        g.add(kind, row);
                    }
                    const Result r = fold(g, t, ignore_delete);
                    // a retraction is refused only by an aggregator without
                    // retract(), only without ignore-retract, and only when
                    // a retract with a non-empty tuple acts
                    const bool can_refuse =
                        !ign && (agg == PAC_MAX || agg == PAC_MIN ||
                                 agg == PAC_FIRST_VALUE ||
                                 agg == PAC_FIRST_NON_NULL);
                    if (!can_refuse || !any_retract_acts)
                        CHECK(r.unsupported == 0);
                    bool has_add = false;
                    for (int8_t k : g.kinds) has_add |= !(k & 1);
                    CHECK(r.kind == (has_add ? 0 : 3));
                    CHECK(r.last >= -1 && r.last < n);
                    if (!ignore_delete) CHECK(r.last == n - 1);
                    // a null result carries zero bits; an integer result
                    // lies inside its column's range
                    for (int c = 0; c < 7; c++) {
                        if (!r.valid[c]) CHECK(r.values[c] == 0);
                        if (r.valid[c] && (c == 3 || c == 5) &&
                            dt <= PAC_DT_INT32)
                            CHECK(r.values[c] >= range_min(dt) &&
                                  r.values[c] <= range_max(dt));
                    }
                }
}

int main() {
    check_vectors();
    std::mt19937_64 rng(20240611);
    check_random(rng);
    if (failures) {
        fprintf(stderr, "pu_agg_hostcheck: %d failure(s)\n", failures);
        return 1;
    }
    printf("pu_agg_hostcheck OK\n");
    return 0;
}
