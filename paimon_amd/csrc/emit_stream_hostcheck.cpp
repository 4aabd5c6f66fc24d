// Stand-alone host check of k_emit_stream's slot mapping and group plan
// (emit_stream_core.h), meant to be built with -fsanitize=address,undefined
// (make hostcheck). Tiles are generated the way the partition cuts them:
// per-run cut sequences that rise monotonically and sum to b * tile_rows.
// Checked per tile: slot -> (run, row) -> slot is the identity on [0, M);
// every (run, row) a winner may name maps inside [0, M), each to its own
// slot; M never exceeds the tile maximum. No GPU, no HIP.
#include "emit_stream_core.h"

#include <cstdio>
#include <cstdlib>
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

// the merge's tile geometry (kernels.h)
static const int MAX_RUNS = 32;
static const int64_t TILE_ROWS = 3584;
static const int TILE_MAX = (int)TILE_ROWS + MAX_RUNS;

// cuts[(b * k) + r] for b = 0 .. n_tiles: how many of run r's rows lie in
// the first min(b * TILE_ROWS, total) merged rows. `skew` > 0 lets a run
// drain early or sit out whole tiles (empty slices).
static std::vector<int32_t> gen_cuts(const std::vector<int64_t> &lens,
                                     std::mt19937_64 &rng, int skew) {
    const int k = (int)lens.size();
    int64_t total = 0;
    for (int64_t l : lens) total += l;
    const int64_t n_tiles = total ? (total + TILE_ROWS - 1) / TILE_ROWS : 1;
    std::vector<int32_t> cuts((size_t)(n_tiles + 1) * k, 0);
    std::vector<int64_t> at(k, 0);
    for (int64_t b = 1; b <= n_tiles; b++) {
        int64_t want = b * TILE_ROWS < total ? TILE_ROWS
                                             : total - (b - 1) * TILE_ROWS;
        while (want > 0) {
            // a weighted pick among the runs that still have rows
            int r = (int)(rng() % k);
            if (skew && (rng() % (unsigned)(skew + 1)))
                r = (int)(rng() % (unsigned)((k + 1) / 2));
            if (at[r] >= lens[r]) {
                r = -1;
                for (int q = 0; q < k; q++)
                    if (at[q] < lens[q]) r = q;
                if (r < 0) break;
            }
            int64_t take = 1 + (int64_t)(rng() % 97);
            if (take > want) take = want;
            if (take > lens[r] - at[r]) take = lens[r] - at[r];
            at[r] += take;
            want -= take;
        }
        for (int r = 0; r < k; r++) cuts[(size_t)b * k + r] = (int32_t)at[r];
    }
    return cuts;
}

template <int KM>
static void check_tiles(const std::vector<int64_t> &lens,
                        const std::vector<int32_t> &cuts) {
    const int k = (int)lens.size();
    const int64_t n_tiles = (int64_t)cuts.size() / k - 1;
    CHECK(k <= KM);
    // exactly-sized heap copies: a read past k entries is an ASan report
    std::vector<int64_t> hl(lens);
    for (int64_t t = 0; t < n_tiles; t++) {
        std::vector<int32_t> c0(cuts.begin() + t * k,
                                cuts.begin() + (t + 1) * k);
        std::vector<int32_t> c1(cuts.begin() + (t + 1) * k,
                                cuts.begin() + (t + 2) * k);
        EscTile<KM> ts;
        esc_tile_setup<KM>(c0.data(), c1.data(), hl.data(), k, ts);
        const int32_t M = ts.mtotal;
        CHECK(M >= 0 && M <= TILE_MAX);
        int64_t real = 0, ext = 0;
        for (int r = 0; r < k; r++) {
            real += c1[r] - c0[r];
            ext += c1[r] < lens[r] ? 1 : 0;
        }
        CHECK(ts.mreal == real);
        CHECK(M == real + ext);
        CHECK(real <= TILE_ROWS);
        // staging side: slot -> (run, row) -> slot
        for (int32_t e = 0; e < M; e++) {
            int run = -1;
            uint32_t row = 0;
            esc_slot_source<KM>(ts, k, e, &run, &row);
            CHECK(run >= 0 && run < k);
            if (run < 0 || run >= k) continue;
            CHECK((int64_t)row >= c0[run] && (int64_t)row <= c1[run]);
            CHECK((int64_t)row < lens[run]);
            CHECK(esc_winner_slot<KM>(ts, (uint32_t)run, row) == e);
        }
        // permute side: everything a winner may name, each its own slot
        std::vector<uint8_t> hit((size_t)M, 0);
        int64_t named = 0;
        for (int r = 0; r < k; r++) {
            for (int64_t row = c0[r]; row <= c1[r] && row < lens[r]; row++) {
                const int32_t s =
                    esc_winner_slot<KM>(ts, (uint32_t)r, (uint32_t)row);
                CHECK(s >= 0 && s < M);
                if (s < 0 || s >= M) continue;
                CHECK(!hit[(size_t)s]);
                hit[(size_t)s] = 1;
                named++;
            }
        }
        CHECK(named == M);
    }
}

static void check_runs(const std::vector<int64_t> &lens,
                       const std::vector<int32_t> &cuts) {
    const int k = (int)lens.size();
    if (k <= 4) check_tiles<4>(lens, cuts);
    if (k <= 8) check_tiles<8>(lens, cuts);
    if (k <= 16) check_tiles<16>(lens, cuts);
    check_tiles<32>(lens, cuts);
}

static void tiles() {
    std::mt19937_64 rng(20240611);
    const int ks[] = {1, 2, 3, 8, 32};
    for (int k : ks) {
        for (int rep = 0; rep < 6; rep++) {
            std::vector<int64_t> lens(k);
            for (int r = 0; r < k; r++)
                lens[r] = (int64_t)(rng() % (rep < 2 ? 300 : 9000));
            if (rep == 3) lens[0] = 1;             // a run of a single row
            if (rep == 4) lens[k - 1] = 0;         // an empty run
            if (rep == 5 && k > 1) lens[1] = 20000;  // one long run
            check_runs(lens, gen_cuts(lens, rng, rep >= 3 ? 3 : 0));
        }
    }
    {
        // exact tile multiples and one row past them (last partial tile)
        const int64_t totals[] = {TILE_ROWS, TILE_ROWS + 1, 2 * TILE_ROWS, 100};
        for (int64_t tot : totals) {
            std::vector<int64_t> one{tot};
            check_runs(one, gen_cuts(one, rng, 0));
            std::vector<int64_t> three{1, tot / 2, tot - tot / 2 - 1};
            check_runs(three, gen_cuts(three, rng, 2));
        }
    }
    {
        // M = the tile maximum: 32 runs share a full tile evenly and every
        // one of them goes on; the second tile ends every run (no extension)
        const int k = MAX_RUNS;
        const int64_t per = TILE_ROWS / k;  // 112
        std::vector<int64_t> lens(k, 2 * per);
        std::vector<int32_t> cuts((size_t)3 * k, 0);
        for (int r = 0; r < k; r++) {
            cuts[(size_t)k + r] = (int32_t)per;
            cuts[(size_t)2 * k + r] = (int32_t)(2 * per);
        }
        check_tiles<32>(lens, cuts);
        EscTile<32> ts;
        esc_tile_setup<32>(cuts.data(), cuts.data() + k, lens.data(), k, ts);
        CHECK(ts.mtotal == TILE_MAX);
        esc_tile_setup<32>(cuts.data() + k, cuts.data() + 2 * k, lens.data(),
                           k, ts);
        CHECK(ts.mtotal == TILE_ROWS);
    }
    {
        // a run that ends inside the tile next to one that goes on
        std::vector<int64_t> lens{10, 5000};
        std::vector<int32_t> cuts{0, 0, 10, 3574, 10, 5000};
        check_runs(lens, cuts);
    }
}

static void check_plan(const std::vector<uint8_t> &cls,
                       const std::vector<uint8_t> *valid, int64_t budget,
                       int max4, int max8) {
    const int n = (int)cls.size();
    std::vector<uint16_t> bound((size_t)n + 1, 0xffff);
    const int g = esc_plan_groups(cls.data(), valid ? valid->data() : nullptr,
                                  n, TILE_MAX, budget, max4, max8,
                                  bound.data());
    bool fits = true;  // does every single column fit on its own?
    for (int i = 0; i < n; i++)
        fits = fits &&
               esc_col_bytes(cls[i], valid ? (*valid)[i] : 0, TILE_MAX) <=
                   budget;
    if (!fits) {
        CHECK(g == -1);
        return;
    }
    CHECK(g >= (n ? 1 : 0) && g <= n);
    if (g < 0) return;
    CHECK(bound[0] == 0 && bound[(size_t)g] == n);
    for (int i = 0; i < g; i++) {
        const int lo = bound[(size_t)i], hi = bound[(size_t)i + 1];
        CHECK(lo < hi && hi <= n);  // every column in exactly one group
        if (!(lo < hi && hi <= n)) return;
        int64_t bytes = 0;
        for (int c = lo; c < hi; c++) {
            CHECK(cls[c] == cls[lo]);
            bytes += esc_col_bytes(cls[c], valid ? (*valid)[c] : 0, TILE_MAX);
        }
        CHECK(bytes <= budget);
        CHECK(hi - lo <= (esc_stored_width(cls[lo]) == 8 ? max8 : max4));
    }
}

static void plans() {
    std::mt19937_64 rng(7);
    const int ns[] = {1, 12, 13, 256};
    const int64_t budgets[] = {1000,       (int64_t)TILE_MAX * 4,
                               (int64_t)TILE_MAX * 8, 60 * 1024,
                               (int64_t)TILE_MAX * 32 + 5};
    const int caps[][2] = {{2, 1}, {4, 2}, {8, 4}};
    for (int n : ns) {
        for (int rep = 0; rep < 4; rep++) {
            // list order: classes ascend
            std::vector<uint8_t> cls((size_t)n), valid((size_t)n);
            const uint8_t widths[] = {1, 2, 4, 8};
            for (int i = 0; i < n; i++) {
                cls[(size_t)i] =
                    rep == 0 ? 4 : widths[(size_t)i * 4 / (size_t)n];
                if (rep == 2) cls[(size_t)i] = i < n / 3 ? 4 : 8;
                valid[(size_t)i] = (uint8_t)(rng() & 1);
            }
            for (int64_t b : budgets)
                for (const auto &cp : caps) {
                    check_plan(cls, nullptr, b, cp[0], cp[1]);
                    check_plan(cls, &valid, b, cp[0], cp[1]);
                }
        }
    }
    // the flagship's lists at the default budget: kind | 8 x int32 | 3 x int64
    std::vector<uint8_t> cls{1, 4, 4, 4, 4, 4, 4, 4, 4, 8, 8, 8};
    uint16_t bound[13];
    CHECK(esc_plan_groups(cls.data(), nullptr, 12, TILE_MAX, 60 * 1024, 4, 2,
                          bound) == 5);
    CHECK(bound[1] == 1 && bound[2] == 5 && bound[3] == 9 && bound[4] == 11 &&
          bound[5] == 12);
}

int main() {
    tiles();
    plans();
    if (failures) {
        fprintf(stderr, "emit_stream_hostcheck: %d failure(s)\n", failures);
        return 1;
    }
    printf("emit_stream_hostcheck OK\n");
    return 0;
}
