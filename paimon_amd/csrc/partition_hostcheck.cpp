// Stand-alone host check of the partition search core, meant to be built with
// -fsanitize=address,undefined (make hostcheck): ppc_host_partition over
// random and edge-shaped runs held in exactly-sized heap blocks (so a probe
// one element past a run is an ASan report; empty runs pass a null pointer),
// against a k-way merge written out longhand. No GPU, no HIP.
#include "partition_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static uint64_t bias(int64_t v) { return (uint64_t)v ^ 0x8000000000000000ull; }

// cuts by a plain k-way merge in (key, run) order
static std::vector<int32_t> model(const std::vector<std::vector<int64_t>> &runs,
                                  int64_t tile_rows, int64_t n_bounds) {
    const int k = (int)runs.size();
    std::vector<int32_t> at(k, 0), cuts((size_t)n_bounds * k, 0);
    int64_t taken = 0, b = 1;
    for (;;) {
        if (b < n_bounds && (taken == b * tile_rows)) {
            memcpy(&cuts[(size_t)b * k], at.data(), k * 4);
            b++;
            continue;
        }
        int best = -1;
        for (int r = 0; r < k; r++)
            if (at[r] < (int32_t)runs[r].size() &&
                (best < 0 || bias(runs[r][at[r]]) < bias(runs[best][at[best]])))
                best = r;
        if (best < 0) break;
        at[best]++;
        taken++;
    }
    for (; b < n_bounds; b++) memcpy(&cuts[(size_t)b * k], at.data(), k * 4);
    return cuts;
}

static void check(const std::vector<std::vector<int64_t>> &runs, int key_width,
                  int64_t tile_rows) {
    const int k = (int)runs.size();
    std::vector<void *> heap(k, nullptr);
    std::vector<int64_t> lens(k);
    int64_t total = 0;
    for (int r = 0; r < k; r++) {
        lens[r] = (int64_t)runs[r].size();
        total += lens[r];
        if (!lens[r]) continue;
        heap[r] = malloc((size_t)lens[r] * key_width);
        for (int64_t i = 0; i < lens[r]; i++)
            if (key_width == 8) ((int64_t *)heap[r])[i] = runs[r][i];
            else ((int32_t *)heap[r])[i] = (int32_t)runs[r][i];
    }
    const int64_t n_bounds = (total + tile_rows - 1) / tile_rows + 1;
    const std::vector<int32_t> want = model(runs, tile_rows, n_bounds);
    // both level rules: coarse stride 16 where there are enough bounds, and
    // one full-width window per bound
    const int64_t gs[2] = {n_bounds > 17 ? 16 : 1,
                           n_bounds > 1 ? n_bounds - 1 : 1};
    for (int64_t G : gs) {
        int32_t *cuts = (int32_t *)malloc((size_t)n_bounds * k * 4);
        ppc_host_partition(k, heap.data(), lens.data(), key_width, tile_rows,
                           n_bounds, total, G, cuts);
        CHECK(memcmp(cuts, want.data(), (size_t)n_bounds * k * 4) == 0);
        free(cuts);
    }
    for (void *p : heap) free(p);
}

// n sorted unique keys: start + a running sum of steps in [1, max_step]
static std::vector<int64_t> draw(std::mt19937_64 &rng, int64_t start, int n,
                                 uint64_t max_step) {
    std::vector<int64_t> v(n);
    uint64_t x = (uint64_t)start;
    for (int i = 0; i < n; i++) {
        x += 1 + rng() % max_step;
        v[i] = (int64_t)x;
    }
    return v;
}

int main() {
    std::mt19937_64 rng(12345);
    const int ks[] = {1, 2, 3, 4, 5, 8, 9, 16, 17, 32};
    for (int k : ks)
        for (int key_width : {8, 4}) {
            // dense overlapping runs of uneven length, some empty or 1 long
            std::vector<std::vector<int64_t>> runs(k);
            for (int r = 0; r < k; r++) {
                int n = 250 + (int)(rng() % 150);
                if (k > 2 && r == k / 2) n = 0;
                if (k > 3 && r == k - 1) n = 1;
                runs[r] = draw(rng, -500, n, 3 * k);
            }
            check(runs, key_width, 64);
            check(runs, key_width, 3584);
            // every run the same keys: bounds fall inside groups
            std::vector<std::vector<int64_t>> same(k, draw(rng, -100, 200, 5));
            check(same, key_width, 64);
            // disjoint runs: empty refine windows
            std::vector<std::vector<int64_t>> dis(k);
            for (int r = 0; r < k; r++)
                dis[r] = draw(rng, (int64_t)r * 10000, 120, 20);
            check(dis, key_width, 64);
            // all but one run empty
            std::vector<std::vector<int64_t>> one(k);
            one[k - 1] = draw(rng, 0, 1500, 4);
            check(one, key_width, 64);
        }
    // key-domain edges: the whole int64 range, and the whole int32 range
    for (int k : {3, 8, 17}) {
        std::vector<std::vector<int64_t>> wide(k), wide32(k);
        for (int r = 0; r < k; r++) {
            wide[r] = draw(rng, INT64_MIN, 300, (uint64_t)1 << 54);
            wide[r].front() = INT64_MIN;
            wide[r].back() = INT64_MAX;
            wide32[r] = draw(rng, INT32_MIN, 300, (uint64_t)1 << 22);
            wide32[r].front() = INT32_MIN;
            wide32[r].back() = INT32_MAX;
        }
        check(wide, 8, 64);
        check(wide32, 4, 64);
    }
    if (failures) {
        fprintf(stderr, "partition_hostcheck: %d failure(s)\n", failures);
        return 1;
    }
    printf("partition_hostcheck OK\n");
    return 0;
}
