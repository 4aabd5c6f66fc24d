// Point lookup into sorted key runs — the search core of the lookup
// changelog producer (LookupLevels.lookup via LookupUtils.lookup,
// mergetree/LookupUtils.java:35-57: levels are searched in ascending order
// and the first level that holds the key wins).
//
// Shared scalar core, like zstd_core.h: k_lookup_probe (kernels.hip) and the
// host entry pmh_debug_lookup_probe (plan.cpp) run exactly this code, so the
// CPU tests pin what the kernel executes.
//
// The search is two-level, following the partition kernels: a block of
// probe keys first bounds ONE window per level from its smallest and largest
// key (plk_window), then every probe bisects only inside that window
// (plk_probe). Probe keys arrive sorted, so a block's window is a small
// slice of the level and the per-probe bisections stay cache-resident.
#ifndef PMH_LOOKUP_CORE_H
#define PMH_LOOKUP_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define PLK_HD __host__ __device__ inline
#else
#define PLK_HD inline
#endif

// probe keys handled per block-level window (k_lookup_probe: one workgroup
// iteration; the host entry walks its queries in chunks of the same size)
constexpr int PLK_CHUNK = 1024;
constexpr uint32_t PLK_MISS = 0xFFFFFFFFu;

// One sorted lookup level: `rows` ascending unique keys of stored width
// `esize` (4 or 8 bytes — TINYINT..INT keys stage as INT32, BIGINT as INT64).
struct PlkLevel {
    uint64_t keys;  // address of element 0
    int64_t rows;
    int32_t esize;
    int32_t pad;
};

PLK_HD int64_t plk_key_at(uint64_t base, int64_t i, int es) {
    return es == 8 ? *reinterpret_cast<const int64_t *>(base + (uint64_t)i * 8)
                   : (int64_t) *
                         reinterpret_cast<const int32_t *>(base +
                                                           (uint64_t)i * 4);
}

// first index in [lo, hi) whose key is >= q (hi when none)
PLK_HD int64_t plk_lower_bound(const PlkLevel &lv, int64_t lo, int64_t hi,
                               int64_t q) {
    while (lo < hi) {
        int64_t mid = lo + ((hi - lo) >> 1);
        if (plk_key_at(lv.keys, mid, lv.esize) < q) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// first index in [lo, hi) whose key is > q (hi when none)
PLK_HD int64_t plk_upper_bound(const PlkLevel &lv, int64_t lo, int64_t hi,
                               int64_t q) {
    while (lo < hi) {
        int64_t mid = lo + ((hi - lo) >> 1);
        if (plk_key_at(lv.keys, mid, lv.esize) <= q) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Window of one level that can hold any key in [kmin, kmax]: every probe of
// the block searches only [*wlo, *whi).
PLK_HD void plk_window(const PlkLevel &lv, int64_t kmin, int64_t kmax,
                       int64_t *wlo, int64_t *whi) {
    int64_t lo = plk_lower_bound(lv, 0, lv.rows, kmin);
    *wlo = lo;
    *whi = plk_upper_bound(lv, lo, lv.rows, kmax);
}

// Probe one key: levels in ascending order, first hit wins. Returns the
// level index and writes the row inside it, or -1 when no level holds q.
PLK_HD int plk_probe(const PlkLevel *lv, int n_levels, const int64_t *wlo,
                     const int64_t *whi, int64_t q, int64_t *row) {
    for (int l = 0; l < n_levels; l++) {
        int64_t i = plk_lower_bound(lv[l], wlo[l], whi[l], q);
        if (i < whi[l] && plk_key_at(lv[l].keys, i, lv[l].esize) == q) {
            *row = i;
            return l;
        }
    }
    return -1;
}

#endif  // PMH_LOOKUP_CORE_H
