// Merge-path partition over k sorted key runs — the search core of
// k_partition_wave / k_partition_refine.
//
// Shared core, like lookup_core.h and zstd_core.h: the kernels (kernels.hip)
// and the host mode of pmh_debug_partition (plan.cpp) run exactly this code,
// so the CPU tests pin what the kernels execute. The device build loads
// through the global address space (global_load_*), the host build reads
// plain memory.
//
// Contract: bound b is the prefix of length D = min(b * tile_rows, total) of
// all rows ordered by (unsigned-biased key, run index); cuts[b * k + r] is
// the number of run r's rows in that prefix; ties are taken in run order.
//
// The partition's wall-clock is one chain of dependent loads, so everything
// here is shaped to keep that chain short: one search step issues the probes
// of ALL runs back to back and waits once. That needs straight-line code
// between the loads — no per-run condition around a load (the compiler would
// branch around each one and drain the memory counter after it). Hence:
//  - the key width ES is a template parameter;
//  - every run probes every step: a finished or empty window probes row 0,
//    which exists in every column it can be asked of (see ppc_safe_addrs),
//    and ignores the result;
//  - slots r >= k of a KM-wide instantiation are ordinary empty runs;
//  - window state is 32-bit (a run holds < 2^27 rows by the winner packing),
//    which keeps KM = 16 / 32 in registers.
#ifndef PMH_PARTITION_CORE_H
#define PMH_PARTITION_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define PPC_HD __host__ __device__ __forceinline__
#else
#define PPC_HD inline
#endif
#if defined(__clang__)  // the per-run loops must unroll: arrays in registers
#define PPC_UNROLL _Pragma("unroll")
#else
#define PPC_UNROLL
#endif

template <typename T>
PPC_HD T ppc_load(uint64_t addr) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *reinterpret_cast<const __attribute__((address_space(1))) T *>(
        addr);
#else
    return *reinterpret_cast<const T *>((uintptr_t)addr);
#endif
}

// unsigned-biased key of row idx (stored width ES = 4 or 8 bytes)
template <int ES>
PPC_HD uint64_t ppc_ukey_at(uint64_t base, uint32_t idx) {
    int64_t v;
    if (ES == 8) v = ppc_load<int64_t>(base + (uint64_t)idx * 8);
    else v = (int64_t)ppc_load<int32_t>(base + (uint64_t)idx * 4);
    return (uint64_t)v ^ 0x8000000000000000ull;
}

PPC_HD int ppc_bits32(uint32_t x) {  // 32 - clz(x), 0 for x == 0
#if defined(__HIP_DEVICE_COMPILE__)
    return 32 - __clz((int)x);
#else
    return x ? 32 - __builtin_clz(x) : 0;
#endif
}

// Give every empty slot (len[r] == 0: an empty run, whose address may be
// null, or a slot r >= k) the address of the first non-empty run, so that a
// probe of row 0 reads a real row in EVERY slot. Needs one non-empty run.
template <int KM>
PPC_HD void ppc_safe_addrs(uint64_t *addr, const uint32_t *len) {
    uint64_t safe = 0;
    PPC_UNROLL
    for (int r = KM - 1; r >= 0; r--) safe = len[r] > 0 ? addr[r] : safe;
    PPC_UNROLL
    for (int r = 0; r < KM; r++) addr[r] = len[r] > 0 ? addr[r] : safe;
}

// Lockstep multi-run bound: the KM binary searches advance together, one
// probe per run per step, all of a step's loads issued before the first
// compare. LE: first index in [lo, hi) with ukey > v; else with ukey >= v.
// The trip count comes from the widest window (a window of n rows is done
// after bits(n) halvings); narrower windows finish early and then probe
// row 0 of their (safe) column. On the device the count is per lane: the
// wave runs to its largest count with the finished lanes masked off, and
// the loop holds no other branch (in k_partition_wave all lanes of a wave
// share their windows, so the count is uniform there).
template <bool LE, int ES, int KM>
PPC_HD void ppc_bound_multi(const uint64_t *addr, const uint32_t *lo_in,
                            const uint32_t *hi_in, uint64_t v,
                            uint32_t *out) {
    uint32_t lo[KM], n[KM];
    uint32_t widest = 0;
    PPC_UNROLL
    for (int r = 0; r < KM; r++) {
        lo[r] = lo_in[r];
        n[r] = hi_in[r] > lo_in[r] ? hi_in[r] - lo_in[r] : 0u;
        widest |= n[r];
    }
    const int steps = ppc_bits32(widest);
    for (int s = 0; s < steps; s++) {
        uint64_t kk[KM];
        PPC_UNROLL
        for (int r = 0; r < KM; r++) {
            const uint32_t idx = n[r] > 0 ? lo[r] + (n[r] >> 1) : 0u;
            kk[r] = ppc_ukey_at<ES>(addr[r], idx);
        }
        PPC_UNROLL
        for (int r = 0; r < KM; r++) {
            const uint32_t half = n[r] >> 1;
            const bool go = (LE ? (kk[r] <= v) : (kk[r] < v)) && n[r] > 0;
            lo[r] = go ? lo[r] + half + 1 : lo[r];
            n[r] = go ? n[r] - half - 1 : half;
        }
    }
    PPC_UNROLL
    for (int r = 0; r < KM; r++) out[r] = lo[r];
}

// Smallest and largest key over the non-empty windows [wlo, whi): all 2*KM
// edge keys load together. Returns klo > khi when every window is empty.
template <int ES, int KM>
PPC_HD void ppc_window_keys(const uint64_t *addr, const uint32_t *wlo,
                            const uint32_t *whi, uint64_t *klo,
                            uint64_t *khi) {
    uint64_t a[KM], z[KM];
    PPC_UNROLL
    for (int r = 0; r < KM; r++) {
        const bool ne = wlo[r] < whi[r];
        a[r] = ppc_ukey_at<ES>(addr[r], ne ? wlo[r] : 0u);
        z[r] = ppc_ukey_at<ES>(addr[r], ne ? whi[r] - 1 : 0u);
    }
    uint64_t lo = ~0ull, hi = 0;
    PPC_UNROLL
    for (int r = 0; r < KM; r++) {
        const bool ne = wlo[r] < whi[r];
        lo = ne && a[r] < lo ? a[r] : lo;
        hi = ne && z[r] > hi ? z[r] : hi;
    }
    *klo = lo;
    *khi = hi;
}

// Tie-take finish: v is the key of the D-th row. Rows below v are all in;
// of the rows equal to v (at most one per run) the first D - base in run
// order are. The KM candidate keys load together before the serial walk.
template <int ES, int KM>
PPC_HD void ppc_tie_finish(const uint64_t *addr, const uint32_t *len,
                           const uint32_t *wlo, const uint32_t *whi,
                           uint64_t v, int64_t D, uint32_t *c) {
    ppc_bound_multi<false, ES, KM>(addr, wlo, whi, v, c);
    int64_t base = 0;
    uint64_t ck[KM];
    PPC_UNROLL
    for (int r = 0; r < KM; r++) {
        base += c[r];
        ck[r] = ppc_ukey_at<ES>(addr[r], c[r] < len[r] ? c[r] : 0u);
    }
    int64_t t = D - base;
    PPC_UNROLL
    for (int r = 0; r < KM; r++) {
        const bool take = t > 0 && c[r] < len[r] && ck[r] == v;
        c[r] += take ? 1u : 0u;
        t -= take ? 1 : 0;
    }
}

// One interior bound, bisected on the key domain inside the windows given by
// two enclosing bounds whose cuts are known: cuts_g0 below, cuts_g1 above
// (k entries each; full-width windows are cuts_g0 = zeros, cuts_g1 = lens).
// 0 < D < total. addr must have been through ppc_safe_addrs; len[r] == 0
// for r >= k. Writes the k cuts of this bound to cuts_b.
template <int ES, int KM>
PPC_HD void ppc_refine_bound(const uint64_t *addr, const uint32_t *len, int k,
                             int64_t D, const int32_t *cuts_g0,
                             const int32_t *cuts_g1, int32_t *cuts_b) {
    uint32_t wlo[KM], whi[KM], pos[KM];
    // all 2*KM window loads together; slots r >= k re-read slot 0 and drop it
    PPC_UNROLL
    for (int r = 0; r < KM; r++) {
        const int rr = r < k ? r : 0;
        wlo[r] = (uint32_t)ppc_load<int32_t>((uint64_t)(uintptr_t)(cuts_g0 + rr));
        whi[r] = (uint32_t)ppc_load<int32_t>((uint64_t)(uintptr_t)(cuts_g1 + rr));
    }
    PPC_UNROLL
    for (int r = 0; r < KM; r++) {
        wlo[r] = r < k ? wlo[r] : 0u;
        whi[r] = r < k ? whi[r] : 0u;
    }
    uint64_t klo, khi;
    ppc_window_keys<ES, KM>(addr, wlo, whi, &klo, &khi);
    if (khi < klo) {  // every window empty: the lower cuts already sum to D
    PPC_UNROLL
        for (int r = 0; r < KM; r++)
            if (r < k) cuts_b[r] = (int32_t)wlo[r];
        return;
    }
    while (klo < khi) {
        const uint64_t mid = klo + ((khi - klo) >> 1);
        ppc_bound_multi<true, ES, KM>(addr, wlo, whi, mid, pos);
        int64_t cnt = 0;
    PPC_UNROLL
        for (int r = 0; r < KM; r++) cnt += pos[r];
        const bool up = cnt >= D;
        khi = up ? mid : khi;
        klo = up ? klo : mid + 1;
    PPC_UNROLL
        for (int r = 0; r < KM; r++) {
            whi[r] = up ? pos[r] : whi[r];
            wlo[r] = up ? wlo[r] : pos[r];
        }
    }
    ppc_tie_finish<ES, KM>(addr, len, wlo, whi, klo, D, pos);
    PPC_UNROLL
    for (int r = 0; r < KM; r++)
        if (r < k) cuts_b[r] = (int32_t)pos[r];
}

// ---------------------------------------------------------------- host walk
//
// The whole partition on the host (mode 0 of pmh_debug_partition and the
// stand-alone sanitizer check): the end bounds are seeded, every G-th bound
// is refined inside full-width windows (the wave kernel's job on the
// device), the interior bounds inside their enclosing coarse cuts — the
// routine and the search k_partition_refine runs.
constexpr int PPC_MAX_RUNS = 32;

template <int ES, int KM>
inline void ppc_host_walk(int k, const void *const *keys, const int64_t *lens,
                          int64_t tile_rows, int64_t n_bounds, int64_t total,
                          int64_t G, int32_t *cuts) {
    uint64_t addr[KM];
    uint32_t len[KM];
    for (int r = 0; r < KM; r++) {
        addr[r] = r < k ? (uint64_t)(uintptr_t)keys[r] : 0;
        len[r] = r < k ? (uint32_t)lens[r] : 0u;
    }
    int32_t *last = cuts + (n_bounds - 1) * k;
    for (int r = 0; r < k; r++) {
        cuts[r] = 0;
        last[r] = (int32_t)lens[r];
    }
    if (total == 0) return;
    ppc_safe_addrs<KM>(addr, len);
    for (int64_t b = G; b < n_bounds - 1; b += G)
        ppc_refine_bound<ES, KM>(addr, len, k, b * tile_rows, cuts, last,
                                 cuts + b * k);
    for (int64_t b = 1; b < n_bounds - 1; b++) {
        if (b % G == 0) continue;
        const int64_t g0 = (b / G) * G;
        const int64_t g1 = g0 + G < n_bounds - 1 ? g0 + G : n_bounds - 1;
        ppc_refine_bound<ES, KM>(addr, len, k, b * tile_rows, cuts + g0 * k,
                                 cuts + g1 * k, cuts + b * k);
    }
}

template <int ES>
inline void ppc_host_walk_k(int k, const void *const *keys,
                            const int64_t *lens, int64_t tile_rows,
                            int64_t n_bounds, int64_t total, int64_t G,
                            int32_t *cuts) {
    // the launcher's instantiations (pmh_launch_partition)
    if (k <= 4)
        ppc_host_walk<ES, 4>(k, keys, lens, tile_rows, n_bounds, total, G,
                             cuts);
    else if (k <= 8)
        ppc_host_walk<ES, 8>(k, keys, lens, tile_rows, n_bounds, total, G,
                             cuts);
    else if (k <= 16)
        ppc_host_walk<ES, 16>(k, keys, lens, tile_rows, n_bounds, total, G,
                              cuts);
    else
        ppc_host_walk<ES, PPC_MAX_RUNS>(k, keys, lens, tile_rows, n_bounds,
                                        total, G, cuts);
}

// 1 <= k <= PPC_MAX_RUNS, key_width 4 | 8, cuts holds n_bounds * k entries.
inline void ppc_host_partition(int k, const void *const *keys,
                               const int64_t *lens, int key_width,
                               int64_t tile_rows, int64_t n_bounds,
                               int64_t total, int64_t G, int32_t *cuts) {
    if (key_width == 8)
        ppc_host_walk_k<8>(k, keys, lens, tile_rows, n_bounds, total, G, cuts);
    else
        ppc_host_walk_k<4>(k, keys, lens, tile_rows, n_bounds, total, G, cuts);
}

#endif  // PMH_PARTITION_CORE_H
