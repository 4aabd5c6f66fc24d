// CDNA4 (gfx950) kernels for Paimon's merge-on-read hot path.
//
// MI355X-first design (NOT a translation of the reference's Java loops):
// the reference's LoserTree (mergetree/compact/LoserTree.java) stalls per
// key on a pointer-chasing tournament; here the same total order
// (ascending userKey, sequenceNumber, isAdd —
// SortMergeReaderWithLoserTree.java:48-75) is produced by a merge-path
// partition over k sorted runs into independent tiles, an LDS-staged
// pairwise-stable merge inside each tile, and a segmented winner reduction
// per equal-key group (DeduplicateMergeFunction.java:48-62 +
// ReducerMergeFunctionWrapper.java:53-73 + DropDeleteReader.java:53-61).
// This path is HBM-bandwidth-bound integer work: no MFMA, wide coalesced
// loads, LDS staging, grid-stride launches.
//
// Capacity limits (checked host-side): runs per section <= PMH_MAX_RUNS,
// rows per run < 2^PMH_ROW_BITS (packed winner format run:5 | row:27).

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <type_traits>

#include "../../include/paimon_hip.h"
#include "changelog_core.h"
#include "column_core.h"
#include "emit_stream_core.h"
#include "kernels.h"
#include "lookup_core.h"
#include "partition_core.h"
#include "pu_agg_core.h"
#include "zstd_core.h"

#define DEV __device__ __forceinline__

namespace pmh {

// ------------------------------------------------------------ column access

template <typename T>
DEV T col_load(const DevCol &c, int64_t row) {
    return *reinterpret_cast<const T *>(c.addr0 + (uint64_t)row * sizeof(T));
}

// validity byte of a row; a column without staged nulls is all valid
DEV uint8_t col_valid(const DevCol &c, int64_t row) {
    return c.valid0 ? ((const uint8_t *)c.valid0)[row] : 1;
}

// staged at 8 bytes; every other dtype is staged at 4 (pmh_stored_width)
DEV bool dt_wide(int dt) { return dt == PMH_DT_INT64 || dt == PMH_DT_FLOAT64; }

// a row's stored element as 64 bits (4-byte elements sign-extend)
DEV int64_t col_load_wide(const DevCol &c, int64_t row, int dt) {
    return dt_wide(dt) ? col_load<int64_t>(c, row)
                       : (int64_t)col_load<int32_t>(c, row);
}

// packed winner / member word (run:5 | row:27): its column descriptor and row
DEV const DevCol &member_col(const DevCol *cols, int n_cols, uint32_t m,
                             int c) {
    return cols[(m >> PMH_ROW_BITS) * n_cols + c];
}
DEV int64_t member_row(uint32_t m) { return m & PMH_ROW_MASK; }
// the word's column c: validity byte, and stored element as 64 bits
DEV uint8_t member_valid(const DevCol *cols, int n_cols, uint32_t m, int c) {
    return col_valid(member_col(cols, n_cols, m, c), member_row(m));
}
DEV int64_t member_load(const DevCol *cols, int n_cols, uint32_t m, int c,
                        int dt) {
    return col_load_wide(member_col(cols, n_cols, m, c), member_row(m), dt);
}
// its row's packed validity mask (k_pack_valid: bit c = column c non-null)
DEV uint64_t member_mask(uint64_t *const *run_masks, uint32_t m) {
    return run_masks[m >> PMH_ROW_BITS][m & PMH_ROW_MASK];
}

// out[i] = bits, narrowed to the column's output width (pmh_out_width)
DEV void out_store(void *out, int dt, int64_t i, int64_t bits) {
    switch (dt) {
    case PMH_DT_INT8: ((int8_t *)out)[i] = (int8_t)bits; break;
    case PMH_DT_INT16: ((int16_t *)out)[i] = (int16_t)bits; break;
    case PMH_DT_INT32:
    case PMH_DT_FLOAT32:
    case PMH_DT_STRING:  // string ids ride as int32
        ((int32_t *)out)[i] = (int32_t)bits;
        break;
    case PMH_DT_INT64:
    case PMH_DT_FLOAT64: ((int64_t *)out)[i] = bits; break;
    }
}

// Contiguous output slice [slice_lo, slice_hi) of this block: `total` rows
// dealt to the grid's blocks in equal shares (the last ones may be empty).
DEV int64_t slice_rows(int64_t total) {
    return (total + (int64_t)gridDim.x - 1) / (int64_t)gridDim.x;
}
DEV int64_t slice_lo_of(int64_t total) {
    return (int64_t)blockIdx.x * slice_rows(total);
}
DEV int64_t slice_hi_of(int64_t total) {
    const int64_t hi = slice_lo_of(total) + slice_rows(total);
    return hi < total ? hi : total;
}

// Tile cursor over tile_offsets (the exclusive scan of the tile counts):
// tile_seek finds the tile that owns output rank i; tile_walk advances a
// cursor t that is at or before that tile (ranks visited in ascending order).
DEV int64_t tile_seek(const int64_t *tile_offsets, int64_t n_tiles,
                      int64_t i) {
    int64_t lo = 0, hi = n_tiles - 1;
    while (lo < hi) {
        int64_t mid = (lo + hi + 1) >> 1;
        if (tile_offsets[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
DEV int64_t tile_walk(const int64_t *tile_offsets, int64_t n_tiles, int64_t t,
                      int64_t i) {
    while (t + 1 < n_tiles && tile_offsets[t + 1] <= i) t++;
    return t;
}

DEV uint64_t ukey(int64_t k) { return (uint64_t)k ^ 0x8000000000000000ull; }

// key column element (stored width 4 or 8 bytes — TINYINT..INT stage as
// INT32; the key TYPE is uniform across runs, so es is a scalar)
DEV int64_t key_at(uint64_t addr, int64_t idx, int es) {
    return es == 8 ? *reinterpret_cast<const int64_t *>(addr + idx * 8)
                   : (int64_t)*reinterpret_cast<const int32_t *>(addr +
                                                                 idx * 4);
}

// The lockstep multi-run search (ppc_bound_multi), the edge-key and
// tie-take helpers and the per-bound refine routine live in
// partition_core.h, shared with the host mode of pmh_debug_partition.

// Run addresses and 32-bit lengths of a KM-wide instantiation: slots r >= k
// re-read run 0 and become empty runs, so the loads carry no branch.
template <int KM>
DEV void partition_runs(const DevCol *__restrict__ keys,
                        const int64_t *__restrict__ lens, int k,
                        uint64_t *addr, uint32_t *len) {
#pragma unroll
    for (int r = 0; r < KM; r++) {
        const int rr = r < k ? r : 0;
        addr[r] = keys[rr].addr0;
        len[r] = (uint32_t)lens[rr];
    }
#pragma unroll
    for (int r = 0; r < KM; r++) len[r] = r < k ? len[r] : 0u;
}

// --------------------------------------------------------- k_partition_wave
//
// Wave-parallel 64-ary key-domain search: ONE WAVE per tile boundary; per
// round the 64 lanes probe 64 evenly spaced pivots of the remaining key
// domain (each lane runs the lockstep multi-run count for its pivot), a
// ballot picks the bracketing pair, and domain + per-run windows narrow
// ~65x. Exact counts, so the cuts follow the contract in partition_core.h.
// The dependent-load chain is one round trip per search step: about
// log65(key span) rounds, each with log2(widest window) steps, every step
// probing all runs at once (at 8 x 10M rows: 5 rounds, ~61 steps, plus 2
// trips of setup and 2 of finish). Validated against a brute-force model on
// randomized runs (tests/test_partition_*.py, tests/test_tile_algorithm.py).
template <int KM, int ES>
DEV void partition_wave_body(const DevCol *__restrict__ keys,
                             const int64_t *__restrict__ lens, int k,
                             int64_t tile_rows, int64_t n_bounds,
                             int64_t total_rows, int64_t stride,
                             int32_t *cuts) {
    // stride > 1: coarse pass of the two-level partition — bounds
    // {0, stride, 2*stride, ...} u {n_bounds-1}; interior bounds follow in
    // k_partition_refine with windows clamped by the enclosing coarse cuts
    // (their probes then stay inside small, L2-resident windows: the wave
    // kernel's 64 probes/round cost ~12x the old kernel's probe TRAFFIC
    // when used for every bound — measured 2.4 ms vs 1.2 — so it only runs
    // where its short chain matters: the full-depth coarse cuts)
    const int lane = (int)(threadIdx.x & 63);
    int64_t b =
        ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) *
        stride;
    if (b > n_bounds - 1) b = n_bounds - 1;
    int64_t D = b * tile_rows;
    if (D > total_rows) D = total_rows;
    uint64_t addr[KM];
    uint32_t len[KM], wlo[KM], whi[KM], pos[KM];
    partition_runs<KM>(keys, lens, k, addr, len);
    if (D == 0 || D >= total_rows) {
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < KM; r++) {
                if (r >= k) continue;
                cuts[b * k + r] = D == 0 ? 0 : (int32_t)len[r];
            }
        }
        return;
    }
    ppc_safe_addrs<KM>(addr, len);  // 0 < D < total: a non-empty run exists
#pragma unroll
    for (int r = 0; r < KM; r++) {
        wlo[r] = 0;
        whi[r] = len[r];
    }
    uint64_t klo, khi;
    ppc_window_keys<ES, KM>(addr, wlo, whi, &klo, &khi);
    while (klo < khi) {
        const uint64_t span = khi - klo;
        uint64_t pv;
        if (span <= 63) {
            pv = klo + (uint64_t)lane;
            if (pv > khi) pv = khi;
        } else {
            // overflow-safe klo + span*(lane+1)/65, monotone in lane
            const uint64_t q = span / 65, rm = span % 65;
            pv = klo + q * (uint64_t)(lane + 1) +
                 (rm * (uint64_t)(lane + 1)) / 65;
        }
        ppc_bound_multi<true, ES, KM>(addr, wlo, whi, pv, pos);
        int64_t cnt = 0;
#pragma unroll
        for (int r = 0; r < KM; r++) cnt += pos[r];
        const uint64_t ge = __ballot(cnt >= D);
        const int f = ge ? (int)(__ffsll((unsigned long long)ge) - 1) : 64;
        const int fc = f < 64 ? f : 63;   // lane holding the new upper
        const int fm = f > 0 ? f - 1 : 0; // lane holding the new lower
        const uint64_t pv_f = __shfl(pv, fc, 64);
        const uint64_t pv_m = __shfl(pv, fm, 64);
        if (f == 64) klo = pv_f + 1;        // even the last pivot counts < D
        else if (f == 0) khi = pv_f;
        else { klo = pv_m + 1; khi = pv_f; }
#pragma unroll
        for (int r = 0; r < KM; r++) {
            const uint32_t pf = __shfl(pos[r], fc, 64);
            const uint32_t pm = __shfl(pos[r], fm, 64);
            if (f == 64) wlo[r] = pf;
            else if (f == 0) whi[r] = pf;
            else { wlo[r] = pm; whi[r] = pf; }
        }
    }
    // klo == v*: tie-take finish (redundant across lanes; lane 0 stores)
    ppc_tie_finish<ES, KM>(addr, len, wlo, whi, klo, D, pos);
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < KM; r++) {
            if (r >= k) continue;
            cuts[b * k + r] = (int32_t)pos[r];
        }
    }
}

// (launch bounds = the launcher's block sizes: the default bound of 1024
// threads caps a kernel at 128 VGPRs, which KM >= 16 does not fit in)
template <int KM>
__launch_bounds__(256) __global__
void k_partition_wave(const DevCol *__restrict__ keys,
                      const int64_t *__restrict__ lens, int k,
                      int64_t tile_rows, int64_t n_bounds, int64_t total_rows,
                      int64_t stride, int32_t *cuts) {
    // the key width is uniform across runs: decide it once for the whole body
    if (keys[0].esize == 8)
        partition_wave_body<KM, 8>(keys, lens, k, tile_rows, n_bounds,
                                   total_rows, stride, cuts);
    else
        partition_wave_body<KM, 4>(keys, lens, k, tile_rows, n_bounds,
                                   total_rows, stride, cuts);
}

// ------------------------------------------------------- k_partition_refine
//
// Level 2 of the two-level partition: each interior bound bisects inside
// the windows of its enclosing coarse cuts (ppc_refine_bound). Correct
// because a coarse cut is two-sided: every element below it keys <= its
// pivot and the pivot keys of bounds >= tile_rows ranks apart differ
// strictly (an equal-key group has <= k << tile_rows members, one per run),
// so no element outside the window can tie with any probed pivot in a way
// that changes a count comparison.
template <int KM, int ES>
DEV void partition_refine_body(const DevCol *__restrict__ keys,
                               const int64_t *__restrict__ lens, int k,
                               int64_t tile_rows, int64_t n_bounds,
                               int64_t G, int32_t *cuts) {
    int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_bounds - 1) return;
    if (b % G == 0) return;  // coarse pass computed it
    int64_t D = b * tile_rows;  // b interior => 0 < D < total_rows
    int64_t g0 = (b / G) * G;
    int64_t g1 = g0 + G;
    if (g1 > n_bounds - 1) g1 = n_bounds - 1;
    uint64_t addr[KM];
    uint32_t len[KM];
    partition_runs<KM>(keys, lens, k, addr, len);
    ppc_safe_addrs<KM>(addr, len);
    ppc_refine_bound<ES, KM>(addr, len, k, D, cuts + g0 * k, cuts + g1 * k,
                             cuts + b * k);
}

template <int KM>
__launch_bounds__(128) __global__
void k_partition_refine(const DevCol *__restrict__ keys,
                        const int64_t *__restrict__ lens, int k,
                        int64_t tile_rows, int64_t n_bounds,
                        int64_t total_rows, int64_t G, int32_t *cuts) {
    if (keys[0].esize == 8)
        partition_refine_body<KM, 8>(keys, lens, k, tile_rows, n_bounds, G,
                                     cuts);
    else
        partition_refine_body<KM, 4>(keys, lens, k, tile_rows, n_bounds, G,
                                     cuts);
}


// ------------------------------------------------------------ k_merge_tiles
//
// Phase 1: per tile, stage (key, seq, kind) segments in LDS, stable
// pairwise-merge into (key, run) order, mark equal-key group heads, run a
// segmented (seq, isAdd) argmax per group (groups have <= k records: one
// per run — SortedRun invariant, SortedRun.java), apply Deduplicate +
// wrapper + drop-delete rules, and emit packed winners per owned group.
// Staging is flat (thread tid owns segment elements tid + s * 512, all of a
// tile's loads issued together) and, where registers allow, pipelined: a
// block's next tile is loaded into registers while this one is merged.

// Per-tile segment setup. Double-buffered: the staging prefetch of a block's
// next tile fills the other buffer while the current tile is merged.
struct TileSetup {
    int32_t segoff[PMH_MAX_RUNS + 1];  // entries past k hold mtotal
    int32_t rowoff[PMH_MAX_RUNS];  // run row of segment element sx is
                                   // sx + rowoff[run]
    int32_t mtotal;                // extended element count
    int32_t mreal;  // real element count (rank width of this tile)
};

struct TileSmem {
    int64_t skey[PMH_TILE_MAX];
    int64_t sseq[PMH_TILE_MAX];  // packed (sequenceNumber << 1) | isAdd:
                                 // ascending == ascending (seq, isAdd) —
                                 // the merge-order tie-break of
                                 // SortMergeReaderWithLoserTree.java:53-63.
                                 // Requires |seq| < 2^62 (Paimon sequence
                                 // numbers are non-negative counters).
    uint16_t perm[2][PMH_TILE_MAX];
    uint8_t head[PMH_TILE_MAX];    // group head flags (merged order)
    int32_t wave_tot[2 * (PMH_TILE_THREADS / 64)];
    TileSetup setup[2];
    // per-run column bases, copied once per block (tomb 0 = no tombstones);
    // one record per run, so a slot's four lookups share one LDS address
    struct RunBase {
        uint64_t key, seq, kind, tomb;
    } rb[PMH_MAX_RUNS];
    int64_t predkey;  // largest key before any run's first element
    int32_t haspred;
};

// One tile's staged elements in registers: thread tid owns segment elements
// tid + s * PMH_TILE_THREADS. Filled by tile_prefetch, drained by tile_store.
template <bool TOMBS>
struct TileRegs {
    int64_t key[PMH_TILE_ITER];
    int64_t seq[PMH_TILE_ITER];
    int32_t kind[PMH_TILE_ITER];
    uint8_t tomb[TOMBS ? PMH_TILE_ITER : 1];  // deletion-vector bytes
    int64_t pred;  // threads tid < k: key before run tid's first element,
                   // if the run's cut is not 0
};

// stable 2-way co-rank: number of A elements among the first d outputs of
// merge(A, B), ties take A first. A/B are perm-index sequences; key lookup
// through skey[.]. For i in [max(0,d-lb), min(d,la)), j = d-1-i is always
// in [0, lb). Advance while A[i] <= B[j] (A[i] belongs in the first d).
template <typename KT>
DEV int32_t corank(int64_t d, const uint16_t *pa, int32_t la,
                   const uint16_t *pb, int32_t lb, const KT *skey) {
    int64_t ilo = d > lb ? d - lb : 0;
    int64_t ihi = d < la ? d : la;
    while (ilo < ihi) {
        int64_t i = ilo + ((ihi - ilo) >> 1);
        int64_t j = d - 1 - i;
        if (skey[pa[i]] <= skey[pb[j]]) ilo = i + 1;
        else ihi = i;
    }
    return (int32_t)ilo;
}

DEV bool kind_is_add(uint8_t k) { return k == 0 || k == 2; }

// user-defined sequence fields (CoreOptions sequence.field;
// utils/UserDefinedSeqComparator.java:38-80, wired at
// MergeFileSplitRead.java:543-545): listed value columns compare BEFORE
// the sequence number, ascending, nulls FIRST (codegen nullIsLast=false).
DEV int useq_cmp(const DevCol *cols, const uint8_t *col_dtype, int n_cols,
                 const int16_t *ucols, int nu, int runA, int64_t rowA,
                 int runB, int64_t rowB) {
    for (int j = 0; j < nu; j++) {
        const int c = ucols[j];
        const DevCol &a = cols[runA * n_cols + c];
        const DevCol &b = cols[runB * n_cols + c];
        const uint8_t va = col_valid(a, rowA);
        const uint8_t vb = col_valid(b, rowB);
        if (va != vb) return va ? 1 : -1;  // null sorts first
        if (!va) continue;
        const int dt = col_dtype[c];
        const int64_t x = col_load_wide(a, rowA, dt);
        const int64_t y = col_load_wide(b, rowB, dt);
        if (x != y) return x > y ? 1 : -1;
    }
    return 0;
}
// k_merge_tiles packs (seq << 1) | isAdd (the fused kernel uses the 2-bit
// ps2_* packing); helper so call sites read uniformly
DEV bool ps2m_isadd(int64_t w) { return w & 1; }

// Load through a global-address-space pointer: a generic (flat) load would
// also count on the LDS counter, and the first LDS wait of the merge would
// then drain the whole prefetch.
template <typename T>
DEV T gload(uint64_t addr) {
    return *reinterpret_cast<const __attribute__((address_space(1))) T *>(
        addr);
}

// Issue every global load of one tile's staging at once: the 2k cuts and
// run lengths (block-uniform addresses; KM is the unrolled run bound, as in
// k_partition_wave), then the predecessor keys and all key / seq / kind /
// tombstone loads of this thread's slots, into registers. Nothing here
// waits on element data, so the caller may run other work (the previous
// tile's merge) before the registers go to LDS. The tile's segment setup goes
// to `st`; the caller's next barrier publishes it. [S0, S0 + NS) is the slot
// range: a caller short of registers stages a tile in two halves (the
// first call writes the setup). TAG only names a separate copy: a kernel
// instantiation added later passes its own, so the copies the existing
// kernels inline keep the callers they had (the inliner treats a copy with
// one caller differently, and their code would change with it).
template <int KM, bool TOMBS, int HS, int S0 = 0, int NS = PMH_TILE_ITER,
          int TAG = 0>
DEV void tile_prefetch(const TileSmem &sm, TileSetup &st,
                       const int32_t *__restrict__ cuts,
                       const int64_t *__restrict__ lens, int64_t tile, int k,
                       int kes, int tid, TileRegs<TOMBS> &rg) {
    const int32_t *c0 = cuts + tile * k;
    const int32_t *c1 = c0 + k;
    int32_t a[KM], len[KM];
    int32_t M = 0, Mreal = 0;
#pragma unroll
    for (int r = 0; r < KM; r++) {
        const int rr = r < k ? r : 0;  // loads stay unconditional
        const int32_t ar = c0[rr], br = c1[rr];
        const int32_t ln = (int32_t)lens[rr];
        // extended: +1 element per run when available
        a[r] = ar;
        len[r] = r < k ? (br - ar) + (br < ln ? 1 : 0) : 0;
        Mreal += r < k ? br - ar : 0;
        M += len[r];
    }
    // segment setup of the tile: thread r publishes run r's offsets
    int32_t so = 0, my_so = 0, my_a = 0;
    if constexpr (S0 == 0) {
#pragma unroll
        for (int r = 0; r < KM; r++) {
            if (tid == r) {
                my_so = so;
                my_a = a[r];
            }
            so += len[r];
        }
        if (tid <= KM) st.segoff[tid] = tid < k ? my_so : M;
        if (tid < k) st.rowoff[tid] = my_a - my_so;
        if (tid == 0) {
            st.mtotal = M;
            st.mreal = Mreal;
        }
        rg.pred = 0;
    }
    if (M <= 0) return;  // block-uniform: no element, no valid address
    // Slots go in fenced groups of HS (4, or 2 where registers are short),
    // column by column within a group, so only one group's lookups and
    // addresses are live at a time (registers); every load of the tile is
    // still issued before anything waits on element data.
#pragma unroll
    for (int h = S0; h < S0 + NS; h += HS) {
        // slot -> (run, row): the last run whose segment offset is <= e
        // (that run is non-empty because e < M). Dead slots clamp to element
        // M - 1, so every slot loads from a valid address and only the LDS
        // store is guarded.
        int32_t e[HS], rowd[HS];
        int run[HS];
#pragma unroll
        for (int s = 0; s < HS; s++) {
            const int32_t x = tid + (h + s) * PMH_TILE_THREADS;
            e[s] = x < M ? x : M - 1;
            rowd[s] = 0;
            run[s] = 0;
        }
        int32_t off = 0;
#pragma unroll
        for (int r = 0; r < KM; r++) {
#pragma unroll
            for (int s = 0; s < HS; s++) {
                const bool in = r < k && e[s] >= off;
                run[s] = in ? r : run[s];
                rowd[s] = in ? a[r] - off : rowd[s];
            }
            off += len[r];
        }
        uint32_t row[HS];  // unsigned: widens for free in the address
#pragma unroll
        for (int s = 0; s < HS; s++) row[s] = (uint32_t)(e[s] + rowd[s]);
        // The key width is uniform: one hoisted branch, a whole batch per
        // arm. Keys stay raw (a 4-byte key is widened when it goes to LDS):
        // converting here would wait for the load inside the arm.
        if (kes == 8) {
#pragma unroll
            for (int s = 0; s < HS; s++)
                rg.key[h + s] = gload<int64_t>(sm.rb[run[s]].key +
                                               (uint64_t)row[s] * 8);
        } else {
#pragma unroll
            for (int s = 0; s < HS; s++)
                rg.key[h + s] = (int64_t)gload<uint32_t>(
                    sm.rb[run[s]].key + (uint64_t)row[s] * 4);
        }
#pragma unroll
        for (int s = 0; s < HS; s++)
            rg.seq[h + s] =
                gload<int64_t>(sm.rb[run[s]].seq + (uint64_t)row[s] * 8);
#pragma unroll
        for (int s = 0; s < HS; s++)
            rg.kind[h + s] =
                gload<int32_t>(sm.rb[run[s]].kind + (uint64_t)row[s] * 4);
        if constexpr (TOMBS) {
            // a run without tombstones reads byte 1 of the row's kind
            // instead: valid memory, and zero (row kinds are 0..3), i.e.
            // "not deleted"
#pragma unroll
            for (int s = 0; s < HS; s++) {
                const uint64_t t = sm.rb[run[s]].tomb;
                rg.tomb[h + s] = gload<uint8_t>(
                    t ? t + (uint64_t)row[s]
                      : sm.rb[run[s]].kind + (uint64_t)row[s] * 4 + 1);
            }
        }
        if (h == 0 && tid < 64) {
            // Predecessor keys ride in wave 0 (a wave-uniform branch); a
            // thread without one re-reads its first slot's key, so the load
            // is unconditional.
            const bool haspred = tid < k && my_a > 0;
            const uint64_t pbase =
                haspred ? sm.rb[tid & (PMH_MAX_RUNS - 1)].key
                        : sm.rb[run[0]].key;
            const uint64_t prow = haspred ? (uint32_t)(my_a - 1) : row[0];
            rg.pred = kes == 8 ? gload<int64_t>(pbase + prow * 8)
                               : (int64_t)gload<uint32_t>(pbase + prow * 4);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// PU=true: PartialUpdate mode — no winner reduction; emit every owned
// group's member list (ascending (seq, isAdd) order within the group) for
// the per-field overlay in k_emit_pu. v1 accepts INSERT-only streams (the
// reference's default partial-update rejects retracts,
// PartialUpdateMergeFunction.java:170-186) — retracts set err_flag.
// Separate template instantiations keep the PU path's extra registers out
// of the deduplicate kernel.
//
// LK=true: lookup changelog producer (flags bit PMH_FLAG_LOOKUP) — the winner
// walk applies LookupMergeFunction's level rules and reads k_lookup_probe's
// per-row probe words; its own instantiation, so the other modes' code is
// untouched.
//
// PCL=true (with PU): full-compaction changelog for the folding engines
// (partial-update / aggregation; flags bit PMH_FLAG_FOLD_CL). The member-list
// walk also writes provisional changelog entries: a before-type row names
// the group's top-level member, an after-type row the engine's folded result
// by the group's tile-local index among the kept groups (changelog_core.h).
// Its own instantiation again.
template <bool PU, bool FR, bool LK, int KM, bool TOMBS, bool PCL = false>
__attribute__((amdgpu_waves_per_eu(4))) __launch_bounds__(PMH_TILE_THREADS, 2)
__global__
void k_merge_tiles(const DevCol *keys, const DevCol *seqs, const DevCol *kinds,
                   const int64_t *__restrict__ lens, int k,
                   const int32_t *__restrict__ cuts,
                   int64_t n_tiles, int64_t tile_rows, int flags,
                   const uint64_t *tombs, uint32_t *winners,
                   int32_t *tile_counts, uint16_t *group_start,
                   uint32_t *err_flag,
                   // full-compaction changelog (cl_entries != nullptr):
                   // per-run levels, the table's max level, and the
                   // per-group provisional changelog entries (2 slots per
                   // group; k_cl_finalize compacts them to rows)
                   const uint8_t *run_levels, int max_level,
                   uint64_t *cl_entries, int32_t *cl_counts,
                   // lookup changelog (LK): one word per row of the level-0
                   // runs (k_lookup_probe), run r's rows at probe_off[r];
                   // keys/seqs/kinds then carry the lookup-level slots
                   // after the k merge runs
                   const uint32_t *probe_words, const int64_t *probe_off) {
    const bool drop_delete = flags & PMH_FLAG_DROP_DELETE;
    const bool ignore_delete = flags & PMH_FLAG_IGNORE_DELETE;
    // FR = first-row engine (FirstRowMergeFunction.java:32-77): keep the
    // FIRST record per key in ascending (seq, isAdd) order; retracts throw
    // unless ignore-delete (then skipped); singleton groups bypass the merge
    // function (wrapper) exactly as deduplicate does. A template parameter so
    // the deduplicate winner walk carries no extra select.
    constexpr bool first_row = FR;
    // partial-update.remove-record-on-delete (PU mode): DELETE members are
    // legal; a group whose LAST member (max packed sseq) is a DELETE yields
    // a DELETE result and is dropped here under drop_delete. UPDATE_BEFORE
    // is rejected at staging (v1: INSERT/DELETE streams).
    const bool rrod = (flags & PMH_FLAG_RROD) != 0;
    // sequence groups (PartialUpdateMergeFunction.java:219-377): retracts
    // are legal members (they retract their groups); result kind is DELETE
    // only when the group has NO add member (getResult :389-397)
    const bool seqg = (flags & PMH_FLAG_SEQ_GROUPS) != 0;
    // aggregation with retract-capable aggregators (FieldSumAgg.retract /
    // FieldPrimaryKeyAgg / ignore-retract wrappers): retract members are
    // legal and fold through aggregator.retract in k_emit_agg
    const bool aggr = (flags & PMH_FLAG_AGG_RETRACT) != 0;
    // ablation levels (profiling only, the PMH_FLAG_ABLATE field): 1=stage,
    // 2=+merge, 3=+scan, 0/absent=full. Partial levels publish a checksum so
    // the compiler cannot dead-code the ablated phases' inputs.
    const int ablate =
        (flags >> PMH_FLAG_ABLATE_SHIFT) & PMH_FLAG_ABLATE_MASK;
    __shared__ TileSmem sm;
    const int tid = threadIdx.x;
    // the staged columns are contiguous: keep their bases in LDS, once
    if (tid < k) {
        sm.rb[tid].key = keys[tid].addr0;
        sm.rb[tid].seq = seqs[tid].addr0;
        sm.rb[tid].kind = kinds[tid].addr0;
        sm.rb[tid].tomb = tombs ? tombs[tid] : 0;
    }
    const int kes = keys[0].esize;  // the key type is uniform across runs
    __syncthreads();
    // Staging is software-pipelined across this block's tiles: the loads of
    // tile t + gridDim.x are issued into registers right after tile t's
    // registers went to LDS, and land during tile t's merge and walk.
    // The partial-update walk, and the tombstone bytes, leave no registers
    // for a tile in flight (it would spill): there a tile's loads are
    // issued, flat, at its own start, in two halves.
    constexpr bool PIPE = !PU && !TOMBS;
    constexpr int HALF = PMH_TILE_ITER / 2;
    TileRegs<TOMBS> rg;
    if (PIPE && (int64_t)blockIdx.x < n_tiles)
        tile_prefetch<KM, TOMBS, 4>(sm, sm.setup[0], cuts, lens, blockIdx.x,
                                    k, kes, tid, rg);
    int cb = 0;
    for (int64_t tile = blockIdx.x; tile < n_tiles;
         tile += gridDim.x, cb ^= 1) {
        if (!PIPE)
            tile_prefetch<KM, TOMBS, 2, 0, HALF, PCL>(
                sm, sm.setup[cb], cuts, lens, tile, k, kes, tid, rg);
        // publishes setup[cb] and ends the previous tile's LDS reads
        __syncthreads();
        const TileSetup &st = sm.setup[cb];
        const int32_t M = st.mtotal;
        const int32_t Mreal = st.mreal;

        // --- registers -> LDS (flat slots), then prefetch the next tile
        auto store_slots = [&](int s0, int ns) {
#pragma unroll
            for (int s = s0; s < s0 + ns; s++) {
                const int32_t e = tid + s * PMH_TILE_THREADS;
                if (e < M) {
                    const int32_t kd = rg.kind[s];
                    const bool dead = TOMBS && rg.tomb[TOMBS ? s : 0];
                    if (PU && rrod && !seqg && kd == 1 && !dead && err_flag)
                        // UPDATE_BEFORE: not in v1 RROD (sequence groups
                        // accept it)
                        atomicOr(err_flag, PMH_ERR_RETRACT);
                    sm.skey[e] =
                        kes == 8 ? rg.key[s] : (int64_t)(int32_t)rg.key[s];
                    sm.sseq[e] = dead ? PMH_DEAD
                                      : (rg.seq[s] << 1) |
                                            (int64_t)(kd == 0 || kd == 2);
                    sm.perm[0][e] = (uint16_t)e;
                }
            }
        };
        if constexpr (PIPE) {
            store_slots(0, PMH_TILE_ITER);
        } else {
            store_slots(0, HALF);
            tile_prefetch<KM, TOMBS, 2, HALF, HALF, PCL>(
                sm, sm.setup[cb], cuts, lens, tile, k, kes, tid, rg);
            store_slots(HALF, HALF);
        }
        if (tid < 64) {
            // predecessor key: max over the runs' candidates, which sit in
            // the first k <= 32 lanes of wave 0
            // (a run has one iff its cut, rowoff + segoff, is not 0)
            int64_t pk = kes == 8 ? rg.pred : (int64_t)(int32_t)rg.pred;
            const int pr = tid & (PMH_MAX_RUNS - 1);
            int hp = tid < k && st.rowoff[pr] + st.segoff[pr] > 0;
            for (int off = PMH_MAX_RUNS / 2; off > 0; off >>= 1) {
                const int64_t opk = __shfl_xor(pk, off, 64);
                const int ohp = __shfl_xor(hp, off, 64);
                if (ohp && (!hp || opk > pk)) pk = opk;
                hp |= ohp;
            }
            if (tid == 0) {
                sm.predkey = pk;
                sm.haspred = hp;
            }
        }
        if (PIPE && tile + gridDim.x < n_tiles)
            tile_prefetch<KM, TOMBS, 4>(sm, sm.setup[cb ^ 1], cuts, lens,
                                        tile + gridDim.x, k, kes, tid, rg);
        __syncthreads();
        if (Mreal == 0) {
            if (tid == 0) {
                tile_counts[tile] = 0;
                if (cl_counts) cl_counts[tile] = 0;
            }
            continue;
        }
        if (ablate == 1) {
            // keep staged data live; counts stay in {0,1} so the downstream
            // scan/emit of an ablated (profiling-only) run never goes OOB
            if (tid == 0) {
                int64_t x = sm.skey[M - 1] ^ sm.sseq[M - 1];
                tile_counts[tile] = (int32_t)((x ^ (x >> 32)) & 1);
            }
            continue;
        }

        // --- pairwise stable merge, ceil(log2(k)) levels
        int cur = 0;
        for (int width = 1; width < k; width <<= 1) {
            // sequences at this level: [segoff[q*width], segoff[min((q+1)*width,k)])
            // merge pairs (2q, 2q+1)
            const int nxt = cur ^ 1;
            // per-thread chunks of 8 outputs, grid-stride over all chunks
            const int CH = 8;
            int n_chunks = (M + CH - 1) / CH;
            for (int ch = tid; ch < n_chunks; ch += blockDim.x) {
                int64_t o = (int64_t)ch * CH;  // global output rank
                int remaining = (int)(M - o < CH ? M - o : CH);
                int p = 0;
                // a chunk may span several pairs (pairs can be tiny):
                // walk pairs until the chunk's outputs are all produced
                while (remaining > 0) {
                    // pair p covers output ranks [segoff[a0], segoff[b1])
                    while ((p + 1) * 2 * width < k &&
                           st.segoff[(p + 1) * 2 * width] <= o)
                        p++;
                    int a0 = p * 2 * width;
                    int amid = a0 + width < k ? a0 + width : k;
                    int b1 = a0 + 2 * width < k ? a0 + 2 * width : k;
                    int32_t abase = st.segoff[a0];
                    int32_t la = st.segoff[amid] - abase;
                    int32_t lb = st.segoff[b1] - st.segoff[amid];
                    int64_t d = o - abase;  // rank within pair
                    int32_t lim = la + lb - (int32_t)d;
                    if (lim <= 0) break;  // past the last pair
                    int n_out = lim < remaining ? lim : remaining;
                    const uint16_t *pa = &sm.perm[cur][abase];
                    const uint16_t *pb = &sm.perm[cur][abase + la];
                    int32_t ai = corank(d, pa, la, pb, lb, sm.skey);
                    int32_t bi = (int32_t)d - ai;
                    uint16_t *out = &sm.perm[nxt][abase + d];
                    for (int x = 0; x < n_out; x++) {
                        bool takeA;
                        if (ai >= la) takeA = false;
                        else if (bi >= lb) takeA = true;
                        else takeA = !(sm.skey[pa[ai]] > sm.skey[pb[bi]]);
                        out[x] = takeA ? pa[ai++] : pb[bi++];
                    }
                    o += n_out;
                    remaining -= n_out;
                }
            }
            cur = nxt;
            __syncthreads();
        }
        const uint16_t *mo = sm.perm[cur];
        if (ablate == 2) {
            if (tid == 0)
                tile_counts[tile] = ((int32_t)mo[M - 1] ^ (int32_t)mo[0]) & 1;
            continue;
        }

        // --- group heads + previous-tile continuation skip
        const int64_t predkey = sm.predkey;
        const bool haspred = sm.haspred;
        for (int32_t i = tid; i < M; i += blockDim.x) {
            int64_t kk = sm.skey[mo[i]];
            uint8_t h = (i == 0) ? 1 : (kk != sm.skey[mo[i - 1]]);
            // records continuing the previous tile's last group are not
            // heads here (that tile consumed them as its extras)
            if (haspred && kk == predkey) h = 0;
            sm.head[i] = h;
        }
        __syncthreads();
        // segment element -> run, branch-free (segoff entries past k hold
        // M > sx). Up to 8 runs: the block-uniform offsets are read once per
        // tile into scalar registers and an element's run is a count of
        // compares; beyond, a log2(KM)-step search in LDS.
        int32_t sseg[KM <= 8 ? KM : 1];
        if constexpr (KM <= 8) {
#pragma unroll
            for (int j = 1; j < KM; j++)
                sseg[j] = __builtin_amdgcn_readfirstlane(st.segoff[j]);
        }
        auto run_of = [&](int32_t sx) -> int {
            int r = 0;
            if constexpr (KM <= 8) {
#pragma unroll
                for (int j = 1; j < KM; j++) r += sseg[j] <= sx ? 1 : 0;
            } else {
#pragma unroll
                for (int step = KM / 2; step > 0; step >>= 1)
                    r += st.segoff[r + step] <= sx ? step : 0;
            }
            return r;
        };

        // block-wide exclusive scan (wave shuffle scans + one barrier):
        // the former Hillis-Steele block scans cost 16 __syncthreads per
        // tile and dominated the kernel's wave-parked time.
        const int lane = tid & 63;
        const int wv = tid >> 6;
        constexpr int NW = PMH_TILE_THREADS / 64;

        if constexpr (PU) {
            // --- PartialUpdate: emit owned groups' member lists
            const int32_t per =
                (Mreal + (int32_t)blockDim.x - 1) / blockDim.x;
            int32_t my_lo = tid * per;
            int32_t my_hi = my_lo + per < Mreal ? my_lo + per : Mreal;
            uint32_t *mout = &winners[tile * (tile_rows + PMH_MAX_RUNS)];
            uint16_t *gout = &group_start[tile * (tile_rows + 1)];
            bool bad_kind = false;
            int32_t g_off = 0, m_off = 0, total_g = 0, total_m = 0;
            // PCL: slot of this thread's first changelog entry pair
            [[maybe_unused]] int32_t c_off = 0;
            [[maybe_unused]] uint64_t *clout = nullptr;
            if constexpr (PCL)
                clout = &cl_entries[tile * 2 * (tile_rows + PMH_MAX_RUNS)];
            for (int pass = 0; pass < 2; pass++) {
                int32_t ng = 0, nm = 0;
                [[maybe_unused]] int32_t ncl = 0;
                for (int32_t i = my_lo; i < my_hi; i++) {
                    if (!sm.head[i]) continue;
                    // pre-scan the group: LIVE members only (deletion-
                    // vector tombstones stage as PMH_DEAD and never reach
                    // the merge — ApplyDeletionVectorReader semantics)
                    int32_t tail = i;
                    int32_t nlive = 0;
                    int64_t mx = INT64_MIN;
                    bool any_add = false;
                    uint16_t live1 = 0;
                    [[maybe_unused]] uint16_t s_top = 0;
                    [[maybe_unused]] int n_top = 0;
                    for (int32_t x = i;; x++) {
                        int64_t v = sm.sseq[mo[x]];
                        if (v != PMH_DEAD) {
                            if (nlive == 0) live1 = mo[x];
                            nlive++;
                            if (v > mx) mx = v;
                            any_add |= ps2m_isadd(v);
                            if constexpr (PCL) {
                                if (run_levels[run_of(mo[x])] == max_level) {
                                    s_top = mo[x];
                                    n_top++;
                                }
                            }
                        }
                        if (!(x + 1 < M && !sm.head[x + 1])) {
                            tail = x;
                            break;
                        }
                    }
                    if (nlive == 0) continue;
                    if constexpr (PCL) {
                        // changelog decision of every live group, before a
                        // dropped result leaves the walk: entries do not
                        // depend on drop-delete. merged = the wrapper's
                        // result; its kind follows the drop rules below.
                        if (n_top > 1 && err_flag)
                            // checkState :76-78
                            atomicOr(err_flag, PMH_ERR_TOP_LEVEL_DUP);
                        const bool m_add =
                            nlive == 1 ? ps2m_isadd(sm.sseq[live1])
                            : seqg     ? any_add
                            : rrod     ? ps2m_isadd(mx)
                                       : true;
                        const ClcDecision d = clc_decide(
                            nlive, n_top, m_add,
                            (flags & PMH_FLAG_CL_ROW_DEDUP) != 0);
                        if (d.n) {
                            if (pass == 1) {
                                const uint64_t pd =
                                    CLC_VALID | (d.pending ? CLC_PENDING : 0);
                                // a group with an after-type row is kept
                                // (merged is an add): g_off + ng is its
                                // tile-local index in the main output
                                const uint64_t after =
                                    (uint64_t)(uint32_t)(g_off + ng) |
                                    CLC_FROM_OUT | pd;
                                const int tr = run_of(s_top);
                                const uint64_t before =
                                    ((uint32_t)tr << PMH_ROW_BITS) |
                                    (uint32_t)((int32_t)s_top +
                                               st.rowoff[tr]) |
                                    pd;
                                const uint64_t k0 = (uint64_t)d.kind0
                                                    << CLC_KIND_SHIFT;
                                const uint64_t k1 = (uint64_t)d.kind1
                                                    << CLC_KIND_SHIFT;
                                clout[2 * (c_off + ncl)] =
                                    (d.n == 2 || !d.after_is_merged ? before
                                                                    : after) |
                                    k0;
                                clout[2 * (c_off + ncl) + 1] =
                                    d.n == 2 ? after | k1 : 0;
                            }
                            ncl++;
                        }
                    }
                    if (nlive == 1) {
                        // ReducerMergeFunctionWrapper singleton bypass
                        // (ReducerMergeFunctionWrapper.java:53-73): the lone
                        // record is served as-is (any kind, incl. retracts);
                        // a retract result drops under drop-delete
                        // (DropDeleteReader.java:53-61)
                        if (drop_delete && !ps2m_isadd(sm.sseq[live1]))
                            continue;
                    } else if (seqg && drop_delete) {
                        // result kind DELETE iff no add member
                        if (!any_add) continue;
                    } else if (rrod && drop_delete) {
                        // result kind = last member's kind (max packed
                        // sseq); DELETE results drop here (DropDeleteReader)
                        if (!ps2m_isadd(mx)) continue;
                    }
                    if (pass == 1) {
                        gout[g_off + ng] = (uint16_t)(m_off + nm);
                        // merged order within a group is (key, run); the
                        // overlay consumes records in ascending (seq, isAdd)
                        // order — insertion-sort the <= k LIVE members by
                        // the packed sseq.
                        uint16_t gm[PMH_MAX_RUNS];
                        int gn = 0;
                        for (int32_t x2 = i; x2 <= tail; x2++) {
                            uint16_t s = mo[x2];
                            if (sm.sseq[s] == PMH_DEAD) continue;
                            int y = gn;
                            while (y > 0 &&
                                   sm.sseq[gm[y - 1]] > sm.sseq[s]) {
                                gm[y] = gm[y - 1];
                                y--;
                            }
                            gm[y] = s;
                            gn++;
                        }
                        for (int x = 0; x < gn; x++) {
                            uint16_t s = gm[x];
                            // retracts only fail MULTI-record groups: the
                            // wrapper bypasses the merge function for
                            // singletons (gn == 1), so a lone retract
                            // passes; sequence groups accept retracts
                            // outright (retractWithSequenceGroup)
                            if (!rrod && !seqg && !aggr && gn > 1 &&
                                !ps2m_isadd(sm.sseq[s]))
                                bad_kind = true;
                            const int r = run_of(s);
                            uint32_t grow =
                                (uint32_t)((int32_t)s + st.rowoff[r]);
                            mout[m_off + nm + x] = ((uint32_t)r << PMH_ROW_BITS) | grow;
                        }
                    }
                    ng++;
                    nm += nlive;
                }
                if (pass == 0) {
                    // dual wave scan of (ng, nm). PCL: the changelog pair
                    // count rides in the high half of the group word — a
                    // tile holds at most PMH_TILE_MAX < 2^16 groups, so
                    // neither half carries into the other
                    int32_t ig = ng, im = nm;
                    if constexpr (PCL) ig |= ncl << 16;
                    for (int off = 1; off < 64; off <<= 1) {
                        int32_t ug = __shfl_up(ig, off, 64);
                        int32_t um = __shfl_up(im, off, 64);
                        if (lane >= off) {
                            ig += ug;
                            im += um;
                        }
                    }
                    if (lane == 63) {
                        sm.wave_tot[wv] = ig;
                        sm.wave_tot[NW + wv] = im;
                    }
                    __syncthreads();
                    int32_t addg = 0, addm = 0;
                    total_g = 0;
                    total_m = 0;
#pragma unroll
                    for (int w = 0; w < NW; w++) {
                        if (w < wv) {
                            addg += sm.wave_tot[w];
                            addm += sm.wave_tot[NW + w];
                        }
                        total_g += sm.wave_tot[w];
                        total_m += sm.wave_tot[NW + w];
                    }
                    if constexpr (PCL) {
                        c_off = ((addg + ig) >> 16) - ncl;
                        addg &= 0xffff;
                        ig &= 0xffff;
                        if (tid == 0) cl_counts[tile] = total_g >> 16;
                        total_g &= 0xffff;
                    }
                    g_off = addg + ig - ng;
                    m_off = addm + im - nm;
                }
            }
            if (bad_kind && err_flag) atomicOr(err_flag, PMH_ERR_RETRACT);
            if (tid == 0) {
                tile_counts[tile] = total_g;
                gout[total_g] = (uint16_t)total_m;  // sentinel
            }
            continue;
        }

        if (ablate == 3) {
            if (tid == 0)
                tile_counts[tile] = ((int32_t)mo[0] ^ (int32_t)sm.head[0]) & 1;
            continue;
        }
        // --- emit winners of owned groups, in key order.
        // A group is owned iff its head is a real (rank < Mreal) head; the
        // winner — DeduplicateMergeFunction's surviving record — is found
        // inline while walking the group's <= k members (max by packed
        // (eligible, seq, isAdd)). Each thread walks a contiguous head range
        // and writes at the scanned offset; only the changelog producers
        // walk twice (count, then write).
        const int32_t per = (Mreal + (int32_t)blockDim.x - 1) / blockDim.x;
        int32_t my_lo = tid * per;
        int32_t my_hi = my_lo + per < Mreal ? my_lo + per : Mreal;
        uint32_t *wout = &winners[tile * (tile_rows + PMH_MAX_RUNS)];
        // full-compaction changelog (FullChangelogMergeFunctionWrapper.java:
        // 96-126): per live group, up to two provisional entries, written
        // INDEPENDENTLY of drop-delete (a dropped DELETE result still emits
        // DELETE(topLevelKv)). PMH_FLAG_CL_ROW_DEDUP = row-deduplicate pending
        // (k_cl_finalize compares values and may drop the UB/UA pair).
        const bool cl = cl_entries != nullptr;
        const bool cl_pend = (flags & PMH_FLAG_CL_ROW_DEDUP) != 0;
        uint64_t *clout =
            cl ? &cl_entries[tile * 2 * (tile_rows + PMH_MAX_RUNS)] : nullptr;
        // map seg index -> packed (run, global row)
        auto packm = [&](uint16_t sx) -> uint64_t {
            const int r = run_of(sx);
            return ((uint32_t)r << PMH_ROW_BITS) |
                   (uint32_t)((int32_t)sx + st.rowoff[r]);
        };
        // Without changelog entries the walk runs once: the count pass parks
        // each kept winner at its head's rank in skey[] (dead after the head
        // pass; a thread reads back only its own <= PMH_TILE_ITER ranks) and
        // `kept` marks them; after the scan they are just stored.
        const bool one_walk = !LK && !cl;
        uint32_t *wpark = reinterpret_cast<uint32_t *>(sm.skey);
        uint32_t kept = 0;
        int32_t total = 0;
        int32_t my_off = 0;
        int32_t my_cl = 0;
        for (int pass = 0; pass < 2; pass++) {
            if (pass == 1 && one_walk) {
                int32_t n = 0;
                for (int32_t j = 0; j < my_hi - my_lo; j++)
                    if ((kept >> j) & 1)
                        wout[my_off + n++] = wpark[my_lo + j];
                break;
            }
            int32_t nloc = 0, ncl = 0;
            for (int32_t i = my_lo; i < my_hi; i++) {
                if (!sm.head[i]) continue;
                if constexpr (LK) {
                    // lookup changelog (LookupChangelogMergeFunctionWrapper
                    // .java:104-163 over LookupMergeFunction.java:66-135):
                    // the merge sees the level-0 members plus `high`, the
                    // member of the lowest level > 0 (other upper members
                    // are dropped); without such a member `high` is the
                    // probe hit in the lookup levels, if any.
                    uint16_t s_lo = 0, s_l0 = 0, s_hi = 0;
                    int64_t v_lo = 0, v_hi = 0;
                    int lv_hi = 0;
                    bool has_lo = false, has_hi = false;
                    for (int32_t x = i;; x++) {
                        const uint16_t sx = mo[x];
                        const int64_t v = sm.sseq[sx];
                        if (v != PMH_DEAD) {
                            const int lv = run_levels[run_of(sx)];
                            if (lv > 0) {
                                // pickHighLevel: lowest level; a level tie
                                // goes to the earlier record in merge order
                                if (!has_hi || lv < lv_hi ||
                                    (lv == lv_hi && v < v_hi)) {
                                    s_hi = sx;
                                    v_hi = v;
                                    lv_hi = lv;
                                    has_hi = true;
                                }
                            } else {
                                if (!has_lo) s_l0 = sx;
                                if (!has_lo || v > v_lo) {
                                    s_lo = sx;
                                    v_lo = v;
                                }
                                has_lo = true;  // containLevel0
                            }
                        }
                        if (!(x + 1 < M && !sm.head[x + 1])) break;
                    }
                    if (!has_lo && !has_hi) continue;  // no live member
                    uint32_t loc_hi = 0;
                    int64_t w_hi = 0;
                    bool hh = has_hi, hit = false;
                    if (has_hi) {
                        loc_hi = (uint32_t)packm(s_hi);
                        w_hi = v_hi;
                    } else {
                        const uint32_t pm = (uint32_t)packm(s_l0);
                        const uint32_t w =
                            probe_words[probe_off[pm >> PMH_ROW_BITS] +
                                        (int64_t)(pm & PMH_ROW_MASK)];
                        if (w != PLK_MISS) {
                            // a record of ANY kind counts (a DELETE too)
                            const int slot = w >> PMH_ROW_BITS;
                            const int64_t row = w & PMH_ROW_MASK;
                            const int64_t sq = reinterpret_cast<const int64_t *>(
                                seqs[slot].addr0)[row];
                            const int32_t kd = reinterpret_cast<const int32_t *>(
                                kinds[slot].addr0)[row];
                            w_hi = (sq << 1) | (int64_t)(kd == 0 || kd == 2);
                            loc_hi = w;
                            hh = hit = true;
                        }
                    }
                    // deduplicate result = last candidate. A member `high`
                    // sorts by (seq, isAdd); a looked-up one is inserted
                    // before the first candidate with a strictly greater
                    // sequence number (KeyValueBuffer.insertInto), so it
                    // wins exactly when its seq >= every member's.
                    const bool take_hi =
                        hh && (!has_lo || (hit ? (w_hi >> 1) >= (v_lo >> 1)
                                               : w_hi >= v_lo));
                    const uint32_t loc_res =
                        take_hi ? loc_hi : (uint32_t)packm(s_lo);
                    const int64_t w_res = take_hi ? w_hi : v_lo;
                    if (has_lo) {
                        // setChangelog(before = high, after = result),
                        // independent of drop-delete
                        const bool b_add = hh && (w_hi & 1);
                        const bool a_add = w_res & 1;
                        auto mkl = [&](uint32_t loc, uint64_t kd,
                                       bool pd) -> uint64_t {
                            return (uint64_t)loc | (kd << 32) | (1ull << 35) |
                                   (pd ? (1ull << 36) : 0);
                        };
                        uint64_t e0 = 0, e1 = 0;
                        int cl_n = 0;
                        if (!b_add) {
                            if (a_add) {  // INSERT(after)
                                e0 = mkl(loc_res, 0, false);
                                cl_n = 1;
                            }
                        } else if (!a_add) {  // DELETE(before)
                            e0 = mkl(loc_hi, 3, false);
                            cl_n = 1;
                        } else {  // UPDATE_BEFORE(before), UPDATE_AFTER(after)
                            e0 = mkl(loc_hi, 1, cl_pend);
                            e1 = mkl(loc_res, 2, cl_pend);
                            cl_n = 2;
                        }
                        if (cl_n) {
                            if (pass == 1) {
                                clout[2 * (my_cl + ncl)] = e0;
                                clout[2 * (my_cl + ncl) + 1] = e1;
                            }
                            ncl++;
                        }
                    }
                    if (drop_delete && !(w_res & 1)) continue;
                    if (pass == 1) wout[my_off + nloc] = loc_res;
                    nloc++;
                    continue;
                }
                // walk the group's LIVE members (deletion-vector tombstones
                // stage as PMH_DEAD), tracking the winner by (elig, sseq):
                // deduplicate keeps the LAST record, first-row the FIRST
                uint16_t s_best = 0;
                int64_t v_best = 0;
                bool e_best = false, any_retract = false;
                int32_t nlive = 0;
                uint16_t s_top = 0;
                int n_top = 0;
                for (int32_t x = i;; x++) {
                    int64_t v = sm.sseq[mo[x]];
                    if (v != PMH_DEAD) {
                        bool e = !ignore_delete || (v & 1);
                        any_retract |= !(v & 1);
                        bool take = nlive == 0 || (e && !e_best) ||
                                    (e == e_best &&
                                     (first_row ? v < v_best : v > v_best));
                        if (take) {
                            s_best = mo[x];
                            v_best = v;
                            e_best = e;
                        }
                        if (cl) {
                            if (run_levels[run_of(mo[x])] == max_level) {
                                s_top = mo[x];
                                n_top++;
                            }
                        }
                        nlive++;
                    }
                    if (!(x + 1 < M && !sm.head[x + 1])) break;
                }
                if (nlive == 0) continue;
                if (cl) {
                    if (n_top > 1 && err_flag)
                        // checkState :76-78
                        atomicOr(err_flag, PMH_ERR_TOP_LEVEL_DUP);
                    // merged = wrapper result; singletons bypass the merge
                    // function (so an ignored lone record still serves)
                    bool m_ok = nlive == 1 || e_best;
                    bool m_add = m_ok && (v_best & 1);
                    uint64_t e0 = 0, e1 = 0;
                    int cl_n = 0;
                    auto mk = [&](uint16_t sx, uint64_t kd,
                                  bool pd) -> uint64_t {
                        return packm(sx) | (kd << 32) | (1ull << 35) |
                               (pd ? (1ull << 36) : 0);
                    };
                    if (n_top == 0) {
                        if (m_add) {  // INSERT(merged) — also the singleton
                                      // "initial is add" rule (:117-119)
                            e0 = mk(s_best, 0, false);
                            cl_n = 1;
                        }
                    } else if (nlive > 1) {
                        if (!m_add) {  // DELETE(topLevelKv) (:106-107)
                            e0 = mk(s_top, 3, false);
                            cl_n = 1;
                        } else {  // UPDATE_BEFORE(top) + UPDATE_AFTER(merged)
                            e0 = mk(s_top, 1, cl_pend);
                            e1 = mk(s_best, 2, cl_pend);
                            cl_n = 2;
                        }
                    }  // singleton that IS the top level: no change (:120-123)
                    if (cl_n) {
                        if (pass == 1) {
                            clout[2 * (my_cl + ncl)] = e0;
                            clout[2 * (my_cl + ncl) + 1] = e1;
                        }
                        ncl++;
                    }
                }
                if (first_row && !ignore_delete && any_retract && nlive > 1 &&
                    err_flag)
                    // FirstRow rejects retracts
                    atomicOr(err_flag, PMH_ERR_FIRST_ROW_RETRACT);
                if (!e_best && nlive > 1) continue;  // all records ignored
                if (drop_delete && !(v_best & 1)) continue;
                if (one_walk) {
                    wpark[i] = (uint32_t)packm(s_best);
                    kept |= 1u << (i - my_lo);
                } else if (pass == 1) {
                    wout[my_off + nloc] = (uint32_t)packm(s_best);
                }
                nloc++;
            }
            if (pass == 0) {
                int32_t incl = nloc, iccl = ncl;
                for (int off = 1; off < 64; off <<= 1) {
                    int32_t up = __shfl_up(incl, off, 64);
                    int32_t uc = __shfl_up(iccl, off, 64);
                    if (lane >= off) {
                        incl += up;
                        iccl += uc;
                    }
                }
                if (lane == 63) {
                    sm.wave_tot[wv] = incl;
                    sm.wave_tot[NW + wv] = iccl;
                }
                __syncthreads();
                int32_t add = 0, addc = 0, totc = 0;
                total = 0;
#pragma unroll
                for (int w = 0; w < NW; w++) {
                    if (w < wv) {
                        add += sm.wave_tot[w];
                        addc += sm.wave_tot[NW + w];
                    }
                    total += sm.wave_tot[w];
                    totc += sm.wave_tot[NW + w];
                }
                my_off = add + incl - nloc;
                my_cl = addc + iccl - ncl;
                if (cl && tid == 0) cl_counts[tile] = totc;
            }
        }
        if (tid == 0) tile_counts[tile] = total;
    }
}

// ------------------------------------------------------------ k_merge_emit
//
// FUSED single-pass merge + emit for the deduplicate / first-row engines:
// the partition cuts in, the merged output columns out — one kernel.
// Replaces the k_merge_tiles -> k_scan_tiles -> k_emit chain (and its
// winners round-trip through HBM) for non-member-list engines:
//
//  - tiles are taken from a global TICKET (atomic counter), so tile t-1 is
//    always owned by a workgroup that started no later than tile t's — the
//    forward-progress precondition for a decoupled-lookback prefix without
//    any dispatch-order assumption (HIP promises none, MI355X_MICROARCH.md
//    §Workgroup dispatch);
//  - each tile stages key/seq/kind in LDS, merges, walks group winners
//    (exactly k_merge_tiles' order contract), then publishes its survivor
//    count through a PACKED agent-scope atomic word (flag:2 | value:62) and
//    resolves its global output offset by wave-parallel lookback — the
//    payload rides in the atomic itself, so no separate fence choreography
//    is needed (per-XCD L2s are not coherent; agent-scope rel/acq is);
//  - emission happens from LDS: key/seq/kind come from the already-staged
//    merge arrays (full RowKind is recoverable from the packed seq word),
//    and each remaining output column is staged COALESCED per run into a
//    double-buffered LDS slab that reuses the merge arrays' space, then
//    scattered to the dense output by winner index — LDS gathers + coalesced
//    stores instead of the 4-8 B HBM gathers that left k_emit 96% latency-
//    parked (profiles/r01_final_pmc_sq.md).
//
// Packed seq word: (sequenceNumber << 2) | (isAdd << 1) | (kind >> 1).
// Ascending order == ascending (seq, isAdd) — the merge-order tie-break of
// SortMergeReaderWithLoserTree.java:53-63 (the kind>>1 bit only breaks ties
// between records with equal (seq, isAdd), which valid buckets never have —
// sequence numbers are unique). RowKind = ((w & 1) << 1) | (1 - ((w >> 1) & 1)).
// Requires |seq| < 2^61 (Paimon sequence numbers are non-negative counters).

DEV int64_t ps2_pack(int64_t seq, int32_t kd) {
    return (seq << 2) | ((int64_t)(kd == 0 || kd == 2) << 1) |
           (int64_t)((kd >> 1) & 1);
}
DEV bool ps2_isadd(int64_t w) { return (w >> 1) & 1; }
DEV int32_t ps2_kind(int64_t w) {
    return (int32_t)(((w & 1) << 1) | (1 - ((w >> 1) & 1)));
}

struct FusedSmem {
    union {
        struct {
            int64_t skey[PMH_TILE_MAX];
            int64_t sseq[PMH_TILE_MAX];
        };
        // emission phase (skey/sseq dead after the key/seq/kind emit):
        // two column-staging slabs, PMH_TILE_MAX elements of up to 8 B
        uint8_t vbuf[2][PMH_TILE_MAX * 8];
    };
    uint16_t perm[2][PMH_TILE_MAX];
    uint8_t head[PMH_TILE_MAX];
    int32_t wave_tot[PMH_TILE_THREADS / 64];
    int32_t segoff[PMH_MAX_RUNS + 1];
    int32_t seglen[PMH_MAX_RUNS];
    int64_t predcand[PMH_MAX_RUNS];
    int64_t predkey;
    int64_t s_tile;
    int64_t s_goff;
    int32_t haspred;
    int32_t mtotal;
    int32_t mreal;
    // 32-bit tile-relative key mode: real merge tiles span ~3.6k sorted
    // keys, so (max-min) almost always fits 32 bits — staged keys repack
    // in place to uint32 offsets from tile_kmin (ukey space), halving the
    // LDS bank pressure of the merge's random key compares
    uint64_t wkmin[PMH_TILE_THREADS / 64];
    uint64_t wkmax[PMH_TILE_THREADS / 64];
    uint64_t tile_kmin;
    uint32_t predkey32;
    int32_t narrow;
};

constexpr uint64_t LOOK_AGG = 1ull << 62;
constexpr uint64_t LOOK_PREFIX = 2ull << 62;
constexpr uint64_t LOOK_VAL = (1ull << 62) - 1;

template <bool FR>
__attribute__((amdgpu_waves_per_eu(4))) __launch_bounds__(PMH_TILE_THREADS, 2)
__global__
void k_merge_emit(const DevCol *keys, const DevCol *seqs, const DevCol *kinds,
                  const int64_t *lens, int k, const int32_t *cuts,
                  int64_t tile_base, int64_t tile_limit, int64_t n_tiles,
                  int64_t tile_rows, int flags, const uint64_t *tombs,
                  const DevCol *cols /* k * n_cols, run-major */,
                  const uint8_t *col_dtype, const uint8_t *col_nullable,
                  int n_cols, int key_col /* -1: composite */, int seq_col,
                  int kind_col, const int16_t *useq_cols, int n_useq,
                  uint64_t *status, uint64_t *ticket,
                  int64_t *total_out, uint32_t *dense_winners,
                  void *const *out_ptrs,
                  uint8_t *const *out_valid, uint32_t *err_flag) {
    const bool drop_delete = flags & PMH_FLAG_DROP_DELETE;
    const bool ignore_delete = flags & PMH_FLAG_IGNORE_DELETE;
    __shared__ FusedSmem sm;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    constexpr int NW = PMH_TILE_THREADS / 64;
    for (;;) {
        if (tid == 0)
            sm.s_tile = tile_base + (int64_t)__hip_atomic_fetch_add(
                ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        const int64_t tile = sm.s_tile;
        if (tile >= tile_limit) return;
        const int32_t *c0 = &cuts[tile * k];
        const int32_t *c1 = &cuts[(tile + 1) * k];
        int32_t my_lo = 0, my_hi = 0, my_off = 0;
        int32_t C = 0;  // this tile's survivor count
        int cur = 0;
        uint16_t *wl = nullptr;
        // one group-walk body for both passes (count, then emit): walks the
        // thread's head range applying Deduplicate/FirstRow + wrapper +
        // drop-delete rules, calling emit(n-th-winner, seg-index)
        auto seg_rr = [&](uint16_t s, int *rr, int64_t *row) {
            int r = 0;
            while (r + 1 < k && sm.segoff[r + 1] <= (int32_t)s) r++;
            *rr = r;
            *row = c0[r] + ((int32_t)s - sm.segoff[r]);
        };
        auto walk_pass = [&](int32_t lo_i, int32_t hi_i, auto emit) {
            const uint16_t *mo = sm.perm[cur];
            const int32_t M = sm.mtotal;
            int32_t nloc = 0;
            for (int32_t i = lo_i; i < hi_i; i++) {
                if (!sm.head[i]) continue;
                // walk the group's members, skipping deletion-vector
                // tombstones (PMH_DEAD) — the reference's reader never
                // shows deleted rows to the merge, so LIVE members define
                // group size for the wrapper's singleton bypass too
                uint16_t s_best = 0;
                int64_t v_best = 0;
                bool e_best = false, any_retract = false;
                int32_t nlive = 0;
                for (int32_t x = i;; x++) {
                    int64_t v = sm.sseq[mo[x]];
                    if (v != PMH_DEAD) {
                        bool e = !ignore_delete || ps2_isadd(v);
                        any_retract |= !ps2_isadd(v);
                        bool take;
                        if (nlive == 0) {
                            take = true;
                        } else if (e != e_best) {
                            take = e;
                        } else if (n_useq > 0) {
                            // (seq fields..., seq, isAdd) ascending: the
                            // fields compare before the sequence number
                            int ra, rb;
                            int64_t qa, qb;
                            seg_rr(mo[x], &ra, &qa);
                            seg_rr(s_best, &rb, &qb);
                            const int cu =
                                useq_cmp(cols, col_dtype, n_cols, useq_cols,
                                         n_useq, ra, qa, rb, qb);
                            take = FR ? (cu < 0 || (cu == 0 && v < v_best))
                                      : (cu > 0 || (cu == 0 && v > v_best));
                        } else {
                            take = FR ? v < v_best : v > v_best;
                        }
                        if (take) {
                            s_best = mo[x];
                            v_best = v;
                            e_best = e;
                        }
                        nlive++;
                    }
                    if (!(x + 1 < M && !sm.head[x + 1])) break;
                }
                if (nlive == 0) continue;
                if (FR && !ignore_delete && any_retract && nlive > 1 &&
                    err_flag)
                    atomicOr(err_flag, PMH_ERR_FIRST_ROW_RETRACT);
                if (!e_best && nlive > 1) continue;
                if (drop_delete && !ps2_isadd(v_best)) continue;
                emit(nloc, s_best);
                nloc++;
            }
            return nloc;
        };

        // --- segment setup (k_merge_tiles' protocol: +1 extra per run)
        if (tid < k) {
            int32_t a = c0[tid], b = c1[tid];
            int32_t ext = (b < (int32_t)lens[tid]) ? 1 : 0;
            sm.seglen[tid] = (b - a) + ext;
            sm.predcand[tid] =
                a > 0 ? key_at(keys[tid].addr0, a - 1, keys[tid].esize)
                      : INT64_MIN;
            sm.head[tid] = a > 0;
        }
        __syncthreads();
        if (tid == 0) {
            int32_t off = 0, real = 0;
            int64_t pred = 0;
            int hp = 0;
            for (int r = 0; r < k; r++) {
                sm.segoff[r] = off;
                real += c1[r] - c0[r];
                off += sm.seglen[r];
                if (sm.head[r]) {
                    if (!hp || sm.predcand[r] > pred) pred = sm.predcand[r];
                    hp = 1;
                }
            }
            sm.segoff[k] = off;
            sm.mtotal = off;
            sm.mreal = real;
            sm.predkey = pred;
            sm.haspred = hp;
        }
        __syncthreads();
        const int32_t M = sm.mtotal;
        const int32_t Mreal = sm.mreal;
        if (Mreal > 0) {
            // --- stage key / packed-seq segments (coalesced per run);
            // deletion-vector tombstones stage as PMH_DEAD (the walk skips
            // them — ApplyDeletionVectorReader semantics)
            uint64_t tkmin = ~0ull, tkmax = 0;
            for (int r = 0; r < k; r++) {
                int32_t off = sm.segoff[r], len = sm.seglen[r];
                int64_t base = c0[r];
                const int kes = keys[r].esize;
                const uint64_t kaddr0 = keys[r].addr0 + (uint64_t)base * kes;
                const int64_t *saddr =
                    reinterpret_cast<const int64_t *>(seqs[r].addr0) + base;
                const int32_t *daddr =
                    reinterpret_cast<const int32_t *>(kinds[r].addr0) + base;
                const uint8_t *tb =
                    tombs && tombs[r]
                        ? reinterpret_cast<const uint8_t *>(tombs[r]) + base
                        : nullptr;
                for (int32_t i = tid; i < len; i += blockDim.x) {
                    const int64_t kv = key_at(kaddr0, i, kes);
                    const uint64_t uk = ukey(kv);
                    if (uk < tkmin) tkmin = uk;
                    if (uk > tkmax) tkmax = uk;
                    sm.skey[off + i] = kv;
                    sm.sseq[off + i] = (tb && tb[i])
                                           ? PMH_DEAD
                                           : ps2_pack(saddr[i], daddr[i]);
                    sm.perm[0][off + i] = (uint16_t)(off + i);
                }
            }
            // block-reduce the tile key range, then repack the staged keys
            // to 32-bit tile-relative offsets when they fit
            for (int off2 = 32; off2; off2 >>= 1) {
                const uint64_t a = __shfl_down(tkmin, off2, 64);
                const uint64_t b = __shfl_down(tkmax, off2, 64);
                if (a < tkmin) tkmin = a;
                if (b > tkmax) tkmax = b;
            }
            if (lane == 0) {
                sm.wkmin[wv] = tkmin;
                sm.wkmax[wv] = tkmax;
            }
            __syncthreads();
            if (tid == 0) {
                uint64_t mn = ~0ull, mx = 0;
#pragma unroll
                for (int w = 0; w < NW; w++) {
                    if (sm.wkmin[w] < mn) mn = sm.wkmin[w];
                    if (sm.wkmax[w] > mx) mx = sm.wkmax[w];
                }
                sm.tile_kmin = mn;
                sm.narrow = (mx - mn) < 0xfffffffeull;
                const uint64_t up = ukey(sm.predkey);
                sm.predkey32 =
                    (sm.haspred && up >= mn && up - mn < 0xfffffffeull)
                        ? (uint32_t)(up - mn)
                        : 0xffffffffu;
            }
            __syncthreads();
            if (sm.narrow) {
                // in-place 64->32-bit repack in two barriered halves (the
                // destination bytes of each half never overlap the other
                // half's pending reads); 4 held values per thread per half
                uint32_t *k32 = reinterpret_cast<uint32_t *>(sm.skey);
#pragma unroll
                for (int half = 0; half < 2; half++) {
                    int64_t hold[4];
#pragma unroll
                    for (int h = 0; h < 4; h++) {
                        const int32_t i =
                            tid + (half * 4 + h) * (int32_t)blockDim.x;
                        hold[h] = i < M ? sm.skey[i] : 0;
                    }
                    __syncthreads();
#pragma unroll
                    for (int h = 0; h < 4; h++) {
                        const int32_t i =
                            tid + (half * 4 + h) * (int32_t)blockDim.x;
                        if (i < M)
                            k32[i] =
                                (uint32_t)(ukey(hold[h]) - sm.tile_kmin);
                    }
                    __syncthreads();
                }
            }

            // --- pairwise stable merge + group heads, generic over the
            // staged key width (uint32 tile-relative fast path; int64
            // fallback for tiles spanning >= 2^32 of key space)
            auto merge_heads = [&](auto *skeyT, auto predk, bool haspred2) {
                for (int width = 1; width < k; width <<= 1) {
                    const int nxt = cur ^ 1;
                    const int CH = 8;
                    int n_chunks = (M + CH - 1) / CH;
                    for (int ch = tid; ch < n_chunks; ch += blockDim.x) {
                        int64_t o = (int64_t)ch * CH;
                        int remaining = (int)(M - o < CH ? M - o : CH);
                        int p = 0;
                        while (remaining > 0) {
                            while ((p + 1) * 2 * width < k &&
                                   sm.segoff[(p + 1) * 2 * width] <= o)
                                p++;
                            int a0 = p * 2 * width;
                            int amid = a0 + width < k ? a0 + width : k;
                            int b1 = a0 + 2 * width < k ? a0 + 2 * width : k;
                            int32_t abase = sm.segoff[a0];
                            int32_t la = sm.segoff[amid] - abase;
                            int32_t lb = sm.segoff[b1] - sm.segoff[amid];
                            int64_t d = o - abase;
                            int32_t lim = la + lb - (int32_t)d;
                            if (lim <= 0) break;
                            int n_out = lim < remaining ? lim : remaining;
                            const uint16_t *pa = &sm.perm[cur][abase];
                            const uint16_t *pb = &sm.perm[cur][abase + la];
                            int32_t ai = corank(d, pa, la, pb, lb, skeyT);
                            int32_t bi = (int32_t)d - ai;
                            uint16_t *out = &sm.perm[nxt][abase + d];
                            for (int x = 0; x < n_out; x++) {
                                bool takeA;
                                if (ai >= la) takeA = false;
                                else if (bi >= lb) takeA = true;
                                else takeA =
                                    !(skeyT[pa[ai]] > skeyT[pb[bi]]);
                                out[x] = takeA ? pa[ai++] : pb[bi++];
                            }
                            o += n_out;
                            remaining -= n_out;
                        }
                    }
                    cur = nxt;
                    __syncthreads();
                }
                const uint16_t *mo2 = sm.perm[cur];
                for (int32_t i = tid; i < M; i += blockDim.x) {
                    auto kk = skeyT[mo2[i]];
                    uint8_t h = (i == 0) ? 1 : (kk != skeyT[mo2[i - 1]]);
                    if (haspred2 && kk == predk) h = 0;
                    sm.head[i] = h;
                }
                __syncthreads();
            };
            if (sm.narrow)
                merge_heads(reinterpret_cast<const uint32_t *>(sm.skey),
                            sm.predkey32, sm.haspred != 0);
            else
                merge_heads(sm.skey, sm.predkey, sm.haspred != 0);

            // --- winner walk (k_merge_tiles' dedup/first-row rules).
            // Pass 0 counts winners per thread; the global offset then
            // arrives via lookback, and pass 1 (below, after the barrier)
            // emits — in split mode STRAIGHT to the output arrays.
            wl = sm.perm[cur ^ 1];
            const int32_t per =
                (Mreal + (int32_t)blockDim.x - 1) / blockDim.x;
            my_lo = tid * per;
            my_hi = my_lo + per < Mreal ? my_lo + per : Mreal;
            int32_t nloc = walk_pass(my_lo, my_hi, [](int32_t, uint16_t) {});
            {
                int32_t incl = nloc;
                for (int off = 1; off < 64; off <<= 1) {
                    int32_t up = __shfl_up(incl, off, 64);
                    if (lane >= off) incl += up;
                }
                if (lane == 63) sm.wave_tot[wv] = incl;
                __syncthreads();
                int32_t add = 0;
                C = 0;
#pragma unroll
                for (int w = 0; w < NW; w++) {
                    if (w < wv) add += sm.wave_tot[w];
                    C += sm.wave_tot[w];
                }
                my_off = add + incl - nloc;
                // publish the aggregate NOW (the emit pass only writes):
                // successors' lookbacks unblock one pass earlier. The count
                // rides in the packed atomic word, so a successor that
                // acquires the flag also gets the payload — no extra fence.
                if (tid == 0 && tile > 0)
                    __hip_atomic_store(&status[tile],
                                       LOOK_AGG | (uint64_t)C,
                                       __ATOMIC_RELEASE,
                                       __HIP_MEMORY_SCOPE_AGENT);
            }
        }

        // --- decoupled lookback for the global offset (empty tiles still
        // publish their zero count here)
        if (tid == 0 && tile > 0 && Mreal == 0)
            __hip_atomic_store(&status[tile], LOOK_AGG | (uint64_t)C,
                               __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        if (wv == 0) {
            int64_t excl = 0;
            if (tile > 0) {
                int64_t look = tile - 1;
                bool done = false;
                while (!done) {
                    int64_t idx = look - lane;
                    uint64_t st = LOOK_PREFIX;  // virtual prefix 0 before t0
                    if (idx >= 0) {
                        int64_t spins = 0;
                        do {
                            st = __hip_atomic_load(&status[idx],
                                                   __ATOMIC_ACQUIRE,
                                                   __HIP_MEMORY_SCOPE_AGENT);
                        } while ((st >> 62) == 0 && ++spins < (1ll << 27));
                        if ((st >> 62) == 0) {  // bounded spin: fail loudly
                            if (err_flag) atomicOr(err_flag, PMH_ERR_LOOKBACK);
                            st = LOOK_PREFIX;
                        }
                    }
                    bool isp = (st >> 62) == 2;
                    uint64_t pm = __ballot(isp);
                    int first = pm ? (int)(__ffsll((unsigned long long)pm) - 1)
                                   : 64;
                    int64_t contrib =
                        (lane <= first) ? (int64_t)(st & LOOK_VAL) : 0;
                    for (int off = 32; off; off >>= 1)
                        contrib += __shfl_down(contrib, off, 64);
                    excl += __shfl(contrib, 0, 64);
                    if (first < 64) done = true;
                    else look -= 64;
                }
            }
            if (lane == 0) {
                __hip_atomic_store(&status[tile],
                                   LOOK_PREFIX | (uint64_t)(excl + C),
                                   __ATOMIC_RELEASE,
                                   __HIP_MEMORY_SCOPE_AGENT);
                sm.s_goff = excl;
                if (tile == n_tiles - 1) *total_out = excl + C;
            }
        }
        __syncthreads();
        if (C == 0) continue;  // nothing to emit (all threads agree: C is
                               // uniform after the pass-0 block reduction)
        // profiling-only: 1 = skip value loop, 2 = skip all emission
        const int ablate =
            (flags >> PMH_FLAG_FABL_SHIFT) & PMH_FLAG_FABL_MASK;
        if (ablate == 2) continue;
        const int64_t goff = sm.s_goff;
        // staged keys may be 32-bit tile-relative: reconstruct the original
        // key as (tile_kmin + rel) mapped back from ukey space
        auto key_of = [&](uint16_t s) -> int64_t {
            if (sm.narrow)
                return (int64_t)((sm.tile_kmin +
                                  reinterpret_cast<const uint32_t *>(
                                      sm.skey)[s]) ^
                                 0x8000000000000000ull);
            return sm.skey[s];
        };

        // emit pass fills the LDS winner list in key order (direct global
        // writes from the walk measured SLOWER: per-thread ranges scatter,
        // while wl-indexed loops below stream perfectly coalesced)
        walk_pass(my_lo, my_hi, [&](int32_t n, uint16_t s_best) {
            wl[my_off + n] = s_best;
        });
        __syncthreads();

        // per-thread slot map over the flat element space (computed once,
        // reused by every column): slot s covers element tid + s*T
        constexpr int RMAX =
            (PMH_TILE_MAX + PMH_TILE_THREADS - 1) / PMH_TILE_THREADS;
        // packed (run << PMH_ROW_BITS) | row per slot; ~0u = dead slot
        uint32_t smap[RMAX];
#pragma unroll
        for (int s = 0; s < RMAX; s++) {
            int32_t e = tid + s * PMH_TILE_THREADS;
            smap[s] = ~0u;
            if (e < M) {
                int r = 0;
                while (r + 1 < k && sm.segoff[r + 1] <= e) r++;
                smap[s] = ((uint32_t)r << PMH_ROW_BITS) |
                          (uint32_t)(c0[r] + (e - sm.segoff[r]));
            }
        }

        // register staging: issue a column's gathers into registers FIRST
        // (no LDS write yet, so the loads stay in flight), do independent
        // work (emit the previous column from the other slab), then write
        // the registers to LDS — the vmcnt wait lands after the overlap
        // work instead of before it.
        int64_t rg[RMAX];
        auto stage_load = [&](int c, int64_t *regs) {
#pragma unroll
            for (int s = 0; s < RMAX; s++) {
                if (smap[s] == ~0u) continue;
                const DevCol &dc =
                    cols[(smap[s] >> PMH_ROW_BITS) * n_cols + c];
                const int64_t row = smap[s] & PMH_ROW_MASK;
                regs[s] = dc.esize == 8
                    ? reinterpret_cast<const int64_t *>(dc.addr0)[row]
                    : (int64_t)reinterpret_cast<const int32_t *>(
                          dc.addr0)[row];
            }
        };
        auto stage_write = [&](int c, const int64_t *regs, uint8_t *slab) {
            const bool wide = dt_wide(col_dtype[c]);
#pragma unroll
            for (int s = 0; s < RMAX; s++) {
                if (smap[s] == ~0u) continue;
                int32_t e = tid + s * PMH_TILE_THREADS;
                if (wide)
                    reinterpret_cast<int64_t *>(slab)[e] = regs[s];
                else
                    reinterpret_cast<int32_t *>(slab)[e] = (int32_t)regs[s];
            }
        };
        auto stage_valid = [&](int c, uint8_t *slab) {
#pragma unroll
            for (int s = 0; s < RMAX; s++) {
                if (smap[s] == ~0u) continue;
                int32_t e = tid + s * PMH_TILE_THREADS;
                slab[e] = member_valid(cols, n_cols, smap[s], c);
            }
        };
        auto emit_col = [&](int c, const uint8_t *slab,
                            const uint8_t *vslab) {
            if (ablate == 3) return;  // profiling: staging without emission
            const int dt = col_dtype[c];
            const bool wide = dt_wide(dt);
            uint8_t *ov = (col_nullable[c] && out_valid[c]) ? out_valid[c]
                                                            : nullptr;
            for (int32_t i = tid; i < C; i += blockDim.x) {
                uint16_t s = wl[i];
                int64_t v = wide
                    ? reinterpret_cast<const int64_t *>(slab)[s]
                    : (int64_t)reinterpret_cast<const int32_t *>(slab)[s];
                out_store(out_ptrs[c], dt, goff + i, v);
                if (ov) ov[goff + i] = vslab ? vslab[s] : 1;
            }
        };
        auto next_col = [&](int c) -> int {
            for (c++; c < n_cols; c++)
                if (c != seq_col && c != kind_col && c != key_col) return c;
            return -1;
        };

        bool any_null = false;
        for (int c = 0; c < n_cols; c++)
            if (col_nullable[c]) any_null = true;
        // emission mode (the PMH_FLAG_FSTAGE field): 0 = direct gather per
        // winner (high MLP, no per-column barriers — winners are ~72% dense
        // within their run segments, so the 64B gather lines are mostly reused
        // and the working set stays XCD-L2-resident); 1 = LDS-staged columns
        // (coalesced loads but burst-and-wait per column: measured slower,
        // kept for A/B via PMH_FSTAGE)
        const bool staged =
            (flags >> PMH_FLAG_FSTAGE_SHIFT) & PMH_FLAG_FSTAGE_MASK;

        // --- overlap window 1: first column's gathers fly while the
        // key/seq/kind emit reads the merge arrays
        int cfirst = ablate == 1 ? -1 : next_col(-1);
        if (staged && cfirst >= 0 && !any_null) stage_load(cfirst, rg);

        // emit key / seq / kind straight from the merge arrays
        if (key_col >= 0) {
            const int kdt = col_dtype[key_col];
            for (int32_t i = tid; i < C; i += blockDim.x) {
                out_store(out_ptrs[key_col], kdt, goff + i, key_of(wl[i]));
            }
        }
        for (int32_t i = tid; i < C; i += blockDim.x) {
            int64_t w = sm.sseq[wl[i]];
            ((int64_t *)out_ptrs[seq_col])[goff + i] = w >> 2;
            ((int8_t *)out_ptrs[kind_col])[goff + i] = (int8_t)ps2_kind(w);
        }
        if (dense_winners) {
            // SPLIT mode: publish packed winners densely; value columns are
            // emitted by k_emit_dense (full occupancy, no LDS) right after
            // this kernel
            for (int32_t i = tid; i < C; i += blockDim.x) {
                uint16_t s = wl[i];
                int r = 0;
                while (r + 1 < k && sm.segoff[r + 1] <= (int32_t)s) r++;
                dense_winners[goff + i] =
                    ((uint32_t)r << PMH_ROW_BITS) |
                    (uint32_t)(c0[r] + ((int32_t)s - sm.segoff[r]));
            }
            __syncthreads();
            continue;
        }
        if (cfirst < 0) {
            __syncthreads();
            continue;
        }
        if (!staged) {
            // --- direct-gather emission: thread i owns winners i, i+T,
            // i+2T, ... R at a time wave-strided (coalesced stores); per
            // column R independent gathers stay in flight. No barriers, no
            // LDS traffic — overlaps freely with the other workgroup's
            // merge phase on the CU.
            constexpr int R = 4;
            for (int32_t base = 0; base < C;
                 base += (int32_t)blockDim.x * R) {
                int32_t i0 = base + tid;
                if (i0 >= C) break;
                int run[R];
                int64_t row[R];
                int32_t idx[R];
                int nr = 0;
#pragma unroll
                for (int x = 0; x < R; x++) {
                    int32_t i = i0 + x * (int32_t)blockDim.x;
                    bool live = i < C;
                    idx[x] = i;
                    if (live) {
                        nr = x + 1;
                        uint16_t s = wl[i];
                        int r = 0;
                        while (r + 1 < k && sm.segoff[r + 1] <= (int32_t)s)
                            r++;
                        run[x] = r;
                        row[x] = c0[r] + ((int32_t)s - sm.segoff[r]);
                    } else {
                        run[x] = run[0];
                        row[x] = row[0];
                    }
                }
                for (int c = cfirst; c >= 0; c = next_col(c)) {
                    const int dt = col_dtype[c];
                    uint8_t *ov = (col_nullable[c] && out_valid[c])
                                      ? out_valid[c] : nullptr;
                    if (ov) {
                        uint8_t vv[R];
#pragma unroll
                        for (int x = 0; x < R; x++)
                            vv[x] = col_valid(cols[run[x] * n_cols + c],
                                              row[x]);
#pragma unroll
                        for (int x = 0; x < R; x++)
                            if (x < nr) ov[goff + idx[x]] = vv[x];
                    }
                    if (dt_wide(dt)) {
                        int64_t v[R];
#pragma unroll
                        for (int x = 0; x < R; x++)
                            v[x] = reinterpret_cast<const int64_t *>(
                                cols[run[x] * n_cols + c].addr0)[row[x]];
#pragma unroll
                        for (int x = 0; x < R; x++)
                            if (x < nr)
                                ((int64_t *)out_ptrs[c])[goff + idx[x]] =
                                    v[x];
                    } else {
                        int32_t v[R];
#pragma unroll
                        for (int x = 0; x < R; x++)
                            v[x] = reinterpret_cast<const int32_t *>(
                                cols[run[x] * n_cols + c].addr0)[row[x]];
#pragma unroll
                        for (int x = 0; x < R; x++) {
                            if (x >= nr) continue;
                            switch (dt) {
                            case PMH_DT_INT8:
                                ((int8_t *)out_ptrs[c])[goff + idx[x]] =
                                    (int8_t)v[x];
                                break;
                            case PMH_DT_INT16:
                                ((int16_t *)out_ptrs[c])[goff + idx[x]] =
                                    (int16_t)v[x];
                                break;
                            default: ((int32_t *)out_ptrs[c])[goff + idx[x]] =
                                        v[x]; break;
                            }
                        }
                    }
                }
            }
            __syncthreads();  // wl/segoff stay live until every thread done
            continue;
        }
        __syncthreads();  // skey/sseq die; vbuf slabs take their space
        if (any_null) {
            // nullable plans: values in slab 0, validity bytes in slab 1
            // (single-buffered; the dedup headline configs carry no nulls)
            for (int c = cfirst; c >= 0; c = next_col(c)) {
                stage_load(c, rg);
                stage_write(c, rg, sm.vbuf[0]);
                const bool nul = col_nullable[c];
                if (nul) stage_valid(c, sm.vbuf[1]);
                __syncthreads();
                emit_col(c, sm.vbuf[0], nul ? sm.vbuf[1] : nullptr);
                __syncthreads();
            }
        } else {
            // double slab + register pipeline: column c+1's gathers are in
            // flight while column c is emitted; one barrier per column
            stage_write(cfirst, rg, sm.vbuf[0]);
            int prev = cfirst, slot = 0;
            for (int c = next_col(cfirst); c >= 0; c = next_col(c)) {
                stage_load(c, rg);  // loads fly across the barrier + emit
                __syncthreads();  // slab `slot` ready; slot^1 drained
                emit_col(prev, sm.vbuf[slot], nullptr);
                stage_write(c, rg, sm.vbuf[slot ^ 1]);
                prev = c;
                slot ^= 1;
            }
            __syncthreads();
            emit_col(prev, sm.vbuf[slot], nullptr);
        }
        __syncthreads();  // all slabs drained before the next tile
    }
}


// ------------------------------------------------------------ k_emit_dense
//
// Value emission for the SPLIT fused path: k_merge_emit already wrote key/
// seq/kind and the packed winners DENSELY in output order, so this kernel
// is a pure gather — no LDS, no tile search, 60-VGPR occupancy (8 waves/
// SIMD vs the merge kernel's 4). Winners are ~72% dense inside their run
// segments, so gather lines are mostly reused and stay XCD-L2-resident.
__global__ void k_emit_dense(const DevCol *cols, const uint8_t *col_dtype,
                             const uint8_t *col_nullable, int n_cols,
                             int key_col, int seq_col, int kind_col,
                             const uint32_t *winners,
                             int64_t t0, int64_t t1,
                             const uint64_t *status,
                             void *const *out_ptrs,
                             uint8_t *const *out_valid) {
    // output range of tile chunk [t0, t1): the inclusive lookback prefixes
    // of t0-1 / t1-1 (both PREFIX-published — the chunk's merge pass
    // completed before this launch was released by its event)
    constexpr int R = 4;
    const int64_t lo =
        t0 > 0 ? (int64_t)(status[t0 - 1] & LOOK_VAL) : 0;
    const int64_t total = (int64_t)(status[t1 - 1] & LOOK_VAL);
    const int64_t slice_lo = lo + slice_lo_of(total - lo);
    const int64_t slice_hi = lo + slice_hi_of(total - lo);
    for (int64_t base = slice_lo; base < slice_hi;
         base += (int64_t)blockDim.x * R) {
        int64_t i0 = base + threadIdx.x;
        if (i0 >= slice_hi) break;
        int run[R];
        int64_t row[R], idx[R];
        int nr = 0;
#pragma unroll
        for (int x = 0; x < R; x++) {
            int64_t i = i0 + (int64_t)x * blockDim.x;
            bool live = i < slice_hi;
            idx[x] = i;
            if (live) {
                nr = x + 1;
                uint32_t packed = winners[i];
                run[x] = packed >> PMH_ROW_BITS;
                row[x] = packed & PMH_ROW_MASK;
            } else {
                run[x] = run[0];
                row[x] = row[0];
            }
        }
        for (int c = 0; c < n_cols; c++) {
            if (c == key_col || c == seq_col || c == kind_col) continue;
            const int dt = col_dtype[c];
            if (col_nullable[c] && out_valid[c]) {
                uint8_t vv[R];
#pragma unroll
                for (int x = 0; x < R; x++)
                    vv[x] = col_valid(cols[run[x] * n_cols + c], row[x]);
#pragma unroll
                for (int x = 0; x < R; x++)
                    if (x < nr) out_valid[c][idx[x]] = vv[x];
            }
            if (dt_wide(dt)) {
                int64_t v[R];
#pragma unroll
                for (int x = 0; x < R; x++)
                    v[x] = reinterpret_cast<const int64_t *>(
                        cols[run[x] * n_cols + c].addr0)[row[x]];
#pragma unroll
                for (int x = 0; x < R; x++)
                    if (x < nr) ((int64_t *)out_ptrs[c])[idx[x]] = v[x];
            } else {
                int32_t v[R];
#pragma unroll
                for (int x = 0; x < R; x++)
                    v[x] = reinterpret_cast<const int32_t *>(
                        cols[run[x] * n_cols + c].addr0)[row[x]];
#pragma unroll
                for (int x = 0; x < R; x++) {
                    if (x >= nr) continue;
                    switch (dt) {
                    case PMH_DT_INT8:
                        ((int8_t *)out_ptrs[c])[idx[x]] = (int8_t)v[x];
                        break;
                    case PMH_DT_INT16:
                        ((int16_t *)out_ptrs[c])[idx[x]] = (int16_t)v[x];
                        break;
                    default: ((int32_t *)out_ptrs[c])[idx[x]] =
                                 v[x]; break;
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------ k_scan_tiles
// Exclusive scan of tile_counts (single workgroup, chunked).
__global__ void k_scan_tiles(const int32_t *tile_counts, int64_t n_tiles,
                             int64_t *tile_offsets, int64_t *total_out) {
    // wave shuffle scan + one barrier per chunk (k_merge_tiles' block scan);
    // the wave totals alternate between two buffers, so the next chunk's
    // barrier also orders this chunk's reads before the buffer's reuse
    constexpr int NW = PMH_TILE_THREADS / 64;
    __shared__ int64_t wave_tot[2][NW];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    int64_t running = 0;  // every thread carries the same value
    int buf = 0;
    int64_t i = threadIdx.x;
    int64_t v = i < n_tiles ? tile_counts[i] : 0;
    for (int64_t base = 0; base < n_tiles; base += PMH_TILE_THREADS) {
        // next chunk's load in flight across the scan
        const int64_t in = i + PMH_TILE_THREADS;
        const int64_t vn = in < n_tiles ? tile_counts[in] : 0;
        int64_t incl = v;
        for (int off = 1; off < 64; off <<= 1) {
            int64_t up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        if (lane == 63) wave_tot[buf][wv] = incl;
        __syncthreads();
        int64_t add = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) {
            const int64_t t = wave_tot[buf][w];
            if (w < wv) add += t;
            tot += t;
        }
        if (i < n_tiles) tile_offsets[i] = running + add + incl - v;
        running += tot;
        buf ^= 1;
        i = in;
        v = vn;
    }
    if (threadIdx.x == 0) *total_out = running;
}

// ------------------------------------------------------------ k_emit
// Phase 2: gather winner rows into contiguous output columns.
// One workgroup per tile (grid-stride); thread per output row; inner loop
// over columns. Output writes are coalesced per column.
template <int R>
__global__ void k_emit(const DevCol *cols /* n_runs * n_cols, run-major */,
                       const uint8_t *col_dtype, const uint8_t *col_nullable,
                       int n_cols, int n_emit, int k, const uint32_t *winners,
                       const int32_t *tile_counts,
                       const int64_t *tile_offsets, int64_t n_tiles,
                       int64_t tile_rows, const int64_t *total_out,
                       void *const *out_ptrs, uint8_t *const *out_valid) {
    // n_emit == n_cols except under the profiling-only PMH_EMIT_COLS knob
    // (the columns past it are then left unwritten).
    // Flat grid-stride over the DENSE output index space (tile_offsets is an
    // exclusive scan of tile_counts, so tile t owns output ranks
    // [off[t], off[t]+cnt[t]) contiguously). R rows per thread iteration:
    // independent gathers per column keep R x n_cols loads in flight (emit
    // was 96% latency-parked, profiles/r01_c2_pmc.md) without idling tile
    // remainders.
    // Each block owns a CONTIGUOUS output slice so its gathers stay within a
    // few tiles' source segments (~130 KB working set -> XCD-L2 resident;
    // grid-striding spread every block over the whole output and thrashed L2).
    const int64_t total = *total_out;
    const int64_t slice_lo = slice_lo_of(total);
    const int64_t slice_hi = slice_hi_of(total);
    // one tile binary search per thread; ranks then advance monotonically
    // within the slice, so the tile cursor just walks forward. The R rows
    // per thread are WAVE-STRIDED (i = base + tid + x*blockDim), so every
    // access stays fully coalesced while keeping R loads in flight —
    // thread-contiguous R strides the lanes by R and breaks coalescing.
    int64_t t = -1;
    for (int64_t base = slice_lo; base < slice_hi;
         base += (int64_t)blockDim.x * R) {
        int64_t i_first = base + threadIdx.x;
        if (i_first >= slice_hi) break;
        // first iteration: locate owning tile
        if (t < 0) t = tile_seek(tile_offsets, n_tiles, i_first);
        int64_t idx[R];
        int run[R];
        uint32_t row[R];
        int nr = 0;
#pragma unroll
        for (int x = 0; x < R; x++) {
            int64_t i = base + threadIdx.x + (int64_t)x * blockDim.x;
            bool live = i < slice_hi;
            idx[x] = i;
            if (live) {
                nr = x + 1;
                // dense ranks: advance tile while i falls past its count
                t = tile_walk(tile_offsets, n_tiles, t, i);
                uint32_t packed =
                    winners[t * (tile_rows + PMH_MAX_RUNS) +
                            (i - tile_offsets[t])];
                run[x] = packed >> PMH_ROW_BITS;
                row[x] = packed & PMH_ROW_MASK;
            } else {  // dead lane: duplicate x=0's gather, stores are guarded
                run[x] = run[0];
                row[x] = row[0];
            }
        }
        for (int c = 0; c < n_emit; c++) {
            if (col_nullable[c] && out_valid[c]) {
                // winner's validity byte (dedup keeps the record as-is)
#pragma unroll
                for (int x = 0; x < R; x++) {
                    if (x >= nr) continue;
                    out_valid[c][idx[x]] =
                        col_valid(cols[run[x] * n_cols + c], row[x]);
                }
            }
            switch (col_dtype[c]) {
            case PMH_DT_INT8: {  // from INT32-stored parquet TINYINT
                int32_t v[R];
#pragma unroll
                for (int x = 0; x < R; x++)
                    v[x] = col_load<int32_t>(cols[run[x] * n_cols + c], row[x]);
#pragma unroll
                for (int x = 0; x < R; x++)
                    if (x < nr)
                        ((int8_t *)out_ptrs[c])[idx[x]] = (int8_t)v[x];
                break;
            }
            case PMH_DT_INT16: {  // from INT32-stored parquet SMALLINT
                int32_t v[R];
#pragma unroll
                for (int x = 0; x < R; x++)
                    v[x] = col_load<int32_t>(cols[run[x] * n_cols + c], row[x]);
#pragma unroll
                for (int x = 0; x < R; x++)
                    if (x < nr)
                        ((int16_t *)out_ptrs[c])[idx[x]] = (int16_t)v[x];
                break;
            }
            case PMH_DT_INT32:
            case PMH_DT_FLOAT32:
            case PMH_DT_STRING: {  // string ids ride as int32
                int32_t v[R];
#pragma unroll
                for (int x = 0; x < R; x++)
                    v[x] = col_load<int32_t>(cols[run[x] * n_cols + c], row[x]);
#pragma unroll
                for (int x = 0; x < R; x++)
                    if (x < nr) ((int32_t *)out_ptrs[c])[idx[x]] = v[x];
                break;
            }
            case PMH_DT_INT64:
            case PMH_DT_FLOAT64: {
                int64_t v[R];
#pragma unroll
                for (int x = 0; x < R; x++)
                    v[x] = col_load<int64_t>(cols[run[x] * n_cols + c], row[x]);
#pragma unroll
                for (int x = 0; x < R; x++)
                    if (x < nr) ((int64_t *)out_ptrs[c])[idx[x]] = v[x];
                break;
            }
            default: break;
            }
        }
    }
}

// ------------------------------------------------------ k_emit_contig
//
// k_emit with its descriptors in LDS, for plans whose tables fit. Same work
// division: a contiguous output slice per block, wave-strided rows, dead lanes
// repeat row 0's gather with their stores guarded. What differs is that
// nothing inside the row / column loops depends on a descriptor read from
// global memory -- k_emit pays dependent round trips per row and column
// (descriptor, then data), with every wait a full drain, so its R "parallel"
// gathers run one after another (profiles/emit_phases.md):
//  * addr0 / valid0 of the n_desc runs the winners can name, and per column
//    {list position, output pointer, validity output pointer}, are staged in
//    LDS once per block; a gather address is one LDS read + row * width;
//  * the tile that owns slice_lo is searched once per block and EMIT_WIN + 1
//    tile offsets from there are staged; each thread's tile cursor walks that
//    window in registers/LDS (global reads only past the window, which takes
//    a run of empty tiles or a very coarse grid);
//  * the R winner loads of an iteration are issued together;
//  * columns are ordered into four lists by OUTPUT width (1 / 2 / 4 / 8
//    bytes; the first three load 4-byte stored values) and each list is
//    walked in groups of G: all G x R gathers are issued, then the G x R
//    stores, each waiting on its own gather only;
//  * data moves through address_space(1) pointers (global_*, not flat_*).
// Barriers: three, all in the prologue, reached by every thread of a block
// that has a non-empty slice; a block with an empty slice leaves before the
// first one (block-uniform). The per-thread exit sits after the last barrier.
constexpr int EMIT_WIN = 64;
constexpr int EMIT_THREADS = 256;
constexpr int EMIT_LDS_MAX = 16384;  // LDS never the occupancy limit

// LDS bytes of k_emit_contig's tables (the launcher falls back to k_emit
// when they exceed EMIT_LDS_MAX)
static inline int64_t emit_contig_lds(int64_t n_desc, int64_t n_cols) {
    return 16 * n_desc * n_cols + 16 * n_cols + 8 * (EMIT_WIN + 1) + 16 +
           2 * n_cols;
}

template <typename T>
DEV void gstore(uint64_t addr, T v) {
    *reinterpret_cast<__attribute__((address_space(1))) T *>(addr) = v;
}

DEV uint64_t uniform64(uint64_t v) {  // block-uniform value -> SGPR pair
    // the builtin returns int: widen each half as unsigned, or a low half
    // with bit 31 set would sign-extend over the high half
    const uint32_t hi =
        (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    const uint32_t lo =
        (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    return ((uint64_t)hi << 32) | (uint64_t)lo;
}

// Store row x of this thread's R rows at output index base + x *
// EMIT_THREADS + tid. ob = column base + base * sizeof(T) is block-uniform
// (a scalar register pair), so the store addresses as scalar base + one
// small per-lane offset shared by all x + an immediate.
template <typename T>
DEV void emit_store(uint64_t ob, int x, uint32_t tid, T v) {
    gstore<T>(ob + (uint64_t)(tid * (uint32_t)sizeof(T)) +
                  (uint64_t)(x * EMIT_THREADS * (int)sizeof(T)),
              v);
}

// G columns at list positions [p, p + G) for this thread's R rows: all G x R
// gathers are issued, then the G x R stores. L is the stored (loaded) type, S
// the output type the store narrows to. s_addr / s_valid are indexed
// [run * n_cols + position]; dl[x] is row x's run * n_cols. FULL: every lane
// of the block has all R rows live (block-uniform), so no store is guarded.
// With FULL every loaded register is consumed on every path; that and the
// absence of any dtype branch between loads and stores is what lets the
// compiler issue the next group's gathers without first draining this
// group's stores.
template <typename L, typename S, int G, int R, bool FULL>
DEV void emit_group(const uint64_t *s_addr, const uint64_t *s_valid,
                    const uint64_t *s_out, const uint64_t *s_ov, int p,
                    const int (&dl)[R], const uint32_t (&row)[R],
                    int64_t base, uint32_t tid, int nr) {
    // validity bytes of the group's nullable columns (valid0 == 0: the run
    // staged no nulls for this column)
#pragma nounroll
    for (int g = 0; g < G; g++) {
        const uint64_t ov0 = uniform64(s_ov[p + g]);
        if (!ov0) continue;
        const uint64_t ov = ov0 + (uint64_t)base;
        uint8_t vb[R];
#pragma unroll
        for (int x = 0; x < R; x++) {
            const uint64_t va = s_valid[dl[x] + p + g];
            vb[x] = va ? gload<uint8_t>(va + row[x]) : (uint8_t)1;
        }
#pragma unroll
        for (int x = 0; x < R; x++)
            if (FULL || x < nr) emit_store<uint8_t>(ov, x, tid, vb[x]);
    }
    L v[G][R];
#pragma unroll
    for (int g = 0; g < G; g++)
#pragma unroll
        for (int x = 0; x < R; x++)
            v[g][x] = gload<L>(
                s_addr[dl[x] + p + g] +
                (uint64_t)(row[x] * (uint32_t)sizeof(L)));  // row < 2^27
#pragma unroll
    for (int g = 0; g < G; g++) {
        const uint64_t ob =
            uniform64(s_out[p + g] + (uint64_t)base * sizeof(S));
#pragma unroll
        for (int x = 0; x < R; x++)
            if (FULL || x < nr) emit_store<S>(ob, x, tid, (S)v[g][x]);
    }
}

// One list of columns, positions [p_lo, p_hi): groups of G, then the
// remainder in groups of G / 2 ... 1.
template <typename L, typename S, int G, int R, bool FULL>
DEV void emit_list(const uint64_t *s_addr, const uint64_t *s_valid,
                   const uint64_t *s_out, const uint64_t *s_ov, int p_lo,
                   int p_hi, const int (&dl)[R], const uint32_t (&row)[R],
                   int64_t base, uint32_t tid, int nr) {
    int p = p_lo;
    for (; p + G <= p_hi; p += G)
        emit_group<L, S, G, R, FULL>(s_addr, s_valid, s_out, s_ov, p, dl, row,
                                     base, tid, nr);
    if constexpr (G > 1)
        emit_list<L, S, G / 2, R, FULL>(s_addr, s_valid, s_out, s_ov, p, p_hi,
                                        dl, row, base, tid, nr);
}

template <int R, int G4, int G8>
__launch_bounds__(EMIT_THREADS) __global__
void k_emit_contig(const DevCol *cols /* n_desc * n_cols, run-major */,
                   const uint8_t *col_dtype, const uint8_t *col_nullable,
                   int n_cols, int n_emit, int n_desc,
                   const uint32_t *winners, const int64_t *tile_offsets,
                   int64_t n_tiles, int64_t tile_rows,
                   const int64_t *total_out, void *const *out_ptrs,
                   uint8_t *const *out_valid) {
    extern __shared__ uint64_t emit_smem[];
    const int n_ent = n_desc * n_cols;
    uint64_t *s_addr = emit_smem;                  // [n_ent] run, position
    uint64_t *s_valid = s_addr + n_ent;            // [n_ent] run, position
    uint64_t *s_out = s_valid + n_ent;             // [n_cols] by position
    uint64_t *s_ov = s_out + n_cols;               // [n_cols] by position
    int64_t *s_toff = (int64_t *)(s_ov + n_cols);  // [EMIT_WIN + 1]
    int *s_cnt = (int *)(s_toff + EMIT_WIN + 1);   // list lengths {1,2,4,8}
    uint8_t *s_pos = (uint8_t *)(s_cnt + 4);       // [n_cols] column -> position
    uint8_t *s_cls = s_pos + n_cols;               // [n_cols] by column

    const int tid = threadIdx.x;
    const int64_t total = *total_out;
    const int64_t slice_lo = slice_lo_of(total);
    const int64_t slice_hi = slice_hi_of(total);
    if (slice_lo >= slice_hi) return;  // block-uniform, before any barrier

    // a column's list = the width its output is stored at (TINYINT / SMALLINT
    // narrow from their INT32-stored values; floats and string ids move as
    // raw words); 0 = not emitted
    for (int c = tid; c < n_cols; c += EMIT_THREADS)
        s_cls[c] = c < n_emit ? pmh_out_width(col_dtype[c]) : 0;
    // the tile that owns slice_lo (block-uniform search, every thread)
    const int64_t t0 = tile_seek(tile_offsets, n_tiles, slice_lo);
    for (int j = tid; j <= EMIT_WIN; j += EMIT_THREADS)
        s_toff[j] = t0 + j < n_tiles ? tile_offsets[t0 + j] : INT64_MAX;
    __syncthreads();
    // order the columns: the 1-, 2-, 4- and 8-byte lists one after another,
    // each in column order
    for (int c = tid; c < n_cols; c += EMIT_THREADS) {
        const int cls = s_cls[c];
        int n_of[4] = {0, 0, 0, 0};  // list lengths, by log2(width)
        int before = 0;
        for (int j = 0; j < n_cols; j++) {
            const int cj = s_cls[j];
#pragma unroll
            for (int w = 0; w < 4; w++) n_of[w] += cj == (1 << w);
            before += (j < c && cj == cls);
        }
        if (c == 0) {
#pragma unroll
            for (int w = 0; w < 4; w++) s_cnt[w] = n_of[w];
        }
        if (cls) {
            int p = before;
#pragma unroll
            for (int w = 0; w < 3; w++) p += (1 << w) < cls ? n_of[w] : 0;
            s_pos[c] = (uint8_t)p;
            s_out[p] = (uint64_t)out_ptrs[c];
            s_ov[p] = col_nullable[c] ? (uint64_t)out_valid[c] : 0;
        }
    }
    __syncthreads();
    // descriptors of the emitted columns, read once
    for (int e = tid; e < n_ent; e += EMIT_THREADS) {
        const int r = e / n_cols, c = e - r * n_cols;
        if (!s_cls[c]) continue;
        const int d = r * n_cols + s_pos[c];
        s_addr[d] = cols[e].addr0;
        s_valid[d] = cols[e].valid0;
    }
    __syncthreads();
    const int e1 = s_cnt[0], e2 = e1 + s_cnt[1], e4 = e2 + s_cnt[2],
              e8 = e4 + s_cnt[3];  // list ends

    // tile cursor: tile t0 + tr owns ranks [cur, nxt); offsets come from the
    // window, and from global memory only past it
    const int64_t wstride = tile_rows + PMH_MAX_RUNS;
    auto toff = [&](int64_t j) -> int64_t {
        if (j >= n_tiles) return INT64_MAX;
        return j - t0 <= EMIT_WIN
                   ? s_toff[j - t0]
                   : gload<int64_t>((uint64_t)(tile_offsets + j));
    };
    int tr = 0;
    int64_t cur = s_toff[0];
    int64_t nxt = s_toff[1];
    for (int64_t base = slice_lo; base < slice_hi;
         base += (int64_t)EMIT_THREADS * R) {
        const int64_t i0 = base + tid;
        if (i0 >= slice_hi) break;  // after the last barrier
        uint64_t wa[R];
        int nr = 0;
#pragma unroll
        for (int x = 0; x < R; x++) {
            const int64_t i = i0 + x * EMIT_THREADS;
            if (i < slice_hi) {
                nr = x + 1;
                // dense ranks: advance while i falls past the tile's count
                // (nxt is INT64_MAX past the last tile)
                while (nxt <= i) {
                    tr++;
                    cur = nxt;
                    nxt = toff(t0 + tr + 1);
                }
                wa[x] = (uint64_t)(winners + (t0 + tr) * wstride + (i - cur));
            } else {  // dead lane: repeat x = 0's gather, stores are guarded
                wa[x] = wa[0];
            }
        }
        uint32_t packed[R];
#pragma unroll
        for (int x = 0; x < R; x++) packed[x] = gload<uint32_t>(wa[x]);
        int dl[R];
        uint32_t row[R];
#pragma unroll
        for (int x = 0; x < R; x++) {
            dl[x] = (int)(packed[x] >> PMH_ROW_BITS) * n_cols;
            row[x] = packed[x] & PMH_ROW_MASK;
        }
        auto lists = [&](auto full) {
            constexpr bool FULL = decltype(full)::value;
            const uint32_t utid = (uint32_t)tid;
            emit_list<int32_t, int8_t, G4, R, FULL>(
                s_addr, s_valid, s_out, s_ov, 0, e1, dl, row, base, utid, nr);
            emit_list<int32_t, int16_t, G4, R, FULL>(
                s_addr, s_valid, s_out, s_ov, e1, e2, dl, row, base, utid, nr);
            emit_list<int32_t, int32_t, G4, R, FULL>(
                s_addr, s_valid, s_out, s_ov, e2, e4, dl, row, base, utid, nr);
            emit_list<int64_t, int64_t, G8, R, FULL>(
                s_addr, s_valid, s_out, s_ov, e4, e8, dl, row, base, utid, nr);
        };
        // block-uniform: only a slice's last iteration has dead rows
        if (base + (int64_t)EMIT_THREADS * R <= slice_hi)
            lists(std::true_type{});
        else
            lists(std::false_type{});
    }
}

// ------------------------------------------------------ k_emit_stream
//
// Emit without a gather. The winners of tile t that come from run r all lie
// in the slice of run r that k_merge_tiles staged for that tile, so a block
// takes one tile at a time (grid-stride) and, per group of columns,
//  1. loads the tile's per-run slices of the group's columns the way
//     tile_prefetch loads key / seq / kind: consecutive lanes read
//     consecutive rows, dead slots clamp to the last element, everything
//     issued back to back into registers;
//  2. puts them into LDS at the merge's own flat slot;
//  3. has each output row read its winner's slot and store coalesced at
//     out[c] + (tile_offsets[t] + j) * width.
// The 28 % losers of the flagship shape are read too; what goes away is one
// L2 request per 20-30 useful bytes of a 4-byte column and a 64-bit address
// per gather in flight (profiles/emit_stream_phases.md).
// Pipelining: one register set. As soon as a group's registers are in LDS the
// next group's loads (at a tile's last group: the next tile's setup, winner
// words and first group) are issued, ahead of this group's permute and
// stores. The slot mapping and the group plan are emit_stream_core.h's.
// Columns are ordered into lists by output width exactly as in k_emit_contig;
// a group never spans two lists. Validity is not streamed: the launcher
// sends a plan with a nullable emitted column to k_emit_contig.
// Barriers: three in the prologue, two per group; all block-uniform.
constexpr int EMS_THREADS = PMH_TILE_THREADS;
constexpr int EMS_ITER = PMH_TILE_ITER;
constexpr int64_t EMS_LDS_DEFAULT = 60 * 1024;  // data bytes per block

// LDS bytes of k_emit_stream's tables, ahead of the data area
__host__ __device__ static inline int64_t emit_stream_tables(int64_t k,
                                                             int64_t n_cols) {
    const int64_t b = 8 * k * n_cols + 8 * n_cols + 32 +
                      2 * (n_cols + 1) + 3 * n_cols;
    return (b + 15) & ~(int64_t)15;
}

// The group loop's body is full of values that do not change from group to
// group (slot * width + LDS base, tid * width, ... for every slot and every
// width). Hoisted out of the loop they cost more registers than the kernel
// has (230 VGPRs unbounded, 440 bytes of scratch per lane at 128); an empty
// asm on the per-thread inputs keeps the derived values inside the loop.
template <typename T>
DEV T ems_keep(T x) {
    asm volatile("" : "+v"(x));
    return x;
}

// W-byte loads of a group's n columns (list positions p ...) for this
// thread's slots; an 8-byte column takes two of the 32-bit register rows.
template <int W, int GU>
DEV void ems_load(const uint64_t *s_addr, int p, int n, int n_cols,
                  const uint32_t (&src)[EMS_ITER],
                  uint32_t (&v)[GU][EMS_ITER]) {
#pragma unroll
    for (int g = 0; g < GU * 4 / W; g++) {
        if (g >= n) break;  // block-uniform
#pragma unroll
        for (int s = 0; s < EMS_ITER; s++) {
            const uint32_t sr = ems_keep(src[s]);  // run:5 | row:27
            const uint64_t a =
                s_addr[(sr >> PMH_ROW_BITS) * (uint32_t)n_cols + p + g] +
                (uint64_t)((sr & PMH_ROW_MASK) * (uint32_t)W);
            if constexpr (W == 8) {
                const uint64_t x = gload<uint64_t>(a);
                v[2 * g][s] = (uint32_t)x;
                v[2 * g + 1][s] = (uint32_t)(x >> 32);
            } else {
                v[g][s] = gload<uint32_t>(a);
            }
        }
        // one column's lookups and addresses live at a time (registers),
        // as in tile_prefetch; every load is still issued before any wait
        __builtin_amdgcn_sched_barrier(0);
    }
}

// registers -> LDS at slot tid + s * EMS_THREADS; column g at g * TILE_MAX
template <int W, int GU>
DEV void ems_fill(uint8_t *buf, int n, int32_t m, int tid,
                  const uint32_t (&v)[GU][EMS_ITER]) {
#pragma unroll
    for (int g = 0; g < GU * 4 / W; g++) {
        if (g >= n) break;
        const int32_t t = ems_keep(tid);
#pragma unroll
        for (int s = 0; s < EMS_ITER; s++) {
            const int32_t e = t + s * EMS_THREADS;
            if (e >= m) continue;
            uint8_t *d = buf + ((size_t)g * PMH_TILE_MAX + e) * W;
            if constexpr (W == 8)
                *reinterpret_cast<uint64_t *>(d) =
                    ((uint64_t)v[2 * g + 1][s] << 32) | v[2 * g][s];
            else
                *reinterpret_cast<uint32_t *>(d) = v[g][s];
        }
    }
}

// output row j = tid + s * EMS_THREADS reads its winner's slot and stores,
// narrowing to S as k_emit_contig's lists do
template <typename L, typename S>
DEV void ems_permute(const uint8_t *buf, const uint64_t *s_out, int p, int n,
                     int64_t toff, int32_t count, int tid,
                     const uint32_t (&wslot)[EMS_ITER / 2]) {
    for (int g = 0; g < n; g++) {
        const uint64_t ob =
            uniform64(s_out[p + g] + (uint64_t)toff * sizeof(S));
        const uint8_t *cb = buf + (size_t)g * PMH_TILE_MAX * sizeof(L);
        const int32_t t = ems_keep(tid);
#pragma unroll
        for (int s = 0; s < EMS_ITER; s++) {
            const int32_t j = t + s * EMS_THREADS;
            if (j >= count) continue;
            const L x = *reinterpret_cast<const L *>(
                cb + (size_t)((ems_keep(wslot[s / 2]) >> (16 * (s & 1))) &
                              0xffffu) *
                         sizeof(L));
            const uint64_t oa =
                ob + (uint64_t)((uint32_t)t * (uint32_t)sizeof(S)) +
                (uint64_t)(s * EMS_THREADS * (int)sizeof(S));
            gstore<S>(oa, (S)x);
        }
    }
}

template <int KM, int GU>
__attribute__((amdgpu_waves_per_eu(4))) __launch_bounds__(EMS_THREADS, 2)
__global__
void k_emit_stream(const DevCol *cols /* k * n_cols, run-major */,
                   const uint8_t *col_dtype, int n_cols, int n_emit, int k,
                   const int32_t *__restrict__ cuts,
                   const int64_t *__restrict__ lens,
                   const uint32_t *__restrict__ winners,
                   const int32_t *__restrict__ tile_counts,
                   const int64_t *__restrict__ tile_offsets, int64_t n_tiles,
                   int64_t tile_rows, void *const *out_ptrs,
                   int lds_budget) {
    extern __shared__ uint64_t ems_smem[];
    const int n_ent = k * n_cols;
    uint64_t *s_addr = ems_smem;                    // [n_ent] run, position
    uint64_t *s_out = s_addr + n_ent;               // [n_cols] by position
    int *s_cnt = (int *)(s_out + n_cols);           // list lengths, n groups
    uint16_t *s_bound = (uint16_t *)(s_cnt + 8);    // [n_cols + 1] groups
    uint8_t *s_pos = (uint8_t *)(s_bound + n_cols + 1);  // column -> position
    uint8_t *s_cls = s_pos + n_cols;                // [n_cols] by column
    uint8_t *s_clsp = s_cls + n_cols;               // [n_cols] by position
    uint8_t *buf =
        (uint8_t *)ems_smem + emit_stream_tables(k, n_cols);  // data area

    const int tid = threadIdx.x;
    // the lists, as in k_emit_contig
    for (int c = tid; c < n_cols; c += EMS_THREADS)
        s_cls[c] = c < n_emit ? pmh_out_width(col_dtype[c]) : 0;
    __syncthreads();
    for (int c = tid; c < n_cols; c += EMS_THREADS) {
        const int cls = s_cls[c];
        int n_of[4] = {0, 0, 0, 0};  // list lengths, by log2(width)
        int before = 0;
        for (int j = 0; j < n_cols; j++) {
            const int cj = s_cls[j];
#pragma unroll
            for (int w = 0; w < 4; w++) n_of[w] += cj == (1 << w);
            before += (j < c && cj == cls);
        }
        if (c == 0) {
#pragma unroll
            for (int w = 0; w < 4; w++) s_cnt[w] = n_of[w];
        }
        if (cls) {
            int p = before;
#pragma unroll
            for (int w = 0; w < 3; w++) p += (1 << w) < cls ? n_of[w] : 0;
            s_pos[c] = (uint8_t)p;
            s_clsp[p] = (uint8_t)cls;
            s_out[p] = (uint64_t)out_ptrs[c];
        }
    }
    __syncthreads();
    for (int e = tid; e < n_ent; e += EMS_THREADS) {
        const int r = e / n_cols, c = e - r * n_cols;
        if (!s_cls[c]) continue;
        s_addr[r * n_cols + s_pos[c]] = cols[e].addr0;
    }
    if (tid == 0)
        s_cnt[4] = esc_plan_groups(
            s_clsp, nullptr, s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3],
            PMH_TILE_MAX, lds_budget, GU, GU / 2, s_bound);
    __syncthreads();
    const int ng = s_cnt[4];
    int64_t tile = blockIdx.x;
    if (ng <= 0 || tile >= n_tiles) return;  // block-uniform

    const int64_t wstride = tile_rows + PMH_MAX_RUNS;
    EscTile<KM> ts;
    uint32_t src[EMS_ITER];  // this thread's slots: run:5 | row:27
    uint32_t wraw[EMS_ITER], v[GU][EMS_ITER];
    uint32_t wslot[EMS_ITER / 2];  // its output rows' slots, 16 bits each
    int32_t count_n;
    int64_t toff_n;
    // tile t's segments, this thread's slot sources, its winner words
    auto setup = [&](int64_t t) {
        // opaque, or everything below that depends on the next tile's index
        // alone is hoisted out of the group loop and held in registers
        asm volatile("" : "+s"(t));
        esc_tile_setup<KM>(cuts + t * k, cuts + (t + 1) * k, lens, k, ts);
        count_n = tile_counts[t];
        toff_n = tile_offsets[t];
        const int32_t last = ts.mtotal > 0 ? ts.mtotal - 1 : 0;
        const int32_t tk = ems_keep(tid);
#pragma unroll
        for (int s = 0; s < EMS_ITER; s++) {
            const int32_t x = tk + s * EMS_THREADS;
            int run;
            uint32_t row;
            esc_slot_source<KM>(ts, k, x < last ? x : last, &run, &row);
            src[s] = ((uint32_t)run << PMH_ROW_BITS) | row;
        }
        const uint64_t wb = (uint64_t)(winners + t * wstride);
        const uint32_t wlast = (uint32_t)wstride - 1;  // past it: no winner
#pragma unroll
        for (int s = 0; s < EMS_ITER; s++) {
            const uint32_t j = (uint32_t)(tk + s * EMS_THREADS);
            wraw[s] = gload<uint32_t>(wb + (j < wlast ? j : wlast) * 4u);
        }
    };
    auto issue = [&](int gi) {
        if (ts.mtotal <= 0) return;  // no element, no valid address
        const int p = s_bound[gi], n = s_bound[gi + 1] - p;
        if (s_clsp[p] == 8) ems_load<8, GU>(s_addr, p, n, n_cols, src, v);
        else ems_load<4, GU>(s_addr, p, n, n_cols, src, v);
    };
    setup(tile);
    issue(0);
    for (;;) {
        const int32_t count = count_n;
        const int64_t toff = toff_n;
        // a slot is < PMH_TILE_MAX < 2^16 for every live row; the words
        // past the tile's count are not winners and their slots go unread
#pragma unroll
        for (int s = 0; s < EMS_ITER; s += 2) {
            const uint32_t lo = (uint32_t)esc_winner_slot<KM>(
                ts, wraw[s] >> PMH_ROW_BITS, wraw[s] & PMH_ROW_MASK);
            const uint32_t hi = (uint32_t)esc_winner_slot<KM>(
                ts, wraw[s + 1] >> PMH_ROW_BITS, wraw[s + 1] & PMH_ROW_MASK);
            wslot[s / 2] = (lo & 0xffffu) | (hi << 16);
        }
        const int64_t next = tile + gridDim.x;
        for (int gi = 0; gi < ng; gi++) {
            const int p = s_bound[gi], n = s_bound[gi + 1] - p;
            const int cls = s_clsp[p];
            if (cls == 8) ems_fill<8, GU>(buf, n, ts.mtotal, tid, v);
            else ems_fill<4, GU>(buf, n, ts.mtotal, tid, v);
            if (gi + 1 < ng) {
                issue(gi + 1);
            } else if (next < n_tiles) {
                setup(next);
                issue(0);
            }
            __syncthreads();
            if (cls == 1)
                ems_permute<int32_t, int8_t>(buf, s_out, p, n, toff,
                                                 count, tid, wslot);
            else if (cls == 2)
                ems_permute<int32_t, int16_t>(buf, s_out, p, n, toff,
                                                  count, tid, wslot);
            else if (cls == 4)
                ems_permute<int32_t, int32_t>(buf, s_out, p, n, toff,
                                                  count, tid, wslot);
            else
                ems_permute<int64_t, int64_t>(buf, s_out, p, n, toff,
                                                  count, tid, wslot);
            __syncthreads();
        }
        if (next >= n_tiles) break;
        tile = next;
    }
}

// ------------------------------------------------------------ k_composite
//
// Build one run's order-preserving composite key: each integer sub-key is
// biased to unsigned at its declared bit width and concatenated MSB-first
// (first key column highest), then the u64 is sign-flipped back to int64 so
// ukey() in the partition/merge recovers the unsigned order. Paimon compares
// multi-column keys lexicographically (keyComparator over the _KEY_ fields),
// which this encoding preserves exactly for integer columns whose widths sum
// to <= 64 bits. Rebuilt per pass (decode-derived).
// spec packs (shift, bits) per sub-key, 8 bits each, sub-key i at byte i.
__global__ void k_composite(const DevCol *keys, int nk, uint64_t shifts,
                            uint64_t bits, int64_t rows, int64_t *ckey) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows;
         i += stride) {
        uint64_t u = 0;
        for (int j = 0; j < nk; j++) {
            const DevCol &dc = keys[j];
            int64_t v = dc.esize == 8 ? col_load<int64_t>(dc, i)
                                      : (int64_t)col_load<int32_t>(dc, i);
            const int w = (int)((bits >> (8 * j)) & 0xff);
            const int sh = (int)((shifts >> (8 * j)) & 0xff);
            uint64_t b = ((uint64_t)v + (1ull << (w - 1))) &
                         (w >= 64 ? ~0ull : ((1ull << w) - 1));
            u |= b << sh;
        }
        ckey[i] = (int64_t)(u ^ 0x8000000000000000ull);
    }
}

// ------------------------------------------------------------ k_pack_valid
//
// Pack one run's per-column validity bytes into a u64 bitmask per row
// (bit c = column c non-null; columns with no staged nulls contribute 1).
// The PU/aggregation emit then resolves EVERY column's nullability from one
// mask load per group member instead of one byte load per (member, column) —
// the per-column walk was a serial dependent-load chain over up to n_cols
// scattered arrays and dominated the C3 emit.
__global__ void k_pack_valid(const DevCol *cols, int n_cols, int64_t rows,
                             uint64_t *mask) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows;
         i += stride) {
        uint64_t m = 0;
        for (int c = 0; c < n_cols; c++) {
            const uint64_t v = col_valid(cols[c], i);
            m |= (v & 1) << c;
        }
        mask[i] = m;
    }
}

// ------------------------------------------------------------ k_emit_pu
//
// PartialUpdate emit: one output row per owned group; for each value column
// take the LAST member whose field is non-null (updateNonNullFields,
// PartialUpdateMergeFunction.java:188-215; members arrive in ascending
// (seq, isAdd) order). seq = last member's sequenceNumber
// (latestSequenceNumber, :188); kind = INSERT (insert-only streams, v1).
// Singleton groups return the record as-is (ReducerMergeFunctionWrapper
// bypass) — identical to the overlay for INSERT records.
// MASKS: per-row packed validity (k_pack_valid) available — one u64 load per
// member resolves all columns; false = legacy per-column byte walk (>64
// columns).
template <bool MASKS>
__global__ void k_emit_pu(const DevCol *cols, const uint8_t *col_dtype,
                          const uint8_t *col_nullable, int n_cols, int k,
                          int seq_col, int kind_col, int flags,
                          const uint32_t *members,
                          const uint16_t *group_start,
                          const int64_t *tile_offsets, int64_t n_tiles,
                          int64_t tile_rows, const int64_t *total_out,
                          uint64_t *const *run_masks, void *const *out_ptrs,
                          uint8_t *const *out_valid) {
    // remove-record-on-delete (PMH_FLAG_RROD): a DELETE resets the row —
    // per column, overlay only the adds NEWER than the last DELETE and fall
    // back to the DELETE record's own field (initRow semantics,
    // PartialUpdateMergeFunction.java:173-180). Result kind = DELETE when
    // the last member is the DELETE (getResult, :213-221). Groups whose result
    // DELETE were already dropped by the merge pass under drop_delete.
    const bool rrod = (flags & PMH_FLAG_RROD) != 0;
    const int64_t total = *total_out;
    const int64_t slice_lo = slice_lo_of(total);
    const int64_t slice_hi = slice_hi_of(total);
    auto kind_of = [&](uint32_t m) -> int32_t {
        return col_load<int32_t>(member_col(cols, n_cols, m, kind_col),
                                 member_row(m));
    };
    auto valid_of = [&](uint32_t m, int c) -> uint8_t {
        if (MASKS) return (uint8_t)((member_mask(run_masks, m) >> c) & 1);
        return member_valid(cols, n_cols, m, c);
    };
    int64_t t = -1;
    for (int64_t i = slice_lo + threadIdx.x; i < slice_hi; i += blockDim.x) {
        // first iteration: binary-search the owning tile; i then grows
        // monotonically, so a forward cursor walks
        if (t < 0) t = tile_seek(tile_offsets, n_tiles, i);
        t = tile_walk(tile_offsets, n_tiles, t, i);
        int64_t g = i - tile_offsets[t];
        const uint16_t *gs = &group_start[t * (tile_rows + 1)];
        const uint32_t *mem = &members[t * (tile_rows + PMH_MAX_RUNS)];
        int32_t ms = gs[g], me = gs[g + 1];
        // cache the newest members in registers: the per-column non-null
        // walk starts at the newest record and nearly always ends within a
        // few members (group size averages ~1.3), and re-reading the member
        // list from HBM per column dominated this kernel
        uint32_t mc[4];
        uint64_t vm[4];
        const int gn = me - ms;
#pragma unroll
        for (int x = 0; x < 4; x++)
            mc[x] = x < gn ? mem[me - 1 - x] : mem[me - 1];
        if (MASKS) {
#pragma unroll
            for (int x = 0; x < 4; x++)
                vm[x] = x < gn ? member_mask(run_masks, mc[x]) : 0;
        }
        // validity of cached member x: from its cached mask where there is one
        auto valid_cached = [&](int x, int c) -> uint8_t {
            return MASKS ? (uint8_t)((vm[x] >> c) & 1) : valid_of(mc[x], c);
        };
        const uint32_t last = mc[0];
        // singleton bypass serves the record's own RowKind: issue that
        // gather HERE so it overlaps the member prefetch instead of
        // stalling the column loop (measured +65% on emit_pu when loaded
        // at the kind column)
        int32_t single_kind = 0;
        if (gn == 1) single_kind = kind_of(last);
        // newest-first index of the last DELETE member; gn = none (also the
        // value when RROD is off, which neutralizes every bound below)
        int j_del = gn;
        if (rrod) {
#pragma unroll
            for (int x = 0; x < 4; x++) {
                if (x >= gn || j_del < gn) continue;
                if (kind_of(mc[x]) == 3) j_del = x;
            }
            for (int x = 4; x < gn && j_del == gn; x++)
                if (kind_of(mem[me - 1 - x]) == 3) j_del = x;
        }
        for (int c = 0; c < n_cols; c++) {
            if (c == kind_col) {
                // wrapper bypass: singletons keep their own RowKind
                ((int8_t *)out_ptrs[c])[i] = (int8_t)(
                    gn == 1 ? single_kind
                            : ((rrod && j_del == 0) ? 3 : 0));
                continue;
            }
            uint32_t src = last;  // the member whose field is emitted
            uint8_t ok = 1;
            if (col_nullable[c] && gn > 1) {
                ok = 0;
#pragma unroll
                for (int x = 0; x < 4; x++) {
                    if (ok || x >= gn || x >= j_del) continue;
                    if (valid_cached(x, c)) {
                        src = mc[x];
                        ok = 1;
                    }
                }
                for (int32_t x = me - 5; !ok && x >= ms; x--) {
                    if (me - 1 - x >= j_del) break;  // not newer than DELETE
                    const uint32_t m = mem[x];
                    if (valid_of(m, c)) {
                        src = m;
                        ok = 1;
                    }
                }
            } else if (col_nullable[c]) {
                // singleton: the record passes through with its own validity
                ok = valid_cached(0, c);
            }
            if (!ok && j_del < gn && col_nullable[c] && gn > 1) {
                // no add newer than the DELETE set this field: the row was
                // re-initialized from the DELETE record's value (initRow)
                const uint32_t m = mem[me - 1 - j_del];
                if (valid_of(m, c)) {
                    src = m;
                    ok = 1;
                }
            }
            const int dt = col_dtype[c];
            out_store(out_ptrs[c], dt, i,
                      ok ? member_load(cols, n_cols, src, c, dt) : 0);
            if (out_valid[c]) out_valid[c][i] = ok;
        }
    }
}


// ---------------------------------------------------------- k_emit_pu_sg
//
// PartialUpdate with SEQUENCE GROUPS (updateWithSequenceGroup,
// PartialUpdateMergeFunction.java:219-282; retractWithSequenceGroup
// :301-377; isEmptySequenceGroup :284-299; initRow :399-407; getResult
// :389-397). Streams may carry INSERT/UPDATE_AFTER/UPDATE_BEFORE/DELETE;
// retracts act only on their sequence groups. Plans whose group fields carry
// aggregate functions run k_emit_pu_sga below instead; this kernel serves
// the plans without them.
//
// The reference's sequential per-key fold reduces, per group, to the LAST
// PREFIX-MAX ACHIEVER over the members' sequence-field tuples (non-empty
// tuples only; lexicographic ascending, nulls FIRST; ties -> later member):
// each accepted event overwrites every field it touches, so only the last
// accepted event matters. Proven equivalent to the sequential port by
// randomized fuzz (oracle partial_update_seqgroup_model; see git history).
// col_group[c]: group id or 0xff (plain); sg_fields[g*4+j]: the group's
// sequence-field column indices; sg_nseq[g]: how many (<= 4).
__global__ void k_emit_pu_sg(const DevCol *cols, const uint8_t *col_dtype,
                             const uint8_t *col_nullable, int n_cols, int k,
                             int seq_col, int kind_col, int flags,
                             const uint8_t *col_group,
                             const int16_t *sg_fields,
                             const uint8_t *sg_nseq, int n_groups,
                             const uint32_t *members,
                             const uint16_t *group_start,
                             const int64_t *tile_offsets, int64_t n_tiles,
                             int64_t tile_rows, const int64_t *total_out,
                             uint64_t *const *run_masks,
                             void *const *out_ptrs,
                             uint8_t *const *out_valid) {
    const bool ignore_delete = flags & PMH_FLAG_IGNORE_DELETE;
    const int64_t total = *total_out;
    const int64_t slice_lo = slice_lo_of(total);
    const int64_t slice_hi = slice_hi_of(total);
    auto kind_of = [&](uint32_t m) -> int32_t {
        return col_load<int32_t>(member_col(cols, n_cols, m, kind_col),
                                 member_row(m));
    };
    auto valid_of = [&](uint32_t m, int c) -> uint8_t {
        if (run_masks) return (uint8_t)((member_mask(run_masks, m) >> c) & 1);
        return member_valid(cols, n_cols, m, c);
    };
    auto load_of = [&](uint32_t m, int c) -> int64_t {
        return member_load(cols, n_cols, m, c, col_dtype[c]);
    };
    int64_t t = -1;
    for (int64_t i = slice_lo + threadIdx.x; i < slice_hi; i += blockDim.x) {
        if (t < 0) t = tile_seek(tile_offsets, n_tiles, i);
        t = tile_walk(tile_offsets, n_tiles, t, i);
        const int64_t g = i - tile_offsets[t];
        const uint16_t *gs = &group_start[t * (tile_rows + 1)];
        const uint32_t *mem = &members[t * (tile_rows + PMH_MAX_RUNS)];
        const int32_t ms = gs[g], me = gs[g + 1];
        const int gn = me - ms;
        const uint32_t m0 = mem[ms];
        const int32_t kind0 = kind_of(m0);
        const bool first_retract = kind0 == 1 || kind0 == 3;
        if (gn == 1) {
            // ReducerMergeFunctionWrapper singleton bypass: the record is
            // served as-is with its own RowKind
            for (int c = 0; c < n_cols; c++) {
                if (c == kind_col) {
                    ((int8_t *)out_ptrs[c])[i] = (int8_t)kind0;
                    continue;
                }
                uint8_t ok = col_nullable[c] ? valid_of(m0, c) : 1;
                out_store(out_ptrs[c], col_dtype[c], i,
                          ok ? load_of(m0, c) : 0);
                if (out_valid[c]) out_valid[c][i] = ok;
            }
            continue;
        }
        // per-group winner member (last prefix-max achiever), computed once
        // per row; group count bounded by plan validation (<= 16)
        int32_t win[16];
        bool win_r[16];
        for (int gg = 0; gg < n_groups; gg++) {
            win[gg] = -1;
            win_r[gg] = false;
        }
        bool meet_insert = false;
        uint32_t last_m = m0;
        uint32_t last_add = 0;
        bool has_add = false;
        for (int32_t x = 0; x < gn; x++) {
            const uint32_t m = mem[ms + x];
            const int32_t kd = kind_of(m);
            const bool retract = kd == 1 || kd == 3;
            if (!retract) {
                meet_insert = true;
                has_add = true;
                last_add = m;
            }
            if (!(retract && ignore_delete)) last_m = m;
            if (retract && ignore_delete) continue;
            for (int gg = 0; gg < n_groups; gg++) {
                const int ns = sg_nseq[gg];
                // empty tuples (all sequence fields null) never participate
                // (isEmptySequenceGroup)
                bool anyv = false;
                for (int j = 0; j < ns; j++)
                    anyv |= valid_of(m, sg_fields[gg * 4 + j]) != 0;
                if (!anyv) continue;
                if (win[gg] < 0) {
                    win[gg] = x;
                    win_r[gg] = retract;
                    continue;
                }
                // lexicographic tuple compare vs the current winner,
                // nulls FIRST; ties accept (later member wins)
                const uint32_t wm = mem[ms + win[gg]];
                int cmp = 0;
                for (int j = 0; j < ns && cmp == 0; j++) {
                    const int c = sg_fields[gg * 4 + j];
                    const uint8_t va = valid_of(m, c);
                    const uint8_t vb = valid_of(wm, c);
                    if (va != vb) cmp = va ? 1 : -1;  // null sorts first
                    else if (va) {
                        const int64_t a = load_of(m, c);
                        const int64_t b = load_of(wm, c);
                        if (a != b) cmp = a > b ? 1 : -1;
                    }
                }
                if (cmp >= 0) {
                    win[gg] = x;
                    win_r[gg] = retract;
                }
            }
        }
        for (int c = 0; c < n_cols; c++) {
            if (c == kind_col) {
                ((int8_t *)out_ptrs[c])[i] = meet_insert ? 0 : 3;
                continue;
            }
            if (c == seq_col) {
                ((int64_t *)out_ptrs[c])[i] = load_of(last_m, c);
                continue;
            }
            const int gg = col_group[c];
            uint32_t src_m = 0;
            uint8_t ok = 0;
            if (gg != 0xff) {
                const int ns = sg_nseq[gg];
                bool is_seq_field = false;
                for (int j = 0; j < ns; j++)
                    if (sg_fields[gg * 4 + j] == c) is_seq_field = true;
                if (win[gg] >= 0) {
                    if (is_seq_field || !win_r[gg]) {
                        src_m = mem[ms + win[gg]];
                        ok = valid_of(src_m, c);
                    }  // retract winner nulls the member fields
                } else if (first_retract) {  // initRow fallback
                    src_m = m0;
                    ok = valid_of(m0, c);
                }
            } else {
                // plain column: last non-null among ADD members, else the
                // initRow base when the first member was a retract
                if (first_retract && valid_of(m0, c)) {
                    src_m = m0;
                    ok = 1;
                }
                for (int32_t x = 0; x < gn; x++) {
                    const uint32_t m = mem[ms + x];
                    const int32_t kd = kind_of(m);
                    if (kd == 1 || kd == 3) continue;
                    if (valid_of(m, c)) {
                        src_m = m;
                        ok = 1;
                    }
                }
            }
            out_store(out_ptrs[c], col_dtype[c], i,
                      ok ? load_of(src_m, c) : 0);
            if (out_valid[c]) out_valid[c][i] = ok;
        }
    }
}

// --------------------------------------------------------- k_emit_pu_sga
//
// PartialUpdate with sequence groups AND aggregate functions on group fields
// (fields.<f>.aggregate-function / ignore-retract / default-aggregate-
// function). An aggregated field takes a contribution from EVERY member of
// its group, agg or aggReversed by how the member's tuple compared with the
// row's running tuple at that moment, so the last-prefix-max shortcut of
// k_emit_pu_sg does not apply. The fold itself is pu_agg_core.h, shared with
// the host entry pmh_debug_pu_agg_fold.
//
// One thread per output row. The sequence groups loop OUTERMOST and no
// per-thread table is indexed by group (a run-time-indexed local array puts
// the whole array in scratch, see k_emit_agg): per group, one walk over the
// members leaves two 32-bit masks and the tuple holder in registers
// (pac_scan_group), then that group's columns fold and store
// (grp_cols[grp_off[g] .. grp_off[g + 1]): its fields that are no sequence
// fields). Member kinds load once per row into a 64-bit word (2 bits x <= 32
// members). Plain columns go last. Member fields load inside the fold, in
// member order; no register cache of the first members.
// col_agg[c]: PMH_AGG_* | PMH_AGG_IGNORE_RETRACT, or PAC_NONE. A retract that
// reaches an aggregator without retract() sets PMH_ERR_PU_AGG_RETRACT.
struct PuMembers {
    const DevCol *cols;
    const uint8_t *col_dtype;
    uint64_t *const *run_masks;
    const uint32_t *mem;  // the key group's member words
    int n_cols;
    DEV bool valid(int x, int c) const {
        const uint32_t m = mem[x];
        if (run_masks) return ((member_mask(run_masks, m) >> c) & 1) != 0;
        return member_valid(cols, n_cols, m, c) != 0;
    }
    DEV int64_t load(int x, int c) const {
        return member_load(cols, n_cols, mem[x], c, col_dtype[c]);
    }
};

// output row i of the plan's columns; the kernel writes the sequence-number
// and kind columns itself
struct PuRowSink {
    void *const *out_ptrs;
    uint8_t *const *out_valid;
    const uint8_t *col_dtype;
    int64_t i;
    int seq_col, kind_col;
    DEV bool own(int c) const { return c == seq_col || c == kind_col; }
    DEV void put(int c, int64_t bits, bool ok) {
        out_store(out_ptrs[c], col_dtype[c], i, bits);
        if (out_valid[c]) out_valid[c][i] = ok;
    }
};

static_assert(PAC_LAST_NON_NULL == PMH_AGG_LAST_NON_NULL &&
                  PAC_LAST_VALUE == PMH_AGG_LAST_VALUE &&
                  PAC_FIRST_VALUE == PMH_AGG_FIRST_VALUE &&
                  PAC_FIRST_NON_NULL == PMH_AGG_FIRST_NON_NULL &&
                  PAC_SUM == PMH_AGG_SUM && PAC_MAX == PMH_AGG_MAX &&
                  PAC_MIN == PMH_AGG_MIN &&
                  PAC_IGNORE_RETRACT == PMH_AGG_IGNORE_RETRACT,
              "pu_agg_core.h aggregator codes follow PMH_AGG_*");
static_assert(PAC_DT_INT8 == PMH_DT_INT8 && PAC_DT_INT16 == PMH_DT_INT16 &&
                  PAC_DT_INT32 == PMH_DT_INT32 &&
                  PAC_DT_INT64 == PMH_DT_INT64 &&
                  PAC_DT_FLOAT32 == PMH_DT_FLOAT32 &&
                  PAC_DT_FLOAT64 == PMH_DT_FLOAT64,
              "pu_agg_core.h dtype codes follow PMH_DT_*");
static_assert(PAC_MAX_MEMBERS == PMH_MAX_RUNS,
              "a key group has at most one member per run");

__global__ void k_emit_pu_sga(const DevCol *cols, const uint8_t *col_dtype,
                              const uint8_t *col_nullable, int n_cols, int k,
                              int seq_col, int kind_col, int flags,
                              const uint8_t *col_group,
                              const int16_t *sg_fields,
                              const uint8_t *sg_nseq, int n_groups,
                              const int16_t *grp_cols,
                              const uint16_t *grp_off,
                              const uint8_t *col_agg,
                              const uint32_t *members,
                              const uint16_t *group_start,
                              const int64_t *tile_offsets, int64_t n_tiles,
                              int64_t tile_rows, const int64_t *total_out,
                              uint64_t *const *run_masks,
                              void *const *out_ptrs,
                              uint8_t *const *out_valid, uint32_t *err_flag) {
    const bool ignore_delete = flags & PMH_FLAG_IGNORE_DELETE;
    const int64_t total = *total_out;
    const int64_t slice_lo = slice_lo_of(total);
    const int64_t slice_hi = slice_hi_of(total);
    const PacTables tables{n_cols,   n_groups, col_dtype, col_group, sg_fields,
                           sg_nseq,  grp_cols, grp_off,   col_agg};
    int64_t t = -1;
    bool bad = false;
    for (int64_t i = slice_lo + threadIdx.x; i < slice_hi; i += blockDim.x) {
        if (t < 0) t = tile_seek(tile_offsets, n_tiles, i);
        t = tile_walk(tile_offsets, n_tiles, t, i);
        const int64_t g = i - tile_offsets[t];
        const uint16_t *gs = &group_start[t * (tile_rows + 1)];
        const uint32_t *mem = &members[t * (tile_rows + PMH_MAX_RUNS)];
        const int32_t ms = gs[g], me = gs[g + 1];
        // a key group holds at most one member per run
        const int gn = me - ms < PMH_MAX_RUNS ? me - ms : PMH_MAX_RUNS;
        const PuMembers a{cols, col_dtype, run_masks, mem + ms, n_cols};
        PuRowSink sink{out_ptrs, out_valid, col_dtype, i, seq_col, kind_col};
        uint64_t kinds = 0;
        for (int x = 0; x < gn; x++) {
            const int32_t kd = col_load<int32_t>(
                member_col(cols, n_cols, mem[ms + x], kind_col),
                member_row(mem[ms + x]));
            kinds |= (uint64_t)(kd & 3) << (2 * x);
        }
        if (gn == 1) {
            // ReducerMergeFunctionWrapper singleton bypass: the record is
            // served as-is with its own RowKind
            for (int c = 0; c < n_cols; c++) {
                if (c == kind_col)
                    ((int8_t *)out_ptrs[c])[i] = (int8_t)pac_kind(kinds, 0);
                else
                    pac_put_src(a, sink, c, 0);
            }
            continue;
        }
        bool has_add;
        int last;
        pac_row_summary(gn, kinds, ignore_delete, &has_add, &last);
        ((int8_t *)out_ptrs[kind_col])[i] = has_add ? 0 : 3;
        ((int64_t *)out_ptrs[seq_col])[i] =
            last >= 0 ? a.load(last, seq_col) : 0;
        bad |= pac_fold_row(a, gn, kinds, ignore_delete, tables, sink);
    }
    if (bad && err_flag) atomicOr(err_flag, PMH_ERR_PU_AGG_RETRACT);
}

// ------------------------------------------------------------ k_emit_agg
//
// Aggregation emit (AggregateMergeFunction.java:82-125): one output row per
// owned group; each value column folds the group's members in ascending
// (seq, isAdd) order through its FieldAggregator:
//   last_non_null_value (default, :201)  — FieldLastNonNullValueAgg
//   last_value / first_value / first_non_null_value
//   sum  — FieldSumAgg (null skipped; int accumulates in 64-bit then
//          truncates to the column width — Java's addExact overflow check
//          is not replicated, documented in DESIGN.md; float/double add in
//          the column's own precision, in merge order, matching Java)
//   max / min — FieldMaxAgg/FieldMinAgg; floats compare in IEEE total order
//          on the stored bits (= Float.compare/Double.compare up to
//          non-canonical negative NaNs)
// Result: seq = last member's sequenceNumber, kind = INSERT (getResult,
// :119-125). Singleton groups bypass the merge function entirely
// (ReducerMergeFunctionWrapper.java:53-73) and pass through unchanged.
// v1 accepts INSERT-only streams; retracts were flagged by k_merge_tiles.
__device__ inline uint32_t f32_ord(int32_t b) {
    return b < 0 ? ~(uint32_t)b : ((uint32_t)b | 0x80000000u);
}
__device__ inline uint64_t f64_ord(int64_t b) {
    return b < 0 ? ~(uint64_t)b : ((uint64_t)b | 0x8000000000000000ull);
}

template <bool MASKS>
__global__ void k_emit_agg(const DevCol *cols, const uint8_t *col_dtype,
                           const uint8_t *col_nullable,
                           const uint8_t *col_agg, int n_cols, int k,
                           int seq_col, int kind_col, int flags,
                           const uint32_t *members,
                           const uint16_t *group_start,
                           const int64_t *tile_offsets, int64_t n_tiles,
                           int64_t tile_rows, const int64_t *total_out,
                           uint64_t *const *run_masks, void *const *out_ptrs,
                           uint8_t *const *out_valid) {
    // remove-record-on-delete (PMH_FLAG_RROD): a DELETE re-initializes the
    // row from its own value and the aggregators continue FROM those values
    // (AggregateMergeFunction.add, currentDeleteRow path) — so folds seed
    // with the last DELETE's field and consume only newer adds. first_*
    // aggregators are rejected at plan creation under this mode.
    const bool rrod = (flags & PMH_FLAG_RROD) != 0;
    auto kind_of = [&](uint32_t m) -> int32_t {
        return col_load<int32_t>(member_col(cols, n_cols, m, kind_col),
                                 member_row(m));
    };
    auto valid_of = [&](uint32_t m, int c) -> uint8_t {
        if (MASKS) return (uint8_t)((member_mask(run_masks, m) >> c) & 1);
        return member_valid(cols, n_cols, m, c);
    };
    const int64_t total = *total_out;
    const int64_t slice_lo = slice_lo_of(total);
    const int64_t slice_hi = slice_hi_of(total);
    int64_t t = -1;
    for (int64_t i = slice_lo + threadIdx.x; i < slice_hi; i += blockDim.x) {
        // first iteration: binary-search the owning tile; i then grows
        // monotonically, so a forward cursor walks
        if (t < 0) t = tile_seek(tile_offsets, n_tiles, i);
        t = tile_walk(tile_offsets, n_tiles, t, i);
        int64_t g = i - tile_offsets[t];
        const uint16_t *gs = &group_start[t * (tile_rows + 1)];
        const uint32_t *mem = &members[t * (tile_rows + PMH_MAX_RUNS)];
        const int32_t ms = gs[g], me = gs[g + 1];
        const int gn = me - ms;
        // register-cache the first 4 members (oldest-first) + their packed
        // masks; every access below uses CONSTANT indices after unrolling —
        // a dynamically-indexed local array spills the whole array to
        // scratch (64 B/lane measured before this shape)
        uint32_t ma[4];
        uint64_t vma[4];
#pragma unroll
        for (int x = 0; x < 4; x++)
            ma[x] = mem[ms + (x < gn ? x : gn - 1)];
        if (MASKS) {
#pragma unroll
            for (int x = 0; x < 4; x++)
                vma[x] = x < gn ? member_mask(run_masks, ma[x]) : 0;
        }
        // validity of cached member x: from its cached mask where there is one
        auto valid_cached = [&](int x, int c) -> uint8_t {
            return MASKS ? (uint8_t)((vma[x] >> c) & 1) : valid_of(ma[x], c);
        };
        uint32_t last = ma[0];
        uint64_t vlast = MASKS ? vma[0] : 0;
#pragma unroll
        for (int x = 1; x < 4; x++)
            if (x < gn) {
                last = ma[x];
                if (MASKS) vlast = vma[x];
            }
        if (gn > 4) {
            last = mem[me - 1];
            if (MASKS) vlast = member_mask(run_masks, last);
        }
        // singleton bypass kind, issued early to overlap (see k_emit_pu)
        int32_t single_kind = 0;
        if (gn == 1) single_kind = kind_of(last);
        // ascending index of the LAST DELETE member (-1 = none)
        int d_del = -1;
        uint32_t mdel = 0;
        uint64_t vdel = 0;
        if (rrod) {
#pragma unroll
            for (int x = 0; x < 4; x++) {
                if (x >= gn) continue;
                if (kind_of(ma[x]) == 3) d_del = x;
            }
            for (int x = 4; x < gn; x++)
                if (kind_of(mem[ms + x]) == 3) d_del = x;
            if (d_del >= 0) {
                mdel = mem[ms + d_del];
                if (MASKS) vdel = member_mask(run_masks, mdel);
            }
        }
        // retract mode (PMH_FLAG_AGG_RETRACT): per-member kinds drive
        // aggregator.retract; only reached when every column's aggregator
        // is retract-capable (plan validation)
        const bool aggr = (flags & PMH_FLAG_AGG_RETRACT) != 0;
        for (int c = 0; c < n_cols; c++) {
            if (c == kind_col) {
                // wrapper bypass: singletons keep their own RowKind
                ((int8_t *)out_ptrs[c])[i] = (int8_t)(
                    gn == 1 ? single_kind
                            : ((rrod && d_del == gn - 1) ? 3 : 0));
                continue;
            }
            const int dt = col_dtype[c];
            const uint8_t rawagg = col_agg[c];
            const bool ign_retract =
                (rawagg & PMH_AGG_IGNORE_RETRACT) != 0;
            int agg = rawagg & 0x7f;
            if (agg == PMH_AGG_PRIMARY_KEY)
                agg = PMH_AGG_LAST_VALUE;  // agg == retract == input
            if (gn == 1) agg = PMH_AGG_LAST_VALUE;
            auto del_valid = [&]() -> uint8_t {
                if (!col_nullable[c]) return 1;
                if (MASKS) return (uint8_t)((vdel >> c) & 1);
                return member_valid(cols, n_cols, mdel, c);
            };
            uint32_t src = last;  // the member whose field is emitted
            uint8_t ok = 1;
            int64_t bits = 0;  // result payload (raw stored bits / int value)
            bool direct = true;  // bits not set; load from src at store
            bool handled = false;
            if (aggr && ign_retract && gn > 1 &&
                (agg == PMH_AGG_LAST_VALUE || agg == PMH_AGG_FIRST_VALUE ||
                 agg == PMH_AGG_LAST_NON_NULL ||
                 agg == PMH_AGG_FIRST_NON_NULL)) {
                // FieldIgnoreRetractAgg wrapper: retract members leave the
                // accumulator untouched, so only ADD members qualify
                auto is_rt = [&](uint32_t m) -> bool {
                    const int32_t kd = kind_of(m);
                    return kd == 1 || kd == 3;
                };
                const bool want_first = agg == PMH_AGG_FIRST_VALUE ||
                                        agg == PMH_AGG_FIRST_NON_NULL;
                const bool need_nn = agg == PMH_AGG_LAST_NON_NULL ||
                                     agg == PMH_AGG_FIRST_NON_NULL;
                ok = 0;
                for (int32_t x = 0; x < gn; x++) {
                    uint32_t m = mem[ms + x];
                    if (is_rt(m)) continue;
                    uint8_t v = col_nullable[c] ? valid_of(m, c) : 1;
                    if (need_nn && !v) continue;
                    src = m;
                    ok = need_nn ? 1 : v;
                    if (want_first) break;
                }
                handled = true;
            }
            if (!handled) switch (agg) {
            case PMH_AGG_LAST_VALUE:
                // last member as-is, its own validity (also the singleton
                // ReducerMergeFunctionWrapper bypass)
                if (col_nullable[c])
                    ok = MASKS ? (uint8_t)((vlast >> c) & 1)
                               : valid_of(last, c);
                break;
            case PMH_AGG_FIRST_VALUE: {
                src = ma[0];
                if (col_nullable[c])
                    ok = valid_cached(0, c);
                break;
            }
            case PMH_AGG_LAST_NON_NULL:
                if (col_nullable[c] || d_del >= 0) {
                    ok = 0;
                    // newest first: uncached tail (x >= 4), then cached;
                    // only members NEWER than the last DELETE participate
                    for (int32_t x = gn - 1; !ok && x >= 4; x--) {
                        if (x <= d_del) break;
                        uint32_t m = mem[ms + x];
                        if (valid_of(m, c)) {
                            src = m;
                            ok = 1;
                        }
                    }
#pragma unroll
                    for (int x = 3; x >= 0; x--) {
                        if (ok || x >= gn || x <= d_del) continue;
                        if (valid_cached(x, c)) {
                            src = ma[x];
                            ok = 1;
                        }
                    }
                    if (!ok && d_del >= 0 && del_valid()) {
                        src = mdel;  // initRow: the DELETE's field
                        ok = 1;
                    }
                }
                break;
            case PMH_AGG_FIRST_NON_NULL:
                if (col_nullable[c]) {
                    ok = 0;
#pragma unroll
                    for (int x = 0; x < 4; x++) {
                        if (ok || x >= gn) continue;
                        if (valid_cached(x, c)) {
                            src = ma[x];
                            ok = 1;
                        }
                    }
                    for (int32_t x = 4; !ok && x < gn; x++) {
                        uint32_t m = mem[ms + x];
                        if (valid_of(m, c)) {
                            src = m;
                            ok = 1;
                        }
                    }
                } else {
                    src = ma[0];
                }
                break;
            default: {  // SUM / MAX / MIN: full fold, null inputs skipped
                direct = false;
                ok = 0;
                int64_t iacc = 0;
                float facc = 0.f;
                double dacc = 0.0;
                auto fold_one = [&](uint32_t m, bool retract) {
                    const int64_t vb = member_load(cols, n_cols, m, c, dt);
                    if (!ok) {
                        ok = 1;
                        if (agg == PMH_AGG_SUM && dt == PMH_DT_FLOAT32) {
                            facc = __int_as_float((int32_t)vb);
                            if (retract) facc = -facc;  // null acc: negate
                        } else if (agg == PMH_AGG_SUM && dt == PMH_DT_FLOAT64) {
                            dacc = __longlong_as_double(vb);
                            if (retract) dacc = -dacc;
                        } else {
                            iacc = retract && agg == PMH_AGG_SUM ? -vb : vb;
                        }
                        return;
                    }
                    if (agg == PMH_AGG_SUM) {
                        // FieldSumAgg.agg / .retract (:60-110): subtract on
                        // retract, same width/precision rules
                        const double sgn = retract ? -1.0 : 1.0;
                        if (dt == PMH_DT_FLOAT32)
                            facc += (float)sgn * __int_as_float((int32_t)vb);
                        else if (dt == PMH_DT_FLOAT64)
                            dacc += sgn * __longlong_as_double(vb);
                        else
                            iacc += retract ? -vb : vb;
                    } else {
                        bool take;
                        if (dt == PMH_DT_FLOAT32) {
                            uint32_t a = f32_ord((int32_t)iacc);
                            uint32_t b = f32_ord((int32_t)vb);
                            take = agg == PMH_AGG_MAX ? b > a : b < a;
                        } else if (dt == PMH_DT_FLOAT64) {
                            uint64_t a = f64_ord(iacc);
                            uint64_t b = f64_ord(vb);
                            take = agg == PMH_AGG_MAX ? b > a : b < a;
                        } else {
                            take = agg == PMH_AGG_MAX ? vb > iacc : vb < iacc;
                        }
                        if (take) iacc = vb;
                    }
                };
                auto is_retract = [&](uint32_t m) -> bool {
                    if (!aggr) return false;
                    const int32_t kd = kind_of(m);
                    return kd == 1 || kd == 3;
                };
                if (d_del >= 0 && del_valid())
                    fold_one(mdel, false);  // initRow continuation
#pragma unroll
                for (int x = 0; x < 4; x++) {
                    if (x >= gn || x <= d_del) continue;
                    if (col_nullable[c] && !valid_cached(x, c)) continue;
                    const bool rt = is_retract(ma[x]);
                    if (rt && ign_retract) continue;  // FieldIgnoreRetractAgg
                    fold_one(ma[x], rt);
                }
                for (int32_t x = 4; x < gn; x++) {
                    if (x <= d_del) continue;
                    uint32_t m = mem[ms + x];
                    if (col_nullable[c] && !valid_of(m, c)) continue;
                    const bool rt = is_retract(m);
                    if (rt && ign_retract) continue;
                    fold_one(m, rt);
                }
                if (agg == PMH_AGG_SUM && dt == PMH_DT_FLOAT32)
                    bits = (int64_t)__float_as_int(facc);
                else if (agg == PMH_AGG_SUM && dt == PMH_DT_FLOAT64)
                    bits = __double_as_longlong(dacc);
                else
                    bits = iacc;
                break;
            }
            }
            if (direct && ok) bits = member_load(cols, n_cols, src, c, dt);
            if (!ok) bits = 0;
            out_store(out_ptrs[c], dt, i, bits);
            if (out_valid[c]) out_valid[c][i] = ok;
        }
    }
}

// --------------------------------------------------------- k_level_scatter
//
// Decode def-level streams (RLE/bit-packed hybrid, bit width 1) and position
// the dense PLAIN values: valid[row] = level, out[row] = dense[aux + prefix]
// (the null handling of VectorizedColumnReader.readBatch,
// paimon-format/.../reader/VectorizedColumnReader.java:143-241).
__global__ void k_level_scatter(const RleChunk *chunks, int64_t n_chunks) {
    // one WAVE per chunk, barrier-free: the host prescan bounds packed
    // chunks at <= 512 values (parquet) / <= 1040 (ORC byte-RLE groups) and
    // precomputes each chunk's dense prefix (aux), so the only running state
    // is a per-wave register popcount. The previous one-WORKGROUP-per-chunk
    // version chained 3 __syncthreads per 512 values through an LDS running
    // scan and was serialization-bound (62 ms at the 8x10M PU shape; 94 GB/s
    // effective).
    const int lane = (int)(threadIdx.x & 63);
    const int64_t wave_id =
        (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t cidx = wave_id; cidx < n_chunks; cidx += n_waves) {
        RleChunk ch = chunks[cidx];
        const uint8_t *dense = (const uint8_t *)ch.dense_addr;
        uint8_t *out = (uint8_t *)ch.out_addr;
        uint8_t *valid = (uint8_t *)ch.valid_addr;
        const int esize = ch.esize;
        if (ch.kind == 0) {
            if (ch.value) {  // run of non-nulls: dense block copy
                for (int32_t i = lane; i < ch.count; i += 64) {
                    valid[ch.out_start + i] = 1;
                    const uint8_t *s = dense + (ch.aux + i) * esize;
                    uint8_t *d = out + (ch.out_start + i) * esize;
                    if (esize == 4)
                        *(int32_t *)d = *(const int32_t *)s;
                    else
                        *(int64_t *)d = *(const int64_t *)s;
                }
            } else {  // run of nulls
                for (int32_t i = lane; i < ch.count; i += 64) {
                    valid[ch.out_start + i] = 0;
                    uint8_t *d = out + (ch.out_start + i) * esize;
                    if (esize == 4)
                        *(int32_t *)d = 0;
                    else
                        *(int64_t *)d = 0;
                }
            }
            continue;
        }
        // bit-packed: 1 byte per 8 levels; dense index = aux + running
        // popcount (registers only) + lower-lane ballot prefix
        const uint8_t *src = (const uint8_t *)ch.src;
        int32_t running = 0;
        for (int32_t b = 0; b < ch.count; b += 64) {
            int32_t i = b + lane;
            int bit = 0;
            if (i < ch.count) bit = (src[i >> 3] >> (i & 7)) & 1;
            uint64_t mask = __ballot(bit != 0);
            int32_t my_before =
                lane == 0 ? 0 : __popcll(mask << (64 - lane));
            if (i < ch.count) {
                valid[ch.out_start + i] = (uint8_t)bit;
                uint8_t *dp = out + (ch.out_start + i) * esize;
                if (bit) {
                    int64_t didx = ch.aux + running + my_before;
                    const uint8_t *sp = dense + didx * esize;
                    if (esize == 4)
                        *(int32_t *)dp = *(const int32_t *)sp;
                    else
                        *(int64_t *)dp = *(const int64_t *)sp;
                } else {
                    if (esize == 4)
                        *(int32_t *)dp = 0;
                    else
                        *(int64_t *)dp = 0;
                }
            }
            running += __popcll(mask);
        }
    }
}

// ------------------------------------------------------------- k_rlev2
//
// ORC RLEv2 / byte-RLE decode from host-prescanned run chunks (ORC v1 spec;
// the reference consumes this via orc-core 1.9.8 — parity pinned by the
// oracle restatement + pyarrow). One 64-lane wave per chunk
// (runs are <= 512 values); bit order is big-endian MSB-first.

DEV uint64_t be_bits(const uint8_t *src, int64_t bit_off, int width) {
    // read `width` (<= 64) bits starting at bit_off, MSB-first: two aligned
    // 8-byte loads + shift-combine (the byte-at-a-time loop cost ~5 loads
    // per value). Stream uploads are padded by 16 bytes for the window.
    uint64_t addr = (uint64_t)src + (uint64_t)(bit_off >> 3);
    uint64_t base = addr & ~7ull;  // absolute 8-byte alignment
    int off = (int)((addr - base) * 8) + (int)(bit_off & 7);  // 0..63
    uint64_t hi =
        __builtin_bswap64(*reinterpret_cast<const uint64_t *>(base));
    uint64_t lo =
        __builtin_bswap64(*reinterpret_cast<const uint64_t *>(base + 8));
    uint64_t window = off ? ((hi << off) | (lo >> (64 - off))) : hi;
    return width == 64 ? window : window >> (64 - width);
}

DEV int64_t zz_dec(uint64_t v) {
    return (int64_t)(v >> 1) ^ -(int64_t)(v & 1);
}

DEV void dense_store(void *out, int esize, int64_t idx, int64_t v) {
    if (esize == 4)
        ((int32_t *)out)[idx] = (int32_t)v;
    else
        ((int64_t *)out)[idx] = v;
}

__global__ void k_rlev2(const Rlev2Chunk *chunks, int64_t n_chunks) {
    const int wave = (int)(threadIdx.x >> 6);
    const int lane = (int)(threadIdx.x & 63);
    const int waves = (int)(blockDim.x >> 6);
    for (int64_t cidx = (int64_t)blockIdx.x * waves + wave; cidx < n_chunks;
         cidx += (int64_t)gridDim.x * waves) {
        Rlev2Chunk ch = chunks[cidx];
        void *out = (void *)ch.out_addr;
        const uint8_t *src = (const uint8_t *)ch.src;
        switch (ch.kind) {
        case 0:  // SHORT_REPEAT (value already sign-decoded by the host)
        case 4:  // BYTE_RUN
            for (int i = lane; i < ch.count; i += 64)
                dense_store(out, ch.out_esize, ch.out_start + i, ch.base);
            break;
        case 5:  // BYTE_LITERAL (ORC tinyint byte stream, sign-extended)
            for (int i = lane; i < ch.count; i += 64)
                dense_store(out, ch.out_esize, ch.out_start + i,
                            (int8_t)src[i]);
            break;
        case 1: {  // DIRECT
            for (int i = lane; i < ch.count; i += 64) {
                uint64_t raw = be_bits(src, (int64_t)i * ch.width, ch.width);
                int64_t v = ch.is_signed ? zz_dec(raw) : (int64_t)raw;
                dense_store(out, ch.out_esize, ch.out_start + i, v);
            }
            break;
        }
        case 2: {  // PATCHED_BASE: unsigned packed + base; patches on lane 0
            for (int i = lane; i < ch.count; i += 64) {
                uint64_t raw = be_bits(src, (int64_t)i * ch.width, ch.width);
                dense_store(out, ch.out_esize, ch.out_start + i,
                            ch.base + (int64_t)raw);
            }
            __builtin_amdgcn_s_waitcnt(0);  // drain this wave's stores
            if (lane == 0) {
                const uint8_t *psrc = (const uint8_t *)ch.patch_src;
                uint64_t pmask = ch.patch_pw >= 64
                                     ? ~0ull
                                     : ((1ull << ch.patch_pw) - 1);
                int64_t pos = 0, gap = 0;
                int started = 0;
                for (int pidx = 0; pidx < ch.patch_pl; pidx++) {
                    uint64_t e = be_bits(psrc, (int64_t)pidx * ch.patch_cfb,
                                         ch.patch_cfb);
                    uint64_t g = e >> ch.patch_pw;
                    uint64_t pv = e & pmask;
                    gap += (int64_t)g;
                    if (pv == 0 && g == ((1ull << ch.patch_pgw) - 1))
                        continue;
                    pos = started ? pos + gap : gap;
                    started = 1;
                    gap = 0;
                    if (pos >= 0 && pos < ch.count) {
                        uint64_t raw =
                            be_bits(src, pos * (int64_t)ch.width, ch.width) |
                            (pv << ch.width);
                        dense_store(out, ch.out_esize, ch.out_start + pos,
                                    ch.base + (int64_t)raw);
                    }
                }
            }
            break;
        }
        case 3: {  // DELTA
            if (ch.width == 0) {  // fixed delta
                for (int i = lane; i < ch.count; i += 64)
                    dense_store(out, ch.out_esize, ch.out_start + i,
                                ch.base + (int64_t)i * ch.delta);
            } else {
                // packed |deltas| for elements 2..count-1; direction =
                // sign(delta). Wave-parallel prefix over 64-lane rounds.
                if (lane == 0) {
                    dense_store(out, ch.out_esize, ch.out_start, ch.base);
                    if (ch.count > 1)
                        dense_store(out, ch.out_esize, ch.out_start + 1,
                                    ch.base + ch.delta);
                }
                int64_t run = ch.base + ch.delta;  // value at index 1
                int sign = ch.delta < 0 ? -1 : 1;
                for (int b = 0; b < ch.count - 2; b += 64) {
                    int i = b + lane;  // delta index (element 2 + i)
                    int64_t d = 0;
                    if (i < ch.count - 2)
                        d = (int64_t)be_bits(src, (int64_t)i * ch.width,
                                             ch.width);
                    // inclusive wave scan of deltas
                    int64_t acc = d;
                    for (int off = 1; off < 64; off <<= 1) {
                        int64_t up = __shfl_up(acc, off, 64);
                        if (lane >= off) acc += up;
                    }
                    if (i < ch.count - 2)
                        dense_store(out, ch.out_esize, ch.out_start + 2 + i,
                                    run + sign * acc);
                    run += sign * __shfl(acc, 63, 64);
                }
            }
            break;
        }
        default: break;
        }
    }
}


// --------------------------------------------------------- k_orc_varint
//
// ORC DECIMAL DATA decode: zigzag base-128 varints, one per non-null row
// (orc_decimal_core.h). Varints carry no run headers, so the host prescan
// only cuts the stream every 512 values; finding the value boundaries is
// the kernel's work. One 64-lane wave per unit, no workgroup barrier:
//  (a) lanes sweep the unit's bytes with aligned 8-byte loads; a byte ends a
//      value when its high bit is clear, so ~word & 0x80.. is a terminator
//      mask. A wave prefix count numbers the terminators and each value's
//      END offset lands in the wave's LDS table (<= 512 x 2 bytes; a unit
//      is <= 5120 bytes, so offsets fit 16 bits);
//  (b) one lane per value reads its span (end[j-1], end[j]] as up to three
//      aligned words, then runs the shared scalar core: compact, zigzag,
//      rescale to the column scale, range check.
// The table is written and read by the same wave only: LDS operations of
// one wave execute in order, __threadfence_block() keeps the compiler from
// moving the reads up and waits out the writes.
// Loads may touch up to 7 bytes before the unit (same upload) and the
// 16-byte tail pad behind the stream; stores stay in [out_start, +count).
__launch_bounds__(256) __global__
void k_orc_varint(const VarintUnit *units, int64_t n_units) {
    __shared__ uint16_t s_end[4][ODC_UNIT_VALUES];
    const int wave = (int)(threadIdx.x >> 6);
    const int lane = (int)(threadIdx.x & 63);
    const int waves = (int)(blockDim.x >> 6);
    uint16_t *ends = s_end[wave];
    for (int64_t uidx = (int64_t)blockIdx.x * waves + wave; uidx < n_units;
         uidx += (int64_t)gridDim.x * waves) {
        const VarintUnit u = units[uidx];
        const uint64_t base = u.src & ~7ull;     // absolute 8-byte alignment
        const int lead = (int)(u.src - base);    // 0..7 bytes before the unit
        const int span = lead + u.nbytes;        // bytes from base
        const int n_words = (span + 7) >> 3;
        // ---- (a) terminator sweep
        int running = 0;  // terminators in earlier rounds (wave-uniform)
        for (int w0 = 0; w0 < n_words; w0 += 64) {
            const int w = w0 + lane;
            uint64_t term = 0;
            if (w < n_words) {
                const uint64_t word =
                    *reinterpret_cast<const uint64_t *>(base + (uint64_t)w * 8);
                term = ~word & 0x8080808080808080ull;
                // drop bytes outside [lead, span)
                const int lo = lead - w * 8;  // first valid byte of the word
                if (lo > 0) term &= ~0ull << (lo * 8);
                const int hi = span - w * 8;  // bytes of the word in the unit
                if (hi < 8) term &= (1ull << (hi * 8)) - 1;
            }
            const int cnt = __popcll(term);
            int incl = cnt;
            for (int off = 1; off < 64; off <<= 1) {
                const int up = __shfl_up(incl, off, 64);
                if (lane >= off) incl += up;
            }
            int idx = running + incl - cnt;  // index of this lane's first
            while (term) {
                const int byte = (__ffsll((long long)term) - 1) >> 3;
                term &= term - 1;
                if (idx < ODC_UNIT_VALUES)
                    ends[idx] = (uint16_t)(w * 8 + byte - lead);
                idx++;
            }
            running += __shfl(incl, 63, 64);
        }
        __threadfence_block();
        // ---- (b) one lane per value
        // a unit the prescan cut holds exactly `count` terminators; fewer
        // would leave table slots unwritten, so they are not read
        const int n_vals = running < u.count ? running : u.count;
        uint32_t errs =
            running < u.count ? (1u << (ODC_ERR_SHIFT + ODC_ERR_WIDTH)) : 0;
        const int32_t *scales = (const int32_t *)u.scale_addr;
        void *out = (void *)u.out_addr;
        for (int j = lane; j < n_vals; j += 64) {
            const int start = j ? (int)ends[j - 1] + 1 : 0;
            int len = (int)ends[j] - start + 1;
            int err = ODC_OK;
            if (len > ODC_MAX_VARINT) {  // prescan refuses these
                len = ODC_MAX_VARINT;
                err = ODC_ERR_WIDTH;
            }
            const uint64_t a = u.src + (uint64_t)start;
            const uint64_t ab = a & ~7ull;
            const int sh = (int)(a - ab) * 8;  // 0..56
            const int reach = (int)(a - ab) + len;  // bytes from ab
            uint64_t w0 = *reinterpret_cast<const uint64_t *>(ab);
            uint64_t w1 = 0, w2 = 0;
            if (reach > 8) w1 = *reinterpret_cast<const uint64_t *>(ab + 8);
            if (reach > 16) w2 = *reinterpret_cast<const uint64_t *>(ab + 16);
            uint64_t b0 = w0, b1 = w1;
            if (sh) {
                b0 = (w0 >> sh) | (w1 << (64 - sh));
                b1 = (w1 >> sh) | (w2 << (64 - sh));
            }
            const uint64_t raw = odc_compact(b0, b1, len, &err);
            int64_t r = 0;
            if (!err) {
                const int ds = scales ? scales[j] : u.scale;
                err = odc_rescale(zz_dec(raw), ds, u.precision, u.scale,
                                  u.out_esize, &r);
            }
            if (err) errs |= 1u << (ODC_ERR_SHIFT + err);
            dense_store(out, u.out_esize, u.out_start + j, r);
        }
        if (errs && u.err_addr) atomicOr((uint32_t *)u.err_addr, errs);
        // the next unit's sweep overwrites the table: reads must be done
        __threadfence_block();
    }
}

// --------------------------------------------------------- k_bits_expand
//
// BOOLEAN value decode for both formats (bits_core.h): Parquet PLAIN pages
// (1 bit per value, LSB first) and ORC boolean byte-RLE units (MSB first,
// literal bytes or one repeated byte) expand to 0/1 elements, 1 or 4 bytes
// wide. One 64-lane wave per unit, no LDS, no barrier.
// A lane owns one OUTPUT group: the 8 elements of an absolutely aligned
// 8-element block (8 bytes at width 1, 32 bytes at width 4). A unit's first
// element sits at any index (pages and stripes end anywhere, dense counts
// under nulls are arbitrary), so with r = that index modulo 8 the group takes
// the top r bits of source byte g-1 and the low 8 - r bits of byte g. Groups
// wholly inside the unit store wide (one 8-byte or two 16-byte stores per
// lane, consecutive lanes consecutive addresses); the first and the last
// group of a unit may be shared with a neighbouring unit, another wave's, and
// store element by element inside [out_start, out_start + count) only.
// Loads are byte loads of the unit's own ceil(count / 8) source bytes:
// nothing before the unit and nothing of the staging tail pad is touched.
__launch_bounds__(256) __global__
void k_bits_expand(const BitsUnit *units, int64_t n_units) {
    const int wave = (int)(threadIdx.x >> 6);
    const int lane = (int)(threadIdx.x & 63);
    const int waves = (int)(blockDim.x >> 6);
    for (int64_t uidx = (int64_t)blockIdx.x * waves + wave; uidx < n_units;
         uidx += (int64_t)gridDim.x * waves) {
        const BitsUnit u = units[uidx];
        const uint8_t *src = (const uint8_t *)u.src;
        const int r = bits_unit_r(u.out_addr, u.out_start, u.out_esize);
        const int n_groups = bits_unit_groups(r, u.count);
        // element index (from out_addr) of group 0's first element: a
        // multiple of 8 in absolute terms, possibly before out_start
        const int64_t g0 = u.out_start - r;
        for (int g = lane; g < n_groups; g += 64) {
            const uint32_t bits = bits_unit_group(u, src, r, g);
            const int lo = g == 0 ? r : 0;  // first element of the group
                                            // that belongs to the unit
            const int left = r + u.count - 8 * g;
            const int hi = left < 8 ? left : 8;  // one past the last
            const uint64_t bytes = bits_spread(bits);
            if (u.out_esize == 1) {
                uint8_t *p = (uint8_t *)u.out_addr + (g0 + (int64_t)8 * g);
                if (lo == 0 && hi == 8) {
                    *reinterpret_cast<uint64_t *>(p) = bytes;
                } else {
                    for (int t = lo; t < hi; t++)
                        p[t] = (uint8_t)(bytes >> (8 * t));
                }
            } else {
                int32_t *p = (int32_t *)u.out_addr + (g0 + (int64_t)8 * g);
                if (lo == 0 && hi == 8) {
                    const uint32_t b0 = (uint32_t)bytes;
                    const uint32_t b1 = (uint32_t)(bytes >> 32);
                    uint4 v0, v1;
                    v0.x = b0 & 1u;
                    v0.y = (b0 >> 8) & 1u;
                    v0.z = (b0 >> 16) & 1u;
                    v0.w = b0 >> 24;
                    v1.x = b1 & 1u;
                    v1.y = (b1 >> 8) & 1u;
                    v1.z = (b1 >> 16) & 1u;
                    v1.w = b1 >> 24;
                    reinterpret_cast<uint4 *>(p)[0] = v0;
                    reinterpret_cast<uint4 *>(p)[1] = v1;
                } else {
                    for (int t = lo; t < hi; t++)
                        p[t] = (int32_t)((bits >> t) & 1u);
                }
            }
        }
    }
}

// --------------------------------------------------------- k_orc_timestamp
//
// ORC TIMESTAMP combine (orc_timestamp_core.h): k_rlev2 has decoded the DATA
// stream's int64 seconds to the column (or its dense buffer under PRESENT)
// and the SECONDARY stream's stored nanos to the (run, column)'s uint64
// scratch; this elementwise pass replaces each second by the column value
// in milliseconds or microseconds, in place. One workgroup per unit of
// <= OTS_UNIT_VALUES values, one value per thread and step, 8-byte loads and
// stores at consecutive addresses. Refusals OR a bit into the section's
// error word (only threads that met one issue the atomic).
__launch_bounds__(256) __global__
void k_orc_timestamp(const TsUnit *units, int64_t n_units) {
    for (int64_t uidx = blockIdx.x; uidx < n_units; uidx += gridDim.x) {
        const TsUnit u = units[uidx];
        int64_t *out = (int64_t *)u.out_addr + u.out_start;
        const uint64_t *nanos = (const uint64_t *)u.nanos_addr + u.nanos_start;
        uint32_t errs = 0;
        for (int i = (int)threadIdx.x; i < u.count; i += (int)blockDim.x) {
            int64_t v;
            const int err = ots_value(out[i], nanos[i], u.unit, &v);
            if (err) errs |= 1u << (OTS_ERR_SHIFT + err);
            out[i] = v;
        }
        if (errs && u.err_addr) atomicOr((uint32_t *)u.err_addr, errs);
    }
}

// ------------------------------------------------------------ DELTA decode
//
// Parquet DELTA_BINARY_PACKED (VectorizedDeltaBinaryPackedReader.java /
// parquet-format Encodings.md): header <block><miniblocks><count><first>,
// then blocks of [min_delta zigzag][miniblock bit widths][LSB-first packed
// deltas]. value_i = first + sum of deltas. Three batched phases: per-block
// sums (one wave per block), per-page base scan (pages are self-contained
// streams; one workgroup per page), then unpack + wave-scan + base add.

DEV uint64_t le_bits(const uint8_t *src, int64_t bit_off, int width) {
    // LSB-first window like the RLE bit-packed decoder, any width <= 64:
    // two aligned 8-byte loads + shift-combine (uploads padded by 16 B)
    uint64_t addr = (uint64_t)src + (uint64_t)(bit_off >> 3);
    uint64_t base = addr & ~7ull;
    int off = (int)((addr - base) * 8) + (int)(bit_off & 7);
    uint64_t lo = *reinterpret_cast<const uint64_t *>(base);
    uint64_t hi = *reinterpret_cast<const uint64_t *>(base + 8);
    uint64_t window = off ? ((lo >> off) | (hi << (64 - off))) : lo;
    return width == 64 ? window : window & ((1ull << width) - 1);
}

DEV int64_t delta_at(const DeltaChunk &ch, int d) {
    // miniblock of delta d and its packed offset
    const int j = d / ch.vpm;
    int64_t byte_off = 0;
    for (int q = 0; q < j; q++)
        byte_off += (int64_t)ch.vpm * ((ch.widths >> (8 * q)) & 0xff) / 8;
    const int w = (int)((ch.widths >> (8 * j)) & 0xff);
    if (w == 0) return ch.min_delta;
    const uint64_t raw = le_bits((const uint8_t *)ch.src,
                                 (int64_t)(d % ch.vpm) * w + byte_off * 8,
                                 w);
    return ch.min_delta + (int64_t)raw;
}

__global__ void k_delta_sum(const DeltaChunk *chunks, int64_t n_chunks,
                            int64_t *sums) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t wave =
        (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t c = wave; c < n_chunks; c += n_waves) {
        const DeltaChunk ch = chunks[c];
        int64_t acc = 0;
        for (int d = lane; d < ch.count; d += 64) acc += delta_at(ch, d);
        for (int off = 32; off; off >>= 1)
            acc += __shfl_down(acc, off, 64);
        if (lane == 0) sums[c] = acc;
    }
}

__global__ void k_delta_scan(const DeltaStream *streams, int64_t n_streams,
                             const int64_t *sums, int64_t *bases) {
    // one workgroup per stream (page): running exclusive scan over its
    // blocks' sums, seeded by the page's first value; also stores the
    // page's first value itself
    __shared__ int64_t s[256];
    __shared__ int64_t running;
    for (int64_t si = blockIdx.x; si < n_streams; si += gridDim.x) {
        const DeltaStream st = streams[si];
        if (threadIdx.x == 0) {
            running = st.first;
            if (st.out_esize == 8)
                ((int64_t *)st.out_addr)[st.out0] = st.first;
            else
                ((int32_t *)st.out_addr)[st.out0] = (int32_t)st.first;
        }
        __syncthreads();
        for (int64_t b = st.chunk_lo; b < st.chunk_hi; b += blockDim.x) {
            int64_t i = b + threadIdx.x;
            int64_t v = i < st.chunk_hi ? sums[i] : 0;
            s[threadIdx.x] = v;
            __syncthreads();
            for (int d = 1; d < (int)blockDim.x; d <<= 1) {
                int64_t add = threadIdx.x >= d ? s[threadIdx.x - d] : 0;
                __syncthreads();
                s[threadIdx.x] += add;
                __syncthreads();
            }
            if (i < st.chunk_hi) bases[i] = running + s[threadIdx.x] - v;
            __syncthreads();
            if (threadIdx.x == 0) running += s[blockDim.x - 1];
            __syncthreads();
        }
    }
}

__global__ void k_delta_emit(const DeltaChunk *chunks, int64_t n_chunks,
                             const int64_t *bases) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t wave =
        (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t c = wave; c < n_chunks; c += n_waves) {
        const DeltaChunk ch = chunks[c];
        int64_t run = bases[c];
        for (int b = 0; b < ch.count; b += 64) {
            const int d = b + lane;
            int64_t x = d < ch.count ? delta_at(ch, d) : 0;
            // inclusive wave scan
            int64_t acc = x;
            for (int off = 1; off < 64; off <<= 1) {
                int64_t up = __shfl_up(acc, off, 64);
                if (lane >= off) acc += up;
            }
            if (d < ch.count) {
                if (ch.out_esize == 8)
                    ((int64_t *)ch.out_addr)[ch.out_start + d] = run + acc;
                else
                    ((int32_t *)ch.out_addr)[ch.out_start + d] =
                        (int32_t)(run + acc);
            }
            run += __shfl(acc, 63, 64);
        }
    }
}

// ------------------------------------------------------------ k_rle_decode
// Decode Parquet RLE/bit-packed hybrid streams (dictionary ids, def levels)
// from host-prescanned run chunks (VectorizedRleValuesReader.java:977-1018
// wire format; the sequential varint-header walk happens on the host at
// staging time, the bulk expansion here).
__global__ void k_rle_decode(const RleChunk *chunks, int64_t n_chunks,
                             int32_t *out) {
    for (int64_t cidx = blockIdx.x; cidx < n_chunks; cidx += gridDim.x) {
        RleChunk ch = chunks[cidx];
        int bit_width = ch.bit_width;
        uint32_t mask =
            bit_width >= 32 ? 0xffffffffu : ((1u << bit_width) - 1u);
        if (ch.kind == 0) {
            for (int32_t i = threadIdx.x; i < ch.count; i += blockDim.x)
                out[ch.out_start + i] = (int32_t)ch.value;
        } else {
            const uint8_t *src = (const uint8_t *)ch.src;
            for (int32_t i = threadIdx.x; i < ch.count; i += blockDim.x) {
                int64_t g = i >> 3;
                int lane = i & 7;
                const uint8_t *gp = src + g * bit_width;
                int64_t bit_off = (int64_t)lane * bit_width;
                int64_t byte_off = bit_off >> 3;
                int shift = (int)(bit_off & 7);
                uint64_t word = 0;
                for (int b = 0; b < 5 && byte_off + b < bit_width; b++)
                    word |= (uint64_t)gp[byte_off + b] << (8 * b);
                out[ch.out_start + i] = (int32_t)((word >> shift) & mask);
            }
        }
    }
}

// ------------------------------------------------------------ k_dict_gather
template <typename T>
__global__ void k_dict_gather_t(const int32_t *ids, const T *dict, int64_t n,
                                T *out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) out[i] = dict[ids[i]];
}

// endpoint seed for the single-level (k > 8) partition: write cuts for
// b = 0 (all zeros) and b = n_bounds-1 (run lengths) so k_partition_refine
// can treat [0, lens) as one full-width coarse window.
__global__ void k_partition_seed(const int64_t *lens, int k,
                                 int64_t n_bounds, int32_t *cuts) {
    int r = threadIdx.x;
    if (r >= k) return;
    cuts[r] = 0;
    cuts[(n_bounds - 1) * k + r] = (int32_t)lens[r];
}



// --------------------------------------------------------- k_zstd_compress
//
// On-GPU zstd page COMPRESSION (the write side): one wave
// per page, lane-0 serial v0 over the shared scalar encoder (greedy LZ +
// RAW literals + predefined-FSE sequences — spec-valid frames, proven
// against libzstd on the host). Page-level parallelism carries the
// throughput exactly like k_zstd_pages. Scratch: one PzEnc per job.
__global__ void k_zstd_compress(const uint8_t *src, const ZstdJob *jobs,
                                int n, uint8_t *dst, uint8_t *scratch,
                                int64_t *status) {
    // job = one 128 KB zstd BLOCK (matches are block-confined, so blocks
    // compress independently — the host stitches them into frames);
    // dst_len bit 31 carries the last-block flag
    __shared__ int32_t lhtab[4][1 << PZ_ENC_HLOG];  // 16 KB per wave
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int wiw = (threadIdx.x >> 6) & 3;
    const int lane = threadIdx.x & 63;
    const int waves = (int)((gridDim.x * blockDim.x) >> 6);
    for (int j = wave; j < n; j += waves) {
        if (lane != 0) continue;
        PzEnc *e = (PzEnc *)(scratch + (size_t)j * sizeof(PzEnc));
        e->htab = lhtab[wiw];
        int last = (int)(jobs[j].dst_len >> 31);
        int64_t cap = jobs[j].dst_len & 0x7FFFFFFF;
        status[j] = pz_encode_block(src + jobs[j].src_off, jobs[j].src_len,
                                    last, dst + jobs[j].dst_off, cap, e);
    }
}

// ------------------------------------------------------------- k_filter
//
// Value-filter pushdown for SINGLE-RUN sections (MergeFileSplitRead.java:
// 227-239: each key appears once, so dropping rows is safe; overlapping
// sections get no value filters). Failing rows mark the run's tombstone
// byte — the same "never reaches the merge" mechanism deletion vectors
// use. Comparison semantics follow LeafPredicate: a NULL field fails
// every comparison; is_null/is_not_null test validity.
__global__ void k_filter(const DevCol *cols, int n_cols,
                         const FilterTerm *terms, int n_terms, int64_t rows,
                         uint8_t *tomb) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < rows; i += stride) {
        bool pass = true;
        for (int t = 0; t < n_terms && pass; t++) {
            const FilterTerm &ft = terms[t];
            const DevCol &dc = cols[ft.col];
            bool valid = col_valid(dc, i) != 0;
            if (ft.op == 6) {
                pass = !valid;
                continue;
            }
            if (ft.op == 7) {
                pass = valid;
                continue;
            }
            if (!valid) {
                pass = false;  // NULL fails comparisons
                continue;
            }
            int cmp;
            if (ft.is_fp) {
                double v = dc.esize == 8
                               ? *(const double *)(dc.addr0 + i * 8)
                               : (double)*(const float *)(dc.addr0 + i * 4);
                cmp = v < ft.dlit ? -1 : (v > ft.dlit ? 1 : 0);
            } else {
                int64_t v = dc.esize == 8 ? col_load<int64_t>(dc, i)
                                          : (int64_t)col_load<int32_t>(dc, i);
                cmp = v < ft.ilit ? -1 : (v > ft.ilit ? 1 : 0);
            }
            switch (ft.op) {
            case 0: pass = cmp == 0; break;
            case 1: pass = cmp != 0; break;
            case 2: pass = cmp < 0; break;
            case 3: pass = cmp <= 0; break;
            case 4: pass = cmp > 0; break;
            case 5: pass = cmp >= 0; break;
            default: pass = false; break;
            }
        }
        if (!pass) tomb[i] = 1;
    }
}

// ----------------------------------------------------------- k_lookup_probe
//
// Point lookup of the lookup changelog producer (LookupLevels.lookup; the
// reference probes one key at a time through a local file cache): a batched
// sorted-probe search over the device-resident lookup levels. Probe keys
// are the rows of one level-0 run, so they arrive sorted; a workgroup takes
// PLK_CHUNK consecutive keys, ONE wave bounds the chunk's window in every
// level from the chunk's first and last key (lane l serves level l — whole-
// level bisections, once per chunk), and each thread then bisects only
// inside those windows (lookup_core.h), so the per-key probes touch a small
// slice of each level that stays cache-resident. Output words are coalesced
// 4-byte stores. grid = (chunks, k): blockIdx.y is the run.
__launch_bounds__(256) __global__
void k_lookup_probe(const DevCol *keys, const int64_t *lens,
                    const int64_t *probe_off, int k, int n_levels,
                    uint32_t *words) {
    __shared__ PlkLevel s_lv[PMH_MAX_RUNS];
    __shared__ int64_t s_wlo[PMH_MAX_RUNS], s_whi[PMH_MAX_RUNS];
    const int r = blockIdx.y;
    const int64_t off = probe_off[r];
    if (off < 0) return;  // block-uniform: run r is not a level-0 run
    const int64_t n = lens[r];
    const int tid = threadIdx.x;
    if (tid < n_levels) {
        const DevCol &dc = keys[k + tid];
        s_lv[tid] = PlkLevel{dc.addr0, lens[k + tid], dc.esize, 0};
    }
    const uint64_t kaddr = keys[r].addr0;
    const int kes = keys[r].esize;
    __syncthreads();
    for (int64_t base = (int64_t)blockIdx.x * PLK_CHUNK; base < n;
         base += (int64_t)gridDim.x * PLK_CHUNK) {
        const int cnt = (int)(n - base < PLK_CHUNK ? n - base : PLK_CHUNK);
        if (tid < n_levels)
            plk_window(s_lv[tid], plk_key_at(kaddr, base, kes),
                       plk_key_at(kaddr, base + cnt - 1, kes), &s_wlo[tid],
                       &s_whi[tid]);
        __syncthreads();
        for (int i = tid; i < cnt; i += blockDim.x) {
            int64_t row = 0;
            const int l = plk_probe(s_lv, n_levels, s_wlo, s_whi,
                                    plk_key_at(kaddr, base + i, kes), &row);
            words[off + base + i] =
                l < 0 ? PLK_MISS
                      : ((uint32_t)(k + l) << PMH_ROW_BITS) | (uint32_t)row;
        }
        __syncthreads();  // windows are rewritten by the next chunk
    }
}

// ------------------------------------------------------------ k_cl_finalize
//
// Compact the provisional changelog entries into dense per-tile rows.
// Pending UPDATE_BEFORE/UPDATE_AFTER pairs (changelog-producer.
// row-deduplicate) compare the two records' value columns (the reference's
// RecordEqualiser over the read schema) and are dropped when equal.
// Writes the compacted rows into cl_out (same per-tile stride) and
// rewrites cl_counts[tile] from group count to ROW count.
__global__ void k_cl_finalize(const DevCol *cols, const uint8_t *col_dtype,
                              int n_cols, int first_val, int k,
                              const uint64_t *cl_entries, uint64_t *cl_out,
                              int32_t *cl_counts, int64_t n_tiles,
                              int64_t tile_rows) {
    __shared__ int32_t scan[257];
    const int64_t stride2 = 2 * (tile_rows + PMH_MAX_RUNS);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t *in = &cl_entries[tile * stride2];
        uint64_t *out = &cl_out[tile * stride2];
        int32_t ng = cl_counts[tile];
        const int tid = threadIdx.x;
        const int32_t per = (ng + (int32_t)blockDim.x - 1) / blockDim.x;
        int32_t lo = tid * per;
        int32_t hi = lo + per < ng ? lo + per : ng;
        // verdict per group: 2 bits (number of surviving rows, 0/1/2)
        uint32_t verd[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // per <= 128 groups
        int32_t nrows = 0;
        for (int32_t g = lo; g < hi; g++) {
            uint64_t e0 = in[2 * g], e1 = in[2 * g + 1];
            int nv = ((e0 >> 35) & 1) + ((e1 >> 35) & 1);
            if ((e0 >> 36) & 1) {  // pending pair: value-equality check
                uint32_t a = (uint32_t)e0, b = (uint32_t)e1;
                int64_t xa = member_row(a), xb = member_row(b);
                bool eq = true;
                for (int c = first_val; eq && c < n_cols; c++) {
                    const DevCol &da = member_col(cols, n_cols, a, c);
                    const DevCol &db = member_col(cols, n_cols, b, c);
                    uint8_t va = col_valid(da, xa);
                    uint8_t vb = col_valid(db, xb);
                    if (va != vb) {
                        eq = false;
                    } else if (va) {
                        if (da.esize == 8
                                ? (col_load<int64_t>(da, xa) !=
                                   col_load<int64_t>(db, xb))
                                : (col_load<int32_t>(da, xa) !=
                                   col_load<int32_t>(db, xb)))
                            eq = false;
                    }
                }
                if (eq) nv = 0;
            }
            int li = g - lo;
            verd[li >> 4] |= (uint32_t)nv << (2 * (li & 15));
            nrows += nv;
        }
        // block exclusive scan of nrows (group order preserved)
        scan[tid + 1] = nrows;
        if (tid == 0) scan[0] = 0;
        __syncthreads();
        for (int off = 1; off < (int)blockDim.x; off <<= 1) {
            int32_t v = tid + 1 > off ? scan[tid + 1 - off] : 0;
            __syncthreads();
            scan[tid + 1] += v;
            __syncthreads();
        }
        int32_t o = scan[tid];
        for (int32_t g = lo; g < hi; g++) {
            int li = g - lo;
            int nv = (verd[li >> 4] >> (2 * (li & 15))) & 3;
            if (nv >= 1) out[o++] = in[2 * g];
            if (nv == 2) out[o++] = in[2 * g + 1];
        }
        __syncthreads();
        if (tid == (int)blockDim.x - 1) cl_counts[tile] = o;
        __syncthreads();
    }
}

// ---------------------------------------------------------------- k_cl_emit
//
// Gather the compacted changelog rows into the changelog output columns:
// key/seq/value columns come from the source record; the kind column is
// the changelog RowKind carried in the entry (INSERT / UPDATE_BEFORE /
// UPDATE_AFTER / DELETE).
__global__ void k_cl_emit(const DevCol *cols, const uint8_t *col_dtype,
                          const uint8_t *col_nullable, int n_cols,
                          int kind_col, const uint64_t *cl_rows,
                          const int32_t *cl_counts,
                          const int64_t *cl_offsets, int64_t n_tiles,
                          int64_t tile_rows, void *const *out_ptrs,
                          uint8_t *const *out_valid) {
    const int64_t stride2 = 2 * (tile_rows + PMH_MAX_RUNS);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t *in = &cl_rows[tile * stride2];
        const int32_t n = cl_counts[tile];
        const int64_t ob = cl_offsets[tile];
        for (int32_t i = threadIdx.x; i < n; i += blockDim.x) {
            uint64_t e = in[i];
            uint32_t m = (uint32_t)e;
            int8_t kd = (int8_t)((e >> 32) & 7);
            int64_t o = ob + i;
            for (int c = 0; c < n_cols; c++) {
                if (col_nullable[c] && out_valid[c])
                    out_valid[c][o] = member_valid(cols, n_cols, m, c);
                if (c == kind_col) {
                    ((int8_t *)out_ptrs[c])[o] = kd;
                    continue;
                }
                const int dt = col_dtype[c];
                out_store(out_ptrs[c], dt, o,
                          member_load(cols, n_cols, m, c, dt));
            }
        }
        __syncthreads();
    }
}

// ------------------------------------- k_cl_finalize_out / k_cl_emit_out
//
// The changelog chain of the folding engines (partial-update / aggregation).
// An after-type row there is the engine's folded result, which is no (run,
// row) of any input: its entry carries CLC_FROM_OUT and the group's tile-local
// index g among the kept groups, and the row is read from the plan's MAIN
// output at tile_offsets[tile] + g — where k_emit_pu / k_emit_pu_sg /
// k_emit_agg wrote it, so both kernels run after the engine's emit on the
// same stream. Before-type rows name the top-level record as (run, row), as
// in k_cl_finalize / k_cl_emit.
//
// Both kernels keep one workgroup per tile (grid-stride) and read nothing
// but entries and column data inside their loops: per run and column the
// source address / validity address, per column the main and changelog
// output pointers and the output width, are staged in LDS once per block
// (pmh_fold_cl_lds bytes; plan creation refuses a section whose tables exceed
// PMH_FOLD_CL_LDS_MAX). Data moves through
// address_space(1) pointers.
constexpr int FOLD_CL_THREADS = 256;
constexpr int FOLD_CL_G = 4;  // columns whose loads are in flight together

struct FoldClTables {
    uint64_t *addr;    // [k * n_cols] source element 0
    uint64_t *valid;   // [k * n_cols] source validity bytes, 0 = all valid
    uint64_t *out;     // [n_cols] main output column
    uint64_t *ov;      // [n_cols] main output validity, 0 = none
    uint64_t *out2;    // [n_cols] changelog output column
    uint64_t *ov2;     // [n_cols] changelog output validity, 0 = none
    uint8_t *width;    // [n_cols] output width 1 / 2 / 4 / 8; 0 = not moved
};

// Carve the tables out of dynamic LDS and fill them; ends with a barrier
// that every thread of the block reaches.
DEV FoldClTables fold_cl_stage(uint64_t *smem, const DevCol *cols,
                               const uint8_t *col_dtype,
                               const uint8_t *col_nullable, int n_cols, int k,
                               void *const *out_ptrs,
                               uint8_t *const *out_valid,
                               void *const *out_ptrs2,
                               uint8_t *const *out_valid2) {
    FoldClTables t;
    const int n_ent = k * n_cols;
    t.addr = smem;
    t.valid = t.addr + n_ent;
    t.out = t.valid + n_ent;
    t.ov = t.out + n_cols;
    t.out2 = t.ov + n_cols;
    t.ov2 = t.out2 + n_cols;
    t.width = (uint8_t *)(t.ov2 + n_cols);
    for (int e = threadIdx.x; e < n_ent; e += FOLD_CL_THREADS) {
        t.addr[e] = cols[e].addr0;
        t.valid[e] = cols[e].valid0;
    }
    for (int c = threadIdx.x; c < n_cols; c += FOLD_CL_THREADS) {
        t.width[c] = (uint8_t)pmh_out_width(col_dtype[c]);
        t.out[c] = (uint64_t)out_ptrs[c];
        t.ov[c] = col_nullable[c] ? (uint64_t)out_valid[c] : 0;
        t.out2[c] = out_ptrs2 ? (uint64_t)out_ptrs2[c] : 0;
        t.ov2[c] =
            out_valid2 && col_nullable[c] ? (uint64_t)out_valid2[c] : 0;
    }
    __syncthreads();
    return t;
}

// Value of column c (output width w) as the OUTPUT stores it, sign-extended
// to 64 bits. src: the source row `row` of run-table base `rb` (stored width
// 4 for w <= 4, else 8), narrowed the way the emit kernels narrow; else row
// `row` of the main output.
DEV int64_t fold_cl_value(const FoldClTables &t, int c, int w, bool src,
                          int rb, uint64_t row) {
    const uint64_t base = src ? t.addr[rb + c] : t.out[c];
    if (w == 8) return gload<int64_t>(base + row * 8);
    if (w == 4 || src) {
        const int32_t v = gload<int32_t>(base + row * 4);
        return w == 1 ? (int64_t)(int8_t)v : w == 2 ? (int64_t)(int16_t)v : v;
    }
    return w == 2 ? (int64_t)gload<int16_t>(base + row * 2)
                  : (int64_t)gload<int8_t>(base + row);
}

DEV uint8_t fold_cl_validity(const FoldClTables &t, int c, bool src, int rb,
                             uint64_t row) {
    const uint64_t va = src ? t.valid[rb + c] : t.ov[c];
    return va ? gload<uint8_t>(va + row) : (uint8_t)1;
}

// Compact the provisional entries of the folded walk into dense per-tile
// rows, as k_cl_finalize does. A pending UPDATE_BEFORE / UPDATE_AFTER pair
// compares top's source row with the main-output row of its group, value
// columns only: validity first, then the bits the output stores (both sides
// null = equal whatever the bits). cl_counts[tile] goes from pair count to
// row count. A thread owns a contiguous range of <= 16 pairs (2-bit verdicts
// in one register), so rows stay in key order; the block scan is k_scan_tiles'
// (wave shuffles + one barrier per tile, wave totals double-buffered).
__launch_bounds__(FOLD_CL_THREADS) __global__
void k_cl_finalize_out(const DevCol *cols, const uint8_t *col_dtype,
                       const uint8_t *col_nullable, int n_cols, int first_val,
                       int k, const uint64_t *cl_entries, uint64_t *cl_out,
                       int32_t *cl_counts, const int64_t *tile_offsets,
                       int64_t n_tiles, int64_t tile_rows,
                       void *const *out_ptrs, uint8_t *const *out_valid) {
    extern __shared__ uint64_t fold_smem[];
    constexpr int NW = FOLD_CL_THREADS / 64;
    __shared__ int32_t wave_tot[2][NW];
    const FoldClTables t =
        fold_cl_stage(fold_smem, cols, col_dtype, col_nullable, n_cols, k,
                      out_ptrs, out_valid, nullptr, nullptr);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int64_t cap = tile_rows + PMH_MAX_RUNS;  // pairs a tile can hold
    int buf = 0;
    for (int64_t tile = blockIdx.x; tile < n_tiles;
         tile += gridDim.x, buf ^= 1) {
        const uint64_t *in = &cl_entries[tile * 2 * cap];
        uint64_t *out = &cl_out[tile * 2 * cap];
        int32_t ng = cl_counts[tile];
        ng = ng < 0 ? 0 : (ng > cap ? (int32_t)cap : ng);
        const int64_t ob = tile_offsets[tile];
        const int32_t per = (ng + FOLD_CL_THREADS - 1) / FOLD_CL_THREADS;
        const int32_t lo = tid * per;
        const int32_t hi = lo + per < ng ? lo + per : ng;
        uint32_t verd = 0;  // 2 bits per pair: rows that survive
        int32_t nrows = 0;
        for (int32_t g = lo; g < hi; g++) {
            const uint64_t e0 = in[2 * g], e1 = in[2 * g + 1];
            int nv = (int)((e0 >> 35) & 1) + (int)((e1 >> 35) & 1);
            if (e0 & CLC_PENDING) {
                // e0 = UPDATE_BEFORE(top, a source row), e1 = UPDATE_AFTER
                // (merged, a main-output row)
                const uint32_t a = (uint32_t)e0;
                const int rb = (int)(a >> PMH_ROW_BITS) * n_cols;
                const uint64_t xa = a & PMH_ROW_MASK;
                const uint64_t xb = (uint64_t)(ob + (uint32_t)e1);
                bool eq = true;
                for (int c0 = first_val; eq && c0 < n_cols; c0 += FOLD_CL_G) {
                    // the group's validity bytes and values, all in flight
                    // before the first compare
                    uint8_t va[FOLD_CL_G], vb[FOLD_CL_G];
                    int64_t pa[FOLD_CL_G], pb[FOLD_CL_G];
#pragma unroll
                    for (int j = 0; j < FOLD_CL_G; j++) {
                        const int c = c0 + j < n_cols ? c0 + j : n_cols - 1;
                        const int w = t.width[c];
                        va[j] = fold_cl_validity(t, c, true, rb, xa);
                        vb[j] = fold_cl_validity(t, c, false, 0, xb);
                        pa[j] = w ? fold_cl_value(t, c, w, true, rb, xa) : 0;
                        pb[j] = w ? fold_cl_value(t, c, w, false, 0, xb) : 0;
                    }
#pragma unroll
                    for (int j = 0; j < FOLD_CL_G; j++)
                        if ((va[j] != 0) != (vb[j] != 0) ||
                            (va[j] && pa[j] != pb[j]))
                            eq = false;
                }
                if (eq) nv = 0;
            }
            verd |= (uint32_t)nv << (2 * (g - lo));
            nrows += nv;
        }
        int32_t incl = nrows;
        for (int off = 1; off < 64; off <<= 1) {
            const int32_t up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        if (lane == 63) wave_tot[buf][wv] = incl;
        __syncthreads();
        int32_t add = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) {
            const int32_t x = wave_tot[buf][w];
            if (w < wv) add += x;
            tot += x;
        }
        int32_t o = add + incl - nrows;
        for (int32_t g = lo; g < hi; g++) {
            const int nv = (verd >> (2 * (g - lo))) & 3;
            if (nv >= 1) out[o++] = in[2 * g];
            if (nv == 2) out[o++] = in[2 * g + 1];
        }
        if (tid == 0) cl_counts[tile] = tot;
    }
}

// Write the compacted rows into the changelog output columns. A before-type
// row gathers key, sequence number, values and validity from its source
// record, an after-type row copies them from the main output row; the kind
// column takes the changelog RowKind of the entry. Columns go in groups of
// FOLD_CL_G: a row's loads of the group are issued before its stores.
__launch_bounds__(FOLD_CL_THREADS) __global__
void k_cl_emit_out(const DevCol *cols, const uint8_t *col_dtype,
                   const uint8_t *col_nullable, int n_cols, int k,
                   int kind_col, const uint64_t *cl_rows,
                   const int32_t *cl_counts, const int64_t *cl_offsets,
                   const int64_t *tile_offsets, int64_t n_tiles,
                   int64_t tile_rows, void *const *out_ptrs,
                   uint8_t *const *out_valid, void *const *out_ptrs2,
                   uint8_t *const *out_valid2) {
    extern __shared__ uint64_t fold_smem[];
    const FoldClTables t =
        fold_cl_stage(fold_smem, cols, col_dtype, col_nullable, n_cols, k,
                      out_ptrs, out_valid, out_ptrs2, out_valid2);
    const int64_t cap2 = 2 * (tile_rows + PMH_MAX_RUNS);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t *in = &cl_rows[tile * cap2];
        int32_t n = cl_counts[tile];
        n = n < 0 ? 0 : (n > cap2 ? (int32_t)cap2 : n);
        const int64_t ob = cl_offsets[tile];
        const int64_t mb = tile_offsets[tile];
        for (int32_t i = threadIdx.x; i < n; i += FOLD_CL_THREADS) {
            const uint64_t e = in[i];
            const bool src = !(e & CLC_FROM_OUT);
            const uint32_t m = (uint32_t)e;
            const int rb = src ? (int)(m >> PMH_ROW_BITS) * n_cols : 0;
            const uint64_t row =
                src ? (uint64_t)(m & PMH_ROW_MASK) : (uint64_t)(mb + m);
            const int8_t kd = (int8_t)((e >> CLC_KIND_SHIFT) & 7);
            const uint64_t o = (uint64_t)(ob + i);
            for (int c0 = 0; c0 < n_cols; c0 += FOLD_CL_G) {
                uint8_t vb[FOLD_CL_G];
                int64_t v[FOLD_CL_G];
#pragma unroll
                for (int j = 0; j < FOLD_CL_G; j++) {
                    const int c = c0 + j < n_cols ? c0 + j : n_cols - 1;
                    const int w = t.width[c];
                    vb[j] = fold_cl_validity(t, c, src, rb, row);
                    v[j] = c == kind_col ? (int64_t)kd
                           : w ? fold_cl_value(t, c, w, src, rb, row)
                               : 0;
                }
#pragma unroll
                for (int j = 0; j < FOLD_CL_G; j++) {
                    const int c = c0 + j;
                    if (c >= n_cols) break;
                    const int w = t.width[c];
                    if (t.ov2[c]) gstore<uint8_t>(t.ov2[c] + o, vb[j]);
                    const uint64_t d = t.out2[c];
                    if (c == kind_col || w == 1)
                        gstore<int8_t>(d + o, (int8_t)v[j]);
                    else if (w == 2)
                        gstore<int16_t>(d + o * 2, (int16_t)v[j]);
                    else if (w == 4)
                        gstore<int32_t>(d + o * 4, (int32_t)v[j]);
                    else if (w == 8)
                        gstore<int64_t>(d + o * 8, v[j]);
                }
            }
        }
    }
}

// ------------------------------------------------------------ k_zstd_pages
//
// On-GPU zstd page decompression: one WAVEFRONT per parquet
// page frame. The scalar RFC 8878 core (zstd_core.h — fuzz-pinned against
// libzstd on the host) does all header/table parsing; the wave supplies the
// parallelism where the bytes move:
//  - raw/RLE blocks and raw/RLE literals: 64-lane copies/fills;
//  - huffman literals: the 4 interleaved streams decode on 4 lanes in SIMD
//    lockstep, each with a register 64-bit bit-window (one 8-byte refill
//    per ~7 symbols instead of 6 dependent byte loads per symbol), LUT in
//    LDS;
//  - sequence execution: 64-lane literal copies and match copies (overlap
//    handled with the period trick: byte j of a match reads
//    dst[start - off + j % off]), __threadfence_block between dependent
//    phases (same-CU L1 visibility);
//  - sequence DECODE stays serial on lane 0 (FSE state chain), buffered 64
//    sequences at a time through LDS.
// Scratch per job: 128 KB literals buffer + decode context.

// per-wave LDS workspace
struct ZWaveLds {
    PzHuf hlut[1 << PZ_HUF_LOG_MAX];  // 4 KB huffman LUT
    uint32_t ll[64], ml[64];          // sequence ring (lane 0 -> wave)
    uint64_t off[64];
    int32_t stat[4];                  // per-stream literal decode status
    int64_t flag;                     // lane-0 -> wave broadcast / error
};

// backward bit reader with a register window (device hot loops)
struct ZBack {
    const uint8_t *buf;
    int64_t bp;    // absolute bit position of the next read's top
    uint64_t win;  // bits [wlo, wlo+64)
    int64_t wlo;
    DEV void init(const uint8_t *b, int64_t sentinel_bp) {
        buf = b;
        bp = sentinel_bp;
        wlo = INT64_MIN / 2;
        win = 0;
    }
    DEV void refill(int64_t lo) {
        int64_t byte0 = lo >> 3;  // floor, works for negative lo
        wlo = byte0 << 3;
        uint64_t v = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            int64_t by = byte0 + i;
            v |= (uint64_t)(by >= 0 ? buf[by] : (uint8_t)0) << (8 * i);
        }
        win = v;
    }
    DEV uint32_t peek(int n) {  // bits [bp-n, bp), n <= 57
        int64_t lo = bp - n;
        if (lo < wlo || bp > wlo + 64) refill(lo);
        return (uint32_t)((win >> (lo - wlo)) &
                          ((n >= 32) ? 0xFFFFFFFFu : ((1u << n) - 1u)));
    }
    DEV uint32_t peek_abs(int n) {  // bits [bp, bp+n) — bp pre-decremented
        if (n == 0) return 0;
        if (bp < wlo || bp + n > wlo + 64) refill(bp);
        return (uint32_t)((win >> (bp - wlo)) &
                          ((n >= 32) ? 0xFFFFFFFFu : ((1u << n) - 1u)));
    }
};

// lane-0 sequence decode over the register bit-window (the scalar
// pz_seq_next re-gathers 6 bytes per field read; ZBack refills once per
// ~56 bits — the "next lever" for k_zstd_pages' match-heavy frames)
static DEV int zdev_seq_next(ZBack &rb, const PzFse *llT, const PzFse *ofT,
                             const PzFse *mlT, uint32_t &sll, uint32_t &sof,
                             uint32_t &sml, uint64_t rep[3], int last,
                             PzSeq *out) {
    int llc = llT[sll].sym;
    int ofc = ofT[sof].sym;
    int mlc = mlT[sml].sym;
    if (llc > 35 || mlc > 52 || ofc > 31) return PZ_ERR_SEQ;
    uint64_t ofv;
    if (ofc > 0) {
        rb.bp -= ofc;
        ofv = ((uint64_t)1 << ofc) + rb.peek_abs(ofc);
    } else {
        ofv = 1;
    }
    int mb = pz_ml_bits(mlc);
    rb.bp -= mb;
    uint32_t ml = pz_ml_base(mlc) + rb.peek_abs(mb);
    int lb = pz_ll_bits(llc);
    rb.bp -= lb;
    uint32_t ll = pz_ll_base(llc) + rb.peek_abs(lb);
    uint64_t off;
    if (ofv > 3) {
        off = ofv - 3;
        rep[2] = rep[1];
        rep[1] = rep[0];
        rep[0] = off;
    } else {
        int idx = (int)ofv - 1 + (ll == 0 ? 1 : 0);
        if (idx == 0) {
            off = rep[0];
        } else if (idx == 1) {
            off = rep[1];
            rep[1] = rep[0];
            rep[0] = off;
        } else if (idx == 2) {
            off = rep[2];
            rep[2] = rep[1];
            rep[1] = rep[0];
            rep[0] = off;
        } else {
            off = rep[0] - 1;
            if (off == 0) return PZ_ERR_OFFSET;
            rep[2] = rep[1];
            rep[1] = rep[0];
            rep[0] = off;
        }
    }
    out->ll = ll;
    out->ml = ml;
    out->off = off;
    if (!last) {
        rb.bp -= llT[sll].nbits;
        sll = llT[sll].base + rb.peek_abs(llT[sll].nbits);
        rb.bp -= mlT[sml].nbits;
        sml = mlT[sml].base + rb.peek_abs(mlT[sml].nbits);
        rb.bp -= ofT[sof].nbits;
        sof = ofT[sof].base + rb.peek_abs(ofT[sof].nbits);
        if (rb.bp < 0) return PZ_ERR_SEQ;
    }
    return 0;
}

static DEV void z_fence() { __threadfence_block(); }

// decode one frame with one wave. Returns decompressed size or PZ_ERR_*.
static DEV int64_t zdev_page(const uint8_t *src, int64_t slen, uint8_t *dst,
                             int64_t dcap, uint8_t *lit, PzCtx *cx,
                             ZWaveLds *L) {
    const int lane = threadIdx.x & 63;
    PzFrame F;
    int fh = pz_parse_frame(src, slen, &F);  // all lanes, redundant+uniform
    if (fh < 0) return fh;
    int64_t sp = fh, dp = 0;
    int htl = -1;
    PzSeqState st;  // lane 0 only (sequence states + repeat offsets)
    st.rep[0] = 1;
    st.rep[1] = 4;
    st.rep[2] = 8;
    if (lane == 0) {
        cx->htl = -1;
        cx->have_ll = cx->have_of = cx->have_ml = 0;
    }
    int last = 0;
    while (!last) {
        if (sp + 3 > slen) return PZ_ERR_SRC_SMALL;
        uint32_t bh = (uint32_t)src[sp] | ((uint32_t)src[sp + 1] << 8) |
                      ((uint32_t)src[sp + 2] << 16);
        sp += 3;
        last = bh & 1;
        int btype = (bh >> 1) & 3;
        int64_t bsize = bh >> 3;
        if (btype == 0) {  // raw block
            if (sp + bsize > slen || dp + bsize > dcap)
                return PZ_ERR_SRC_SMALL;
            for (int64_t j = lane; j < bsize; j += 64)
                dst[dp + j] = src[sp + j];
            z_fence();
            sp += bsize;
            dp += bsize;
            continue;
        }
        if (btype == 1) {  // RLE block
            if (sp + 1 > slen || dp + bsize > dcap) return PZ_ERR_SRC_SMALL;
            uint8_t v = src[sp];
            for (int64_t j = lane; j < bsize; j += 64) dst[dp + j] = v;
            z_fence();
            sp += 1;
            dp += bsize;
            continue;
        }
        if (btype != 2 || bsize > slen - sp) return PZ_ERR_BLOCK;
        const uint8_t *bb = src + sp;
        int64_t bn = bsize;
        sp += bsize;
        PzLits Lh;
        int rc = pz_parse_lits(bb, bn, &Lh);  // uniform on all lanes
        if (rc < 0) return rc;
        int64_t pos = Lh.hdr;
        int64_t nlit = Lh.regen;
        if (nlit > PZ_BLOCK_MAX) return PZ_ERR_LITERALS;
        if (Lh.type == 0) {  // raw literals
            if (pos + nlit > bn) return PZ_ERR_SRC_SMALL;
            for (int64_t j = lane; j < nlit; j += 64) lit[j] = bb[pos + j];
            pos += nlit;
        } else if (Lh.type == 1) {  // RLE literals
            if (pos + 1 > bn) return PZ_ERR_SRC_SMALL;
            uint8_t v = bb[pos];
            for (int64_t j = lane; j < nlit; j += 64) lit[j] = v;
            pos += 1;
        } else {  // huffman literals (2 = new tree, 3 = treeless)
            if (pos + Lh.comp > bn) return PZ_ERR_SRC_SMALL;
            const uint8_t *hp = bb + pos;
            int64_t hn = Lh.comp;
            int64_t off = 0;
            if (Lh.type == 2) {
                if (lane == 0) {
                    int nw;
                    int used = pz_huf_read_weights(hp, hn, cx->weights, &nw,
                                                   cx->wksp64, cx->norm);
                    int tl = used < 0
                                 ? used
                                 : pz_huf_build(cx->weights, nw, L->hlut);
                    L->flag = used < 0 ? used
                                       : (tl < 0 ? tl
                                                 : (((int64_t)tl << 32) |
                                                    (uint32_t)used));
                }
                z_fence();
                int64_t f = L->flag;
                if (f < 0) return f;
                htl = (int)(f >> 32);
                off = (int64_t)(uint32_t)f;
            }
            if (htl < 0) return PZ_ERR_HUFFMAN;
            // stream layout: 1 stream, or 4 with a 6-byte jump table
            int ns = Lh.n_streams;
            const uint8_t *s0 = hp + off;
            int64_t szs[4], outs[4], oofs[4], sofs[4];
            if (ns == 1) {
                szs[0] = hn - off;
                outs[0] = nlit;
                oofs[0] = 0;
                sofs[0] = 0;
            } else {
                if (hn - off < 6) return PZ_ERR_SRC_SMALL;
                int64_t s1 = s0[0] | ((int64_t)s0[1] << 8);
                int64_t s2 = s0[2] | ((int64_t)s0[3] << 8);
                int64_t s3 = s0[4] | ((int64_t)s0[5] << 8);
                int64_t s4 = (hn - off - 6) - s1 - s2 - s3;
                if (s4 <= 0) return PZ_ERR_LITERALS;
                int64_t q = (nlit + 3) / 4;
                if (3 * q > nlit) return PZ_ERR_LITERALS;
                s0 += 6;
                szs[0] = s1;
                szs[1] = s2;
                szs[2] = s3;
                szs[3] = s4;
                outs[0] = outs[1] = outs[2] = q;
                outs[3] = nlit - 3 * q;
                sofs[0] = 0;
                sofs[1] = s1;
                sofs[2] = s1 + s2;
                sofs[3] = s1 + s2 + s3;
                oofs[0] = 0;
                oofs[1] = q;
                oofs[2] = 2 * q;
                oofs[3] = 3 * q;
            }
            if (lane < ns) {
                const uint8_t *sb = s0 + sofs[lane];
                int64_t want = outs[lane];
                int64_t bp0 = pz_back_init(sb, szs[lane]);
                int rcs = 0;
                if (bp0 < 0) {
                    rcs = PZ_ERR_HUFFMAN;
                } else {
                    ZBack rb;
                    rb.init(sb, bp0);
                    uint8_t *out = lit + oofs[lane];
                    for (int64_t i = 0; i < want; i++) {
                        uint32_t idx = rb.peek(htl);
                        PzHuf e = L->hlut[idx];
                        out[i] = e.sym;
                        rb.bp -= e.nbits;
                        if (rb.bp < 0) {
                            rcs = PZ_ERR_HUFFMAN;
                            break;
                        }
                    }
                    if (!rcs && rb.bp != 0) rcs = PZ_ERR_HUFFMAN;
                }
                L->stat[lane] = rcs;
            }
            z_fence();
            for (int i = 0; i < ns; i++)
                if (L->stat[i] < 0) return L->stat[i];
            pos += hn;
        }
        z_fence();  // literals visible to the whole wave
        // ---------------- sequences
        if (pos >= bn) return PZ_ERR_SEQ;
        const uint8_t *sq = bb + pos;
        int64_t sn = bn - pos;
        int b0 = sq[0];
        int nseq;
        int64_t so = 1;
        if (b0 < 128) {
            nseq = b0;
        } else if (b0 < 255) {
            if (sn < 2) return PZ_ERR_SRC_SMALL;
            nseq = ((b0 - 128) << 8) + sq[1];
            so = 2;
        } else {
            if (sn < 3) return PZ_ERR_SRC_SMALL;
            nseq = sq[1] + (sq[2] << 8) + 0x7F00;
            so = 3;
        }
        if (nseq == 0) {  // literals only
            if (dp + nlit > dcap) return PZ_ERR_DST_SMALL;
            for (int64_t j = lane; j < nlit; j += 64) dst[dp + j] = lit[j];
            z_fence();
            dp += nlit;
            continue;
        }
        if (so >= sn) return PZ_ERR_SRC_SMALL;
        int modes = sq[so++];
        if (modes & 3) return PZ_ERR_SEQ;
        if (lane == 0) {  // FSE table builds + stream init, serial
            int64_t f = 0;
            int used = pz_seq_table(sq + so, sn - so, (modes >> 6) & 3, 0, 9,
                                    35, cx->llT, &cx->ll_al, cx->have_ll,
                                    cx->norm);
            if (used >= 0) {
                cx->have_ll = 1;
                int64_t so2 = so + used;
                int u2 = pz_seq_table(sq + so2, sn - so2, (modes >> 4) & 3, 1,
                                      8, 31, cx->ofT, &cx->of_al,
                                      cx->have_of, cx->norm);
                if (u2 >= 0) {
                    cx->have_of = 1;
                    so2 += u2;
                    int u3 = pz_seq_table(sq + so2, sn - so2,
                                          (modes >> 2) & 3, 2, 9, 52,
                                          cx->mlT, &cx->ml_al, cx->have_ml,
                                          cx->norm);
                    if (u3 >= 0) {
                        cx->have_ml = 1;
                        so2 += u3;
                        f = so2 - so;
                    } else {
                        f = u3;
                    }
                } else {
                    f = u2;
                }
            } else {
                f = used;
            }
            if (f >= 0) {
                uint64_t k0 = st.rep[0], k1 = st.rep[1], k2 = st.rep[2];
                int rci = pz_seq_init(sq + so + f, sn - so - f, cx->ll_al,
                                      cx->of_al, cx->ml_al, &st);
                st.rep[0] = k0;  // repeat offsets persist across blocks
                st.rep[1] = k1;
                st.rep[2] = k2;
                if (rci < 0) f = rci;
            }
            L->flag = f;
        }
        z_fence();
        {
            int64_t f = L->flag;
            if (f < 0) return f;
            so += f;
        }
        const uint8_t *bs = sq + so;
        int64_t lpos = 0;
        int done = 0;
        ZBack rb;  // lane-0 register bit-window over the sequence stream
        if (lane == 0) {
            rb.init(bs, st.bp);
            rb.bp = st.bp;
        }
        while (done < nseq) {
            int cnt = nseq - done < 64 ? nseq - done : 64;
            if (lane == 0) {
                int64_t f = 0;
                for (int i = 0; i < cnt; i++) {
                    PzSeq q;
                    int rcq = zdev_seq_next(rb, cx->llT, cx->ofT, cx->mlT,
                                            st.s_ll, st.s_of, st.s_ml,
                                            st.rep,
                                            done + i == nseq - 1, &q);
                    if (rcq < 0) {
                        f = rcq;
                        break;
                    }
                    L->ll[i] = q.ll;
                    L->ml[i] = q.ml;
                    L->off[i] = q.off;
                }
                if (done + cnt >= nseq) st.bp = rb.bp;  // final check uses it
                L->flag = f;
            }
            z_fence();
            if (L->flag < 0) return L->flag;
            for (int i = 0; i < cnt; i++) {
                int64_t ll = L->ll[i], ml = L->ml[i];
                int64_t mo = (int64_t)L->off[i];
                if (lpos + ll > nlit) return PZ_ERR_SEQ;
                if (dp + ll + ml > dcap) return PZ_ERR_DST_SMALL;
                for (int64_t j = lane; j < ll; j += 64)
                    dst[dp + j] = lit[lpos + j];
                z_fence();
                dp += ll;
                lpos += ll;
                if (mo > dp) return PZ_ERR_OFFSET;
                if (mo >= ml) {  // non-overlapping: plain parallel copy
                    for (int64_t j = lane; j < ml; j += 64)
                        dst[dp + j] = dst[dp + j - mo];
                } else {  // overlapping: period-mo pattern replication
                    for (int64_t j = lane; j < ml; j += 64)
                        dst[dp + j] = dst[dp - mo + (j % mo)];
                }
                z_fence();
                dp += ml;
            }
            done += cnt;
        }
        if (lane == 0) L->flag = st.bp == 0 ? 0 : PZ_ERR_SEQ;
        z_fence();
        if (L->flag < 0) return L->flag;
        int64_t rem = nlit - lpos;
        if (rem < 0 || dp + rem > dcap) return PZ_ERR_DST_SMALL;
        for (int64_t j = lane; j < rem; j += 64) dst[dp + j] = lit[lpos + j];
        z_fence();
        dp += rem;
    }
    if (F.content_size >= 0 && dp != F.content_size) return PZ_ERR_CORRUPT;
    return dp;
}

__launch_bounds__(256) __global__
void k_zstd_pages(const uint8_t *src, const ZstdJob *jobs, int n,
                  uint8_t *dst, uint8_t *scratch, int64_t *status) {
    __shared__ ZWaveLds lds[4];
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int wiw = (threadIdx.x >> 6) & 3;
    const int waves = (int)((gridDim.x * blockDim.x) >> 6);
    for (int j = wave; j < n; j += waves) {
        uint8_t *lit = scratch + (size_t)j * PZ_SLOT;
        PzCtx *cx = (PzCtx *)(lit + PZ_BLOCK_MAX);
        int64_t r = zdev_page(src + jobs[j].src_off, jobs[j].src_len,
                              dst + jobs[j].dst_off, jobs[j].dst_len, lit,
                              cx, &lds[wiw]);
        if ((threadIdx.x & 63) == 0) status[j] = r;
    }
}

// emit-family x-block count: 4096 measured ~5% faster than 2048 at C2
// (smaller contiguous output slices balance the tail); PMH_EMIT_BLOCKS
// is the A/B override (read per launch: tests vary it within a process).
static int emit_grid() {
    const char *b = getenv("PMH_EMIT_BLOCKS");
    const int xblocks = b ? atoi(b) : 0;
    return xblocks > 0 && xblocks <= 65535 ? xblocks : 4096;
}

// ---------------------------------------------------------------- launchers
// Each unpacks its argument structs (kernels.h) into its kernel's argument
// list; tiles are PMH_TILE_ROWS rows everywhere but in pmh_launch_partition.

hipError_t pmh_launch_partition(const DevCol *keys, const int64_t *lens, int k,
                                int64_t tile_rows, int64_t n_bounds,
                                int64_t total_rows, int32_t *cuts,
                                hipStream_t stream) {
    // k <= 8 two-level: wave-coarse cuts every PMH_COARSE_G tiles (64-ary
    // domain search, ~5 probe rounds deep), then windowed refine for the
    // interior bounds (probes confined to the enclosing coarse windows).
    // k > 8: seed the endpoints and run the refine kernel with a single
    // full-width window per bound. Two-level measured SLOWER there, before
    // the lockstep search (16x20M: 3.9 ms two-level vs 3.2 one-level, the
    // wave kernel's 64-bit per-lane state spilled at KM >= 16) and after it
    // (no scratch at any KM: 3.04 ms two-level vs 1.35 one-level, same box —
    // DESIGN.md §7): the wave kernel's time is its probe traffic, 64 pivots
    // x k runs per step, and that doubles with k.
    // PMH_PART_G (profiling only, read per launch): a coarse stride >= 1
    // forces the two-level scheme with that stride for every k.
    int64_t coarse_g = PMH_COARSE_G;
    bool two_level = k <= 8;
    if (const char *e = getenv("PMH_PART_G")) {
        const int64_t g = atoll(e);
        if (g >= 1 && g <= 4096) {
            coarse_g = g;
            two_level = true;
        }
    }
    const int64_t G = two_level
                          ? (n_bounds > coarse_g + 1 ? coarse_g : 1)
                          : (n_bounds > 1 ? n_bounds - 1 : 1);
    const int64_t n_coarse = (n_bounds - 2) / G + 2;  // {0,G,..} u {last}
    int cblocks = (int)((n_coarse + 3) / 4);  // one wave per coarse bound
    int rblocks = (int)((n_bounds + 127) / 128);
    auto launch = [&](auto coarse, auto refiner) {
        if (two_level)
            hipLaunchKernelGGL(coarse, dim3(cblocks), dim3(256), 0, stream,
                               keys, lens, k, tile_rows, n_bounds, total_rows,
                               G, cuts);
        else
            hipLaunchKernelGGL(k_partition_seed, dim3(1), dim3(64), 0,
                               stream, lens, k, n_bounds, cuts);
        if (G > 1)
            hipLaunchKernelGGL(refiner, dim3(rblocks), dim3(128), 0, stream,
                               keys, lens, k, tile_rows, n_bounds,
                               total_rows, G, cuts);
    };
    if (k <= 4)
        launch(k_partition_wave<4>, k_partition_refine<4>);
    else if (k <= 8)
        launch(k_partition_wave<8>, k_partition_refine<8>);
    else if (k <= 16)
        launch(k_partition_wave<16>, k_partition_refine<16>);
    else
        launch(k_partition_wave<PMH_MAX_RUNS>,
               k_partition_refine<PMH_MAX_RUNS>);
    return hipGetLastError();
}

hipError_t pmh_launch_merge_tiles(const RunSet &runs, const TileSet &tiles,
                                  int flags, const ChangelogSet &cl,
                                  const ProbeSet &probe, hipStream_t stream) {
    // A block pipelines its staging across its tiles, but fewer, longer-lived
    // blocks did not pay: 512 / 1024 / 2048 / 4096 blocks measured 1.47 /
    // 1.47 / 1.45 / 1.44 ms at 8 x 10M rows and 7.33 / 7.34 / 7.29 / 7.05 ms
    // at 16 x 20M (profiles/merge_phases.md), so the grid stays at 4096.
    // PMH_MERGE_BLOCKS overrides it (read per launch: tests vary it within
    // a process).
    constexpr int64_t PMH_MERGE_BLOCKS_DEFAULT = 4096;
    int64_t max_blocks = PMH_MERGE_BLOCKS_DEFAULT;
    if (const char *e = getenv("PMH_MERGE_BLOCKS")) {
        const long long v = atoll(e);
        if (v >= 1 && v <= 65535) max_blocks = v;
    }
    const int k = runs.k;
    int blocks =
        tiles.n_tiles < max_blocks ? (int)tiles.n_tiles : (int)max_blocks;
    const bool pu = flags & PMH_FLAG_MEMBERS, fr = flags & PMH_FLAG_FIRST_ROW,
               lk = flags & PMH_FLAG_LOOKUP;
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(PMH_TILE_THREADS), 0,
                           stream, runs.keys, runs.seqs, runs.kinds,
                           runs.lens, k, tiles.cuts, tiles.n_tiles,
                           PMH_TILE_ROWS, flags, runs.tombs, tiles.winners,
                           tiles.counts, tiles.group_start, tiles.err,
                           runs.levels, cl.max_level, cl.entries, cl.counts,
                           probe.words, probe.off);
    };
    // KM = unrolled run bound of the staging setup (k_partition_wave's)
    // and TOMBS = deletion-vector bytes ride along (their registers stay out
    // of the plain kernels)
    auto launch_km = [&](auto km, auto tb) {
        constexpr int KM = decltype(km)::value;
        constexpr bool TB = decltype(tb)::value;
        if (lk)
            launch(k_merge_tiles<false, false, true, KM, TB>);  // dedup only
        else if (pu && (flags & PMH_FLAG_FOLD_CL))
            launch(k_merge_tiles<true, false, false, KM, TB, true>);
        else if (pu)
            launch(k_merge_tiles<true, false, false, KM, TB>);  // never FR
        else if (fr)
            launch(k_merge_tiles<false, true, false, KM, TB>);
        else
            launch(k_merge_tiles<false, false, false, KM, TB>);
    };
    auto launch_k = [&](auto tb) {
        if (k <= 4)
            launch_km(std::integral_constant<int, 4>{}, tb);
        else if (k <= 8)
            launch_km(std::integral_constant<int, 8>{}, tb);
        else if (k <= 16)
            launch_km(std::integral_constant<int, 16>{}, tb);
        else
            launch_km(std::integral_constant<int, PMH_MAX_RUNS>{}, tb);
    };
    if (runs.tombs)
        launch_k(std::true_type{});
    else
        launch_k(std::false_type{});
    return hipGetLastError();
}

static int g_last_pu_emit_kernel = PMH_PU_EMIT_NONE;
int pmh_last_pu_emit_kernel() { return g_last_pu_emit_kernel; }

hipError_t pmh_launch_emit_pu(const RunSet &runs, const ColumnSet &columns,
                              const TileSet &tiles, int flags,
                              const OutputSet &out, hipStream_t stream) {
    g_last_pu_emit_kernel = PMH_PU_EMIT_OVERLAY;
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(emit_grid()), dim3(256), 0, stream,
                           runs.cols, columns.dtype, columns.nullable,
                           columns.n_cols, runs.k, columns.seq_col(),
                           columns.kind_col(), flags, tiles.winners,
                           tiles.group_start, tiles.offsets, tiles.n_tiles,
                           PMH_TILE_ROWS, tiles.total, runs.masks, out.ptrs,
                           out.valid);
    };
    if (runs.masks)
        launch(k_emit_pu<true>);
    else
        launch(k_emit_pu<false>);
    return hipGetLastError();
}

hipError_t pmh_launch_composite(const DevCol *keys, int nk, uint64_t shifts,
                                uint64_t bits, int64_t rows, int64_t *ckey,
                                hipStream_t stream) {
    hipLaunchKernelGGL(k_composite, dim3(1024), dim3(256), 0, stream, keys,
                       nk, shifts, bits, rows, ckey);
    return hipGetLastError();
}

hipError_t pmh_launch_pack_valid(const DevCol *cols, int n_cols, int64_t rows,
                                 uint64_t *mask, hipStream_t stream) {
    hipLaunchKernelGGL(k_pack_valid, dim3(1024), dim3(256), 0, stream, cols,
                       n_cols, rows, mask);
    return hipGetLastError();
}

hipError_t pmh_launch_emit_pu_sg(const RunSet &runs, const ColumnSet &columns,
                                 const SeqGroupSet &groups,
                                 const TileSet &tiles, int flags,
                                 const OutputSet &out, hipStream_t stream) {
    if (groups.col_agg) {
        g_last_pu_emit_kernel = PMH_PU_EMIT_SGA;
        hipLaunchKernelGGL(k_emit_pu_sga, dim3(emit_grid()), dim3(256), 0,
                           stream, runs.cols, columns.dtype, columns.nullable,
                           columns.n_cols, runs.k, columns.seq_col(),
                           columns.kind_col(), flags, groups.col_group,
                           groups.fields, groups.nseq, groups.n_groups,
                           groups.grp_cols, groups.grp_off, groups.col_agg,
                           tiles.winners, tiles.group_start, tiles.offsets,
                           tiles.n_tiles, PMH_TILE_ROWS, tiles.total,
                           runs.masks, out.ptrs, out.valid, tiles.err);
        return hipGetLastError();
    }
    g_last_pu_emit_kernel = PMH_PU_EMIT_SG;
    hipLaunchKernelGGL(k_emit_pu_sg, dim3(emit_grid()), dim3(256), 0, stream,
                       runs.cols, columns.dtype, columns.nullable,
                       columns.n_cols, runs.k, columns.seq_col(),
                       columns.kind_col(), flags, groups.col_group,
                       groups.fields, groups.nseq, groups.n_groups,
                       tiles.winners, tiles.group_start, tiles.offsets,
                       tiles.n_tiles, PMH_TILE_ROWS, tiles.total, runs.masks,
                       out.ptrs, out.valid);
    return hipGetLastError();
}

hipError_t pmh_launch_emit_agg(const RunSet &runs, const ColumnSet &columns,
                               const TileSet &tiles, int flags,
                               const OutputSet &out, hipStream_t stream) {
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(emit_grid()), dim3(256), 0, stream,
                           runs.cols, columns.dtype, columns.nullable,
                           columns.agg, columns.n_cols, runs.k,
                           columns.seq_col(), columns.kind_col(), flags,
                           tiles.winners, tiles.group_start, tiles.offsets,
                           tiles.n_tiles, PMH_TILE_ROWS, tiles.total,
                           runs.masks, out.ptrs, out.valid);
    };
    if (runs.masks)
        launch(k_emit_agg<true>);
    else
        launch(k_emit_agg<false>);
    return hipGetLastError();
}

hipError_t pmh_launch_level_scatter(const RleChunk *chunks, int64_t n_chunks,
                                    hipStream_t stream) {
    int blocks = pmh_grid(n_chunks);
    hipLaunchKernelGGL(k_level_scatter, dim3(blocks), dim3(PMH_TILE_THREADS),
                       0, stream, chunks, n_chunks);
    return hipGetLastError();
}

hipError_t pmh_launch_merge_emit(const RunSet &runs, const ColumnSet &columns,
                                 const TileSet &tiles, int flags,
                                 const OutputSet &out, hipStream_t stream) {
    // persistent workgroups: 2 resident per CU (LDS-bound) x 256 CUs; the
    // ticket (zeroed before this launch) hands out the tiles in order, so
    // any residency is safe
    const int64_t n_tiles = tiles.n_tiles;
    int blocks = n_tiles < 512 ? (int)n_tiles : 512;
    const bool fr = flags & PMH_FLAG_FIRST_ROW;
    auto launch = [&](auto kern) {
        // tile_base / tile_limit: the whole tile space in one launch
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(PMH_TILE_THREADS), 0,
                           stream, runs.keys, runs.seqs, runs.kinds,
                           runs.lens, runs.k, tiles.cuts, (int64_t)0, n_tiles,
                           n_tiles, PMH_TILE_ROWS, flags, runs.tombs,
                           runs.cols, columns.dtype, columns.nullable,
                           columns.n_cols, columns.key_col(),
                           columns.seq_col(), columns.kind_col(),
                           columns.useq, columns.n_useq, tiles.status,
                           tiles.ticket, tiles.total, tiles.dense_winners,
                           out.ptrs, out.valid, tiles.err);
    };
    if (fr)
        launch(k_merge_emit<true>);
    else
        launch(k_merge_emit<false>);
    return hipGetLastError();
}

hipError_t pmh_launch_emit_dense(const RunSet &runs, const ColumnSet &columns,
                                 const TileSet &tiles, const OutputSet &out,
                                 hipStream_t stream) {
    // t0 / t1: the whole tile space
    hipLaunchKernelGGL(k_emit_dense, dim3(emit_grid()), dim3(256), 0, stream,
                       runs.cols, columns.dtype, columns.nullable,
                       columns.n_cols, columns.key_col(), columns.seq_col(),
                       columns.kind_col(), tiles.dense_winners, (int64_t)0,
                       tiles.n_tiles, tiles.status, out.ptrs, out.valid);
    return hipGetLastError();
}

hipError_t pmh_launch_scan_tiles(const int32_t *tile_counts, int64_t n_tiles,
                                 int64_t *tile_offsets, int64_t *total_out,
                                 hipStream_t stream) {
    hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(PMH_TILE_THREADS), 0,
                       stream, tile_counts, n_tiles, tile_offsets, total_out);
    return hipGetLastError();
}

// which kernel the last pmh_launch_emit chose (PMH_EMIT_*); tests tell a
// streamed read from a fallback by it
static int g_last_emit_kernel = PMH_EMIT_NONE;
int pmh_last_emit_kernel() { return g_last_emit_kernel; }

// Winner emit. Three kernels, most specific first:
//  - k_emit_stream (tile slices streamed through LDS, no gather) when every
//    run slot a winner can name is a merge run (n_desc == k: a lookup winner
//    may name a slot outside the tile's slices), n_cols <= 256, no emitted
//    column is nullable (validity is not streamed), the tables fit, and
//    PMH_EMIT_STREAM is not 0;
//  - k_emit_contig (descriptors in LDS) for the other plans whose tables fit;
//  - k_emit (descriptors read from global memory) for the rest, such as 32
//    runs x 32 columns, and under PMH_EMIT_LEGACY=1.
hipError_t pmh_launch_emit(const RunSet &runs, const ColumnSet &columns,
                           const TileSet &tiles, const OutputSet &out,
                           hipStream_t stream) {
    const int k = runs.k, n_desc = runs.n_slots, n_cols = columns.n_cols;
    const int64_t n_tiles = tiles.n_tiles;
    // Every knob is read per launch (tests vary them within a process).
    // R = rows per thread iteration, G = 4-byte columns per gather group
    // (8-byte columns go G / 2 at a time). PMH_EMIT_R sweeps 2/4 (legacy
    // kernel: 4/6/8) and PMH_EMIT_G 2/4/8 (16 with R = 4). The defaults,
    // R = 4 and G = 8, are the measured best although 126 VGPRs halve the
    // occupancy: 32 gathers in flight per wave beat 8 waves per SIMD
    // (DESIGN.md §7).
    auto env_int = [](const char *name, int dflt) {
        const char *e = getenv(name);
        return e ? atoi(e) : dflt;
    };
    const int r_rows = env_int("PMH_EMIT_R", 4);
    const int g_cols = env_int("PMH_EMIT_G", 8);
    // profiling-only: emit just the first PMH_EMIT_COLS columns (the rest of
    // the output is then garbage; only emit_ms means anything under it)
    int n_emit = env_int("PMH_EMIT_COLS", n_cols);
    if (n_emit < 0 || n_emit > n_cols) n_emit = n_cols;
    const int grid = emit_grid();
    const int64_t lds = emit_contig_lds(n_desc, n_cols);
    // k_emit_contig serves plans whose tables fit; position -> column bytes
    // cap n_cols at 256
    const bool contig = n_desc >= 1 && n_cols <= 256 && lds <= EMIT_LDS_MAX &&
                        env_int("PMH_EMIT_LEGACY", 0) == 0;
    const int64_t tables = emit_stream_tables(k, n_cols);
    const bool streamed = contig && n_desc == k && !columns.any_nullable &&
                          tables <= EMIT_LDS_MAX && tiles.cuts && runs.lens &&
                          env_int("PMH_EMIT_STREAM", 1) != 0;
    if (streamed) {
        // PMH_EMIT_STREAM_LDS: data bytes per block. It sets the columns per
        // group: 4 four-byte or 2 eight-byte ones at the default (two blocks
        // per CU), half that below two 8-byte columns' worth. The sweep is in
        // profiles/emit_stream_phases.md; one 8-byte column is the floor.
        int64_t budget = env_int("PMH_EMIT_STREAM_LDS", (int)EMS_LDS_DEFAULT);
        const int64_t col8 = (int64_t)PMH_TILE_MAX * 8;
        if (budget < col8) budget = col8;
        if (budget > EMS_LDS_DEFAULT) budget = EMS_LDS_DEFAULT;
        // tables + data stay within the 64 KB a launch gets without asking
        // (tables <= EMIT_LDS_MAX, so one 8-byte column always fits)
        if (budget > 64 * 1024 - tables) budget = 64 * 1024 - tables;
        const int gu = budget >= 2 * col8 ? 4 : 2;
        int64_t max_blocks = 4096;  // k_merge_tiles' grid, see there
        if (const char *e = getenv("PMH_EMIT_STREAM_BLOCKS")) {
            const long long v = atoll(e);
            if (v >= 1 && v <= 65535) max_blocks = v;
        }
        const int blocks = n_tiles < max_blocks ? (int)n_tiles : (int)max_blocks;
        const size_t bytes = (size_t)(tables + budget);
        auto launch = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(blocks), dim3(EMS_THREADS), bytes,
                               stream, runs.cols, columns.dtype, n_cols,
                               n_emit, k, tiles.cuts, runs.lens,
                               tiles.winners, tiles.counts, tiles.offsets,
                               n_tiles, PMH_TILE_ROWS, out.ptrs, (int)budget);
        };
        auto launch_g = [&](auto km) {
            constexpr int KM = decltype(km)::value;
            if (gu == 2) launch(k_emit_stream<KM, 2>);
            else launch(k_emit_stream<KM, 4>);
        };
        if (k <= 8) launch_g(std::integral_constant<int, 8>{});
        else if (k <= 16) launch_g(std::integral_constant<int, 16>{});
        else launch_g(std::integral_constant<int, PMH_MAX_RUNS>{});
        g_last_emit_kernel = PMH_EMIT_STREAM;
        return hipGetLastError();
    }
    g_last_emit_kernel = contig ? PMH_EMIT_CONTIG : PMH_EMIT_GATHER;
    if (contig) {
        auto launch = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(grid), dim3(EMIT_THREADS), (size_t)lds,
                               stream, runs.cols, columns.dtype,
                               columns.nullable, n_cols, n_emit, n_desc,
                               tiles.winners, tiles.offsets, n_tiles,
                               PMH_TILE_ROWS, tiles.total, out.ptrs,
                               out.valid);
        };
        if (r_rows == 2) {
            if (g_cols == 2) launch(k_emit_contig<2, 2, 1>);
            else if (g_cols == 4) launch(k_emit_contig<2, 4, 2>);
            else launch(k_emit_contig<2, 8, 4>);
        } else {
            if (g_cols == 2) launch(k_emit_contig<4, 2, 1>);
            else if (g_cols == 4) launch(k_emit_contig<4, 4, 2>);
            else if (g_cols == 16) launch(k_emit_contig<4, 16, 8>);
            else launch(k_emit_contig<4, 8, 4>);
        }
        return hipGetLastError();
    }
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, stream, runs.cols,
                           columns.dtype, columns.nullable, n_cols, n_emit, k,
                           tiles.winners, tiles.counts, tiles.offsets,
                           n_tiles, PMH_TILE_ROWS, tiles.total, out.ptrs,
                           out.valid);
    };
    if (r_rows == 6)
        launch(k_emit<6>);
    else if (r_rows == 8)
        launch(k_emit<8>);
    else
        launch(k_emit<4>);
    return hipGetLastError();
}



hipError_t pmh_launch_filter(const DevCol *cols, int n_cols,
                             const FilterTerm *terms, int n_terms,
                             int64_t rows, uint8_t *tomb,
                             hipStream_t stream) {
    int64_t want = (rows + 255) / 256;
    int blocks = pmh_grid(want);
    hipLaunchKernelGGL(k_filter, dim3(blocks), dim3(256), 0, stream, cols,
                       n_cols, terms, n_terms, rows, tomb);
    return hipGetLastError();
}

hipError_t pmh_launch_lookup_probe(const RunSet &runs, const ProbeSet &probe,
                                   hipStream_t stream) {
    if (runs.k <= 0 || probe.max_rows <= 0) return hipSuccess;
    int64_t chunks = (probe.max_rows + PLK_CHUNK - 1) / PLK_CHUNK;
    hipLaunchKernelGGL(k_lookup_probe, dim3(pmh_grid(chunks, 2048), runs.k),
                       dim3(256), 0, stream, runs.keys, runs.lens, probe.off,
                       runs.k, probe.n_levels, probe.words);
    return hipGetLastError();
}

hipError_t pmh_launch_cl_finalize(const RunSet &runs, const ColumnSet &columns,
                                  const TileSet &tiles, const ChangelogSet &cl,
                                  hipStream_t stream) {
    hipLaunchKernelGGL(k_cl_finalize, dim3(pmh_grid(tiles.n_tiles)),
                       dim3(256), 0, stream, runs.cols, columns.dtype,
                       columns.n_cols, columns.first_val(), runs.k,
                       cl.entries, cl.rows, cl.counts, tiles.n_tiles,
                       PMH_TILE_ROWS);
    return hipGetLastError();
}

hipError_t pmh_launch_cl_emit(const RunSet &runs, const ColumnSet &columns,
                              const TileSet &tiles, const ChangelogSet &cl,
                              const OutputSet &out2, hipStream_t stream) {
    hipLaunchKernelGGL(k_cl_emit, dim3(pmh_grid(tiles.n_tiles)), dim3(256), 0,
                       stream, runs.cols, columns.dtype, columns.nullable,
                       columns.n_cols, columns.kind_col(), cl.rows, cl.counts,
                       cl.offsets, tiles.n_tiles, PMH_TILE_ROWS, out2.ptrs,
                       out2.valid);
    return hipGetLastError();
}

hipError_t pmh_launch_cl_finalize_out(const RunSet &runs,
                                      const ColumnSet &columns,
                                      const TileSet &tiles,
                                      const ChangelogSet &cl,
                                      const OutputSet &out,
                                      hipStream_t stream) {
    const int64_t lds = pmh_fold_cl_lds(runs.k, columns.n_cols);
    // a thread keeps its pairs' verdicts in one 32-bit register
    static_assert(PMH_TILE_ROWS + PMH_MAX_RUNS <= 16 * FOLD_CL_THREADS,
                  "k_cl_finalize_out: 16 pairs per thread");
    if (lds > PMH_FOLD_CL_LDS_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cl_finalize_out, dim3(pmh_grid(tiles.n_tiles)),
                       dim3(FOLD_CL_THREADS), (size_t)lds, stream, runs.cols,
                       columns.dtype, columns.nullable, columns.n_cols,
                       columns.first_val(), runs.k, cl.entries, cl.rows,
                       cl.counts, tiles.offsets, tiles.n_tiles, PMH_TILE_ROWS,
                       out.ptrs, out.valid);
    return hipGetLastError();
}

hipError_t pmh_launch_cl_emit_out(const RunSet &runs, const ColumnSet &columns,
                                  const TileSet &tiles, const ChangelogSet &cl,
                                  const OutputSet &out, const OutputSet &out2,
                                  hipStream_t stream) {
    const int64_t lds = pmh_fold_cl_lds(runs.k, columns.n_cols);
    if (lds > PMH_FOLD_CL_LDS_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cl_emit_out, dim3(pmh_grid(tiles.n_tiles)),
                       dim3(FOLD_CL_THREADS), (size_t)lds, stream, runs.cols,
                       columns.dtype, columns.nullable, columns.n_cols, runs.k,
                       columns.kind_col(), cl.rows, cl.counts, cl.offsets,
                       tiles.offsets, tiles.n_tiles, PMH_TILE_ROWS, out.ptrs,
                       out.valid, out2.ptrs, out2.valid);
    return hipGetLastError();
}

hipError_t pmh_launch_zstd_compress(const uint8_t *src,
                                    const ZstdJob *jobs, int n,
                                    uint8_t *dst, uint8_t *scratch,
                                    int64_t *status, hipStream_t stream) {
    int want = (n + 3) / 4;
    int blocks = pmh_grid(want);
    hipLaunchKernelGGL(k_zstd_compress, dim3(blocks), dim3(256), 0, stream,
                       src, jobs, n, dst, scratch, status);
    return hipGetLastError();
}

hipError_t pmh_launch_zstd_pages(const uint8_t *src, const ZstdJob *jobs,
                                 int n, uint8_t *dst, uint8_t *scratch,
                                 int64_t *status, hipStream_t stream) {
    int want = (n + 3) / 4;  // 4 waves (pages) per 256-thread block
    int blocks = pmh_grid(want);
    hipLaunchKernelGGL(k_zstd_pages, dim3(blocks), dim3(256), 0, stream, src,
                       jobs, n, dst, scratch, status);
    return hipGetLastError();
}

hipError_t pmh_launch_rlev2(const Rlev2Chunk *chunks, int64_t n_chunks,
                            hipStream_t stream) {
    int waves_per_block = 4;  // 256 threads
    int64_t want = (n_chunks + waves_per_block - 1) / waves_per_block;
    int blocks = pmh_grid(want);
    hipLaunchKernelGGL(k_rlev2, dim3(blocks), dim3(256), 0, stream, chunks,
                       n_chunks);
    return hipGetLastError();
}


hipError_t pmh_launch_orc_varint(const VarintUnit *units, int64_t n_units,
                                 hipStream_t stream) {
    int waves_per_block = 4;  // 256 threads
    int64_t want = (n_units + waves_per_block - 1) / waves_per_block;
    int blocks = pmh_grid(want);
    hipLaunchKernelGGL(k_orc_varint, dim3(blocks), dim3(256), 0, stream,
                       units, n_units);
    return hipGetLastError();
}

hipError_t pmh_launch_bits_expand(const BitsUnit *units, int64_t n_units,
                                  hipStream_t stream) {
    int waves_per_block = 4;  // 256 threads
    int64_t want = (n_units + waves_per_block - 1) / waves_per_block;
    int blocks = pmh_grid(want);
    hipLaunchKernelGGL(k_bits_expand, dim3(blocks), dim3(256), 0, stream,
                       units, n_units);
    return hipGetLastError();
}

hipError_t pmh_launch_orc_timestamp(const TsUnit *units, int64_t n_units,
                                    hipStream_t stream) {
    int blocks = pmh_grid(n_units);
    hipLaunchKernelGGL(k_orc_timestamp, dim3(blocks), dim3(256), 0, stream,
                       units, n_units);
    return hipGetLastError();
}

hipError_t pmh_launch_delta_sum(const DeltaChunk *chunks, int64_t n_chunks,
                                int64_t *sums, hipStream_t stream) {
    int64_t want = (n_chunks + 3) / 4;
    int blocks = pmh_grid(want);
    hipLaunchKernelGGL(k_delta_sum, dim3(blocks), dim3(256), 0, stream,
                       chunks, n_chunks, sums);
    return hipGetLastError();
}

hipError_t pmh_launch_delta_scan(const DeltaStream *streams,
                                 int64_t n_streams, const int64_t *sums,
                                 int64_t *bases, hipStream_t stream) {
    int blocks = pmh_grid(n_streams, 2048);
    hipLaunchKernelGGL(k_delta_scan, dim3(blocks), dim3(256), 0, stream,
                       streams, n_streams, sums, bases);
    return hipGetLastError();
}

hipError_t pmh_launch_delta_emit(const DeltaChunk *chunks, int64_t n_chunks,
                                 const int64_t *bases, hipStream_t stream) {
    int64_t want = (n_chunks + 3) / 4;
    int blocks = pmh_grid(want);
    hipLaunchKernelGGL(k_delta_emit, dim3(blocks), dim3(256), 0, stream,
                       chunks, n_chunks, bases);
    return hipGetLastError();
}

hipError_t pmh_launch_rle_decode(const RleChunk *chunks, int64_t n_chunks,
                                 int32_t *out, hipStream_t stream) {
    int blocks = pmh_grid(n_chunks);
    hipLaunchKernelGGL(k_rle_decode, dim3(blocks), dim3(256), 0, stream,
                       chunks, n_chunks, out);
    return hipGetLastError();
}

hipError_t pmh_launch_dict_gather(const int32_t *ids, const void *dict,
                                  int64_t n, void *out, int esize,
                                  hipStream_t stream) {
    int threads = 256;
    int64_t want = (n + threads - 1) / threads;
    int blocks = pmh_grid(want);
    if (esize == 4)
        hipLaunchKernelGGL(k_dict_gather_t<int32_t>, dim3(blocks),
                           dim3(threads), 0, stream, ids,
                           (const int32_t *)dict, n, (int32_t *)out);
    else if (esize == 8)
        hipLaunchKernelGGL(k_dict_gather_t<int64_t>, dim3(blocks),
                           dim3(threads), 0, stream, ids,
                           (const int64_t *)dict, n, (int64_t *)out);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace pmh
