// Tile slot mapping and column grouping of k_emit_stream.
//
// Shared core, like partition_core.h: the kernel (kernels.hip) and
// emit_stream_hostcheck.cpp run exactly this code, so the host check pins
// what the kernel executes.
//
// A tile t of the merge covers, of every run r, the contiguous slice
// [cuts[t][r], cuts[t+1][r]) plus one extension element where the run goes
// on (a group headed in the tile may have one member per run past the tile's
// end). k_merge_tiles stages those slices back to back as one flat segment:
// slot = segoff[run] + (row - cuts[t][run]). Every winner of tile t names a
// (run, row) inside those slices, so k_emit_stream loads the slices of a
// value column as coalesced streams into LDS at the same slots and permutes
// from there. The three functions below are that mapping, in the order
// tile_prefetch computes it (extension element included).
//
// The group plan cuts the emitted columns (in list order: all 1-byte outputs,
// then 2-, 4- and 8-byte ones) into the groups that share one LDS fill.
#ifndef PMH_EMIT_STREAM_CORE_H
#define PMH_EMIT_STREAM_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define ESC_HD __host__ __device__ __forceinline__
#else
#define ESC_HD inline
#endif
#if defined(__clang__)  // the per-run loops must unroll: arrays in registers
#define ESC_UNROLL _Pragma("unroll")
#else
#define ESC_UNROLL
#endif

// One tile's segments. Entries r >= k of a KM-wide instantiation are empty.
template <int KM>
struct EscTile {
    int32_t a[KM];       // first row of run r's slice (cuts[t][r])
    int32_t len[KM];     // slice length, extension element included
    int32_t segoff[KM];  // slot of the slice's first element
    int32_t mtotal;      // extended element count (slots in use)
    int32_t mreal;       // elements without the extensions
};

// c0 = cuts[t], c1 = cuts[t + 1] (k entries each), lens = the k run lengths.
// Loads stay unconditional (slots r >= k re-read run 0), as in tile_prefetch.
template <int KM>
ESC_HD void esc_tile_setup(const int32_t *c0, const int32_t *c1,
                           const int64_t *lens, int k, EscTile<KM> &t) {
    int32_t so = 0, mr = 0;
    ESC_UNROLL
    for (int r = 0; r < KM; r++) {
        const int rr = r < k ? r : 0;
        const int32_t ar = c0[rr], br = c1[rr];
        const int32_t ln = (int32_t)lens[rr];
        t.a[r] = ar;
        t.len[r] = r < k ? (br - ar) + (br < ln ? 1 : 0) : 0;
        t.segoff[r] = so;
        so += t.len[r];
        mr += r < k ? br - ar : 0;
    }
    t.mtotal = so;
    t.mreal = mr;
}

// slot -> (run, row), for 0 <= e < t.mtotal: the last run whose segment
// offset is <= e (non-empty, because e < mtotal).
template <int KM>
ESC_HD void esc_slot_source(const EscTile<KM> &t, int k, int32_t e, int *run,
                            uint32_t *row) {
    int rn = 0;
    int32_t rowd = 0;
    ESC_UNROLL
    for (int r = 0; r < KM; r++) {
        const bool in = r < k && e >= t.segoff[r];
        rn = in ? r : rn;
        rowd = in ? t.a[r] - t.segoff[r] : rowd;
    }
    *run = rn;
    *row = (uint32_t)(e + rowd);
}

// (run, row) of a packed winner -> slot. Inside [0, mtotal) for every row
// with cuts[t][run] <= row <= cuts[t+1][run] and row < len[run]; a run >= KM
// (a word that is no winner of this tile) yields row itself.
template <int KM>
ESC_HD int32_t esc_winner_slot(const EscTile<KM> &t, uint32_t run,
                               uint32_t row) {
    int32_t off = 0;
    ESC_UNROLL
    for (int r = 0; r < KM; r++)
        off = run == (uint32_t)r ? t.segoff[r] - t.a[r] : off;
    return (int32_t)row + off;
}

// Stored (loaded) width of a column of output-width class cls (1 / 2 / 4 / 8
// bytes): narrow integers are staged as INT32.
ESC_HD int esc_stored_width(int cls) { return cls == 8 ? 8 : 4; }

// LDS bytes one column takes in a group: a full tile of its stored width,
// plus a byte per slot when its validity rides along.
ESC_HD int64_t esc_col_bytes(int cls, int has_valid, int tile_max) {
    return (int64_t)tile_max * (esc_stored_width(cls) + (has_valid ? 1 : 0));
}

// Cut the n columns (cls[i] = output-width class by list position, valid[i]
// != 0 where the validity bytes ride along; valid may be null) into groups of
// consecutive columns. A group holds one class only, at most max4 columns of
// stored width 4 or max8 of stored width 8, and at most `budget` LDS bytes.
// Writes the group boundaries bound[0 .. g] (bound[0] = 0, bound[g] = n) and
// returns g; -1 if a single column does not fit the budget. bound needs
// n + 1 entries.
ESC_HD int esc_plan_groups(const uint8_t *cls, const uint8_t *valid, int n,
                           int tile_max, int64_t budget, int max4, int max8,
                           uint16_t *bound) {
    int g = 0;
    bound[0] = 0;
    int i = 0;
    while (i < n) {
        const int c = cls[i];
        const int cap = esc_stored_width(c) == 8 ? max8 : max4;
        int64_t used = 0;
        int j = i;
        while (j < n && cls[j] == c && j - i < cap) {
            const int64_t b =
                esc_col_bytes(c, valid ? valid[j] : 0, tile_max);
            if (used + b > budget) break;
            used += b;
            j++;
        }
        if (j == i) return -1;  // one column over the budget (or cap < 1)
        bound[++g] = (uint16_t)j;
        i = j;
    }
    return g;
}

#endif  // PMH_EMIT_STREAM_CORE_H
