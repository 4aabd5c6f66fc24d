// Decision table of the full-compaction changelog producer
// (FullChangelogMergeFunctionWrapper.getResult, FullChangelogMergeFunction-
// Wrapper.java:96-126) — independent of the merge function: it needs a key
// group's live-record count, its top-level (run level == max level) member
// count and whether mergeFunction.getResult() is an add.
//
// Shared scalar core, like lookup_core.h: the folded (partial-update /
// aggregation) walk of k_merge_tiles (kernels.hip) and the host entry
// pmh_debug_changelog_decide (plan.cpp) run exactly this code, so the CPU
// tests pin what the kernel executes. Also the entry-word layout the folded
// changelog kernels (k_cl_finalize_out, k_cl_emit_out) decode.
#ifndef PMH_CHANGELOG_CORE_H
#define PMH_CHANGELOG_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define CLC_HD __host__ __device__ inline
#else
#define CLC_HD inline
#endif

// changelog RowKinds (types/RowKind.java byte values)
constexpr int CLC_INSERT = 0;
constexpr int CLC_UPDATE_BEFORE = 1;
constexpr int CLC_UPDATE_AFTER = 2;
constexpr int CLC_DELETE = 3;

// Provisional entry word (two per key group, k_merge_tiles -> finalize):
//   bits  0..31  before-type / source rows: packed (run:5 | row:27);
//                "from output" rows: the group's tile-local index g among the
//                tile's KEPT groups (main-output row tile_offsets[tile] + g)
//   bits 32..34  changelog RowKind
//   bit  35      entry holds a row
//   bit  36      row-deduplicate pending (set on both halves of a pair)
//   bit  37      from output: the row is the engine's folded result, read
//                from the plan's main output columns (folded engines only)
constexpr int CLC_KIND_SHIFT = 32;
constexpr uint64_t CLC_VALID = 1ull << 35;
constexpr uint64_t CLC_PENDING = 1ull << 36;
constexpr uint64_t CLC_FROM_OUT = 1ull << 37;

struct ClcDecision {
    int n;                 // changelog rows of the group: 0, 1 or 2
    int kind0, kind1;      // their RowKinds (kind1 only when n == 2)
    bool after_is_merged;  // row n - 1 carries the merged result (INSERT /
                           // UPDATE_AFTER); false: every row carries top
    bool pending;          // the pair still needs the value-equality check
};

// nlive: live records of the group (deletion-vector tombstones excluded),
// >= 1. n_top: members from a max-level run (0 or 1; 2+ is the caller's
// checkState error and decides as 1). merged_is_add: the kind of the
// wrapper's result — the lone record itself when nlive == 1 (the wrapper
// bypasses the merge function), mergeFunction.getResult() otherwise.
// pending: changelog-producer.row-deduplicate is on.
CLC_HD ClcDecision clc_decide(int nlive, int n_top, bool merged_is_add,
                              bool pending) {
    ClcDecision d{0, CLC_INSERT, CLC_INSERT, false, false};
    if (n_top == 0) {
        // no top-level record: INSERT(merged) if it is an add — also the
        // singleton "initial is add" rule (:117-119)
        if (merged_is_add) {
            d.n = 1;
            d.kind0 = CLC_INSERT;
            d.after_is_merged = true;
        }
    } else if (nlive > 1) {
        if (!merged_is_add) {  // DELETE(topLevelKv) (:106-107)
            d.n = 1;
            d.kind0 = CLC_DELETE;
        } else {  // UPDATE_BEFORE(top) + UPDATE_AFTER(merged) (:108-113)
            d.n = 2;
            d.kind0 = CLC_UPDATE_BEFORE;
            d.kind1 = CLC_UPDATE_AFTER;
            d.after_is_merged = true;
            d.pending = pending;
        }
    }  // a singleton that IS the top-level record: no change (:120-123)
    return d;
}

#endif  // PMH_CHANGELOG_CORE_H
