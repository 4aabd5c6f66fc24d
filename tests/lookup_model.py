"""Sequential model of the lookup changelog producer over the deduplicate
engine: LookupChangelogMergeFunctionWrapper.getResult / setChangelog
(mergetree/compact/LookupChangelogMergeFunctionWrapper.java:104-163) on top
of LookupMergeFunction (LookupMergeFunction.java:66-135), with the lookup
of LookupUtils.lookup (mergetree/LookupUtils.java:35-57) and the insertion
rule of KeyValueBuffer.insertInto (KeyValueBuffer.java:239-263).

Deliberately plain: one key group at a time, Python lists, no vectorised
shortcuts — it is the yardstick the GPU path is compared with, and it is
itself pinned to the reference's literal test vectors
(tests/test_lookup_changelog_cpu.py).

A run / lookup level is a dict {key, seq, kind, values: [col arrays]} with
ascending unique keys (paimon_amd.datagen layout). Records are addressed as
(source, row): source < len(runs) is a compaction run, source >= len(runs)
is lookup level `source - len(runs)` (lookup levels are given lowest level
first). Masks are per source, per value column: True = NULL.
"""

KIND_INSERT, KIND_UPDATE_BEFORE, KIND_UPDATE_AFTER, KIND_DELETE = 0, 1, 2, 3


def _is_add(kind):
    return kind in (KIND_INSERT, KIND_UPDATE_AFTER)


class _Rec:
    __slots__ = ("src", "row", "seq", "kind", "level")

    def __init__(self, src, row, seq, kind, level):
        self.src, self.row, self.seq = src, row, seq
        self.kind, self.level = kind, level

    @property
    def is_add(self):
        return _is_add(self.kind)


def lookup_changelog_model(runs, levels, lookup_levels=(), row_dedup=False,
                           drop_delete=True, masks=None, lookup_masks=None):
    """Returns (changelog, result):
    changelog = [(source, row, changelog_kind), ...] in key order
    (UPDATE_BEFORE directly before its UPDATE_AFTER); result = [(source,
    row), ...] the main stream (one record per key group, DELETE results
    dropped under drop_delete).

    levels: the level of each compaction run. masks / lookup_masks: NULL
    masks of the runs / lookup levels (None = no nulls)."""
    n_runs = len(runs)
    sources = list(runs) + list(lookup_levels)
    all_masks = None
    if masks is not None or lookup_masks is not None:
        all_masks = (list(masks) if masks is not None else [None] * n_runs) \
            + (list(lookup_masks) if lookup_masks is not None
               else [None] * len(lookup_levels))

    # members per key, in input order (run by run)
    groups = {}
    for s, run in enumerate(runs):
        keys = run["key"].tolist()
        seqs = run["seq"].tolist()
        kinds = run["kind"].tolist()
        for i in range(len(keys)):
            groups.setdefault(keys[i], []).append(
                _Rec(s, i, seqs[i], kinds[i], levels[s]))
    lookup_index = [{k: i for i, k in enumerate(lv["key"].tolist())}
                    for lv in lookup_levels]

    def values_equal(a, b):
        # the RecordEqualiser over the read schema: every value column,
        # null == null, null != value
        va, vb = sources[a.src]["values"], sources[b.src]["values"]
        for c in range(len(va)):
            ma = all_masks[a.src] if all_masks else None
            mb = all_masks[b.src] if all_masks else None
            na = bool(ma[c][a.row]) if ma is not None else False
            nb = bool(mb[c][b.row]) if mb is not None else False
            if na != nb:
                return False
            if not na and va[c][a.row] != vb[c][b.row]:
                return False
        return True

    changelog, result = [], []
    for key in sorted(groups):
        # merge order: ascending (sequenceNumber, isAdd), stable
        members = sorted(groups[key], key=lambda m: (m.seq, m.is_add))
        # rule 1
        contain_level0 = any(m.level == 0 for m in members)
        # rule 2: lowest level among level > 0; a tie keeps the earlier
        high = None
        for m in members:
            if m.level > 0 and (high is None or m.level < high.level):
                high = m
        # rule 4 (first half): the merge sees level <= 0 members plus high
        candidates = [m for m in members if m.level <= 0 or m is high]
        # rule 3: lookup when no member supplies high
        if high is None:
            for l, index in enumerate(lookup_index):
                row = index.get(key)
                if row is not None:
                    lv = lookup_levels[l]
                    high = _Rec(n_runs + l, row, int(lv["seq"][row]),
                                int(lv["kind"][row]), None)
                    break
            if high is not None:
                pos = len(candidates)
                for i, m in enumerate(candidates):
                    if m.seq > high.seq:
                        pos = i
                        break
                candidates.insert(pos, high)
        # rule 4: deduplicate keeps the last candidate
        after = candidates[-1]
        # rule 5
        if contain_level0:
            before = high
            if before is None or not before.is_add:
                if after.is_add:
                    changelog.append((after.src, after.row, KIND_INSERT))
            elif not after.is_add:
                changelog.append((before.src, before.row, KIND_DELETE))
            elif not (row_dedup and values_equal(before, after)):
                changelog.append((before.src, before.row,
                                  KIND_UPDATE_BEFORE))
                changelog.append((after.src, after.row, KIND_UPDATE_AFTER))
        # rule 6
        if after.is_add or not drop_delete:
            result.append((after.src, after.row))
    return changelog, result

