"""Expected full-compaction changelog for the folding merge engines
(partial-update, aggregation): a literal sequential port of
FullChangelogMergeFunctionWrapper.add / getResult (FullChangelogMerge-
FunctionWrapper.java:74-130) around a merge function whose result is taken
from one of the oracle's engine models.

The wrapper needs, per key group, mergeFunction.getResult() as a whole row
(key, sequence number, kind, values, validity). `model(runs)` must return
that row for EVERY distinct key, i.e. an oracle engine model called with
drop_delete=False:

    fold_changelog(runs, levels, max_level,
                   lambda r: partial_update_model(r, drop_delete=False))

Rows are tuples (key, seq, kind, values, valid); a null field has value None.
Deletion-vector tombstones are applied by the caller (pass the filtered
runs), as ApplyDeletionVectorReader feeds the merge.
"""
import numpy as np

INSERT, UPDATE_BEFORE, UPDATE_AFTER, DELETE = 0, 1, 2, 3


def is_add(kind):
    return int(kind) in (INSERT, UPDATE_AFTER)


def _run_valid(run, c, i):
    valid = run.get("valid")
    return True if valid is None else bool(valid[c][i])


def _source_row(runs, ri, i):
    run = runs[ri]
    n_cols = len(run["values"])
    valid = tuple(_run_valid(run, c, i) for c in range(n_cols))
    values = tuple(run["values"][c][i] if valid[c] else None
                   for c in range(n_cols))
    return (int(run["key"][i]), int(run["seq"][i]), int(run["kind"][i]),
            values, valid)


def _model_row(res, dtypes, g):
    n_cols = len(res["values"])
    valid = tuple(bool(res["valid"][c][g]) for c in range(n_cols))
    values = tuple(dtypes[c].type(res["values"][c][g]) if valid[c] else None
                   for c in range(n_cols))
    return (int(res["key"][g]), int(res["seq"][g]), int(res["kind"][g]),
            values, valid)


def values_equal(a, b):
    """The row-deduplicate equaliser over two rows' value columns: validity
    first, then the stored bits (k_cl_finalize's rule)."""
    if a[4] != b[4]:
        return False
    for va, vb, ok in zip(a[3], b[3], a[4]):
        if ok and np.asarray(va).tobytes() != np.asarray(vb).tobytes():
            return False
    return True


class _Wrapper:
    """FullChangelogMergeFunctionWrapper, field for field. The merge function
    is the model's row for the group: merge() only records that it ran."""

    def __init__(self, max_level, row_dedup):
        self.max_level = max_level
        self.row_dedup = row_dedup

    def reset(self, merged):
        self.merged = merged  # mergeFunction.getResult() of this group
        self.n_merged = 0
        self.top = None
        self.initial = None
        self.is_initialized = False

    def add(self, kv, level):
        if self.max_level == level:
            assert self.top is None, \
                "Top level key-value already exists! This is unexpected."
            self.top = kv
        if self.initial is None:
            self.initial = kv
        else:
            if not self.is_initialized:
                self.n_merged += 1  # merge(initialKv)
                self.is_initialized = True
            self.n_merged += 1  # merge(kv)

    def get_result(self):
        """-> (changelog rows, result row or None)"""
        cl = []
        replace = lambda kind, kv: (kv[0], kv[1], kind, kv[3], kv[4])
        if self.is_initialized:
            merged = self.merged
            if self.top is None:
                if is_add(merged[2]):
                    cl.append(replace(INSERT, merged))
            else:
                if not is_add(merged[2]):
                    cl.append(replace(DELETE, self.top))
                elif not self.row_dedup or \
                        not values_equal(self.top, merged):
                    cl.append(replace(UPDATE_BEFORE, self.top))
                    cl.append(replace(UPDATE_AFTER, merged))
            res = merged
        else:
            if self.top is None and is_add(self.initial[2]):
                cl.append(replace(INSERT, self.initial))
            res = self.initial
        return cl, (res if is_add(res[2]) else None)  # setResultIfNotRetract


def fold_changelog(runs, levels, max_level, model, row_dedup=False):
    """-> (changelog rows, result rows), both in key order."""
    recs = []
    for ri, r in enumerate(runs):
        for i in range(len(r["key"])):
            recs.append((int(r["key"][i]), int(r["seq"][i]),
                         is_add(r["kind"][i]), ri, i))
    recs.sort()  # (key, seq, isAdd): the merge order
    res = model(runs)
    keys = sorted({t[0] for t in recs})
    # exactly one merged row per distinct live key: no group left out
    assert len(res["key"]) == len(keys), (len(res["key"]), len(keys))
    assert (np.asarray(res["key"], np.int64) ==
            np.asarray(keys, np.int64)).all()
    dtypes = [np.asarray(v).dtype for v in runs[0]["values"]]
    w = _Wrapper(max_level, row_dedup)
    changelog, results = [], []
    gi, g = 0, 0
    while gi < len(recs):
        gj = gi
        while gj < len(recs) and recs[gj][0] == recs[gi][0]:
            gj += 1
        w.reset(_model_row(res, dtypes, g))
        for _, _, _, ri, i in recs[gi:gj]:
            w.add(_source_row(runs, ri, i), levels[ri])
        assert w.n_merged in (0, gj - gi)
        cl, r = w.get_result()
        # a row that carries the merged result belongs to a group the main
        # batch keeps under any drop_delete: merged is an add
        for row in cl:
            if row[2] in (INSERT, UPDATE_AFTER):
                assert r is not None
        changelog += cl
        if r is not None:
            results.append(r)
        gi, g = gj, g + 1
    return changelog, results


def rows_to_columns(rows, dtypes):
    """Row tuples -> {"key", "seq", "kind", "values": [...], "valid": [...]}
    with null fields stored as 0."""
    n_cols = len(dtypes)
    return {
        "key": np.array([r[0] for r in rows], np.int64),
        "seq": np.array([r[1] for r in rows], np.int64),
        "kind": np.array([r[2] for r in rows], np.int8),
        "values": [np.array([r[3][c] if r[4][c] else 0 for r in rows],
                            dtypes[c]) for c in range(n_cols)],
        "valid": [np.array([r[4][c] for r in rows], bool)
                  for c in range(n_cols)],
    }


def dedup_fold(runs):
    """A deduplicate merge function in the model shape: the last record of
    every key in (seq, isAdd) order, retracts kept."""
    recs = {}
    order = []
    for ri, r in enumerate(runs):
        for i in range(len(r["key"])):
            order.append((int(r["key"][i]), int(r["seq"][i]),
                          is_add(r["kind"][i]), ri, i))
    order.sort()
    for key, _, _, ri, i in order:
        recs[key] = (ri, i)
    rows = [_source_row(runs, ri, i) for _, (ri, i) in sorted(recs.items())]
    return rows_to_columns(rows, [np.asarray(v).dtype
                                  for v in runs[0]["values"]])
