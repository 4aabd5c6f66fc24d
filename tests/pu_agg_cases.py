"""Streams and plans of the partial-update aggregate-function tests
(tests/test_pu_agg_cpu.py checks the seeds on the CPU, tests/test_pu_agg_gpu
.py reads them on the GPU): int64 v_k plus nullable int32 / int64 / float
columns, 35% nulls, integer values in 0..50 so sequence tuples tie, two
sequence groups, one of them with two sequence fields.

Every case is the smallest shape that reaches one way k_emit_pu_sga can go
wrong (a tile is 3 584 rows): see CASES. A case's expected rows are computed
once per (case, drop_delete) and shared (expected()).
"""
import functools

import numpy as np

from tests.pu_agg_model import pu_agg_model

I, UB, UA, D = 0, 1, 2, 3

# column layout of the retract cases: index into the runs' values list,
# name in the files, numpy dtype, role
#   0 v_k   int64    plain (the key, never null)
#   1 v_c0  int32    group A sequence field
#   2 v_c1  int32    group A  sum
#   3 v_c2  int64    group A  last_value
#   4 v_c3  float32  group A  sum (rounds in float, in member order)
#   5 v_c4  int32    group A  no aggregate function
#   6 v_c5  int32    group B sequence field 1
#   7 v_c6  int32    group B sequence field 2
#   8 v_c7  int32    group B  first_value, ignore-retract (it has no
#                    retract of its own)
#   9 v_c8  int64    group B  last_non_null_value
#  10 v_c9  float32  group B  max, ignore-retract
#  11 v_c10 int32    plain
MIXED_DTYPES = ["int32", "int32", "int64", "float32", "int32", "int32",
                "int32", "int32", "int64", "float32", "int32"]
SG_IDX = [{"sequence_fields": [1], "group_fields": [2, 3, 4, 5]},
          {"sequence_fields": [6, 7], "group_fields": [8, 9, 10]}]
MIXED_AGGS = {2: "sum", 3: "last_value", 4: "sum", 8: "first_value",
              9: "last_non_null_value", 10: "max"}
MIXED_IGNORE = (8, 10)

# insert-only case:
#   0 v_k   int64    plain, named last_non_null_value
#   1 v_c0  int32    group A sequence field
#   2 v_c1  int32    group A  min
#   3 v_c2  int64    group A  first_non_null_value
#   4 v_c3  int32    group A  default (sum)
#   5 v_c4  float64  group A  default (sum)
#   6 v_c5  int32    group B sequence field 1 (named "max": a sequence field
#                    takes no aggregate function, the entry is dropped)
#   7 v_c6  int32    group B sequence field 2
#   8 v_c7  float32  group B  default (sum)
#   9 v_c8  int32    group B  min
#  10 v_c9  int32    plain, named last_non_null_value
INSERT_DTYPES = ["int32", "int32", "int64", "int32", "float64", "int32",
                 "int32", "float32", "int32", "int32"]
INSERT_SG_IDX = [{"sequence_fields": [1], "group_fields": [2, 3, 4, 5]},
                 {"sequence_fields": [6, 7], "group_fields": [8, 9]}]
INSERT_AGGS = {0: "last_non_null_value", 2: "min",
               3: "first_non_null_value", 6: "max", 9: "min",
               10: "last_non_null_value"}

TYPE_NAMES = {"int32": "int32", "int64": "int64", "float32": "float",
              "float64": "double"}
KEY_COLS = [{"name": "_KEY_k", "type": "int64"}]
KIND_P = {I: .45, UA: .2, UB: .15, D: .2}


def col_name(c):
    return "v_k" if c == 0 else f"v_c{c - 1}"


def value_cols(dtypes):
    return ([{"name": "v_k", "type": "int64"}] +
            [{"name": f"v_c{i}", "type": TYPE_NAMES[dt]}
             for i, dt in enumerate(dtypes)])


def named_groups(sg_idx):
    return [{"sequence_fields": [col_name(c) for c in sg["sequence_fields"]],
             "group_fields": [col_name(c) for c in sg["group_fields"]]}
            for sg in sg_idx]


def gen_runs(seed, n_runs, rows, dtypes, same_keys=False, kinds=(I, UA, UB, D),
             top_run=False, null_frac=0.35):
    """n_runs sorted runs of `rows` unique keys: drawn from a key space of
    0.6 x the total, or one key set for all (same_keys: every key group has
    n_runs members). Sequence numbers are a permutation of the total, so the
    merge order is independent of the sequence-field tuples. top_run: the
    last run holds the oldest sequence numbers (a max-level file): INSERTs,
    15% DELETEs, so that a group can fold to a DELETE over a top-level
    record."""
    rng = np.random.default_rng(seed)
    total = n_runs * rows
    space = max(int(total * 0.6), rows)
    seqs = rng.permutation(total).astype(np.int64)
    if top_run:
        seqs = np.concatenate([rows + rng.permutation(total - rows),
                               np.arange(rows)]).astype(np.int64)
    shared = np.sort(rng.choice(space, rows, replace=False)).astype(np.int64)
    p = np.array([KIND_P[k] for k in kinds])
    runs = []
    for r in range(n_runs):
        key = shared.copy() if same_keys else np.sort(
            rng.choice(space, rows, replace=False)).astype(np.int64)
        kind = rng.choice(kinds, rows, p=p / p.sum()).astype(np.int8)
        if top_run and r == n_runs - 1:
            kind = np.where(rng.random(rows) < 0.15, D, I).astype(np.int8)
        vals, msks = [key.copy()], [np.ones(rows, bool)]
        for dt in dtypes:
            if dt.startswith("float"):
                vals.append((rng.random(rows) * 50).astype(dt))
            else:
                vals.append(rng.integers(0, 50, rows).astype(dt))
            msks.append(rng.random(rows) >= null_frac)
        runs.append({"key": key, "seq": seqs[r * rows:(r + 1) * rows],
                     "kind": kind, "values": vals, "valid": msks})
    return runs


# name -> stream and plan. `need`: what the model's counters must reach
# before the case counts as exercising what it is for.
CASES = {
    # 3 tiles, groups of 1..5, all four row kinds
    "mixed": dict(seed=11, n_runs=5, rows=2000, dtypes=MIXED_DTYPES,
                  sg=SG_IDX, aggs=MIXED_AGGS, ignore=MIXED_IGNORE,
                  need=dict(reversed=50, in_order=50, retract_in_order=50,
                            retract_out_of_order=50, skipped_empty=50,
                            first_member_retract=50),
                  group=(2, 5)),
    # every group has 9 members: past the 4 the sibling kernels cache
    "deep": dict(seed=12, n_runs=9, rows=600, dtypes=MIXED_DTYPES,
                 same_keys=True, sg=SG_IDX, aggs=MIXED_AGGS,
                 ignore=MIXED_IGNORE,
                 need=dict(reversed=50, in_order=50, retract_in_order=50,
                           retract_out_of_order=50, skipped_empty=50),
                 group=(9, 9)),
    # 32-member groups (mask bit 31), two tiles
    "widest": dict(seed=13, n_runs=32, rows=120, dtypes=MIXED_DTYPES,
                   same_keys=True, sg=SG_IDX, aggs=MIXED_AGGS,
                   ignore=MIXED_IGNORE,
                   need=dict(reversed=50, in_order=50, retract_in_order=50,
                             retract_out_of_order=50, skipped_empty=50),
                   group=(32, 32)),
    # min, first_non_null_value and the default function, no retracts
    "insert_only": dict(seed=14, n_runs=4, rows=2000, dtypes=INSERT_DTYPES,
                        kinds=(I, UA), sg=INSERT_SG_IDX, aggs=INSERT_AGGS,
                        ignore=(), default_agg="sum",
                        need=dict(reversed=50, in_order=50,
                                  skipped_empty=50),
                        group=(2, 4)),
    # retracts are swallowed, but a leading one still seeds the row
    "ignore_delete": dict(seed=15, n_runs=4, rows=2000, dtypes=MIXED_DTYPES,
                          sg=SG_IDX, aggs=MIXED_AGGS, ignore=MIXED_IGNORE,
                          ignore_delete=True,
                          need=dict(reversed=50, in_order=50,
                                    skipped_empty=50,
                                    first_member_retract=50),
                          group=(2, 4)),
}


@functools.lru_cache(maxsize=None)
def case_runs(name):
    c = CASES[name]
    return gen_runs(c["seed"], c["n_runs"], c["rows"], c["dtypes"],
                    same_keys=c.get("same_keys", False),
                    kinds=c.get("kinds", (I, UA, UB, D)))


def model_kwargs(c):
    return dict(aggs=c["aggs"], ignore_retract=c["ignore"],
                default_agg=c.get("default_agg"),
                ignore_delete=c.get("ignore_delete", False))


@functools.lru_cache(maxsize=None)
def expected(name, drop_delete=True):
    """The model's rows of a case; computed once, shared, never modified."""
    c = CASES[name]
    return pu_agg_model(case_runs(name), c["sg"], drop_delete=drop_delete,
                        **model_kwargs(c))


def plan_kwargs(c):
    """MergeReadPlan keywords of a case."""
    kw = dict(merge_engine="partial-update",
              sequence_groups=named_groups(c["sg"]),
              aggregations={col_name(i): f for i, f in c["aggs"].items()},
              ignore_retract=[col_name(i) for i in c["ignore"]],
              ignore_delete=c.get("ignore_delete", False))
    if c.get("default_agg"):
        kw["default_aggregation"] = c["default_agg"]
    return kw


def check_counters(name):
    """The case's stream exercises what the case is for. A seed that misses
    is replaced, not tolerated."""
    c = CASES[name]
    cnt = expected(name, False)["counters"]
    for what, floor in c["need"].items():
        assert cnt[what] >= floor, (name, what, cnt)
    lo, hi = c["group"]
    assert cnt["largest_group"] == hi, (name, cnt)
    runs = case_runs(name)
    _, sizes = np.unique(np.concatenate([r["key"] for r in runs]),
                         return_counts=True)
    assert sizes.max() == hi and (sizes >= lo).sum() > 0, (name, sizes.max())
    if name == "mixed":
        assert set(sizes.tolist()) == {1, 2, 3, 4, 5}, set(sizes.tolist())
    return cnt
