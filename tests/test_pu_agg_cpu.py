"""Partial-update aggregate functions inside sequence groups, on the CPU:

 - tests/pu_agg_model.py (the sequential port) reproduces the reference's
   PartialUpdateMergeFunctionTest vectors, typed in below as data;
 - without aggregate functions it equals oracle.partial_update_seqgroup_model;
 - pmh_debug_pu_agg_fold — the host entry to pu_agg_core.h, the code
   k_emit_pu_sga runs per output row — equals the model for every aggregate
   function x dtype x {plain, ignore-retract} over random member lists, and
   on the reference vectors;
 - the GPU cases' streams exercise what they are for (tests/pu_agg_cases.py).
"""
import numpy as np
import pytest

from oracle import partial_update_seqgroup_model
from paimon_amd.reader import (PU_AGG_CODES, PU_AGG_IGNORE_RETRACT,
                               PU_AGG_NONE, debug_pu_agg_fold)
from tests import pu_agg_cases as cases
from tests.pu_agg_model import (PartialUpdateMerge, UnsupportedRetract,
                                pu_agg_model, resolve_aggs)

I, UB, UA, D = 0, 1, 2, 3
N = None

# ---------------------------------------------------------------- vectors
# PartialUpdateMergeFunctionTest: (sequence groups, aggregate functions,
# ignore-retract columns, default function, steps); a step is ("add", kind,
# row) or ("validate", row). Column 0 is the test's key column f0 (its
# listagg / primary-key function is not part of this port: the column is in
# no group and always 1).
VECTORS = {
    "testFirstValue": dict(
        sg=[{"sequence_fields": [1], "group_fields": [2, 3]}],
        aggs={2: "first_value", 3: "last_value"}, ignore=(), default=None,
        steps=[("add", I, [1, 1, 1, 1]),
               ("add", I, [1, 2, 2, 2]),
               ("validate", [1, 2, 1, 2]),
               ("add", I, [1, 0, 3, 3]),
               ("validate", [1, 2, 3, 2])]),
    "testMultiSequenceFieldsFirstValue": dict(
        sg=[{"sequence_fields": [1, 2], "group_fields": [3, 4]}],
        aggs={3: "first_value", 4: "last_value"}, ignore=(), default=None,
        steps=[("add", I, [1, 1, 1, 1, 1]),
               ("add", I, [1, 2, 2, 2, 2]),
               ("validate", [1, 2, 2, 1, 2]),
               ("add", I, [1, 0, 1, 3, 3]),
               ("validate", [1, 2, 2, 3, 2])]),
    "testPartialUpdateWithAggregation": dict(
        sg=[{"sequence_fields": [1], "group_fields": [2, 3, 4]},
            {"sequence_fields": [7], "group_fields": [6]}],
        aggs={2: "sum", 4: "last_value", 6: "last_non_null_value"},
        ignore=(4, 6), default=None,
        steps=[("add", I, [1, 1, 1, 1, 1, 1, 1, 1]),
               ("add", I, [1, 2, 1, 2, 2, 2, 2, 0]),
               ("validate", [1, 2, 2, 2, 2, 2, 1, 1]),
               # g_1, g_2 not advanced
               ("add", I, [1, 1, 1, 1, 1, 1, 2, 0]),
               ("validate", [1, 2, 3, 2, 2, 1, 1, 1]),
               ("add", I, [1, 1, -1, 1, 1, 2, 2, 0]),
               # test null
               ("add", I, [1, 3, N, N, N, N, N, 2]),
               ("validate", [1, 3, 2, N, N, 2, 1, 2]),
               # test retract
               ("add", I, [1, 3, 1, 1, 1, 1, 1, 3]),
               ("validate", [1, 3, 3, 1, 1, 1, 1, 3]),
               ("add", UB, [1, 3, 2, 1, 1, 1, 1, 3]),
               ("validate", [1, 3, 1, N, 1, 1, 1, 3]),
               ("add", D, [1, 3, 2, 1, 1, 1, 1, 3]),
               ("validate", [1, 3, -1, N, 1, 1, 1, 3]),
               # retract for old sequence
               ("add", D, [1, 2, 2, 1, 1, 1, 1, 3]),
               ("validate", [1, 3, -3, N, 1, 1, 1, 3])]),
    "testMultiSequenceFieldsPartialUpdateWithAggregation": dict(
        sg=[{"sequence_fields": [1, 2], "group_fields": [3, 4, 5]},
            {"sequence_fields": [7, 8], "group_fields": [6]}],
        aggs={3: "sum", 4: "first_value", 5: "last_value",
              6: "last_non_null_value"},
        ignore=(4, 6), default=None,
        steps=[  # test null retract
               ("add", I, [1, N, N, 1, 1, 1, 1, 1, 1]),
               ("validate", [1, N, N, N, N, N, 1, 1, 1]),
               ("add", D, [1, N, N, 1, 1, 1, 0, 1, 1]),
               ("validate", [1, N, N, N, N, N, 1, 1, 1]),
               ("add", I, [1, 1, 1, 1, 1, 1, 1, 1, 1]),
               ("add", I, [1, 1, 2, 1, 2, 2, N, 2, 0]),
               ("validate", [1, 1, 2, 2, 1, 2, 1, 2, 0]),
               # sequence group not advanced
               ("add", I, [1, 1, 1, 1, 3, 1, 1, 2, 0]),
               ("validate", [1, 1, 2, 3, 3, 2, 1, 2, 0]),
               # test null
               ("add", I, [1, 1, 3, N, N, N, N, 4, 2]),
               ("validate", [1, 1, 3, 3, 3, N, 1, 4, 2]),
               # test retract
               ("add", I, [1, 2, 3, 1, 1, 1, 1, 4, 3]),
               ("validate", [1, 2, 3, 4, 3, 1, 1, 4, 3]),
               ("add", UB, [1, 2, 3, 2, 1, 2, 1, 4, 3]),
               ("validate", [1, 2, 3, 2, 3, N, 1, 4, 3]),
               # the reference's row has eight fields here; its ninth is
               # never read (f7 = 3 < 4 decides the second group)
               ("add", D, [1, 3, 2, 3, 1, 1, 4, 3, N]),
               ("validate", [1, 3, 2, -1, 3, N, 1, 4, 3]),
               # retract for old sequence
               ("add", D, [1, 2, 2, 2, 1, 1, 1, 1, 3]),
               ("validate", [1, 3, 2, -3, 3, N, 1, 4, 3])]),
    "testSequenceGroupDefaultAggFunc": dict(
        sg=[{"sequence_fields": [3], "group_fields": [1, 2]},
            {"sequence_fields": [6], "group_fields": [4, 5]}],
        aggs={}, ignore=(), default="last_non_null_value",
        steps=[("add", I, [1, 1, 1, 1, 1, 1, 1]),
               ("add", I, [1, 2, 2, 2, 2, 2, N]),
               ("validate", [1, 2, 2, 2, 1, 1, 1]),
               ("add", I, [1, 3, 3, 1, 3, 3, 3]),
               ("validate", [1, 2, 2, 2, 3, 3, 3]),
               ("add", I, [1, 4, N, 4, 5, N, 5]),
               ("validate", [1, 4, 2, 4, 5, 3, 5])]),
    "testMultiSequenceFieldsDefaultAggFunc": dict(
        sg=[{"sequence_fields": [3, 4], "group_fields": [1, 2]},
            {"sequence_fields": [7, 8], "group_fields": [5, 6]}],
        aggs={}, ignore=(), default="last_non_null_value",
        steps=[("add", I, [1, 1, 1, 1, 1, 1, 1, 1, 1]),
               ("add", I, [1, 2, 2, 2, 2, 2, 2, N, N]),
               ("validate", [1, 2, 2, 2, 2, 1, 1, 1, 1]),
               ("add", I, [1, 3, 3, 1, 1, 3, 3, 3, 3]),
               ("validate", [1, 2, 2, 2, 2, 3, 3, 3, 3]),
               ("add", I, [1, 4, N, 4, 4, 5, N, 5, 5]),
               ("validate", [1, 4, 2, 4, 4, 5, 3, 5, 5])]),
}

DT_CODE = {"int8": 1, "int16": 2, "int32": 3, "int64": 4, "float32": 5,
           "float64": 6}


def _typed(row, dtypes):
    return [None if v is None else np.dtype(dt).type(v)
            for v, dt in zip(row, dtypes)]


def _bits(v, dt):
    """a column value as the 64 bits the fold entry takes"""
    if dt == "float32":
        return int(np.float32(v).view(np.int32))
    if dt == "float64":
        return int(np.float64(v).view(np.int64))
    return int(v)


def _from_bits(b, dt):
    if dt == "float32":
        return np.int32(b).view(np.float32)
    if dt == "float64":
        return np.int64(b).view(np.float64)
    return np.dtype(dt).type(b)


def native_fold(members, dtypes, sg, agg_names, ignore=(),
                ignore_delete=False):
    """members: [(kind, row with None for null)] in merge order -> (row with
    None for null, kind, last member index, unsupported flag) from
    pmh_debug_pu_agg_fold."""
    n_cols = len(dtypes)
    kinds = [k for k, _ in members]
    values = np.zeros((len(members), n_cols), np.int64)
    valid = np.zeros((len(members), n_cols), np.uint8)
    for x, (_, row) in enumerate(members):
        for c, v in enumerate(row):
            if v is not None:
                values[x, c] = _bits(v, dtypes[c])
                valid[x, c] = 1
    col_group = np.full(n_cols, 0xff, np.uint8)
    sg_fields = np.full((len(sg), 4), -1, np.int16)
    sg_nseq = np.zeros(len(sg), np.uint8)
    for g, grp in enumerate(sg):
        for c in list(grp["sequence_fields"]) + list(grp["group_fields"]):
            col_group[c] = g
        sg_fields[g, :len(grp["sequence_fields"])] = grp["sequence_fields"]
        sg_nseq[g] = len(grp["sequence_fields"])
    col_agg = np.full(n_cols, PU_AGG_NONE, np.uint8)
    for c, name in agg_names.items():
        col_agg[c] = PU_AGG_CODES[
            "first_non_null_value" if name == "first_not_null_value"
            else name] | (PU_AGG_IGNORE_RETRACT if c in ignore else 0)
    v, ok, kind, last, unsup = debug_pu_agg_fold(
        kinds, [DT_CODE[dt] for dt in dtypes], values, valid, col_group,
        sg_fields, sg_nseq, col_agg, ignore_delete)
    row = [_from_bits(v[c], dtypes[c]) if ok[c] else None
           for c in range(n_cols)]
    return row, kind, last, unsup


def _same_row(a, b):
    assert len(a) == len(b)
    for c, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), (c, a, b)
        if x is not None:
            # bit-exact: a float sum must round as the model's does
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), \
                (c, a, b)


def _vector_prefixes(v):
    """-> [(members so far, expected row)] per validate step"""
    n_cols = len(v["steps"][0][2])
    dtypes = ["int32"] * n_cols
    members, out = [], []
    for step in v["steps"]:
        if step[0] == "add":
            members.append((step[1], _typed(step[2], dtypes)))
        else:
            out.append((list(members), _typed(step[1], dtypes)))
    return dtypes, out


@pytest.mark.parametrize("name", sorted(VECTORS))
def test_model_reproduces_reference_vector(name):
    v = VECTORS[name]
    dtypes, prefixes = _vector_prefixes(v)
    names = resolve_aggs(len(dtypes), v["sg"], v["aggs"], v["ignore"],
                         v["default"])
    for members, want in prefixes:
        mf = PartialUpdateMerge(len(dtypes), v["sg"], names, v["ignore"])
        for seq, (kind, row) in enumerate(members):
            mf.add(kind, seq, row)
        _same_row(mf.get_result()[2], want)


@pytest.mark.parametrize("name", sorted(VECTORS))
def test_native_fold_reproduces_reference_vector(name):
    v = VECTORS[name]
    dtypes, prefixes = _vector_prefixes(v)
    names = resolve_aggs(len(dtypes), v["sg"], v["aggs"], v["ignore"],
                         v["default"])
    checked = 0
    for members, want in prefixes:
        if len(members) < 2:
            continue  # a lone record bypasses the merge function
        row, kind, last, unsup = native_fold(members, dtypes, v["sg"], names,
                                             v["ignore"])
        _same_row(row, want)
        assert not unsup
        assert kind == (0 if any(k in (I, UA) for k, _ in members) else 3)
        assert last == len(members) - 1
        checked += 1
    assert checked >= 2


def test_model_without_aggregators_equals_oracle():
    """all four row kinds, both drop_delete settings, ignore_delete too"""
    dtypes = ["int32"] * 7
    sg = [{"sequence_fields": [1], "group_fields": [2, 3]},
          {"sequence_fields": [4, 5], "group_fields": [6]}]
    for seed in (1, 2, 3):
        runs = cases.gen_runs(seed, 5, 400, dtypes)
        assert {int(k) for r in runs for k in r["kind"]} == {I, UB, UA, D}
        for drop_delete in (True, False):
            for ignore_delete in (False, True):
                got = pu_agg_model(runs, sg, drop_delete=drop_delete,
                                   ignore_delete=ignore_delete)
                exp = partial_update_seqgroup_model(
                    runs, sg, drop_delete=drop_delete,
                    ignore_delete=ignore_delete)
                for k in ("key", "seq", "kind"):
                    assert (got[k] == exp[k]).all(), k
                for c in range(len(exp["values"])):
                    assert (got["valid"][c] == exp["valid"][c]).all(), c
                    m = exp["valid"][c]
                    assert (got["values"][c][m] == exp["values"][c][m]).all()


# ------------------------------------------------------ fold entry vs model
# columns of the random member lists:
#   0 group A sequence field   1, 2 group B sequence fields
#   3 group A aggregated (dtype under test)   4 group A, no aggregator
#   5 group B aggregated (dtype under test)   6 plain
FOLD_SG = [{"sequence_fields": [0], "group_fields": [3, 4]},
           {"sequence_fields": [1, 2], "group_fields": [5]}]
AGG_NAMES = ["last_non_null_value", "last_value", "first_value",
             "first_non_null_value", "sum", "max", "min"]
RETRACTABLE = {"last_non_null_value", "last_value", "sum"}


def _random_members(rng, n, dt):
    info = np.iinfo(dt) if not dt.startswith("float") else None
    members = []
    for _ in range(n):
        kind = int(rng.choice([I, UA, UB, D], p=[.4, .2, .2, .2]))
        row = []
        for c in range(7):
            if rng.random() < 0.35:
                row.append(None)
            elif c in (3, 5):
                if info is None:
                    row.append(np.dtype(dt).type((rng.random() - 0.3) * 1e3))
                elif rng.random() < 0.3:
                    # near the ends of the range: sums wrap
                    row.append(np.dtype(dt).type(
                        rng.choice([info.min, info.min + 1, info.max,
                                    info.max - 1])))
                else:
                    row.append(np.dtype(dt).type(rng.integers(-60, 60)))
            else:
                row.append(np.int32(rng.integers(0, 4)))
        members.append((kind, row))
    return members


@pytest.mark.parametrize("ignore", [False, True], ids=["plain", "ignore"])
@pytest.mark.parametrize("dt", ["int8", "int16", "int32", "int64",
                                "float32", "float64"])
@pytest.mark.parametrize("agg", AGG_NAMES)
def test_native_fold_equals_model(agg, dt, ignore):
    rng = np.random.default_rng(
        1000 * AGG_NAMES.index(agg) + 10 * DT_CODE[dt] + int(ignore))
    dtypes = ["int32", "int32", "int32", dt, "int32", dt, "int32"]
    names = {3: agg, 5: agg}
    ign = (3, 5) if ignore else ()
    sizes = [2, 3, 31, 32] + [int(rng.integers(2, 33)) for _ in range(26)]
    refused = folded = 0
    for trial, n in enumerate(sizes):
        members = _random_members(rng, n, dt)
        ignore_delete = trial % 5 == 4
        mf = PartialUpdateMerge(7, FOLD_SG, names, ign, ignore_delete)
        try:
            for seq, (kind, row) in enumerate(members):
                mf.add(kind, seq, row)
            want = mf.get_result()
        except UnsupportedRetract:
            want = None
        row, kind, last, unsup = native_fold(members, dtypes, FOLD_SG, names,
                                             ign, ignore_delete)
        # an unsupported retraction reports its flag, exactly where the
        # reference throws
        assert unsup == (want is None), (trial, members)
        if want is None:
            refused += 1
            continue
        folded += 1
        seq, wkind, wrow = want
        _same_row(row, wrow)
        assert kind == wkind
        assert (last if last >= 0 else 0) == seq
    if agg in RETRACTABLE or ignore:
        assert refused == 0
    else:
        assert refused >= 5
    assert folded >= 3


def test_fold_entry_refuses_bad_arguments():
    members = [(I, [np.int32(1)] * 2)] * 33
    with pytest.raises(RuntimeError, match="n_members"):
        native_fold(members, ["int32"] * 2,
                    [{"sequence_fields": [0], "group_fields": [1]}],
                    {1: "sum"})


# ----------------------------------------------------------- the GPU cases
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_case_stream_exercises_its_paths(name):
    cases.check_counters(name)
    # both drop_delete settings come from the same stream
    assert len(cases.expected(name, True)["key"]) <= \
        len(cases.expected(name, False)["key"])


# ------------------------------------------------------------- hostcheck
def test_hostcheck_builds_and_passes():
    """pu_agg_core.h under ASan + UBSan, as a stand-alone program"""
    import os
    import subprocess
    csrc = os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "paimon_amd", "csrc")
    b = subprocess.run(["make", "-C", csrc, "build/pu_agg_hostcheck"],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([os.path.join(csrc, "build", "pu_agg_hostcheck")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pu_agg_hostcheck OK" in r.stdout
