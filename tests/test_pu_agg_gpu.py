"""Partial-update with aggregate functions inside sequence groups on the GPU
(k_emit_pu_sga) against the sequential port tests/pu_agg_model.py, which
tests/test_pu_agg_cpu.py pins to the reference's vectors. Bit-exact on keys,
sequence numbers, kinds, validity and values — float sums included: the model
adds in the column's dtype in member order, and so does the kernel.

Streams and plans: tests/pu_agg_cases.py (uncompressed Parquet from
write_runs). Each case first asserts on the model's counters that its stream
exercises what it is for.

Figures this file pins, for the record: none are tolerances; every compare
is on the stored bits.
"""
import numpy as np
import pytest

from oracle import partial_update_seqgroup_model
from paimon_amd import Session, MergeReadPlan, file_descs_from_metas
from paimon_amd.datagen import write_runs
from paimon_amd.reader import (PU_EMIT_SG, PU_EMIT_SGA,
                               debug_last_pu_emit_kernel)
from tests import pu_agg_cases as cases
from tests.changelog_fold_model import fold_changelog, rows_to_columns
from tests.pu_agg_model import UnsupportedRetract, pu_agg_model

pytestmark = pytest.mark.gpu

I, UB, UA, D = 0, 1, 2, 3
MAX_LEVEL = 5


def _read_all(plan, changelog=False):
    main, cl = [], []
    while True:
        b = plan.read_next()
        if b is None:
            break
        main.append({k: v.copy() for k, v in b.items()})
        if changelog:
            cl.append({k: v.copy()
                       for k, v in plan.read_changelog().items()})
    cat = lambda parts: {k: np.concatenate([p[k] for p in parts])
                         for k in parts[0]} if parts else {}
    return (cat(main), cat(cl)) if changelog else cat(main)


def _compare(got, exp, what):
    n = len(exp["key"])
    assert len(got["_KEY_k"]) == n, (what, len(got["_KEY_k"]), n)
    assert (got["_KEY_k"] == exp["key"]).all(), what
    assert (got["_SEQUENCE_NUMBER"] == exp["seq"]).all(), what
    assert (got["_VALUE_KIND"] == exp["kind"]).all(), what
    for c in range(len(exp["values"])):
        nm = cases.col_name(c)
        ev, em = exp["values"][c], exp["valid"][c]
        gm = got.get(nm + "#valid")
        if gm is None:
            gm = np.ones(n, dtype=bool)
        assert (gm.astype(bool) == em).all(), (what, nm)
        assert got[nm].dtype == ev.dtype, (what, nm)
        assert got[nm][em].tobytes() == ev[em].tobytes(), (what, nm)


def _plan(s, metas, dtypes, **kw):
    return MergeReadPlan(s, file_descs_from_metas(metas), cases.KEY_COLS,
                         cases.value_cols(dtypes), **kw)


def _run_case(tmp_path, name, drop_delete):
    c = cases.CASES[name]
    cases.check_counters(name)
    exp = cases.expected(name, drop_delete)
    metas = write_runs(cases.case_runs(name), str(tmp_path),
                       compression="NONE")
    with Session(0) as s:
        with _plan(s, metas, c["dtypes"], drop_delete=drop_delete,
                   **cases.plan_kwargs(c)) as plan:
            got = _read_all(plan)
            assert debug_last_pu_emit_kernel() == PU_EMIT_SGA
    _compare(got, exp, name)


@pytest.mark.parametrize("drop_delete", [True, False],
                         ids=["drop_delete", "keep_delete"])
def test_mixed(tmp_path, drop_delete):
    """3 tiles, key groups of 1..5 members, all four row kinds; sum (int32
    and float), last_value, first_value and max under ignore-retract,
    last_non_null_value, a group field without a function, a plain column.
    The parent commit returns overlay values here."""
    _run_case(tmp_path, "mixed", drop_delete)


def test_deep(tmp_path):
    """every key group has 9 members"""
    _run_case(tmp_path, "deep", True)


def test_widest(tmp_path):
    """32-member key groups: bit 31 of the member masks, two tiles"""
    _run_case(tmp_path, "widest", True)


def test_insert_only(tmp_path):
    """min, first_non_null_value, default_aggregation = sum over int32,
    float and double columns; an aggregations entry on a sequence field is
    dropped"""
    _run_case(tmp_path, "insert_only", True)


@pytest.mark.parametrize("drop_delete", [True, False],
                         ids=["drop_delete", "keep_delete"])
def test_ignore_delete(tmp_path, drop_delete):
    """retracts are swallowed, but a leading one seeds the row and its
    sequence tuples (initRow)"""
    _run_case(tmp_path, "ignore_delete", drop_delete)


# ------------------------------------------------------ refused retraction
REFUSE_AGGS = dict(cases.MIXED_AGGS)
REFUSE_IGNORE = (8,)  # max on v_c9 (group B) no longer ignores retracts


def test_refused_retraction(tmp_path):
    """max without ignore-retract, a retract with a non-empty group-B tuple:
    the read raises, and raises again after reset()"""
    runs = cases.case_runs("mixed")
    with pytest.raises(UnsupportedRetract):
        pu_agg_model(runs, cases.SG_IDX, aggs=REFUSE_AGGS,
                     ignore_retract=REFUSE_IGNORE)
    metas = write_runs(runs, str(tmp_path), compression="NONE")
    c = dict(cases.CASES["mixed"], ignore=REFUSE_IGNORE)
    with Session(0) as s:
        with _plan(s, metas, c["dtypes"], **cases.plan_kwargs(c)) as plan:
            for _ in range(2):
                with pytest.raises(RuntimeError) as ei:
                    _read_all(plan)
                msg = str(ei.value)
                assert "'max'" in msg and "v_c9" in msg, msg
                assert "ignore_retract" in msg, msg
                plan.reset()


def test_retraction_with_empty_tuples_reads(tmp_path):
    """the same plan over a stream whose retracts all carry an empty group-B
    tuple: nothing reaches max.retract, the read matches the model"""
    runs = [dict(r, valid=[m.copy() for m in r["valid"]])
            for r in cases.case_runs("mixed")]
    n_retract = 0
    for r in runs:
        rt = (r["kind"] == UB) | (r["kind"] == D)
        for sf in cases.SG_IDX[1]["sequence_fields"]:
            r["valid"][sf][rt] = False
        n_retract += int(rt.sum())
    assert n_retract >= 50
    exp = pu_agg_model(runs, cases.SG_IDX, aggs=REFUSE_AGGS,
                       ignore_retract=REFUSE_IGNORE)
    assert exp["counters"]["retract_in_order"] >= 50  # group A still acts
    metas = write_runs(runs, str(tmp_path), compression="NONE")
    c = dict(cases.CASES["mixed"], ignore=REFUSE_IGNORE)
    with Session(0) as s:
        with _plan(s, metas, c["dtypes"], **cases.plan_kwargs(c)) as plan:
            got = _read_all(plan)
    _compare(got, exp, "empty-tuple retracts")


# ----------------------------------------------------------- plan refusals
def test_plan_refusals(tmp_path):
    runs = cases.gen_runs(21, 1, 100, cases.MIXED_DTYPES, kinds=(I,))
    # a string column for the type rules
    metas = write_runs(runs, str(tmp_path), compression="NONE")
    sg = cases.named_groups(cases.SG_IDX)

    def refuse(match, value_cols=None, **kw):
        kw.setdefault("sequence_groups", sg)
        with pytest.raises(RuntimeError, match=match):
            MergeReadPlan(s, file_descs_from_metas(metas), cases.KEY_COLS,
                          value_cols or cases.value_cols(cases.MIXED_DTYPES),
                          merge_engine="partial-update", **kw)

    with Session(0) as s:
        # a function other than last_non_null_value outside every group
        refuse("Must use sequence group for aggregation functions but not "
               "found for field v_c10", aggregations={"v_c10": "sum"})
        # ... which covers a plan without sequence groups
        refuse("Must use sequence group for aggregation functions but not "
               "found for field v_c1", aggregations={"v_c1": "sum"},
               sequence_groups=None)
        # ... and the default function reaching a plain column
        refuse("Must use sequence group for aggregation functions but not "
               "found for field v_k", default_aggregation="sum")
        refuse("primary_key", aggregations={"v_c1": "primary_key"})
        refuse("ignore_retract: column 'v_c4' has no aggregate function",
               ignore_retract=["v_c4"])
        refuse("not on the GPU path", aggregations={"v_c1": "listagg"})
        refuse("not on the GPU path", default_aggregation="product")
        refuse("is not a value column", aggregations={"nope": "sum"})
        # the type rules of the aggregation engine
        typed = cases.value_cols(cases.MIXED_DTYPES)
        as_type = lambda nm, t: [dict(v, type=t) if v["name"] == nm else v
                                 for v in typed]
        for fn in ("sum", "max", "min"):
            refuse("on a string column", value_cols=as_type("v_c2", "string"),
                   aggregations={"v_c2": fn})
        for t, word in (("boolean", "boolean"), ("date", "date"),
                        ("time", "time"), ("timestamp(3)", "timestamp")):
            refuse(f"aggregate 'sum' on {word}",
                   value_cols=as_type("v_c1", t),
                   aggregations={"v_c1": "sum"})
        # accepted: last_non_null_value needs no group; a sequence field's
        # entry is dropped
        with MergeReadPlan(s, file_descs_from_metas(metas), cases.KEY_COLS,
                           typed, merge_engine="partial-update",
                           sequence_groups=sg,
                           aggregations={"v_c10": "last_non_null_value",
                                         "v_c0": "sum"}) as plan:
            got = _read_all(plan)
            # no group field carries a function: the plan keeps k_emit_pu_sg
            assert debug_last_pu_emit_kernel() == PU_EMIT_SG
            assert len(got["_KEY_k"]) == 100


# -------------------------------------------------- full-compaction changelog
def test_full_compaction_changelog(tmp_path):
    """the mixed shape with a max-level run: the folded changelog chain reads
    its after-rows from the main output k_emit_pu_sga wrote"""
    c = cases.CASES["mixed"]
    runs = cases.gen_runs(31, c["n_runs"], c["rows"], c["dtypes"],
                          top_run=True)
    levels = [0] * (c["n_runs"] - 1) + [MAX_LEVEL]
    kw = cases.model_kwargs(c)
    model = lambda r, dd: pu_agg_model(r, c["sg"], drop_delete=dd, **kw)
    cl_rows, _ = fold_changelog(runs, levels, MAX_LEVEL,
                                lambda r: model(r, False))
    assert {r[2] for r in cl_rows} == {I, UB, UA, D}
    dtypes = [np.asarray(v).dtype for v in runs[0]["values"]]
    exp_cl = rows_to_columns(cl_rows, dtypes)
    exp_main = model(runs, True)
    assert exp_main["counters"]["reversed"] >= 50
    metas = write_runs(runs, str(tmp_path), compression="NONE")
    for m, lvl in zip(metas, levels):
        m["level"] = lvl
    with Session(0) as s:
        with _plan(s, metas, c["dtypes"],
                   changelog_producer="full-compaction",
                   max_level=MAX_LEVEL, **cases.plan_kwargs(c)) as plan:
            main, cl = _read_all(plan, changelog=True)
            assert debug_last_pu_emit_kernel() == PU_EMIT_SGA
    _compare(cl, exp_cl, "changelog")
    _compare(main, exp_main, "main")


# ------------------------------------------------------------ unchanged path
def test_plan_without_aggregators_keeps_k_emit_pu_sg(tmp_path):
    runs = cases.case_runs("mixed")
    exp = partial_update_seqgroup_model(runs, cases.SG_IDX)
    metas = write_runs(runs, str(tmp_path), compression="NONE")
    with Session(0) as s:
        with _plan(s, metas, cases.MIXED_DTYPES,
                   merge_engine="partial-update",
                   sequence_groups=cases.named_groups(cases.SG_IDX)) as plan:
            got = _read_all(plan)
            assert debug_last_pu_emit_kernel() == PU_EMIT_SG
    _compare(got, exp, "no aggregators")
