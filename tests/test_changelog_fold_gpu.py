"""Full-compaction changelog of the folding engines (partial-update,
aggregation) on the GPU: the changelog walk of the PU k_merge_tiles +
k_cl_finalize_out + k_cl_emit_out against the sequential wrapper port of
tests/changelog_fold_model.py (pinned in tests/test_changelog_fold_cpu.py),
whose merged rows come from the oracle's engine models.

Shape: 4 level-0 runs of 5 000 rows + one max-level run of 3 000 rows, keys
dense in 7 500 — about 23k records in 7 tiles of 3 584, the smallest shape
where groups straddle tile cuts, a tile's kept-group count differs from its
changelog-row count and an after-type row needs tile_offsets to reach its
main-output row.

Every changelog column is compared: key, sequence number, kind, validity,
and the stored bits of every non-null value (a null field's bits mean
nothing: a before-type row carries whatever the decoder left there). The
main batch is compared with the engine model the same way.

Kinds a case must produce (checked on the expected stream, so a seed that
exercises nothing fails): INSERT, UPDATE_BEFORE, UPDATE_AFTER everywhere a
top-level run exists, and DELETE where the engine can return a retract for a
multi-record group — remove-record-on-delete and sequence groups. Plain
partial-update and aggregation (with or without retract-capable aggregators)
always fold to an INSERT, so DELETE(top) cannot occur there."""

import numpy as np
import pytest

from oracle import (aggregation_model, aggregation_retract_model,
                    aggregation_rrod_model, partial_update_model,
                    partial_update_rrod_model, partial_update_seqgroup_model)
from paimon_amd import Session, MergeReadPlan, file_descs_from_metas
from paimon_amd.datagen import write_runs
from tests.changelog_fold_model import fold_changelog, rows_to_columns

import tests.column_cases as cc

pytestmark = pytest.mark.gpu

KEY_COLS = [{"name": "_KEY_k", "type": "int64"}]
MAX_LEVEL = 5
I, UB, UA, D = 0, 1, 2, 3
N_LEVEL0, ROWS_LEVEL0, ROWS_TOP, KEYSPACE = 4, 5_000, 3_000, 7_500
TYPE_NAMES = {"int32": "int32", "int64": "int64", "float64": "float64"}


def _gen(seed, col_dtypes, kinds=(I,), kind_p=None, card=4, null_frac=0.35,
         with_top=True, top_first=False, n_level0=N_LEVEL0,
         top_retract_frac=0.0):
    """Level-0 runs (kinds drawn from `kinds`) + one max-level run holding
    the oldest sequence numbers: INSERTs, but for top_retract_frac DELETEs.
    values[0] = v_k (the key, never null); values[1 + c] has col_dtypes[c],
    `card` distinct values."""
    rng = np.random.default_rng(seed)
    seqs = ROWS_TOP + rng.permutation(n_level0 * ROWS_LEVEL0).astype(np.int64)

    def one(rows, seq, kind):
        key = np.sort(rng.choice(KEYSPACE, rows, replace=False)
                      ).astype(np.int64)
        vals, msks = [key.copy()], [np.ones(rows, bool)]
        for dt in col_dtypes:
            v = rng.integers(0, card, rows)
            vals.append((v * 0.5 - 1.0).astype(dt) if dt == "float64"
                        else v.astype(dt))
            msks.append(rng.random(rows) >= null_frac)
        return {"key": key, "seq": seq, "kind": kind, "values": vals,
                "valid": msks}

    runs = [one(ROWS_LEVEL0, seqs[r * ROWS_LEVEL0:(r + 1) * ROWS_LEVEL0],
                rng.choice(kinds, ROWS_LEVEL0, p=kind_p).astype(np.int8))
            for r in range(n_level0)]
    levels = [0] * n_level0
    if with_top:
        top = one(ROWS_TOP, np.arange(ROWS_TOP, dtype=np.int64),
                  np.where(rng.random(ROWS_TOP) < top_retract_frac, D, I
                           ).astype(np.int8))
        if top_first:
            runs, levels = [top] + runs, [MAX_LEVEL] + levels
        else:
            runs, levels = runs + [top], levels + [MAX_LEVEL]
    return runs, levels


def _value_cols(col_dtypes):
    return ([{"name": "v_k", "type": "int64"}] +
            [{"name": f"v_c{i}", "type": TYPE_NAMES[dt]}
             for i, dt in enumerate(col_dtypes)])


def _read_all(plan):
    main, cl = [], []
    while True:
        b = plan.read_next()
        if b is None:
            break
        main.append({k: v.copy() for k, v in b.items()})
        cl.append({k: v.copy() for k, v in plan.read_changelog().items()})
    cat = lambda parts: {k: np.concatenate([p[k] for p in parts])
                         for k in parts[0]} if parts else {}
    return cat(main), cat(cl)


def _compare(got, exp, what):
    n = len(exp["key"])
    assert len(got["_KEY_k"]) == n, (what, len(got["_KEY_k"]), n)
    assert (got["_KEY_k"] == exp["key"]).all(), what
    assert (got["_SEQUENCE_NUMBER"] == exp["seq"]).all(), what
    assert (got["_VALUE_KIND"] == exp["kind"]).all(), what
    names = ["v_k"] + [f"v_c{i}" for i in range(len(exp["values"]) - 1)]
    for c, nm in enumerate(names):
        ev, em = exp["values"][c], exp["valid"][c]
        gm = got.get(nm + "#valid")
        if gm is None:
            gm = np.ones(n, dtype=bool)
        assert (gm.astype(bool) == em).all(), (what, nm)
        assert got[nm].dtype == ev.dtype, (what, nm)
        assert got[nm][em].tobytes() == ev[em].tobytes(), (what, nm)


def _expected(runs, levels, model, row_dedup, drop_delete):
    cl, _ = fold_changelog(runs, levels, MAX_LEVEL,
                           lambda r: model(r, False), row_dedup=row_dedup)
    dtypes = [np.asarray(v).dtype for v in runs[0]["values"]]
    return cl, rows_to_columns(cl, dtypes), model(runs, drop_delete)


def _run_case(tmp_path, runs, levels, col_dtypes, model, plan_kw,
              require=(I, UB, UA), row_dedup=False, drop_delete=True,
              metas_hook=None, expected_runs=None):
    """model(runs, drop_delete) -> the engine model's output dict.
    expected_runs: the runs the merge sees (deletion vectors applied)."""
    cl_rows, exp_cl, exp_main = _expected(
        runs if expected_runs is None else expected_runs, levels, model,
        row_dedup, drop_delete)
    kinds = {r[2] for r in cl_rows}
    assert kinds == set(require), (sorted(kinds), require)
    metas = write_runs(runs, str(tmp_path), compression="NONE")
    for m, lvl in zip(metas, levels):
        m["level"] = lvl
    if metas_hook:
        metas_hook(metas)
    with Session(0) as s:
        with MergeReadPlan(s, file_descs_from_metas(metas), KEY_COLS,
                           _value_cols(col_dtypes),
                           changelog_producer="full-compaction",
                           changelog_row_dedup=row_dedup,
                           max_level=MAX_LEVEL, drop_delete=drop_delete,
                           **plan_kw) as plan:
            main, cl = _read_all(plan)
    _compare(cl, exp_cl, "changelog")
    _compare(main, exp_main, "main")
    return cl_rows


def _pu(runs, drop_delete):
    return partial_update_model(runs, drop_delete=drop_delete)


def _pu_rrod(runs, drop_delete):
    return partial_update_rrod_model(runs, drop_delete=drop_delete)


PU_KW = {"merge_engine": "partial-update"}
INT3 = ["int32"] * 3


class TestPartialUpdate:
    def test_row_dedup_twins(self, tmp_path):
        runs, levels = _gen(1101, INT3)
        plain = _run_case(tmp_path / "a", runs, levels, INT3, _pu, PU_KW)
        dedup = _run_case(tmp_path / "b", runs, levels, INT3, _pu, PU_KW,
                          row_dedup=True)
        # every suppressed pair is two rows
        assert len(dedup) < len(plain)
        assert (len(plain) - len(dedup)) % 2 == 0

    @pytest.mark.parametrize("drop_delete", [True, False])
    def test_remove_record_on_delete(self, tmp_path, drop_delete):
        runs, levels = _gen(1102, INT3, kinds=(I, D), kind_p=[0.8, 0.2])
        _run_case(tmp_path, runs, levels, INT3, _pu_rrod,
                  dict(PU_KW, remove_record_on_delete=True),
                  require=(I, UB, UA, D), drop_delete=drop_delete)

    def test_sequence_groups_with_retracts(self, tmp_path):
        # indices into the runs' values lists (values[0] = v_k)
        sg_idx = [{"sequence_fields": [1], "group_fields": [2, 3]},
                  {"sequence_fields": [4, 5], "group_fields": [6]}]
        sg_named = [{"sequence_fields": ["v_c0"],
                     "group_fields": ["v_c1", "v_c2"]},
                    {"sequence_fields": ["v_c3", "v_c4"],
                     "group_fields": ["v_c5"]}]
        dts = ["int32"] * 6
        # the result is a DELETE only for a group without any add member, so
        # DELETE(top) needs a top-level record that is itself a retract (a
        # max-level file written with deletes kept)
        runs, levels = _gen(1103, dts, kinds=(I, UA, UB, D),
                            kind_p=[0.55, 0.1, 0.15, 0.2], card=50,
                            top_retract_frac=0.15)
        _run_case(tmp_path, runs, levels, dts,
                  lambda r, dd: partial_update_seqgroup_model(
                      r, sg_idx, drop_delete=dd),
                  dict(PU_KW, sequence_groups=sg_named),
                  require=(I, UB, UA, D))

    def test_no_top_level_run(self, tmp_path):
        runs, levels = _gen(1104, INT3, with_top=False)
        rows = _run_case(tmp_path, runs, [0, 0, 1, 1], INT3, _pu, PU_KW,
                         require=(I,))
        assert len(rows) > 0

    def test_top_run_first(self, tmp_path):
        runs, levels = _gen(1105, INT3, top_first=True)
        assert levels[0] == MAX_LEVEL
        _run_case(tmp_path, runs, levels, INT3, _pu, PU_KW)

    def test_deletion_vector_on_top_run(self, tmp_path):
        # tombstoned rows never reach the wrapper: a deleted top-level record
        # means "no top" for its group
        from scripts.gen_dv_golden import serialize_roaring32, wrap_dv
        rng = np.random.default_rng(1106)
        runs, levels = _gen(1106, INT3)
        top = len(runs) - 1
        dels = {top: sorted(rng.choice(ROWS_TOP, ROWS_TOP // 5,
                                       replace=False).tolist()),
                0: sorted(rng.choice(ROWS_LEVEL0, ROWS_LEVEL0 // 10,
                                     replace=False).tolist())}

        def hook(metas):
            blob = b""
            for fi, pos in dels.items():
                ser = wrap_dv(serialize_roaring32(pos))
                metas[fi]["deletionVector"] = {
                    "file": str(tmp_path / "index.dv"),
                    "offset": len(blob), "length": len(ser)}
                blob += ser
            (tmp_path / "index.dv").write_bytes(blob)

        fruns = []
        for i, r in enumerate(runs):
            keep = np.ones(len(r["key"]), dtype=bool)
            if i in dels:
                keep[np.array(dels[i], dtype=np.int64)] = False
            fruns.append({"key": r["key"][keep], "seq": r["seq"][keep],
                          "kind": r["kind"][keep],
                          "values": [v[keep] for v in r["values"]],
                          "valid": [v[keep] for v in r["valid"]]})
        _run_case(tmp_path, runs, levels, INT3, _pu, PU_KW, metas_hook=hook,
                  expected_runs=fruns)

    def test_single_run_section(self, tmp_path):
        # every group is a singleton: INSERT rows for the adds, nothing for
        # the lone DELETEs
        runs, levels = _gen(1107, INT3, kinds=(I, D), kind_p=[0.8, 0.2],
                            with_top=False, n_level0=1)
        rows = _run_case(tmp_path, runs, levels, INT3, _pu_rrod,
                         dict(PU_KW, remove_record_on_delete=True),
                         require=(I,))
        assert len(rows) == int((runs[0]["kind"] == I).sum())

    def test_ignore_delete_refused(self, tmp_path):
        runs, levels = _gen(1108, INT3, n_level0=1)
        metas = write_runs(runs, str(tmp_path), compression="NONE")
        with Session(0) as s:
            with pytest.raises(RuntimeError, match="ignore_delete"):
                MergeReadPlan(s, file_descs_from_metas(metas), KEY_COLS,
                              _value_cols(INT3),
                              changelog_producer="full-compaction",
                              max_level=MAX_LEVEL, ignore_delete=True,
                              **PU_KW)

    def test_lookup_still_refused(self, tmp_path):
        runs, levels = _gen(1109, INT3, n_level0=1)
        metas = write_runs(runs, str(tmp_path), compression="NONE")
        with Session(0) as s:
            with pytest.raises(RuntimeError,
                               match="lookup is supported for the "
                                     "deduplicate engine"):
                MergeReadPlan(s, file_descs_from_metas(metas), KEY_COLS,
                              _value_cols(INT3), changelog_producer="lookup",
                              **PU_KW)


AGG_KW = {"merge_engine": "aggregation"}


class TestAggregation:
    def test_sum_max_last_non_null(self, tmp_path):
        dts = ["int32", "int64", "float64"]
        aggs = ["last_non_null_value", "sum", "max", "last_non_null_value"]
        runs, levels = _gen(1201, dts)
        plain = _run_case(
            tmp_path / "a", runs, levels, dts,
            lambda r, dd: aggregation_model(r, aggs, drop_delete=dd),
            dict(AGG_KW, aggregations={"v_c0": "sum", "v_c1": "max",
                                       "v_c2": "last_non_null_value"}))
        dedup = _run_case(
            tmp_path / "b", runs, levels, dts,
            lambda r, dd: aggregation_model(r, aggs, drop_delete=dd),
            dict(AGG_KW, aggregations={"v_c0": "sum", "v_c1": "max",
                                       "v_c2": "last_non_null_value"}),
            row_dedup=True)
        assert len(dedup) < len(plain)

    def test_sum_retracts(self, tmp_path):
        aggs = ["primary_key", "sum", "sum", "sum"]
        runs, levels = _gen(1202, INT3, kinds=(I, UA, UB, D),
                            kind_p=[0.5, 0.15, 0.15, 0.2], card=1000)
        _run_case(tmp_path, runs, levels, INT3,
                  lambda r, dd: aggregation_retract_model(r, aggs,
                                                          drop_delete=dd),
                  dict(AGG_KW, aggregations={"v_k": "primary_key",
                                             "v_c0": "sum", "v_c1": "sum",
                                             "v_c2": "sum"}))

    def test_remove_record_on_delete(self, tmp_path):
        aggs = ["last_non_null_value", "sum", "max", "last_non_null_value"]
        runs, levels = _gen(1203, INT3, kinds=(I, D), kind_p=[0.8, 0.2])
        _run_case(tmp_path, runs, levels, INT3,
                  lambda r, dd: aggregation_rrod_model(r, aggs,
                                                       drop_delete=dd),
                  dict(AGG_KW, remove_record_on_delete=True,
                       aggregations={"v_c0": "sum", "v_c1": "max",
                                     "v_c2": "last_non_null_value"}),
                  require=(I, UB, UA, D))


class TestColumnDtypes:
    """Every column dtype, without nulls and (one column per output width)
    with them, through k_cl_finalize_out / k_cl_emit_out behind k_emit_pu:
    before-type rows from the source columns, after-type rows from the main
    output, at the default emit grid and at seven blocks. Shape and columns:
    tests/column_cases.py."""

    def test_partial_update_changelog(self, tmp_path, monkeypatch):
        runs = cc.gen(641, top=True)
        levels = [0] * (cc.N_RUNS - 1) + [MAX_LEVEL]
        metas = cc.write(runs, str(tmp_path), levels)
        cl_rows, exp_cl, exp_main = _expected(runs, levels, _pu, False, True)
        assert {r[2] for r in cl_rows} == {I, UB, UA}
        for blocks in cc.EMIT_BLOCKS:
            monkeypatch.delenv("PMH_EMIT_BLOCKS", raising=False)
            if blocks:
                monkeypatch.setenv("PMH_EMIT_BLOCKS", blocks)
            with Session(0) as s:
                with MergeReadPlan(s, file_descs_from_metas(metas),
                                   cc.KEY_COLS, cc.VALUE_COLS,
                                   changelog_producer="full-compaction",
                                   max_level=MAX_LEVEL, **PU_KW) as plan:
                    main, cl = cc.read_all(plan, changelog=True)
            cc.check(cl, exp_cl, f"changelog, blocks {blocks}", dicts=main)
            cc.check(main, exp_main, f"main, blocks {blocks}")
