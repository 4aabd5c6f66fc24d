"""The host side of one read (pmh_read_next): which stage interval feeds which
pmh_stats field on every path through it, and that a plan whose read was
refused can be read again and leaves the process usable.

Shape: tests/column_cases.py (3 runs x 2 500 rows, three tiles, the last one
ragged); the hierarchical variant is one section of 33 runs x 300 rows.

Stage times. The six stage fields are the intervals between seven events
recorded back to back on the plan's stream, and total_device_ms is the
interval from the first to the last of them, so the fields sum to the total
up to the rounding of the event timestamps. SUM_TOL_MS is ten times the
largest |sum - total| this test measured on the commit before the read path
was restructured (1.481e-7 ms over the eight variants, profiles/read_path.md).
The bound is absolute while float32 rounding grows with the intervals, so the
module first runs one small read that loads the library's code objects: the
measured reads then take fractions of a millisecond whichever variant runs
first. The hierarchical variant also checks that its one section held all 33
runs (a section of more than 32 runs merges hierarchically) and that its row
count is the oracle's.

Refusal, then reuse: the first-row engine refuses a DELETE at read time; the
refusal repeats after reset(), and a deduplicate plan over the same files in
the same process then reads what the oracle computes."""

import numpy as np
import pytest

from oracle import merge_dedup
from paimon_amd import Session, MergeReadPlan, file_descs_from_metas
from paimon_amd.datagen import gen_runs_dedup, write_runs

import tests.column_cases as cc

pytestmark = pytest.mark.gpu

STAGES = ("decode_ms", "partition_ms", "lookup_ms", "merge_ms", "scan_ms",
          "emit_ms")
SUM_TOL_MS = 1.481e-6
MAX_LEVEL = 5
CHAIN, FUSED, FUSED_SPLIT = 0, 1, 2  # pmh_stats.path_mode


HIER_RUNS, HIER_ROWS = 33, 300


def _hier_runs():
    return gen_runs_dedup(HIER_RUNS, HIER_ROWS, n_value_cols=2, seed=7103,
                          delete_frac=0.1)


@pytest.fixture(scope="module", autouse=True)
def _warm_process(tmp_path_factory):
    """One read before any measured one: the first launches of a process
    load the code objects and take milliseconds."""
    with Session(0) as s:
        with _cc_plan(s, tmp_path_factory.mktemp("warm")) as plan:
            assert plan.read_next() is not None


def _hier_plan(s, tmp_path):
    runs = _hier_runs()
    metas = write_runs(runs, str(tmp_path), compression="NONE")
    return MergeReadPlan(
        s, file_descs_from_metas(metas), cc.KEY_COLS,
        [{"name": "v_k", "type": "int64"}] +
        [{"name": f"v_c{i}", "type": "int32"} for i in range(2)])


def _cc_plan(s, tmp_path, gen_kw=None, levels=None, n_lookup=0, **plan_kw):
    """A plan over the column_cases shape; the last n_lookup runs become
    lookup levels (level 3, 4, ...) of a lookup-changelog plan."""
    runs = cc.gen(7101, **(gen_kw or {}))
    if n_lookup:
        levels = [0] * (cc.N_RUNS - n_lookup) + \
            [3 + i for i in range(n_lookup)]
    descs = file_descs_from_metas(cc.write(runs, str(tmp_path), levels))
    if n_lookup:
        plan_kw["lookup_files"] = descs[-n_lookup:]
        descs = descs[:-n_lookup]
    return MergeReadPlan(s, descs, cc.KEY_COLS, cc.VALUE_COLS, **plan_kw)


# name -> (environment, plan factory, path_mode)
VARIANTS = {
    "chain": ({}, lambda s, d: _cc_plan(s, d, {"nulls": False}), CHAIN),
    "nullable": ({}, lambda s, d: _cc_plan(s, d), CHAIN),
    "fused": ({"PMH_FUSED": "1"},
              lambda s, d: _cc_plan(s, d, {"nulls": False}), FUSED_SPLIT),
    "fused_in_kernel": ({"PMH_FUSED": "1", "PMH_FSPLIT": "0"},
                        lambda s, d: _cc_plan(s, d, {"nulls": False}), FUSED),
    "partial_update": ({}, lambda s, d: _cc_plan(
        s, d, merge_engine="partial-update"), CHAIN),
    "aggregation_changelog": ({}, lambda s, d: _cc_plan(
        s, d, {"top": True}, levels=[0] * (cc.N_RUNS - 1) + [MAX_LEVEL],
        merge_engine="aggregation", changelog_producer="full-compaction",
        max_level=MAX_LEVEL), CHAIN),
    "lookup_changelog": ({}, lambda s, d: _cc_plan(
        s, d, n_lookup=1, changelog_producer="lookup"), CHAIN),
    "hierarchical": ({}, _hier_plan, CHAIN),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_stage_times(tmp_path, monkeypatch, name):
    env, make, path_mode = VARIANTS[name]
    for var in ("PMH_FUSED", "PMH_FSPLIT"):
        monkeypatch.delenv(var, raising=False)
    for var, val in env.items():
        monkeypatch.setenv(var, val)
    with Session(0) as s:
        with make(s, tmp_path) as plan:
            assert plan.read_next() is not None
            st = plan.stats()
    total = st["total_device_ms"]
    gap = abs(sum(st[f] for f in STAGES) - total)
    print(f"stage_times[{name}]: " +
          " ".join(f"{f}={st[f]:.6f}" for f in STAGES) +
          f" total={total:.6f} |sum-total|={gap:.3e}")
    for f in STAGES:
        assert st[f] >= 0, (name, f, st[f])
    assert total > 0, name
    assert st["path_mode"] == path_mode, name
    assert gap <= SUM_TOL_MS, (name, gap)
    if name == "hierarchical":
        assert st["rows_in"] == HIER_RUNS * HIER_ROWS, st["rows_in"]
        r, _ = merge_dedup(_hier_runs(), drop_delete=True)
        assert st["rows_out"] == len(r), (st["rows_out"], len(r))


def test_refusal_then_reuse(tmp_path):
    runs = cc.gen(7102, kinds=(0, 3), kind_p=[0.9, 0.1])
    assert any((r["kind"] == 3).any() for r in runs)
    files = file_descs_from_metas(cc.write(runs, str(tmp_path)))
    refusal = "first-row merge engine cannot accept DELETE/UPDATE_BEFORE"
    with Session(0) as s:
        with MergeReadPlan(s, files, cc.KEY_COLS, cc.VALUE_COLS,
                           merge_engine="first-row") as plan:
            with pytest.raises(RuntimeError, match=refusal):
                plan.read_next()
            plan.reset()
            with pytest.raises(RuntimeError, match=refusal):
                plan.read_next()
        with MergeReadPlan(s, files, cc.KEY_COLS, cc.VALUE_COLS) as plan:
            got = cc.read_all(plan)
    r, w = merge_dedup(runs, drop_delete=True)
    cc.check(got, cc.gather(runs, r, w), "deduplicate after a refused read")
