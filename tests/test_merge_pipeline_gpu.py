"""k_merge_tiles staging pipeline: a block that owns several tiles prefetches
tile t + grid while it merges tile t. The other GPU tests use inputs so small
that every tile gets its own block, so they never take that path; here
PMH_MERGE_BLOCKS forces grids of 1, 2 and 3 blocks over inputs of 7-10 tiles
(about 25-36k rows), and every result is compared with the CPU oracle. The
default grid (variable unset) runs the same inputs, so it is pinned to the
same bytes as every forced grid."""

import numpy as np
import pytest

from oracle import merge_dedup, merge_first_row_model
from paimon_amd import Session, MergeReadPlan, file_descs_from_metas
from paimon_amd.datagen import (gen_runs_dedup, gen_runs_partial_update,
                                write_runs)

import tests.test_agg_gpu as agg_t
import tests.test_changelog_gpu as cl_t
import tests.test_dv_gpu as dv_t
import tests.test_lookup_changelog_gpu as lk_t
import tests.test_pu_gpu as pu_t

pytestmark = pytest.mark.gpu

GRIDS = ("1", "2", "3", None)  # None = variable unset (default grid)
TILE_ROWS = 3584
TOTAL_ROWS = 30_000  # 9 tiles: the last one partial, 9 % 2 != 0


def _set_grid(monkeypatch, grid):
    if grid is None:
        monkeypatch.delenv("PMH_MERGE_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("PMH_MERGE_BLOCKS", grid)


def _read_all(plan):
    got = {}
    while True:
        b = plan.read_next()
        if b is None:
            break
        for k, v in b.items():
            got.setdefault(k, []).append(v.copy())
    return {k: np.concatenate(v) for k, v in got.items()}


def _expected(runs, r, w):
    exp = {"_KEY_k": np.array([runs[a]["key"][b] for a, b in zip(r, w)]),
           "_SEQUENCE_NUMBER": np.array([runs[a]["seq"][b]
                                         for a, b in zip(r, w)], np.int64),
           "_VALUE_KIND": np.array([runs[a]["kind"][b]
                                    for a, b in zip(r, w)], np.int8)}
    names = ["v_k"] + [f"v_c{i}" for i in range(len(runs[0]["values"]) - 1)]
    for c, nm in enumerate(names):
        exp[nm] = np.array([runs[a]["values"][c][b] for a, b in zip(r, w)])
    return exp


def _check_grids(tmp_path, monkeypatch, runs, exp, key_type="int64", **kw):
    """One set of files and one expectation; one plan per grid."""
    n_rows = sum(len(r["key"]) for r in runs)
    assert 6 * TILE_ROWS < n_rows <= 10 * TILE_ROWS + TILE_ROWS // 2
    metas = write_runs(runs, str(tmp_path), compression="NONE")
    vt = "int32" if key_type == "int32" else "int64"
    vcols = ([{"name": "v_k", "type": vt}] +
             [{"name": f"v_c{i}", "type": "int32"}
              for i in range(len(runs[0]["values"]) - 1)])
    with Session(0) as s:
        for grid in GRIDS:
            _set_grid(monkeypatch, grid)
            with MergeReadPlan(s, file_descs_from_metas(metas),
                               [{"name": "_KEY_k", "type": key_type}], vcols,
                               **kw) as plan:
                got = _read_all(plan)
            for name, e in exp.items():
                g = got[name]
                assert len(g) == len(e), (grid, name, len(g), len(e))
                assert (g == e).all(), \
                    f"grid {grid} column {name}: {np.flatnonzero(g != e)[:8]}"


def _dedup_exp(runs, **kw):
    r, w = merge_dedup(runs, **kw)
    return _expected(runs, r, w)


class TestDedupGrids:
    @pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 9, 17, 32])
    def test_run_counts(self, tmp_path, monkeypatch, k):
        # every template run bound (4/8/16/32), full and partial
        runs = gen_runs_dedup(k, TOTAL_ROWS // k, n_value_cols=1,
                              seed=7000 + k, delete_frac=0.1)
        n = sum(len(r["key"]) for r in runs)
        assert n % TILE_ROWS != 0  # a short last tile
        _check_grids(tmp_path, monkeypatch, runs, _dedup_exp(runs))

    def test_unequal_runs(self, tmp_path, monkeypatch):
        # a 1-row run, a run exhausted in the first tiles, two long ones:
        # zero-length segments and segments without an "extra" element
        rng = np.random.default_rng(7100)
        lens = [1, 2_500, 14_000, 13_000]
        seqs = rng.permutation(sum(lens)).astype(np.int64)
        runs, off = [], 0
        for i, n in enumerate(lens):
            space = 4_000 if i == 1 else 40_000  # run 1: low keys only
            keys = np.sort(rng.choice(space, n, replace=False)).astype(
                np.int64)
            runs.append({"key": keys, "seq": seqs[off:off + n],
                         "kind": rng.choice([0, 3], n, p=[.8, .2]).astype(
                             np.int8),
                         "values": [keys.copy(),
                                    rng.integers(-2**31, 2**31, n).astype(
                                        np.int32)]})
            off += n
        _check_grids(tmp_path, monkeypatch, runs, _dedup_exp(runs))

    def test_identical_key_sets(self, tmp_path, monkeypatch):
        # every group has one member per run and spans every cut, so each
        # tile's predecessor key decides its first head
        rng = np.random.default_rng(7200)
        k, n = 6, 5_000
        keys = np.sort(rng.choice(50_000, n, replace=False)).astype(np.int64)
        seqs = rng.permutation(k * n).astype(np.int64)
        runs = [{"key": keys.copy(), "seq": seqs[i * n:(i + 1) * n],
                 "kind": rng.choice([0, 3], n, p=[.7, .3]).astype(np.int8),
                 "values": [keys.copy(),
                            rng.integers(-2**31, 2**31, n).astype(np.int32)]}
                for i in range(k)]
        _check_grids(tmp_path, monkeypatch, runs, _dedup_exp(runs))

    def test_int32_keys(self, tmp_path, monkeypatch):
        runs = gen_runs_dedup(5, 6_000, n_value_cols=1, seed=7300,
                              delete_frac=0.1)
        for r in runs:
            r["key"] = r["key"].astype(np.int32)
            r["values"][0] = r["values"][0].astype(np.int32)
        oruns = [{**r, "key": r["key"].astype(np.int64)} for r in runs]
        r_, w_ = merge_dedup(oruns, drop_delete=True)
        exp = _expected(runs, r_, w_)
        _check_grids(tmp_path, monkeypatch, runs, exp, key_type="int32")

    @pytest.mark.parametrize("mode", ["drop", "keep", "ignore"])
    def test_deletes(self, tmp_path, monkeypatch, mode):
        runs = gen_runs_dedup(4, 7_500, n_value_cols=1, seed=7400,
                              delete_frac=0.35)
        kw = {"drop": {"drop_delete": True}, "keep": {"drop_delete": False},
              "ignore": {"ignore_delete": True, "drop_delete": True}}[mode]
        _check_grids(tmp_path, monkeypatch, runs, _dedup_exp(runs, **kw),
                     **kw)

    def test_first_row(self, tmp_path, monkeypatch):
        runs = gen_runs_dedup(6, 5_000, n_value_cols=1, seed=7500,
                              delete_frac=0.0)
        r, w = merge_first_row_model(runs)
        _check_grids(tmp_path, monkeypatch, runs, _expected(runs, r, w),
                     merge_engine="first-row")


class TestOtherModesGrids:
    """The modes that share the staging code, through the existing cases'
    own oracle comparisons, once per grid."""

    @staticmethod
    def _each_grid(tmp_path, monkeypatch):
        for grid in GRIDS:
            _set_grid(monkeypatch, grid)
            d = tmp_path / f"grid_{grid}"
            d.mkdir()
            yield d

    def test_partial_update(self, tmp_path, monkeypatch):
        runs = gen_runs_partial_update(4, 7_500, n_value_cols=4, seed=7600,
                                       update_frac=0.4, update_cols=3)
        for d in self._each_grid(tmp_path, monkeypatch):
            pu_t.TestPartialUpdate()._run(d, runs)

    def test_aggregation(self, tmp_path, monkeypatch):
        runs = gen_runs_partial_update(4, 7_500, n_value_cols=3, seed=7700,
                                       update_frac=0.4, update_cols=2)
        for r in runs:  # bound so int32 sums cannot overflow
            for c in range(1, 4):
                r["values"][c] = (r["values"][c] % 10_000).astype(np.int32)
        aggs = {"v_c0": "sum", "v_c1": "max"}
        for d in self._each_grid(tmp_path, monkeypatch):
            agg_t.TestAggregationEngine()._run(d, runs, aggs)

    def test_deletion_vector(self, tmp_path, monkeypatch):
        rng = np.random.default_rng(7800)
        runs = gen_runs_dedup(5, 6_000, n_value_cols=1, seed=7800,
                              delete_frac=0.1)
        dels = {0: sorted(rng.choice(6_000, 900, replace=False).tolist()),
                3: list(range(0, 6_000, 7))}
        fruns = dv_t._filter_runs(runs, dels)
        r, w = merge_dedup(fruns, drop_delete=True)
        exp = _expected(fruns, r, w)
        for d in self._each_grid(tmp_path, monkeypatch):
            metas = write_runs(runs, str(d), compression="NONE")
            metas = dv_t._attach_dvs(metas, dels, d)
            with Session(0) as s:
                with MergeReadPlan(s, file_descs_from_metas(metas),
                                   [{"name": "_KEY_k", "type": "int64"}],
                                   [{"name": "v_k", "type": "int64"},
                                    {"name": "v_c0", "type": "int32"}]
                                   ) as plan:
                    got = _read_all(plan)
            for name, e in exp.items():
                assert len(got[name]) == len(e), (d.name, name)
                assert (got[name] == e).all(), (d.name, name)

    def test_full_compaction_changelog(self, tmp_path, monkeypatch):
        runs, levels = cl_t._with_top_run(3, 8_000, seed=7900)
        for d in self._each_grid(tmp_path, monkeypatch):
            cl_t._run_case(d, runs, levels)

    def test_lookup_changelog(self, tmp_path, monkeypatch):
        runs = lk_t._level0_runs(seed=8000, n_runs=3, rows=9_000)
        rng = np.random.default_rng(8000)
        lookup = lk_t._two_lookup_levels(rng, lk_t._keyspace(runs),
                                         n3=4_000, n5=3_000)
        for d in self._each_grid(tmp_path, monkeypatch):
            lk_t._run_case(d, runs, [0, 0, 0], lookup)
