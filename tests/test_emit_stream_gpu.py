"""k_emit_stream, the emit of all-contiguous plans without lookup slots and
without nullable columns: per tile, the per-run slices of every column are
streamed through LDS at the merge's flat slots and permuted from there, no
gather. The shapes are the smallest at which the slot mapping, the tile edges
or the column grouping can go wrong (at most about 30k rows, 9 tiles of 3584).

Every case reads the plan with the streamed kernel and asserts through
debug_last_emit_kernel that it ran (or, where the launcher must fall back,
that k_emit_contig ran), compares every output column with the CPU oracle,
reads the same plan with PMH_EMIT_STREAM=0 and compares byte for byte, and
does all of that at PMH_EMIT_STREAM_BLOCKS = 1, 2 and unset."""

import os

import numpy as np
import pytest

from oracle import merge_dedup, merge_first_row_model
from paimon_amd import Session, MergeReadPlan, file_descs_from_metas
from paimon_amd.datagen import gen_runs_dedup, write_runs
from paimon_amd.reader import (EMIT_CONTIG, EMIT_STREAM,
                               debug_last_emit_kernel)
from tests.lookup_model import lookup_changelog_model

import tests.test_emit_gather_gpu as eg_t
import tests.test_lookup_changelog_gpu as lk_t

pytestmark = pytest.mark.gpu

GRIDS = ("1", "2", None)  # None = variable unset (one block per tile)
TILE_ROWS = 3584
KEY64 = eg_t.KEY64


def _read_both(session, monkeypatch, metas, key_cols, vcols,
               expect=EMIT_STREAM, read=eg_t._read_all, **kw):
    """Yields (grid, result of the default emit), after asserting which
    kernel ran and checking the bytes against PMH_EMIT_STREAM=0 at the same
    grid."""
    for grid in GRIDS:
        eg_t._set(monkeypatch, "PMH_EMIT_STREAM_BLOCKS", grid)
        res = []
        for off, kern in ((None, expect), ("0", EMIT_CONTIG)):
            eg_t._set(monkeypatch, "PMH_EMIT_STREAM", off)
            with MergeReadPlan(session, file_descs_from_metas(metas),
                               key_cols, vcols, **kw) as plan:
                res.append(read(plan))
            assert debug_last_emit_kernel() == kern, (grid, off)
        eg_t._set(monkeypatch, "PMH_EMIT_STREAM", None)
        yield grid, res


def _check(tmp_path, monkeypatch, runs, exp, key_type="int64", **kw):
    metas = write_runs(runs, str(tmp_path), compression="NONE")
    with Session(0) as s:
        for grid, (new, old) in _read_both(
                s, monkeypatch, metas,
                [{"name": "_KEY_k", "type": key_type}],
                eg_t._vcols(runs, key_type), **kw):
            eg_t._same_bytes(new, old, f"grid {grid}")
            eg_t._assert_exp(new, exp, f"grid {grid}")


def _runs(lens, seed, spans=None, delete_frac=0.1, n_vals=2):
    """Sorted runs of the given lengths; run r draws unique keys from
    [0, spans[r]) (default: 1.5 x the total, about 50 % collisions)."""
    rng = np.random.default_rng(seed)
    total = sum(lens)
    seqs = rng.permutation(total).astype(np.int64)
    runs, at = [], 0
    for r, n in enumerate(lens):
        span = spans[r] if spans else max(total * 3 // 2, 16)
        keys = np.sort(rng.choice(span, size=n, replace=False)).astype(
            np.int64)
        kind = np.where(rng.random(n) < delete_frac, 3, 0).astype(np.int8)
        values = [keys.copy()] + [
            rng.integers(-2**31, 2**31, n).astype(np.int32)
            for _ in range(n_vals)]
        runs.append({"key": keys, "seq": seqs[at:at + n], "kind": kind,
                     "values": values})
        at += n
    return runs


def _dedup_check(tmp_path, monkeypatch, runs, **kw):
    r, w = merge_dedup(runs, drop_delete=True)
    _check(tmp_path, monkeypatch, runs, eg_t._expected(runs, r, w), **kw)
    return r, w


class TestTileShapes:
    def test_one_run_one_partial_tile(self, tmp_path, monkeypatch):
        r, _ = _dedup_check(tmp_path, monkeypatch, _runs([100], seed=9800))
        assert 0 < len(r) <= 100

    def test_eight_runs_nine_tiles(self, tmp_path, monkeypatch):
        runs = gen_runs_dedup(8, 3_750, n_value_cols=2, seed=9810,
                              delete_frac=0.1)
        n = sum(len(r["key"]) for r in runs)
        assert 8 * TILE_ROWS < n < 9 * TILE_ROWS  # the last tile is partial
        r, _ = _dedup_check(tmp_path, monkeypatch, runs)
        assert 0.6 * n < len(r) < 0.8 * n  # about half the keys collide

    @pytest.mark.parametrize("lens", [(1792, 1792), (1792, 1793),
                                      (3584, 3584)],
                             ids=["3584", "3585", "7168"])
    def test_totals_at_the_tile_size(self, tmp_path, monkeypatch, lens):
        assert sum(lens) in (TILE_ROWS, TILE_ROWS + 1, 2 * TILE_ROWS)
        _dedup_check(tmp_path, monkeypatch, _runs(list(lens), seed=9820))

    def test_single_row_short_and_long_run(self, tmp_path, monkeypatch):
        # run 0 is one row; run 1 ends inside the first tile (empty slices
        # from there on); run 2 spans three tiles
        runs = _runs([1, 500, 8_000], seed=9830, spans=[12_000, 600, 12_000])
        assert runs[1]["key"][-1] < runs[2]["key"][TILE_ROWS - 501]
        _dedup_check(tmp_path, monkeypatch, runs)


def _all_keys_in_all_runs(n_keys, newest):
    """Eight runs that each hold every key 0 .. n_keys - 1; newest(i) is the
    run with key i's highest sequence number."""
    k = 8
    keys = np.arange(n_keys, dtype=np.int64)
    rng = np.random.default_rng(9840)
    runs = []
    for r in range(k):
        rank = (r - newest(keys) + k - 1) % k  # k - 1 at the newest run
        runs.append({"key": keys.copy(), "seq": rank * n_keys + keys,
                     "kind": np.zeros(n_keys, np.int8),
                     "values": [keys.copy(),
                                rng.integers(-2**31, 2**31, n_keys).astype(
                                    np.int32)]})
    return runs


class TestGroupsAcrossCuts:
    # 8000 merged rows in groups of 8: every tile boundary cuts through a
    # group or right behind one, so winners sit on the extension elements
    @pytest.mark.parametrize("newest", [lambda i: 0 * i + 7, lambda i: i % 8],
                             ids=["last_run", "rotating_run"])
    def test_every_key_in_every_run(self, tmp_path, monkeypatch, newest):
        runs = _all_keys_in_all_runs(1_000, newest)
        r, w = _dedup_check(tmp_path, monkeypatch, runs)
        assert len(r) == 1_000
        assert (np.asarray(r) == newest(np.arange(1_000))).all()


class TestEmptyTiles:
    def test_delete_only_range_longer_than_a_tile(self, tmp_path,
                                                  monkeypatch):
        runs = eg_t._insert_delete_runs(21_000, 6_000, 15_000, seed=9850)
        r, w = merge_dedup(runs, drop_delete=True)
        counts = eg_t._winners_per_tile(runs, r, w)
        assert eg_t._longest_inner_empty_run(counts) >= 3
        _check(tmp_path, monkeypatch, runs, eg_t._expected(runs, r, w))


class TestTypes:
    def test_int32_key_and_value_key(self, tmp_path, monkeypatch):
        runs = _runs([2_000, 3_000, 2_500], seed=9860)
        for run in runs:
            run["key"] = run["key"].astype(np.int32)
            run["values"][0] = run["values"][0].astype(np.int32)
        oruns = [{**run, "key": run["key"].astype(np.int64)} for run in runs]
        r, w = merge_dedup(oruns, drop_delete=True)
        _check(tmp_path, monkeypatch, runs, eg_t._expected(runs, r, w),
               key_type="int32")

    @pytest.mark.parametrize("names,lengths", [
        (["v_i8"], {1: 2, 2: 0, 4: 1, 8: 1}),
        # 4-byte list of 4 + 1 and 8-byte list of 2 + 1: remainder groups
        (["v_i8", "v_i16", "v_i32", "v_j32", "v_i64", "v_f", "v_d", "v_d9",
          "v_b"], {1: 3, 2: 1, 4: 5, 8: 3}),
    ], ids=["one_value", "nine_values"])
    def test_narrow_outputs(self, tmp_path, monkeypatch, names, lengths):
        runs = eg_t._typed_runs(3, 4_000, seed=9870, key_dtype=np.int32)
        metas = eg_t._write_typed(runs, str(tmp_path))
        oruns = [{**run, "key": run["key"].astype(np.int64)} for run in runs]
        r, w = merge_dedup(oruns, drop_delete=True)
        assert eg_t._list_lengths(names, key_bytes=4) == lengths
        with Session(0) as s:
            for grid, (new, old) in _read_both(
                    s, monkeypatch, metas,
                    [{"name": "_KEY_k", "type": "int32"}],
                    eg_t._plan_cols(names)):
                eg_t._same_bytes(new, old, f"grid {grid}")
                eg_t._assert_typed(new, runs, r, w, names, f"grid {grid}")


class TestFallbacks:
    def test_nullable_column_takes_the_gather(self, tmp_path, monkeypatch):
        # validity is not streamed: runs 0 and 2 hold nulls, run 1 stages no
        # validity array, and the launcher keeps k_emit_contig
        rng = np.random.default_rng(9880)
        runs = eg_t._typed_runs(3, 5_000, seed=9880)
        names = ["v_i8", "v_i32", "v_i64"]
        nulls = {i: {nm: rng.random(5_000) < 0.3 for nm in names}
                 for i in (0, 2)}
        metas = eg_t._write_typed(runs, str(tmp_path), nulls)
        r, w = merge_dedup(runs, drop_delete=True)
        with Session(0) as s:
            for grid, (new, old) in _read_both(
                    s, monkeypatch, metas, KEY64, eg_t._plan_cols(names),
                    expect=EMIT_CONTIG):
                eg_t._same_bytes(new, old, f"grid {grid}")
                eg_t._assert_typed(new, runs, r, w, names, f"grid {grid}",
                                   nulls)

    def test_lookup_changelog_takes_the_gather(self, tmp_path, monkeypatch):
        # a lookup winner may name a slot outside the tile's slices
        runs = lk_t._level0_runs(seed=9890, n_runs=3, rows=6_000)
        rng = np.random.default_rng(9890)
        lookup = lk_t._two_lookup_levels(rng, lk_t._keyspace(runs),
                                         n3=3_000, n5=2_000)
        lookup_runs = [run for _, run, _ in lookup]
        n_vals = len(runs[0]["values"])
        exp_cl, exp_res = lookup_changelog_model(
            runs, [0, 0, 0], lookup_runs, row_dedup=False, drop_delete=True,
            masks=None, lookup_masks=None)
        sources = list(runs) + lookup_runs
        metas = write_runs(runs, os.path.join(str(tmp_path), "merge"),
                           compression="NONE")
        for m in metas:
            m["level"] = 0
        lookup_descs = lk_t._write_lookup(tmp_path, lookup)
        with Session(0) as s:
            for grid, (new, old) in _read_both(
                    s, monkeypatch, metas, lk_t._key_cols(),
                    lk_t._value_cols(n_vals - 1), expect=EMIT_CONTIG,
                    read=lambda plan: lk_t._read_all(plan)[:2],
                    changelog_producer="lookup", lookup_files=lookup_descs):
                eg_t._same_bytes(new[0], old[0], f"grid {grid} main")
                eg_t._same_bytes(new[1], old[1], f"grid {grid} changelog")
                lk_t._assert_stream(new[0], sources, exp_res, n_vals,
                                    f"grid {grid} main")
                lk_t._assert_stream(new[1], sources,
                                    [(a, b) for a, b, _ in exp_cl], n_vals,
                                    f"grid {grid} changelog",
                                    kinds=[kd for _, _, kd in exp_cl])


class TestOtherEngines:
    def test_first_row_insert_only(self, tmp_path, monkeypatch):
        runs = gen_runs_dedup(6, 4_000, n_value_cols=2, seed=9900,
                              delete_frac=0.0)
        r, w = merge_first_row_model(runs)
        _check(tmp_path, monkeypatch, runs, eg_t._expected(runs, r, w),
               merge_engine="first-row")
