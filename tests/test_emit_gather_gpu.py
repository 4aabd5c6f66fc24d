"""k_emit_contig, the winner gather of all-contiguous plans: descriptors and
a window of tile offsets staged in LDS, columns ordered into lists by output
width and gathered in groups. The other GPU tests run it at its default grid
only; here PMH_EMIT_BLOCKS forces 1, 2 and 3 blocks (slices of many tiles)
next to the default 4096 (slices of 5-6 rows, most blocks empty) over inputs
of about 30k rows (9 tiles of 3584, the last one partial).

Every case compares every output column, and validity where present, with
the CPU oracle, and compares the result byte for byte with the same plan read
through the paged k_emit (PMH_EMIT_LEGACY=1)."""

import decimal
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from oracle import merge_dedup, merge_first_row_model
from paimon_amd import Session, MergeReadPlan, file_descs_from_metas
from paimon_amd.datagen import gen_runs_dedup, write_runs
from tests.lookup_model import lookup_changelog_model

import tests.test_lookup_changelog_gpu as lk_t

pytestmark = pytest.mark.gpu

GRIDS = ("1", "2", "3", None)  # None = variable unset (4096 blocks)
DEFAULT_BLOCKS = 4096
TILE_ROWS = 3584
TOTAL_ROWS = 30_000
EMIT_WIN = 64  # tile offsets a block stages past its first tile
EMIT_LDS_MAX = 16384
KEY64 = [{"name": "_KEY_k", "type": "int64"}]


def _set(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


def _read_all(plan):
    got = {}
    while True:
        b = plan.read_next()
        if b is None:
            break
        for k, v in b.items():
            got.setdefault(k, []).append(v.copy())
    return {k: v[0] if k.endswith("#dict") else np.concatenate(v)
            for k, v in got.items()}


def _same_bytes(new, old, what):
    assert set(new) == set(old), (what, sorted(set(new) ^ set(old)))
    for k in new:
        if new[k].dtype == object:
            assert list(new[k]) == list(old[k]), (what, k)
        else:
            assert new[k].dtype == old[k].dtype, (what, k)
            assert new[k].tobytes() == old[k].tobytes(), (what, k)


def _read_both(session, monkeypatch, metas, key_cols, vcols, grids, **kw):
    """Yields (grid, result of k_emit_contig), after checking it against the
    legacy kernel's bytes at the same grid."""
    for grid in grids:
        _set(monkeypatch, "PMH_EMIT_BLOCKS", grid)
        res = []
        for legacy in (None, "1"):
            _set(monkeypatch, "PMH_EMIT_LEGACY", legacy)
            with MergeReadPlan(session, file_descs_from_metas(metas),
                               key_cols, vcols, **kw) as plan:
                res.append(_read_all(plan))
        _set(monkeypatch, "PMH_EMIT_LEGACY", None)
        _same_bytes(res[0], res[1], f"grid {grid}")
        yield grid, res[0]


def _winner_col(runs, r, w, field, col=None):
    src = [run[field] if col is None else run[field][col] for run in runs]
    return np.array([src[a][b] for a, b in zip(r, w)], dtype=src[0].dtype)


def _expected(runs, r, w):
    exp = {"_KEY_k": _winner_col(runs, r, w, "key"),
           "_SEQUENCE_NUMBER": _winner_col(runs, r, w, "seq"),
           "_VALUE_KIND": _winner_col(runs, r, w, "kind")}
    names = ["v_k"] + [f"v_c{i}" for i in range(len(runs[0]["values"]) - 1)]
    for c, nm in enumerate(names):
        exp[nm] = _winner_col(runs, r, w, "values", c)
    return exp


def _assert_exp(got, exp, what):
    for name, e in exp.items():
        g = got.get(name, np.empty(0, e.dtype))
        assert len(g) == len(e), (what, name, len(g), len(e))
        assert (g == e).all(), \
            f"{what} column {name}: {np.flatnonzero(g != e)[:8]}"


def _vcols(runs, key_type="int64"):
    return ([{"name": "v_k", "type": key_type}] +
            [{"name": f"v_c{i}", "type": "int32"}
             for i in range(len(runs[0]["values"]) - 1)])


def _check(tmp_path, monkeypatch, runs, exp, grids=GRIDS, key_type="int64",
           **kw):
    metas = write_runs(runs, str(tmp_path), compression="NONE")
    with Session(0) as s:
        for grid, got in _read_both(
                s, monkeypatch, metas,
                [{"name": "_KEY_k", "type": key_type}],
                _vcols(runs, key_type), grids, **kw):
            _assert_exp(got, exp, f"grid {grid}")


class TestGrids:
    @pytest.mark.parametrize("k", [1, 2, 8, 9, 32])
    def test_run_counts(self, tmp_path, monkeypatch, k):
        runs = gen_runs_dedup(k, TOTAL_ROWS // k, n_value_cols=2,
                              seed=9000 + k, delete_frac=0.1)
        n = sum(len(r["key"]) for r in runs)
        assert 8 * TILE_ROWS < n < 9 * TILE_ROWS  # 9 tiles, the last partial
        r, w = merge_dedup(runs, drop_delete=True)
        # the default grid leaves most blocks without a slice
        assert 4 * DEFAULT_BLOCKS < len(r) < 8 * DEFAULT_BLOCKS
        _check(tmp_path, monkeypatch, runs, _expected(runs, r, w))

    def test_int32_keys(self, tmp_path, monkeypatch):
        runs = gen_runs_dedup(5, 6_000, n_value_cols=1, seed=9100,
                              delete_frac=0.1)
        for r in runs:
            r["key"] = r["key"].astype(np.int32)
            r["values"][0] = r["values"][0].astype(np.int32)
        oruns = [{**r, "key": r["key"].astype(np.int64)} for r in runs]
        r_, w_ = merge_dedup(oruns, drop_delete=True)
        _check(tmp_path, monkeypatch, runs, _expected(runs, r_, w_),
               key_type="int32")


def _insert_delete_runs(n_keys, del_lo, del_hi, seed, keep=()):
    """Run 0 inserts keys 0 .. n_keys - 1; run 1 deletes [del_lo, del_hi)
    except `keep`, with newer sequence numbers."""
    rng = np.random.default_rng(seed)
    keys = np.arange(n_keys, dtype=np.int64)
    dk = np.setdiff1d(np.arange(del_lo, del_hi, dtype=np.int64),
                      np.asarray(keep, np.int64))
    run0 = {"key": keys, "seq": rng.permutation(n_keys).astype(np.int64),
            "kind": np.zeros(n_keys, np.int8),
            "values": [keys.copy(),
                       rng.integers(-2**31, 2**31, n_keys).astype(np.int32)]}
    run1 = {"key": dk,
            "seq": (n_keys + rng.permutation(len(dk))).astype(np.int64),
            "kind": np.full(len(dk), 3, np.int8),
            "values": [dk.copy(),
                       rng.integers(-2**31, 2**31, len(dk)).astype(np.int32)]}
    return [run0, run1]


def _winners_per_tile(runs, r, w):
    """Winner count per merge tile: merged rank // TILE_ROWS, the merged
    order being (key, sequence number) over every input row."""
    key = np.concatenate([run["key"] for run in runs])
    seq = np.concatenate([run["seq"] for run in runs])
    order = np.lexsort((seq, key))
    rank = np.empty(len(key), np.int64)
    rank[order] = np.arange(len(key))
    base = np.cumsum([0] + [len(run["key"]) for run in runs])
    wr = rank[base[np.asarray(r, np.int64)] + np.asarray(w, np.int64)]
    n_tiles = (len(key) + TILE_ROWS - 1) // TILE_ROWS
    return np.bincount(wr // TILE_ROWS, minlength=n_tiles)


def _longest_inner_empty_run(counts):
    """Longest run of count-0 tiles with winners before and after it."""
    nz = np.flatnonzero(counts)
    return int(np.diff(nz).max() - 1) if len(nz) > 1 else 0


class TestEmptyAndTiny:
    def test_no_output(self, tmp_path, monkeypatch):
        # every key's latest record is a delete: total = 0, every block
        # leaves before the first barrier
        runs = _insert_delete_runs(15_000, 0, 15_000, seed=9200)
        r, w = merge_dedup(runs, drop_delete=True)
        assert len(r) == 0
        _check(tmp_path, monkeypatch, runs, _expected(runs, r, w))

    def test_one_row(self, tmp_path, monkeypatch):
        runs = _insert_delete_runs(15_000, 0, 15_000, seed=9210,
                                   keep=[11_111])
        r, w = merge_dedup(runs, drop_delete=True)
        assert len(r) == 1
        _check(tmp_path, monkeypatch, runs, _expected(runs, r, w))


class TestEmptyTiles:
    def test_consecutive_empty_tiles(self, tmp_path, monkeypatch):
        # keys [6000, 15000) resolve to deletes: 18 000 merged rows without
        # a winner in the middle of the output
        runs = _insert_delete_runs(21_000, 6_000, 15_000, seed=9300)
        r, w = merge_dedup(runs, drop_delete=True)
        counts = _winners_per_tile(runs, r, w)
        assert 3 <= _longest_inner_empty_run(counts) < EMIT_WIN
        _check(tmp_path, monkeypatch, runs, _expected(runs, r, w))

    def test_more_empty_tiles_than_the_window(self, tmp_path, monkeypatch):
        # a block whose slice holds the winners on both sides of the gap
        # walks its tile cursor past the staged window
        n_del = (EMIT_WIN + 4) * TILE_ROWS // 2
        runs = _insert_delete_runs(n_del + 12_000, 5_000, 5_000 + n_del,
                                   seed=9310)
        r, w = merge_dedup(runs, drop_delete=True)
        counts = _winners_per_tile(runs, r, w)
        assert _longest_inner_empty_run(counts) > EMIT_WIN + 1
        _check(tmp_path, monkeypatch, runs, _expected(runs, r, w))


# (name, arrow type, plan type, output list of k_emit_contig in bytes)
TYPED = [
    ("v_i8", pa.int8(), "int8", 1),
    ("v_i16", pa.int16(), "int16", 2),
    ("v_i32", pa.int32(), "int32", 4),
    ("v_j32", pa.int32(), "int32", 4),
    ("v_i64", pa.int64(), "int64", 8),
    ("v_f", pa.float32(), "float32", 4),
    ("v_d", pa.float64(), "float64", 8),
    ("v_d9", pa.decimal128(9, 2), "decimal(9,2)", 4),
    ("v_d18", pa.decimal128(18, 2), "decimal(18,2)", 8),
    ("v_b", pa.bool_(), "boolean", 1),
    ("v_s", pa.dictionary(pa.int32(), pa.string()), "string", 4),
]
STR_DICT = [f"s{i:03d}" for i in range(200)]


def _typed_values(rng, n):
    return {
        "v_i8": rng.integers(-128, 128, n).astype(np.int8),
        "v_i16": rng.integers(-2**15, 2**15, n).astype(np.int16),
        "v_i32": rng.integers(-2**31, 2**31, n).astype(np.int32),
        "v_j32": rng.integers(-2**31, 2**31, n).astype(np.int32),
        "v_i64": rng.integers(-2**62, 2**62, n).astype(np.int64),
        "v_f": rng.standard_normal(n).astype(np.float32),
        "v_d": rng.standard_normal(n),
        "v_d9": rng.integers(-10**8, 10**8, n).astype(np.int32),
        "v_d18": rng.integers(-10**15, 10**15, n).astype(np.int64),
        "v_b": rng.random(n) < 0.5,
        "v_s": rng.integers(0, len(STR_DICT), n).astype(np.int32),
    }


def _typed_runs(k, rows, seed, key_dtype=np.int64):
    rng = np.random.default_rng(seed)
    runs = gen_runs_dedup(k, rows, n_value_cols=0, seed=seed,
                          delete_frac=0.1)
    for run in runs:
        run["key"] = run["key"].astype(key_dtype)
        run["typed"] = _typed_values(rng, rows)
    return runs


def _arrow_column(at, v, mask):
    if pa.types.is_decimal(at):
        v = [decimal.Decimal(int(u)).scaleb(-at.scale) for u in v]
        return pa.array(v, at, mask=mask)
    if pa.types.is_dictionary(at):
        return pa.DictionaryArray.from_arrays(pa.array(v, mask=mask),
                                              pa.array(STR_DICT))
    return pa.array(v, at, mask=mask)


def _write_typed(runs, out_dir, nulls=None, not_null=()):
    """nulls: {run index: {column: bool mask}}; a column of a run listed in
    not_null is written as a required field (no definition levels)."""
    os.makedirs(out_dir, exist_ok=True)
    metas = []
    for i, run in enumerate(runs):
        fields = [pa.field("_KEY_k", pa.from_numpy_dtype(run["key"].dtype),
                           nullable=False),
                  pa.field("_SEQUENCE_NUMBER", pa.int64(), nullable=False),
                  pa.field("_VALUE_KIND", pa.int8(), nullable=False)]
        arrays = [pa.array(run["key"]), pa.array(run["seq"]),
                  pa.array(run["kind"])]
        for name, at, _, _ in TYPED:
            mask = (nulls or {}).get(i, {}).get(name)
            fields.append(pa.field(name, at,
                                   nullable=(i, name) not in not_null))
            arrays.append(_arrow_column(at, run["typed"][name], mask))
        path = os.path.join(out_dir, f"run-{i}.parquet")
        pq.write_table(pa.Table.from_arrays(arrays, schema=pa.schema(fields)),
                       path, compression=None, use_dictionary=["v_s"],
                       store_decimal_as_integer=True,
                       data_page_version="1.0", store_schema=False)
        metas.append({"path": path, "rowCount": len(run["key"]),
                      "minKey": int(run["key"][0]),
                      "maxKey": int(run["key"][-1]), "level": 0})
    return metas


def _assert_typed(got, runs, r, w, names, what, nulls=None):
    for nm, src in (("_KEY_k", "key"), ("_SEQUENCE_NUMBER", "seq"),
                    ("_VALUE_KIND", "kind")):
        e = _winner_col(runs, r, w, src)
        assert len(got[nm]) == len(e) and (got[nm] == e).all(), (what, nm)
    for nm in names:
        e = np.array([runs[a]["typed"][nm][b] for a, b in zip(r, w)])
        valid = np.ones(len(e), bool)
        if nulls:
            valid = np.array([not (a in nulls and nm in nulls[a] and
                                   nulls[a][nm][b]) for a, b in zip(r, w)])
        gv = got.get(nm + "#valid")
        if gv is None:
            assert valid.all(), (what, nm, "validity array missing")
        else:
            assert (gv == valid).all(), \
                f"{what} {nm} validity: {np.flatnonzero(gv != valid)[:8]}"
        g = got[nm]
        if nm == "v_s":
            g = got["v_s#dict"][g[valid]]
            e = np.array([s.encode() for s in STR_DICT], object)[e[valid]]
            assert (g == e).all(), (what, nm)
            continue
        assert len(g) == len(e), (what, nm)
        assert (g.astype(e.dtype)[valid] == e[valid]).all(), \
            f"{what} {nm}: {np.flatnonzero((g.astype(e.dtype) != e) & valid)[:8]}"


def _plan_cols(names):
    return [{"name": nm, "type": pt} for nm, _, pt, _ in TYPED if nm in names]


def _list_lengths(names, key_bytes=8):
    """Columns per output-width list, key / sequence number / kind included
    (the kind is stored as INT32 and emitted as one byte)."""
    n = {1: 1, 2: 0, 4: 0, 8: 1}
    n[key_bytes] += 1
    for nm, _, _, width in TYPED:
        if nm in names:
            n[width] += 1
    return n


class TestTypeMix:
    ALL = [nm for nm, _, _, _ in TYPED]

    @pytest.fixture(scope="class")
    def files(self, tmp_path_factory):
        runs = _typed_runs(5, 6_000, seed=9400)
        metas = _write_typed(runs, str(tmp_path_factory.mktemp("typed")))
        r, w = merge_dedup(runs, drop_delete=True)
        return runs, metas, r, w

    @pytest.mark.parametrize("names,lengths", [
        # 1-byte 3, 2-byte 1, 4-byte 5, 8-byte 5: no multiple of G = 4 / 2
        (ALL, {1: 3, 2: 1, 4: 5, 8: 5}),
        # 4-byte and 2-byte lists of length 0
        (["v_i8", "v_i64"], {1: 2, 2: 0, 4: 0, 8: 3}),
        # a 4-byte list of length 1
        (["v_i32"], {1: 1, 2: 0, 4: 1, 8: 2}),
        # 4-byte list of 2, 8-byte list of 3
        (["v_i16", "v_f", "v_s", "v_d"], {1: 1, 2: 1, 4: 2, 8: 3}),
    ], ids=["all", "narrow_and_wide", "one_int32", "mixed"])
    def test_lists(self, files, monkeypatch, names, lengths):
        runs, metas, r, w = files
        assert _list_lengths(names) == lengths
        with Session(0) as s:
            for grid, got in _read_both(s, monkeypatch, metas, KEY64,
                                        _plan_cols(names), ("2", None)):
                _assert_typed(got, runs, r, w, names, f"grid {grid}")

    def test_int32_key(self, tmp_path, monkeypatch):
        runs = _typed_runs(3, 10_000, seed=9410, key_dtype=np.int32)
        metas = _write_typed(runs, str(tmp_path))
        oruns = [{**run, "key": run["key"].astype(np.int64)} for run in runs]
        r, w = merge_dedup(oruns, drop_delete=True)
        names = ["v_i8", "v_i32", "v_d", "v_b"]
        assert _list_lengths(names, key_bytes=4) == {1: 3, 2: 0, 4: 2, 8: 2}
        with Session(0) as s:
            for grid, got in _read_both(
                    s, monkeypatch, metas,
                    [{"name": "_KEY_k", "type": "int32"}], _plan_cols(names),
                    ("3", None)):
                _assert_typed(got, runs, r, w, names, f"grid {grid}")


class TestNullable:
    def test_nulls_in_some_runs(self, tmp_path, monkeypatch):
        # runs 0 and 2 hold nulls; run 1 is an optional field without any,
        # run 3 a required field: no validity array is staged for it
        rng = np.random.default_rng(9500)
        runs = _typed_runs(4, 7_500, seed=9500)
        names = ["v_i8", "v_i32", "v_i64", "v_d9", "v_b", "v_s"]
        nulls = {i: {nm: rng.random(7_500) < 0.3 for nm in names}
                 for i in (0, 2)}
        not_null = {(3, nm) for nm in names}
        metas = _write_typed(runs, str(tmp_path), nulls, not_null)
        r, w = merge_dedup(runs, drop_delete=True)
        # nulls on both sides of a slice boundary of the default grid
        isnull = np.array([a in nulls and bool(nulls[a]["v_i32"][b])
                           for a, b in zip(r, w)])
        per_block = -(-len(r) // DEFAULT_BLOCKS)
        edge = np.arange(per_block, len(r), per_block)
        assert (isnull[edge - 1] & isnull[edge]).any()
        with Session(0) as s:
            for grid, got in _read_both(s, monkeypatch, metas, KEY64,
                                        _plan_cols(names), GRIDS):
                _assert_typed(got, runs, r, w, names, f"grid {grid}", nulls)


class TestOtherUsers:
    def test_first_row(self, tmp_path, monkeypatch):
        runs = gen_runs_dedup(6, 5_000, n_value_cols=2, seed=9600,
                              delete_frac=0.0)
        r, w = merge_first_row_model(runs)
        _check(tmp_path, monkeypatch, runs, _expected(runs, r, w),
               merge_engine="first-row")

    def test_hierarchical_section(self, tmp_path, monkeypatch):
        # 36 runs: two batches gather into virtual runs (a sub-range of the
        # real runs' descriptors each), then the chain gathers from those;
        # one value column is nullable
        rng = np.random.default_rng(9610)
        runs = gen_runs_dedup(36, 850, n_value_cols=2, seed=9610,
                              delete_frac=0.1)
        for run in runs:
            n = len(run["key"])
            run["valid"] = [np.ones(n, bool), rng.random(n) >= 0.3,
                            np.ones(n, bool)]
        metas = write_runs(runs, str(tmp_path), compression="NONE")
        r, w = merge_dedup(runs, drop_delete=True)
        exp = _expected(runs, r, w)
        valid = _winner_col(runs, r, w, "valid", 1)
        with Session(0) as s:
            for grid, got in _read_both(s, monkeypatch, metas, KEY64,
                                        _vcols(runs), GRIDS):
                assert (got["v_c0#valid"] == valid).all(), grid
                for name, e in exp.items():
                    sel = valid if name == "v_c0" else slice(None)
                    assert len(got[name]) == len(e), (grid, name)
                    assert (got[name][sel] == e[sel]).all(), (grid, name)

    @staticmethod
    def _lookup_reads(tmp_path, monkeypatch, runs, lookup):
        """Yields (grid, main, changelog) of k_emit_contig, each checked
        against the legacy kernel's bytes."""
        metas = write_runs(runs, os.path.join(str(tmp_path), "merge"),
                           compression="NONE")
        for m in metas:
            m["level"] = 0  # every merge run is a level-0 file
        lookup_descs = lk_t._write_lookup(tmp_path, lookup)
        n_vals = len(runs[0]["values"])
        with Session(0) as s:
            for grid in GRIDS:
                _set(monkeypatch, "PMH_EMIT_BLOCKS", grid)
                res = []
                for legacy in (None, "1"):
                    _set(monkeypatch, "PMH_EMIT_LEGACY", legacy)
                    with MergeReadPlan(
                            s, file_descs_from_metas(metas), lk_t._key_cols(),
                            lk_t._value_cols(n_vals - 1),
                            changelog_producer="lookup",
                            lookup_files=lookup_descs) as plan:
                        res.append(lk_t._read_all(plan)[:2])
                _set(monkeypatch, "PMH_EMIT_LEGACY", None)
                _same_bytes(res[0][0], res[1][0], f"grid {grid} main")
                _same_bytes(res[0][1], res[1][1], f"grid {grid} changelog")
                yield grid, res[0][0], res[0][1]

    def test_lookup_changelog(self, tmp_path, monkeypatch):
        runs = lk_t._level0_runs(seed=9620, n_runs=3, rows=9_000)
        rng = np.random.default_rng(9620)
        lookup = lk_t._two_lookup_levels(rng, lk_t._keyspace(runs),
                                         n3=4_000, n5=3_000)
        lookup_runs = [run for _, run, _ in lookup]
        n_vals = len(runs[0]["values"])
        exp_cl, exp_res = lookup_changelog_model(
            runs, [0, 0, 0], lookup_runs, row_dedup=False, drop_delete=True,
            masks=None, lookup_masks=None)
        sources = list(runs) + lookup_runs
        for grid, main, cl in self._lookup_reads(tmp_path, monkeypatch, runs,
                                                 lookup):
            lk_t._assert_stream(main, sources, exp_res, n_vals,
                                f"grid {grid} main")
            lk_t._assert_stream(cl, sources, [(a, b) for a, b, _ in exp_cl],
                                n_vals, f"grid {grid} changelog",
                                kinds=[kd for _, _, kd in exp_cl])

    def test_lookup_level_winners(self, tmp_path, monkeypatch):
        # A winner word may name a lookup level: a run slot PAST the merge
        # runs in the descriptor table. With level-0 sequence numbers below
        # the lookup levels' (not a state a table reaches, so the merge model
        # is not consulted), thousands of results are lookup records. The
        # gather is checked record by record: every output row must be the
        # input record that carries its (key, sequence number), whichever
        # slot it sits in.
        runs = lk_t._level0_runs(seed=9630, n_runs=3, rows=9_000, seq_base=0)
        rng = np.random.default_rng(9630)
        lookup = lk_t._two_lookup_levels(rng, lk_t._keyspace(runs),
                                         n3=4_000, n5=3_000)
        sources = list(runs) + [run for _, run, _ in lookup]
        n_vals = len(runs[0]["values"])
        tag = np.concatenate([(s_["key"] << 20) | s_["seq"] for s_ in sources])
        assert max(int(s_["seq"].max()) for s_ in sources) < 1 << 20
        order = np.argsort(tag)
        assert (np.diff(tag[order]) > 0).all()  # (key, seq) names one record
        cols = [np.concatenate([s_["values"][c] for s_ in sources])[order]
                for c in range(n_vals)]
        kind = np.concatenate([s_["kind"] for s_ in sources])[order]
        level3 = np.zeros(len(tag), bool)
        lo = sum(len(r["key"]) for r in runs)
        level3[lo:lo + len(lookup[0][1]["key"])] = True
        level3 = level3[order]
        for grid, main, _ in self._lookup_reads(tmp_path, monkeypatch, runs,
                                                lookup):
            gt = (main["_KEY_k"] << 20) | main["_SEQUENCE_NUMBER"]
            at = np.searchsorted(tag[order], gt)
            assert (tag[order][np.minimum(at, len(tag) - 1)] == gt).all(), grid
            assert level3[at].sum() > 1000, grid  # results from a lookup slot
            assert (main["_VALUE_KIND"] == kind[at]).all(), grid
            for c in range(n_vals):
                name = "v_k" if c == 0 else f"v_c{c - 1}"
                assert (main[name] == cols[c][at]).all(), (grid, name)


class TestOversizedTable:
    def test_falls_back_to_the_paged_kernel(self, tmp_path, monkeypatch):
        # 32 runs x 32 columns: the descriptor table alone passes the LDS
        # budget, so the launcher takes k_emit by itself
        runs = gen_runs_dedup(32, 940, n_value_cols=28, seed=9700,
                              delete_frac=0.1)
        n_cols = 3 + len(runs[0]["values"])
        assert 16 * len(runs) * n_cols >= EMIT_LDS_MAX
        r, w = merge_dedup(runs, drop_delete=True)
        _check(tmp_path, monkeypatch, runs, _expected(runs, r, w),
               grids=("2", None))
