"""GPU parity for the ORC read path (C3's format half): RLEv2 / byte-RLE /
PRESENT decode on device, feeding the same merge pipeline — against the CPU
oracle on ORC files written by pyarrow (the independent implementation)."""

import os

import numpy as np
import pytest
from pyarrow import orc as pa_orc

from oracle import merge_dedup, partial_update_model
from oracle import orc_light as ol
from paimon_amd import Session, MergeReadPlan, file_descs_from_metas
from paimon_amd.datagen import (gen_runs_dedup, gen_runs_partial_update,
                                run_to_arrow, write_runs)

pytestmark = pytest.mark.gpu

KEY_COLS = [{"name": "_KEY_k", "type": "int64"}]


def _value_cols(n):
    return ([{"name": "v_k", "type": "int64"}] +
            [{"name": f"v_c{i}", "type": "int32"} for i in range(n)])


def _read_all(plan):
    got = {}
    while True:
        b = plan.read_next()
        if b is None:
            break
        for kk, v in b.items():
            got.setdefault(kk, []).append(v.copy())
    return {kk: np.concatenate(v) for kk, v in got.items()}


class TestOrcDedup:
    def _run(self, tmp_path, runs, compression="NONE", **kw):
        metas = write_runs(runs, str(tmp_path), file_format="orc",
                           compression=compression)
        r, w = merge_dedup(runs, **kw)
        with Session(0) as s:
            with MergeReadPlan(s, file_descs_from_metas(metas), KEY_COLS,
                               _value_cols(len(runs[0]["values"]) - 1),
                               **kw) as plan:
                got = _read_all(plan)
        names = (["_KEY_k", "_SEQUENCE_NUMBER", "_VALUE_KIND", "v_k"] +
                 [f"v_c{i}" for i in range(len(runs[0]["values"]) - 1)])
        srcs = (["key", "seq", "kind"] +
                [("values", c) for c in range(len(runs[0]["values"]))])
        for nm, src in zip(names, srcs):
            if isinstance(src, tuple):
                e = np.array([runs[a]["values"][src[1]][b]
                              for a, b in zip(r, w)])
            else:
                e = np.array([runs[a][src][b] for a, b in zip(r, w)])
            assert (got[nm] == e).all(), nm

    def test_orc_dedup_8_runs(self, tmp_path):
        runs = gen_runs_dedup(8, 40_000, n_value_cols=4, seed=81,
                              delete_frac=0.1)
        self._run(tmp_path, runs)

    def test_orc_dedup_monotonic_keys_delta(self, tmp_path):
        # dense monotonic keys exercise the DELTA sub-encoding
        rng = np.random.default_rng(82)
        runs = []
        seqs = rng.permutation(200_000).astype(np.int64)
        for r in range(4):
            keys = (np.arange(50_000, dtype=np.int64) * 2 + r)
            runs.append({"key": keys, "seq": seqs[r*50_000:(r+1)*50_000],
                         "kind": np.zeros(50_000, np.int8),
                         "values": [keys.copy(),
                                    rng.integers(-100, 100, 50_000).astype(np.int32)]})
        self._run(tmp_path, runs)

    def test_orc_dedup_outliers_patched(self, tmp_path):
        # small values + outliers exercise PATCHED_BASE in the values
        rng = np.random.default_rng(83)
        runs = []
        seqs = rng.permutation(80_000).astype(np.int64)
        for r in range(4):
            keys = np.sort(rng.choice(60_000, 20_000, replace=False)).astype(np.int64)
            v = rng.integers(0, 50, 20_000).astype(np.int32)
            v[rng.choice(20_000, 200, replace=False)] = rng.integers(
                2**28, 2**31 - 1, 200).astype(np.int32)
            runs.append({"key": keys, "seq": seqs[r*20_000:(r+1)*20_000],
                         "kind": rng.choice([0, 3], 20_000, p=[.9, .1]).astype(np.int8),
                         "values": [keys.copy(), v]})
        self._run(tmp_path, runs)

    def test_orc_zlib(self, tmp_path):
        # ORC's default codec: streams + footers arrive chunk-compressed
        # (host decompress at staging, ORC spec "Compression")
        runs = gen_runs_dedup(6, 30_000, n_value_cols=3, seed=88,
                              delete_frac=0.1)
        self._run(tmp_path, runs, compression="zlib")

    def test_orc_zstd(self, tmp_path):
        runs = gen_runs_dedup(5, 25_000, n_value_cols=2, seed=89,
                              delete_frac=0.15)
        self._run(tmp_path, runs, compression="zstd")

    def test_orc_snappy(self, tmp_path):
        runs = gen_runs_dedup(4, 20_000, n_value_cols=2, seed=90,
                              delete_frac=0.1)
        self._run(tmp_path, runs, compression="snappy")

    def test_orc_keep_delete(self, tmp_path):
        runs = gen_runs_dedup(4, 15_000, n_value_cols=2, seed=84,
                              delete_frac=0.3)
        self._run(tmp_path, runs, drop_delete=False)


class TestOrcPartialUpdate:
    def test_orc_pu_with_nulls(self, tmp_path):
        # C3 proper: ORC + PartialUpdate + nulls (PRESENT streams on device)
        runs = gen_runs_partial_update(4, 25_000, n_value_cols=8, seed=85,
                                       update_frac=0.3, update_cols=3)
        metas = write_runs(runs, str(tmp_path), file_format="orc",
                           compression="zlib")
        exp = partial_update_model(runs)
        with Session(0) as s:
            with MergeReadPlan(s, file_descs_from_metas(metas), KEY_COLS,
                               _value_cols(8),
                               merge_engine="partial-update") as plan:
                got = _read_all(plan)
        assert (got["_KEY_k"] == exp["key"]).all()
        assert (got["_SEQUENCE_NUMBER"] == exp["seq"]).all()
        names = ["v_k"] + [f"v_c{i}" for i in range(8)]
        for c, nm in enumerate(names):
            ev, em = exp["values"][c], exp["valid"][c]
            gm = got.get(nm + "#valid")
            if gm is None:
                gm = np.ones(len(got[nm]), dtype=bool)
            assert (gm == em).all(), nm
            assert (got[nm][em] == ev[em]).all(), nm


def _alternating(n):
    return np.arange(n) % 2 == 0


def _then_null(n_valid, tail):
    """n_valid valid rows (whole 0xFF PRESENT bytes), one null, tail valid."""
    return np.r_[np.ones(n_valid, bool), False, np.ones(tail, bool)]


# name -> (validity of run 0, validity of run 1, stripe_size or None).
# PRESENT is byte-RLE over MSB-first bit-packed bytes; a byte run holds at
# most 130 bytes = 1040 rows, so 1040 and 1048 rows of one repeated byte sit
# on the edge between one run and a run plus one more byte.
PRESENT_PATTERNS = {
    "all_null": (np.zeros(1000, bool), np.zeros(1003, bool), None),
    "no_nulls": (np.ones(1000, bool), np.ones(1003, bool), None),
    "alternating_130_bytes": (_alternating(1040), ~_alternating(1040), None),
    "alternating_131_bytes": (_alternating(1048), ~_alternating(1048), None),
    "alternating_odd_rows": (_alternating(1043), ~_alternating(1045), None),
    "null_run_then_valid_run": (np.arange(5003) >= 2500,
                                np.arange(4999) < 2400, None),
    "valid_130_bytes": (_then_null(1040, 6), ~_then_null(1040, 6), None),
    "valid_131_bytes": (_then_null(1048, 2), ~_then_null(1048, 2), None),
    # stripe_size 1: the writer cuts a stripe every 1024 rows, so the dense
    # cursor carries over stripe boundaries; in the second case a stripe is
    # all null, the next has no PRESENT stream at all, the last one is mixed
    "two_stripes": (np.arange(2051) % 7 < 3, np.arange(1500) % 5 != 1, 1),
    "stripes_null_full_mixed": (
        np.r_[np.zeros(1024, bool), np.ones(1024, bool), _alternating(501)],
        np.r_[np.ones(1024, bool), np.zeros(1024, bool), _alternating(77)],
        1),
}


def _present_run_headers(path, column):
    """Header bytes of the column's PRESENT byte-RLE runs, per stripe."""
    fi = ol.parse_orc(path)
    cid = fi.column_names.index(column) + 1
    with open(path, "rb") as f:
        raw = f.read()
    out = []
    for st in fi.stripes:
        ps = ol.find_stream(st, cid, ol.STREAM_PRESENT)
        heads = []
        if ps is not None:
            s, p = raw[ps.offset:ps.offset + ps.length], 0
            while p < len(s):
                heads.append(s[p])
                p += 2 if s[p] < 128 else 1 + 256 - s[p]
        out.append(heads)
    return out


class TestOrcPresentPatterns:
    """Nullable int64 (v_k) and int32 (v_c0) columns whose PRESENT streams
    have structure a random null mask never has: the boolean-RLE walk, its
    hand-off to the level scatter and the dense (non-null) cursor, across
    run-length edges, odd row counts and a stripe boundary."""

    @pytest.mark.parametrize("name", list(PRESENT_PATTERNS))
    def test_pattern(self, tmp_path, name):
        v0, v1, stripe_size = PRESENT_PATTERNS[name]
        rng = np.random.default_rng(91)
        runs = []
        n_all = len(v0) + len(v1)
        seqs = rng.permutation(n_all).astype(np.int64)
        lo = 0
        for valid in (v0, v1):
            n = len(valid)
            keys = np.sort(rng.choice(n_all, n, replace=False)).astype(
                np.int64)
            runs.append({
                "key": keys, "seq": seqs[lo:lo + n],
                "kind": np.zeros(n, np.int8),
                "values": [rng.integers(-2**62, 2**62, n),
                           rng.integers(-2**31, 2**31, n).astype(np.int32)],
                # the int32 column gets the mirrored pattern
                "valid": [valid, valid[::-1].copy()]})
            lo += n
        metas = []
        for i, run in enumerate(runs):
            path = os.path.join(str(tmp_path), f"run-{i}.orc")
            kw = {"stripe_size": stripe_size} if stripe_size else {}
            pa_orc.write_table(run_to_arrow(run), path,
                               compression="uncompressed", **kw)
            metas.append({"path": path, "rowCount": len(run["key"]),
                          "minKey": int(run["key"][0]),
                          "maxKey": int(run["key"][-1]), "level": 0})
        # the files must hold what the case is about
        heads = [_present_run_headers(m["path"], "v_k") for m in metas]
        if stripe_size:
            assert all(len(h) >= 2 for h in heads), "one stripe only"
        if name.endswith("130_bytes") or name.endswith("131_bytes"):
            assert all(127 in h[0] for h in heads), "no 130-byte run"
        if name == "no_nulls":
            assert all(h == [[]] for h in heads)
        r, w = merge_dedup(runs)
        with Session(0) as s:
            with MergeReadPlan(s, file_descs_from_metas(metas), KEY_COLS,
                               _value_cols(1)) as plan:
                got = _read_all(plan)
        assert (got["_KEY_k"] ==
                np.array([runs[a]["key"][b] for a, b in zip(r, w)])).all()
        for c, nm in enumerate(("v_k", "v_c0")):
            ev = np.array([runs[a]["values"][c][b] for a, b in zip(r, w)])
            em = np.array([runs[a]["valid"][c][b] for a, b in zip(r, w)],
                          bool)
            gm = got.get(nm + "#valid")
            if gm is None:
                gm = np.ones(len(got[nm]), dtype=bool)
            assert (gm.astype(bool) == em).all(), nm
            assert (got[nm][em] == ev[em]).all(), nm


class TestOrcFloatDouble:
    def test_orc_float_double_columns(self, tmp_path):
        # FLOAT/DOUBLE DATA streams are raw IEEE754: staged as a copy, merged
        # bit-exactly
        rng = np.random.default_rng(86)
        runs = []
        seqs = rng.permutation(45_000).astype(np.int64)
        for i in range(3):
            keys = np.sort(rng.choice(70_000, 15_000,
                                      replace=False)).astype(np.int64)
            runs.append({
                "key": keys, "seq": seqs[i*15_000:(i+1)*15_000],
                "kind": rng.choice([0, 3], 15_000, p=[.9, .1]).astype(np.int8),
                "values": [keys.copy(),
                           rng.standard_normal(15_000).astype(np.float32),
                           rng.standard_normal(15_000)]})
        metas = write_runs(runs, str(tmp_path), file_format="orc",
                           compression="zlib")
        r, w = merge_dedup(runs, drop_delete=True)
        with Session(0) as s:
            with MergeReadPlan(s, file_descs_from_metas(metas), KEY_COLS,
                               [{"name": "v_k", "type": "int64"},
                                {"name": "v_c0", "type": "float32"},
                                {"name": "v_c1", "type": "float64"}]) as plan:
                got = _read_all(plan)
        for nm, c, dt in (("v_c0", 1, np.float32), ("v_c1", 2, np.float64)):
            e = np.array([runs[a]["values"][c][b] for a, b in zip(r, w)], dt)
            assert got[nm].dtype == dt
            assert (got[nm].view(np.uint8) == e.view(np.uint8)).all(), nm

    def test_orc_nullable_double_pu(self, tmp_path):
        rng = np.random.default_rng(87)
        runs = gen_runs_partial_update(3, 12_000, n_value_cols=2, seed=87,
                                       update_frac=0.5, update_cols=1)
        for r in runs:
            n = len(r["key"])
            r["values"][1] = rng.standard_normal(n)
            r["values"][2] = rng.standard_normal(n).astype(np.float32)
        metas = write_runs(runs, str(tmp_path), file_format="orc")
        exp = partial_update_model(runs)
        with Session(0) as s:
            with MergeReadPlan(s, file_descs_from_metas(metas), KEY_COLS,
                               [{"name": "v_k", "type": "int64"},
                                {"name": "v_c0", "type": "float64"},
                                {"name": "v_c1", "type": "float32"}],
                               merge_engine="partial-update") as plan:
                got = _read_all(plan)
        assert (got["_KEY_k"] == exp["key"]).all()
        for c, nm in ((1, "v_c0"), (2, "v_c1")):
            em = exp["valid"][c]
            gm = got.get(nm + "#valid")
            if gm is None:
                gm = np.ones(len(got[nm]), dtype=bool)
            assert (gm == em).all(), nm
            assert (got[nm][em] == exp["values"][c][em]).all(), nm
