"""ORC DECIMAL columns through the product path: pyarrow-written ORC files
(the independent implementation) with a decimal(18,2) column, a nullable
decimal(9,3) column and an int64, merged on the GPU and compared bit-exactly
with the merge oracle run over the unscaled integers."""

import decimal
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
from pyarrow import orc as pa_orc

from oracle import aggregation_model, merge_dedup, partial_update_model
from oracle import orc_light as ol
from paimon_amd import Session, MergeReadPlan, file_descs_from_metas
from paimon_amd.compact import rewrite
from paimon_amd.datagen import gen_runs_dedup, gen_runs_partial_update

pytestmark = pytest.mark.gpu

KEY_COLS = [{"name": "_KEY_k", "type": "int64"}]
VALUE_COLS = [{"name": "v_k", "type": "int64"},
              {"name": "v_dec", "type": "decimal(18,2)"},
              {"name": "v_d9", "type": "decimal(9,3)"}]
NAMES = ["v_k", "v_dec", "v_d9"]
N_RUNS, ROWS = 4, 3000


def _read_all(plan):
    got = {}
    while True:
        b = plan.read_next()
        if b is None:
            break
        for kk, v in b.items():
            got.setdefault(kk, []).append(v.copy())
    return {kk: np.concatenate(v) for kk, v in got.items()}


def _decimal_columns(runs, seed, nullable_dec=False):
    """Give each run values [v_k, v_dec unscaled int64, v_d9 unscaled int32]
    and validity masks (v_d9 nullable; v_dec too when asked)."""
    rng = np.random.default_rng(seed)
    for r in runs:
        n = len(r["key"])
        dec = rng.integers(-10**12, 10**12, n, dtype=np.int64)
        # a few values of every varint length a decimal(18,2) can take
        edge = [0, 1, -1, 63, -64, 64, 10**18 - 1, -(10**18 - 1)]
        edge += [10**k for k in range(1, 18)] + [-10**k for k in range(1, 18)]
        dec[:len(edge)] = edge
        d9 = rng.integers(-(10**9) + 1, 10**9, n).astype(np.int32)
        d9[:4] = [0, -1, 10**9 - 1, -(10**9 - 1)]
        old_valid = r.get("valid")
        r["values"] = [r["values"][0], dec, d9]
        r["valid"] = [np.ones(n, bool),
                      old_valid[1] if nullable_dec else np.ones(n, bool),
                      old_valid[2] if old_valid is not None
                      else rng.random(n) > 0.25]
    return runs


def _dec_array(unscaled, valid, p, s):
    vals = [decimal.Decimal(int(u)).scaleb(-s) if ok else None
            for u, ok in zip(unscaled, valid)]
    return pa.array(vals, pa.decimal128(p, s))


def _arrow_table(run):
    v = run["values"]
    m = run["valid"]
    fields = [pa.field("_KEY_k", pa.int64(), nullable=False),
              pa.field("_SEQUENCE_NUMBER", pa.int64(), nullable=False),
              pa.field("_VALUE_KIND", pa.int8(), nullable=False),
              pa.field("v_k", pa.int64()),
              pa.field("v_dec", pa.decimal128(18, 2)),
              pa.field("v_d9", pa.decimal128(9, 3))]
    arrays = [pa.array(run["key"]), pa.array(run["seq"]),
              pa.array(run["kind"]), pa.array(v[0]),
              _dec_array(v[1], m[1], 18, 2), _dec_array(v[2], m[2], 9, 3)]
    return pa.Table.from_arrays(arrays, schema=pa.schema(fields))


def _meta(run, path):
    return {"path": path, "rowCount": len(run["key"]),
            "minKey": int(run["key"][0]), "maxKey": int(run["key"][-1]),
            "level": 0}


def _write_orc(runs, out_dir, compression="uncompressed", **kw):
    os.makedirs(out_dir, exist_ok=True)
    metas = []
    for i, run in enumerate(runs):
        path = os.path.join(out_dir, f"run-{i}.orc")
        pa_orc.write_table(_arrow_table(run), path, compression=compression,
                           **kw)
        metas.append(_meta(run, path))
    return metas


def _check_rows(got, runs, r, w):
    """Deduplicate result against the oracle's winner (run, row) lists."""
    for nm, src in (("_KEY_k", "key"), ("_SEQUENCE_NUMBER", "seq"),
                    ("_VALUE_KIND", "kind")):
        e = np.array([runs[a][src][b] for a, b in zip(r, w)])
        assert (got[nm] == e).all(), nm
    for c, nm in enumerate(NAMES):
        ev = np.array([runs[a]["values"][c][b] for a, b in zip(r, w)])
        em = np.array([runs[a]["valid"][c][b] for a, b in zip(r, w)], bool)
        gm = got.get(nm + "#valid")
        if gm is None:
            gm = np.ones(len(got[nm]), dtype=bool)
        assert (gm.astype(bool) == em).all(), nm
        assert got[nm].dtype == ev.dtype, nm
        assert (got[nm][em] == ev[em]).all(), nm


def _check_model(got, exp):
    assert (got["_KEY_k"] == exp["key"]).all()
    assert (got["_SEQUENCE_NUMBER"] == exp["seq"]).all()
    for c, nm in enumerate(NAMES):
        ev, em = exp["values"][c], exp["valid"][c]
        gm = got.get(nm + "#valid")
        if gm is None:
            gm = np.ones(len(got[nm]), dtype=bool)
        assert (gm == em).all(), nm
        assert (got[nm][em] == ev[em]).all(), nm


@pytest.fixture(scope="module")
def dedup_runs():
    return _decimal_columns(
        gen_runs_dedup(N_RUNS, ROWS, n_value_cols=1, seed=1001,
                       delete_frac=0.1), 1002)


@pytest.fixture(scope="module")
def dedup_winners(dedup_runs):
    return merge_dedup(dedup_runs)


class TestOrcDecimalDedup:
    @pytest.mark.parametrize("compression",
                             ["uncompressed", "zlib", "snappy", "zstd"])
    def test_dedup_with_deletes(self, tmp_path, dedup_runs, dedup_winners,
                                compression):
        metas = _write_orc(dedup_runs, str(tmp_path), compression)
        assert pa_orc.ORCFile(metas[0]["path"]).compression.lower() == \
            compression
        if compression == "uncompressed":
            # the files hold what the case is about: DECIMAL columns with
            # DATA and SECONDARY streams (the oracle's stream locator reads
            # uncompressed files only)
            fi = ol.parse_orc(metas[0]["path"])
            cid = fi.column_names.index("v_dec") + 1
            assert ol.find_stream(fi.stripes[0], cid, 5) is not None
        with Session(0) as s:
            with MergeReadPlan(s, file_descs_from_metas(metas), KEY_COLS,
                               VALUE_COLS) as plan:
                got = _read_all(plan)
        _check_rows(got, dedup_runs, *dedup_winners)

    def test_several_stripes(self, tmp_path, dedup_runs, dedup_winners):
        # stripe_size 1: the writer cuts a stripe every 1024 rows, so units,
        # the dense cursor of v_d9 and the scale streams restart per stripe
        metas = _write_orc(dedup_runs, str(tmp_path), stripe_size=1)
        assert all(len(ol.parse_orc(m["path"]).stripes) >= 2 for m in metas)
        with Session(0) as s:
            with MergeReadPlan(s, file_descs_from_metas(metas), KEY_COLS,
                               VALUE_COLS) as plan:
                got = _read_all(plan)
        _check_rows(got, dedup_runs, *dedup_winners)

    def test_parquet_and_orc_runs_of_one_column(self, tmp_path, dedup_runs,
                                                dedup_winners):
        # runs 0 and 2 as Parquet decimals (INT64 / INT32 physical), runs 1
        # and 3 as ORC decimals
        metas = []
        for i, run in enumerate(dedup_runs):
            if i % 2:
                path = os.path.join(str(tmp_path), f"run-{i}.orc")
                pa_orc.write_table(_arrow_table(run), path,
                                   compression="zlib")
            else:
                path = os.path.join(str(tmp_path), f"run-{i}.parquet")
                pq.write_table(_arrow_table(run), path, compression=None,
                               use_dictionary=False, data_page_version="1.0",
                               write_statistics=False, store_schema=False,
                               store_decimal_as_integer=True)
            metas.append(_meta(run, path))
        with Session(0) as s:
            with MergeReadPlan(s, file_descs_from_metas(metas), KEY_COLS,
                               VALUE_COLS) as plan:
                got = _read_all(plan)
        _check_rows(got, dedup_runs, *dedup_winners)

    def test_compaction_orc_in_parquet_out(self, tmp_path, dedup_runs):
        metas = _write_orc(dedup_runs, str(tmp_path / "in"), "zstd")
        r, w = merge_dedup(dedup_runs, drop_delete=True)
        with Session(0) as s:
            res = rewrite(s, metas, KEY_COLS, VALUE_COLS,
                          str(tmp_path / "out"), output_level=5,
                          drop_delete=True, target_file_rows=5000)
        parts = [pq.read_table(m["path"]) for m in res["after"]]
        assert len(parts) >= 2
        for p in parts:
            assert p.schema.field("v_dec").type == pa.decimal128(18, 2)
            assert p.schema.field("v_d9").type == pa.decimal128(9, 3)
        keys = np.concatenate([p.column("_KEY_k").to_numpy() for p in parts])
        assert (keys == np.array([dedup_runs[a]["key"][b]
                                  for a, b in zip(r, w)])).all()
        for c, nm, sc in ((1, "v_dec", 2), (2, "v_d9", 3)):
            col = sum((p.column(nm).to_pylist() for p in parts), [])
            exp = [decimal.Decimal(int(dedup_runs[a]["values"][c][b]))
                   .scaleb(-sc) if dedup_runs[a]["valid"][c][b] else None
                   for a, b in zip(r, w)]
            assert col == exp, nm


def _patch_second_scale_run(path, column, col_scale, new_scale):
    """Rewrite, in stripe 0 of an uncompressed pyarrow-written file, the
    data scale of the column's second SECONDARY run (pyarrow writes constant
    runs of 512: DELTA header, count, zigzag base, delta 0). Same length, so
    every offset in the file holds. Returns the first dense position of the
    rewritten run."""
    fi = ol.parse_orc(path)
    cid = fi.column_names.index(column) + 1
    st = ol.find_stream(fi.stripes[0], cid, 5)
    with open(path, "rb") as f:
        raw = bytearray(f.read())
    sec = raw[st.offset:st.offset + st.length]
    assert len(sec) == 8 and sec[:4] == bytes([0xC1, 0xFF, 2 * col_scale, 0])
    assert sec[4] >> 6 == 3 and sec[6:] == bytes([2 * col_scale, 0])
    raw[st.offset + 6] = 2 * new_scale
    with open(path, "wb") as f:
        f.write(raw)
    return 512


class TestOrcDecimalDataScales:
    """Files whose SECONDARY stream is not uniformly the column scale: the
    scales decode through k_rlev2 into the scale scratch and k_orc_varint
    rescales by them. No writer at hand produces such files, so a pyarrow
    file gets one constant scale run rewritten; pyarrow's own reader (ORC
    C++) says what the rewritten file means."""

    def _runs(self):
        runs = _decimal_columns(
            gen_runs_dedup(2, ROWS, n_value_cols=1, seed=1030,
                           delete_frac=0.1), 1031)
        for r in runs:  # room for one more digit
            r["values"][2] = (r["values"][2] // 1000).astype(np.int32)
        return runs

    def test_lower_data_scale_rescales(self, tmp_path):
        runs = self._runs()
        metas = _write_orc(runs, str(tmp_path), stripe_size=1)
        path = metas[0]["path"]
        n0 = ol.parse_orc(path).stripes[0].num_rows
        for c, nm, sc in ((1, "v_dec", 2), (2, "v_d9", 3)):
            first = _patch_second_scale_run(path, nm, sc, sc - 1)
            # rows of stripe 0 whose dense (non-null) position is >= first
            valid = runs[0]["valid"][c][:n0]
            dense_pos = np.cumsum(valid) - 1
            hit = np.flatnonzero(valid & (dense_pos >= first))
            assert hit.size > 100 and hit[-1] < n0
            runs[0]["values"][c][hit] *= 10
        # the independent reader agrees on what the rewritten file holds
        back = pa_orc.read_table(path)
        for c, nm, sc in ((1, "v_dec", 2), (2, "v_d9", 3)):
            exp = [decimal.Decimal(int(u)).scaleb(-sc) if ok else None
                   for u, ok in zip(runs[0]["values"][c],
                                    runs[0]["valid"][c])]
            assert back.column(nm).to_pylist() == exp, nm
        with Session(0) as s:
            with MergeReadPlan(s, file_descs_from_metas(metas), KEY_COLS,
                               VALUE_COLS) as plan:
                got = _read_all(plan)
        _check_rows(got, runs, *merge_dedup(runs))

    def test_higher_data_scale_fails_the_read(self, tmp_path):
        runs = self._runs()
        metas = _write_orc(runs, str(tmp_path), stripe_size=1)
        _patch_second_scale_run(metas[0]["path"], "v_dec", 2, 3)
        with Session(0) as s:
            with MergeReadPlan(s, file_descs_from_metas(metas), KEY_COLS,
                               VALUE_COLS) as plan:
                with pytest.raises(RuntimeError,
                                   match="ORC decimal rescale.*above the "
                                         "column scale"):
                    _read_all(plan)


class TestOrcDecimalEngines:
    def _runs(self, seed):
        runs = gen_runs_partial_update(N_RUNS, ROWS, n_value_cols=2,
                                       seed=seed, update_frac=0.4,
                                       update_cols=1)
        return _decimal_columns(runs, seed + 1, nullable_dec=True)

    def test_partial_update(self, tmp_path):
        runs = self._runs(1010)
        metas = _write_orc(runs, str(tmp_path), "zlib")
        exp = partial_update_model(runs)
        with Session(0) as s:
            with MergeReadPlan(s, file_descs_from_metas(metas), KEY_COLS,
                               VALUE_COLS,
                               merge_engine="partial-update") as plan:
                got = _read_all(plan)
        _check_model(got, exp)

    def test_aggregation_sum(self, tmp_path):
        runs = self._runs(1020)
        for r in runs:  # bound so no sum leaves its column's precision
            r["values"][1] = r["values"][1] % 10**12
            r["values"][2] = (r["values"][2] % 100_000).astype(np.int32)
        metas = _write_orc(runs, str(tmp_path))
        exp = aggregation_model(runs, ["last_non_null_value", "sum", "sum"])
        with Session(0) as s:
            with MergeReadPlan(s, file_descs_from_metas(metas), KEY_COLS,
                               VALUE_COLS, merge_engine="aggregation",
                               aggregations={"v_dec": "sum",
                                             "v_d9": "sum"}) as plan:
                got = _read_all(plan)
        _check_model(got, exp)


class TestOrcDecimalRejected:
    """Plans that must fail at plan creation, naming file and column."""

    def _one_file(self, tmp_path, dec_array):
        n = len(dec_array)
        tbl = pa.table({
            "_KEY_k": pa.array(np.arange(n, dtype=np.int64)),
            "_SEQUENCE_NUMBER": pa.array(np.arange(n, dtype=np.int64)),
            "_VALUE_KIND": pa.array(np.zeros(n, np.int8)),
            "v_dec": dec_array})
        path = os.path.join(str(tmp_path), "bad.orc")
        pa_orc.write_table(tbl, path, compression="uncompressed")
        return [{"path": path, "rowCount": n, "minKey": 0, "maxKey": n - 1,
                 "level": 0}]

    def _rejected(self, metas, typ, match):
        with Session(0) as s:
            with pytest.raises(RuntimeError, match=match):
                MergeReadPlan(s, file_descs_from_metas(metas), KEY_COLS,
                              [{"name": "v_dec", "type": typ}])

    def test_declared_scale_differs(self, tmp_path):
        metas = self._one_file(tmp_path, _dec_array(
            range(100), [True] * 100, 18, 2))
        self._rejected(metas, "decimal(18,3)",
                       r"bad\.orc col v_dec: declared decimal\(18,3\) but "
                       r"the ORC file holds decimal\(18,2\)")

    def test_precision_above_18_in_file(self, tmp_path):
        metas = self._one_file(tmp_path, _dec_array(
            range(100), [True] * 100, 30, 4))
        self._rejected(metas, "decimal(18,4)",
                       r"bad\.orc col v_dec: ORC DECIMAL precision 30 above "
                       r"18")

    def test_decimal_over_long_column(self, tmp_path):
        metas = self._one_file(tmp_path,
                               pa.array(np.arange(100, dtype=np.int64)))
        self._rejected(metas, "decimal(18,2)",
                       r"bad\.orc col v_dec: declared decimal\(18,2\) but "
                       r"ORC kind is 4")

    def test_decimal_column_declared_int64(self, tmp_path):
        metas = self._one_file(tmp_path, _dec_array(
            range(100), [True] * 100, 18, 2))
        self._rejected(metas, "int64",
                       r"bad\.orc col v_dec: ORC DECIMAL\(18,2\) column read "
                       r"as non-decimal")
