"""BOOLEAN, DATE, TIME and TIMESTAMP columns through the product path.

Files are written by pyarrow (the independent implementation). The expected
result is always the merge oracle / numpy model run over the riding integers
pyarrow reads back FROM THOSE VERY FILES (days, milliseconds of the day,
milliseconds / microseconds since the epoch, 0/1), compared bit-exactly:
key, sequence number, kind, value and validity. The ORC TIMESTAMP files are
the fixtures under tests/golden (pyarrow's ORC writer and reader need a
zoneinfo directory for them), with pyarrow's read-back stored beside them.

Shape: 3 runs x 6 000 rows, so key groups cross the 3 584-row tile cut."""

import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
from pyarrow import orc as pa_orc

from oracle import (aggregation_model, merge_dedup, merge_dedup_useq_model,
                    merge_first_row_model, partial_update_model)
from oracle import orc_light as ol
from paimon_amd import (Session, MergeReadPlan, debug_footer,
                        file_descs_from_metas)
from paimon_amd.compact import rewrite
from paimon_amd.datagen import gen_runs_dedup
from tests import orc_streams as S
from tests import orc_timestamp_model as T

pytestmark = pytest.mark.gpu

KEY_COLS = [{"name": "_KEY_k", "type": "int64"}]
N_RUNS, ROWS = 3, 6000

# name, plan type, arrow type, fraction of nulls
PQ_COLS = [
    ("v_k", "int64", pa.int64(), 0.0),
    ("v_flag", "boolean", pa.bool_(), 0.0),
    ("v_flagn", "boolean", pa.bool_(), 0.3),
    ("v_date", "date", pa.date32(), 0.0),          # dictionary-encoded
    ("v_daten", "date", pa.date32(), 0.3),
    ("v_time", "time", pa.time32("ms"), 0.3),
    ("v_ts3", "timestamp(3)", pa.timestamp("ms"), 0.3),  # dictionary
    ("v_ts6", "timestamp(6)", pa.timestamp("us"), 0.0),
    ("v_ts6n", "timestamp(6)", pa.timestamp("us"), 0.3),
    ("v_ltz", "timestamp_ltz(6)", pa.timestamp("us", tz="UTC"), 0.0),  # DELTA
]
ORC_COLS = [
    ("v_k", "int64", pa.int64(), 0.0),
    ("v_flag", "boolean", pa.bool_(), 0.0),
    ("v_flagn", "boolean", pa.bool_(), 0.3),
    ("v_true", "boolean", pa.bool_(), 0.0),    # pure runs
    ("v_false", "boolean", pa.bool_(), 0.3),   # pure runs under PRESENT
    ("v_alt", "boolean", pa.bool_(), 0.0),     # 0x55 bytes: repeated-byte
                                               # runs that are not 00 / FF
    ("v_date", "date", pa.date32(), 0.0),
    ("v_daten", "date", pa.date32(), 0.3),
    ("v_time", "time", pa.int32(), 0.3),       # ORC has no TIME kind: INT
]


def _value_cols(cols):
    return [{"name": nm, "type": typ} for nm, typ, _, _ in cols]


def _riding_dtype(at):
    if pa.types.is_boolean(at):
        return np.uint8
    if pa.types.is_date32(at) or pa.types.is_time32(at) or \
            pa.types.is_int32(at):
        return np.int32
    return np.int64


def _gen_column(name, at, n, rng, key):
    if name == "v_k":
        return key.copy()
    if name == "v_true":
        return np.ones(n, np.uint8)
    if name == "v_false":
        return np.zeros(n, np.uint8)
    if name == "v_alt":
        return (np.arange(n) % 2).astype(np.uint8)
    if pa.types.is_boolean(at):
        # long stretches of equal values too, so ORC writes runs as well as
        # literal groups
        v = rng.integers(0, 2, n).astype(np.uint8)
        v[n // 4:n // 2] = 1
        return v
    if pa.types.is_date32(at):
        return (19000 + rng.integers(-400, 400, n)).astype(np.int32)
    if pa.types.is_time32(at) or name == "v_time":
        return rng.integers(0, 86_400_000, n).astype(np.int32)
    if name == "v_ts3":  # few distinct values: the dictionary sticks
        return (1_600_000_000_000 +
                rng.integers(0, 300, n) * 86_400_123).astype(np.int64)
    if name == "v_ltz":  # slowly rising: what DELTA_BINARY_PACKED is for
        return 1_700_000_000_000_000 + np.cumsum(
            rng.integers(0, 5_000_000, n)).astype(np.int64)
    # microseconds, before and after 1970
    return rng.integers(-10 ** 15, 4 * 10 ** 15, n, dtype=np.int64)


def _gen_runs(cols, seed, delete_frac=0.1):
    rng = np.random.default_rng(seed)
    runs = gen_runs_dedup(N_RUNS, ROWS, n_value_cols=0, seed=seed,
                          delete_frac=delete_frac)
    for r in runs:
        n = len(r["key"])
        r["values"] = [_gen_column(nm, at, n, rng, r["key"])
                       for nm, _, at, _ in cols]
        r["valid"] = [rng.random(n) >= p if p else np.ones(n, bool)
                      for _, _, _, p in cols]
    return runs


def _arrow_table(run, cols):
    fields = [pa.field("_KEY_k", pa.int64(), nullable=False),
              pa.field("_SEQUENCE_NUMBER", pa.int64(), nullable=False),
              pa.field("_VALUE_KIND", pa.int8(), nullable=False)]
    arrays = [pa.array(run["key"]), pa.array(run["seq"]),
              pa.array(run["kind"])]
    for (nm, _, at, _), v, m in zip(cols, run["values"], run["valid"]):
        fields.append(pa.field(nm, at))
        src = v.astype(bool) if pa.types.is_boolean(at) else v
        arr = pa.array(src, mask=~m)
        arrays.append(arr if pa.types.is_boolean(at) else arr.cast(at))
    return pa.Table.from_arrays(arrays, schema=pa.schema(fields))


def _read_back(tbl, cols):
    """pyarrow's view of a written file, as a run of riding integers."""
    run = {"key": tbl.column("_KEY_k").to_numpy(),
           "seq": tbl.column("_SEQUENCE_NUMBER").to_numpy(),
           "kind": tbl.column("_VALUE_KIND").to_numpy(),
           "values": [], "valid": []}
    for nm, _, at, _ in cols:
        col = tbl.column(nm).combine_chunks()
        dt = _riding_dtype(at)
        if pa.types.is_boolean(at):
            vals = np.asarray(col.fill_null(False)).astype(np.uint8)
        else:
            store = pa.int32() if dt == np.int32 else pa.int64()
            vals = np.asarray(col.cast(store).fill_null(0)).astype(dt)
        run["values"].append(vals)
        run["valid"].append(np.asarray(col.is_valid()))
    return run


def _meta(run, path):
    return {"path": path, "rowCount": len(run["key"]),
            "minKey": int(run["key"][0]), "maxKey": int(run["key"][-1]),
            "level": 0}


def _write_parquet(runs, out_dir, compression):
    """Returns (metas, runs as pyarrow reads them back)."""
    os.makedirs(out_dir, exist_ok=True)
    metas, back = [], []
    for i, run in enumerate(runs):
        path = os.path.join(out_dir, f"run-{i}.parquet")
        # pages close after a multiple of 77 values (write_batch_size) once
        # they pass 64 bytes: several pages per chunk, the boolean ones at
        # 539 values, no multiple of 8
        pq.write_table(_arrow_table(run, PQ_COLS), path,
                       compression=compression,
                       use_dictionary=["v_date", "v_ts3"],
                       column_encoding={"v_ltz": "DELTA_BINARY_PACKED"},
                       data_page_version="1.0", write_statistics=False,
                       store_schema=False, data_page_size=64,
                       write_batch_size=77)
        back.append(_read_back(pq.read_table(path), PQ_COLS))
        metas.append(_meta(run, path))
    return metas, back


def _write_orc(runs, out_dir, compression):
    os.makedirs(out_dir, exist_ok=True)
    metas, back = [], []
    for i, run in enumerate(runs):
        path = os.path.join(out_dir, f"run-{i}.orc")
        pa_orc.write_table(_arrow_table(run, ORC_COLS), path,
                           compression=compression, stripe_size=1)
        back.append(_read_back(pa_orc.read_table(path), ORC_COLS))
        metas.append(_meta(run, path))
    return metas, back


def _read_all(plan):
    got = {}
    while True:
        b = plan.read_next()
        if b is None:
            break
        for kk, v in b.items():
            got.setdefault(kk, []).append(v.copy())
    return {kk: np.concatenate(v) for kk, v in got.items()}


def _plan_read(metas, value_cols, **kw):
    with Session(0) as s:
        with MergeReadPlan(s, file_descs_from_metas(metas), KEY_COLS,
                           value_cols, **kw) as plan:
            got = _read_all(plan)
            logicals = dict(plan.logicals)
    return got, logicals


def _check_column(got, nm, at, ev, em):
    gm = got.get(nm + "#valid")
    if gm is None:
        gm = np.ones(len(got[nm]), dtype=bool)
    assert (gm.astype(bool) == em).all(), nm
    want = np.bool_ if pa.types.is_boolean(at) else _riding_dtype(at)
    assert got[nm].dtype == want, (nm, got[nm].dtype)
    assert (got[nm].astype(ev.dtype)[em] == ev[em]).all(), nm


def _check_rows(got, runs, cols, r, w, sel=None):
    """Winner (run, row) lists against a result. sel = indices of `cols`
    present in the plan (all by default)."""
    for nm, src in (("_KEY_k", "key"), ("_SEQUENCE_NUMBER", "seq"),
                    ("_VALUE_KIND", "kind")):
        e = np.array([runs[a][src][b] for a, b in zip(r, w)])
        assert len(got[nm]) == len(e) and (got[nm] == e).all(), nm
    for c in (range(len(cols)) if sel is None else sel):
        nm, _, at, _ = cols[c]
        ev = np.array([runs[a]["values"][c][b] for a, b in zip(r, w)])
        em = np.array([runs[a]["valid"][c][b] for a, b in zip(r, w)], bool)
        _check_column(got, nm, at, ev, em)


def _check_model(got, exp, cols):
    assert (got["_KEY_k"] == exp["key"]).all()
    assert (got["_SEQUENCE_NUMBER"] == exp["seq"]).all()
    assert (got["_VALUE_KIND"] == exp["kind"]).all()
    for c, (nm, _, at, _) in enumerate(cols):
        _check_column(got, nm, at, exp["values"][c], exp["valid"][c])


EXPECTED_LOGICALS = {"v_date": 1, "v_daten": 1, "v_time": 2, "v_ts3": 3,
                     "v_ts6": 4, "v_ts6n": 4, "v_ltz": 6}


class TestParquet:
    @pytest.mark.parametrize("compression", [None, "zstd"],
                             ids=["uncompressed", "zstd"])
    def test_dedup_all_types(self, tmp_path, compression):
        metas, runs = _write_parquet(_gen_runs(PQ_COLS, 2001),
                                     str(tmp_path), compression)
        # the files hold what the case is about
        foot = debug_footer(metas[0]["path"])
        chunks = {c["name"]: c for c in foot["row_groups"][0]["chunks"]}
        assert chunks["v_flag"]["n_data_pages"] >= 3
        assert chunks["v_flagn"]["n_data_pages"] >= 3
        assert chunks["v_date"]["dict_page_offset"] > 0
        assert chunks["v_ts3"]["dict_page_offset"] > 0
        enc = pq.ParquetFile(metas[0]["path"]).metadata.row_group(0)
        names = [enc.column(i).path_in_schema for i in range(enc.num_columns)]
        assert "DELTA_BINARY_PACKED" in \
            enc.column(names.index("v_ltz")).encodings
        assert "RLE_DICTIONARY" in enc.column(names.index("v_ts3")).encodings
        got, logicals = _plan_read(metas, _value_cols(PQ_COLS))
        _check_rows(got, runs, PQ_COLS, *merge_dedup(runs))
        assert logicals == EXPECTED_LOGICALS

    def test_keep_deletes_single_boolean_column(self, tmp_path):
        # a plan that reads ONE nullable boolean column of the files
        metas, runs = _write_parquet(_gen_runs(PQ_COLS, 2002),
                                     str(tmp_path), None)
        got, _ = _plan_read(metas, [{"name": "v_flagn", "type": "boolean"}],
                            drop_delete=False)
        _check_rows(got, runs, PQ_COLS, *merge_dedup(runs, drop_delete=False),
                    sel=[2])


class TestEngines:
    @pytest.fixture(scope="class")
    def insert_only(self, tmp_path_factory):
        d = str(tmp_path_factory.mktemp("engines"))
        return _write_parquet(_gen_runs(PQ_COLS, 2010, delete_frac=0.0), d,
                              None)

    def test_partial_update(self, insert_only):
        metas, runs = insert_only
        got, _ = _plan_read(metas, _value_cols(PQ_COLS),
                            merge_engine="partial-update")
        _check_model(got, partial_update_model(runs), PQ_COLS)

    def test_aggregation(self, insert_only):
        metas, runs = insert_only
        aggs = {"v_flag": "max", "v_flagn": "last_non_null_value",
                "v_date": "min", "v_daten": "first_non_null_value",
                "v_time": "max", "v_ts3": "last_value", "v_ts6": "max",
                "v_ts6n": "max", "v_ltz": "first_value"}
        names = [c[0] for c in PQ_COLS]
        got, _ = _plan_read(metas, _value_cols(PQ_COLS),
                            merge_engine="aggregation", aggregations=aggs)
        exp = aggregation_model(
            runs, [aggs.get(nm, "last_non_null_value") for nm in names])
        _check_model(got, exp, PQ_COLS)

    def test_first_row(self, insert_only):
        metas, runs = insert_only
        got, _ = _plan_read(metas, _value_cols(PQ_COLS),
                            merge_engine="first-row")
        _check_rows(got, runs, PQ_COLS, *merge_first_row_model(runs))

    def test_timestamp_sequence_field(self, tmp_path):
        # sequence.field = a nullable timestamp(3) column of few distinct
        # values (real ties, nulls first), then a date
        metas, runs = _write_parquet(_gen_runs(PQ_COLS, 2011),
                                     str(tmp_path), None)
        names = [c[0] for c in PQ_COLS]
        idx = [names.index("v_ts3"), names.index("v_daten")]
        got, _ = _plan_read(metas, _value_cols(PQ_COLS),
                            sequence_fields=["v_ts3", "v_daten"])
        _check_rows(got, runs, PQ_COLS, *merge_dedup_useq_model(runs, idx))

    def test_filters_on_a_single_run(self, tmp_path):
        metas, runs = _write_parquet(_gen_runs(PQ_COLS, 2012,
                                               delete_frac=0.0),
                                     str(tmp_path), None)
        run = runs[0]
        names = [c[0] for c in PQ_COLS]
        flag = run["values"][names.index("v_flag")]
        ts = run["values"][names.index("v_ts6")]
        lo, hi = 0, 2 * 10 ** 15
        got, _ = _plan_read(
            metas[:1], _value_cols(PQ_COLS),
            filters=[{"field": "v_flag", "op": "eq", "literal": 1}])
        assert (got["_KEY_k"] == run["key"][flag == 1]).all()
        got, _ = _plan_read(
            metas[:1], _value_cols(PQ_COLS),
            filters=[{"field": "v_ts6", "op": "ge", "literal": lo},
                     {"field": "v_ts6", "op": "lt", "literal": hi}])
        keep = (ts >= lo) & (ts < hi)
        assert 100 < keep.sum() < ROWS
        assert (got["_KEY_k"] == run["key"][keep]).all()
        assert (got["v_ts6"] == ts[keep]).all()


class TestOrcBooleanDate:
    @pytest.mark.parametrize("compression", ["uncompressed", "zlib"])
    def test_dedup(self, tmp_path, compression):
        metas, runs = _write_orc(_gen_runs(ORC_COLS, 2020), str(tmp_path),
                                 compression)
        if compression == "uncompressed":
            fi = ol.parse_orc(metas[0]["path"])
            assert len(fi.stripes) >= 3
        got, logicals = _plan_read(metas, _value_cols(ORC_COLS))
        _check_rows(got, runs, ORC_COLS, *merge_dedup(runs))
        assert logicals == {"v_date": 1, "v_daten": 1, "v_time": 2}

    def test_partial_update(self, tmp_path):
        metas, runs = _write_orc(_gen_runs(ORC_COLS, 2021, delete_frac=0.0),
                                 str(tmp_path), "zlib")
        got, _ = _plan_read(metas, _value_cols(ORC_COLS),
                            merge_engine="partial-update")
        _check_model(got, partial_update_model(runs), ORC_COLS)


TS_COLS = [("v_ts", "timestamp(6)", pa.timestamp("us"), 0.3)]


def _ts_fixture(golden_dir, unit_div=1):
    metas, runs = [], []
    for i in range(3):
        e = np.load(os.path.join(golden_dir, f"orc_ts_run{i}.npy"))
        run = {"key": e[0], "seq": e[1], "kind": e[2].astype(np.int8),
               "values": [e[3] // unit_div], "valid": [e[4].astype(bool)]}
        runs.append(run)
        metas.append(_meta(run, os.path.join(golden_dir,
                                             f"orc_ts_run{i}.orc")))
    return metas, runs


class TestOrcTimestamp:
    @pytest.mark.parametrize("typ,div,logical", [("timestamp(6)", 1, 4),
                                                 ("timestamp(3)", 1000, 3)])
    def test_dedup(self, golden_dir, typ, div, logical):
        metas, runs = _ts_fixture(golden_dir, div)
        got, logicals = _plan_read(metas, [{"name": "v_ts", "type": typ}])
        _check_rows(got, runs, TS_COLS, *merge_dedup(runs))
        assert logicals == {"v_ts": logical}

    def test_timestamp_sequence_field(self, golden_dir):
        metas, runs = _ts_fixture(golden_dir)
        got, _ = _plan_read(metas, [{"name": "v_ts", "type": "timestamp(6)"}],
                            sequence_fields=["v_ts"])
        _check_rows(got, runs, TS_COLS, *merge_dedup_useq_model(runs, [0]))

    def test_first_row_ignoring_deletes(self, golden_dir):
        metas, runs = _ts_fixture(golden_dir)
        got, _ = _plan_read(metas, [{"name": "v_ts", "type": "timestamp(6)"}],
                            merge_engine="first-row", ignore_delete=True)
        _check_rows(got, runs, TS_COLS,
                    *merge_first_row_model(runs, ignore_delete=True))

    def test_pre_1970_fraction_fails_the_read(self, golden_dir, tmp_path):
        # rows 0..2 of run 0 share second 0 (0, 1 and 999 999 us), stored as
        # one SHORT_REPEAT run; rewritten to second -1 the last two become
        # values before 1970 with a fraction
        src = os.path.join(golden_dir, "orc_ts_run0.orc")
        raw = bytearray(open(src, "rb").read())
        fi = ol.parse_orc(src)
        st = ol.find_stream(fi.stripes[0], fi.column_names.index("v_ts") + 1,
                            1)
        h = raw[st.offset]
        width = ((h >> 3) & 7) + 1
        assert h >> 6 == S.SHORT_REPEAT and (h & 7) + 3 == 3 and width == 4
        old = int.from_bytes(raw[st.offset + 1:st.offset + 5], "big")
        assert old == S.zigzag(T.unix(0))
        raw[st.offset + 1:st.offset + 5] = \
            S.zigzag(T.unix(-1)).to_bytes(4, "big")
        path = str(tmp_path / "pre1970.orc")
        open(path, "wb").write(raw)
        metas, _ = _ts_fixture(golden_dir)
        metas[0]["path"] = path
        with Session(0) as s:
            with MergeReadPlan(s, file_descs_from_metas(metas), KEY_COLS,
                               [{"name": "v_ts", "type": "timestamp(6)"}]
                               ) as plan:
                with pytest.raises(RuntimeError,
                                   match="ORC timestamp refused: value "
                                         "before 1970 with a fractional "
                                         "second"):
                    _read_all(plan)


PQ_TYPES = {"v_flag": pa.bool_(), "v_flagn": pa.bool_(),
            "v_date": pa.date32(), "v_daten": pa.date32(),
            "v_time": pa.time32("ms"), "v_ts3": pa.timestamp("ms"),
            "v_ts6": pa.timestamp("us"), "v_ts6n": pa.timestamp("us"),
            "v_ltz": pa.timestamp("us", tz="UTC")}


def _check_compacted(res, runs, cols, types):
    """The rewritten files, by pyarrow (Arrow types and values) and by the
    GPU reader."""
    r, w = merge_dedup(runs, drop_delete=True)
    parts = [pq.read_table(m["path"]) for m in res["after"]]
    assert len(parts) >= 2
    for p in parts:
        for nm, at in types.items():
            assert p.schema.field(nm).type == at, nm
    whole = pa.concat_tables(parts)
    back = _read_back(whole, cols)
    assert (back["key"] == np.array([runs[a]["key"][b]
                                     for a, b in zip(r, w)])).all()
    for c, (nm, _, at, _) in enumerate(cols):
        ev = np.array([runs[a]["values"][c][b] for a, b in zip(r, w)])
        em = np.array([runs[a]["valid"][c][b] for a, b in zip(r, w)], bool)
        assert (back["valid"][c] == em).all(), nm
        assert (back["values"][c][em] == ev[em]).all(), nm
    metas = [dict(m, level=5) for m in res["after"]]
    got, _ = _plan_read(metas, _value_cols(cols))
    assert (got["_KEY_k"] == back["key"]).all()
    for c, (nm, _, at, _) in enumerate(cols):
        _check_column(got, nm, at, back["values"][c], back["valid"][c])


class TestCompaction:
    def test_parquet_mixed_types(self, tmp_path):
        metas, runs = _write_parquet(_gen_runs(PQ_COLS, 2030),
                                     str(tmp_path / "in"), "zstd")
        with Session(0) as s:
            res = rewrite(s, metas, KEY_COLS, _value_cols(PQ_COLS),
                          str(tmp_path / "out"), output_level=5,
                          drop_delete=True, target_file_rows=5000)
        _check_compacted(res, runs, PQ_COLS, PQ_TYPES)

    def test_orc_in_parquet_out(self, tmp_path):
        metas, runs = _write_orc(_gen_runs(ORC_COLS, 2031),
                                 str(tmp_path / "in"), "zlib")
        with Session(0) as s:
            res = rewrite(s, metas, KEY_COLS, _value_cols(ORC_COLS),
                          str(tmp_path / "out"), output_level=5,
                          drop_delete=True, target_file_rows=5000)
        # the ORC INT column declared `time` comes back as Parquet TIME
        _check_compacted(res, runs, ORC_COLS,
                         dict({nm: at for nm, _, at, _ in ORC_COLS[1:]},
                              v_time=pa.time32("ms")))


class TestRejected:
    @pytest.fixture(scope="class")
    def files(self, tmp_path_factory):
        d = str(tmp_path_factory.mktemp("rejected"))
        return _write_parquet(_gen_runs(PQ_COLS, 2040), d, None)[0]

    def _rejected(self, metas, match, key_cols=KEY_COLS,
                  value_cols=None, **kw):
        with Session(0) as s:
            with pytest.raises(RuntimeError, match=match):
                MergeReadPlan(s, file_descs_from_metas(metas), key_cols,
                              value_cols or _value_cols(PQ_COLS), **kw)

    def test_key_column_of_a_new_type(self, files):
        self._rejected(files, "key column '_KEY_k': a date key column is a "
                              "later round",
                       key_cols=[{"name": "_KEY_k", "type": "date"}])

    def test_timestamp_precision_9(self, files):
        self._rejected(files, r"timestamp\(9\): timestamp precision 9 is "
                              "not supported",
                       value_cols=[{"name": "v_ts6", "type": "timestamp(9)"}])

    def test_sum_over_a_boolean(self, files):
        self._rejected(files, "aggregate 'sum' on boolean column 'v_flag' "
                              "is not supported",
                       merge_engine="aggregation",
                       aggregations={"v_flag": "sum"})

    def test_parquet_unit_mismatch(self, files):
        self._rejected(files, r"column v_ts6 declared timestamp\(3\) "
                              r"\(MILLIS\) but the file's TIMESTAMP unit is "
                              r"MICROS",
                       value_cols=[{"name": "v_ts6", "type": "timestamp(3)"}])

    def test_non_utc_writer_timezone(self, golden_dir, tmp_path):
        raw = bytearray(open(os.path.join(golden_dir, "orc_ts_run0.orc"),
                             "rb").read())
        at = raw.rfind(b"\x1a\x03GMT")
        assert at > 0
        raw[at + 2:at + 5] = b"PST"
        path = str(tmp_path / "pst.orc")
        open(path, "wb").write(raw)
        metas, _ = _ts_fixture(golden_dir)
        self._rejected([dict(metas[0], path=path)],
                       "ORC TIMESTAMP written in timezone 'PST' is not "
                       "supported",
                       value_cols=[{"name": "v_ts", "type": "timestamp(6)"}])
