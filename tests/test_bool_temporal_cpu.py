"""BOOLEAN, DATE, TIME and TIMESTAMP columns, everything that needs no GPU:
the host modes of the two stream-level debug entries against plain-Python
models (tests/bits_model.py, tests/orc_timestamp_model.py) and the oracle's
ORC boolean decoder, the Parquet footer annotations and the staging checks
of a declared type against a file, and the native Parquet writer's output
read back by pyarrow."""

import os
import re

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from oracle import orc_light as ol
from oracle.oracle import orc_boolrle_decode
from paimon_amd import (debug_bits, debug_check_column, debug_footer,
                        debug_orc_timestamp, write_parquet)
from paimon_amd.reader import (BITS_BYTE_RLE, BITS_HOST, BITS_LSB, BITS_MSB,
                               BITS_RAW, LT_DATE, LT_TIME_MILLIS,
                               LT_TIMESTAMP_LTZ_MICROS, LT_TIMESTAMP_MICROS,
                               LT_TIMESTAMP_MILLIS, ORC_TS_HOST,
                               ORC_TS_MICROS, ORC_TS_MILLIS)
from tests import bits_model as B
from tests import orc_streams as S
from tests import orc_timestamp_model as T

ORDERS = [BITS_LSB, BITS_MSB]


def _host(stream, n, order, fmt, **kw):
    return debug_bits(stream, n, order, fmt, BITS_HOST, **kw)


class TestBitsHost:
    @pytest.mark.parametrize("order", ORDERS)
    @pytest.mark.parametrize("n", B.COUNTS)
    def test_raw_bits(self, n, order):
        rng = np.random.default_rng(n * 2 + order)
        vals = [int(x) for x in rng.integers(0, 2, n)]
        got = _host(B.pack(vals, order), n, order, BITS_RAW)
        assert got.dtype == np.uint8 and got.tolist() == vals

    @pytest.mark.parametrize("order", ORDERS)
    @pytest.mark.parametrize("n", B.COUNTS)
    def test_byte_rle(self, n, order):
        rng = np.random.default_rng(1000 + n * 2 + order)
        stream, data, _ = B.random_byte_rle(rng, n)
        exp = B.expand_raw(data, n, order)
        assert B.expand_byte_rle(stream, n, order) == exp  # model vs model
        assert _host(stream, n, order, BITS_BYTE_RLE).tolist() == exp
        if order == BITS_MSB:  # ORC's own order: the oracle's C decoder
            assert orc_boolrle_decode(stream, n).astype(int).tolist() == exp

    @pytest.mark.parametrize("order", ORDERS)
    @pytest.mark.parametrize("plan", [[("run", 3)], [("run", 130)],
                                      [("lit", 1)], [("lit", 128)]],
                             ids=["run3", "run130", "lit1", "lit128"])
    def test_extreme_units(self, plan, order):
        rng = np.random.default_rng(7)
        kind, k = plan[0]
        data = bytes([0xB1]) * k if kind == "run" else \
            bytes(int(x) for x in rng.integers(0, 256, k))
        stream = B.byte_rle_segments(data, plan)
        for n in (k * 8, k * 8 - 5):  # whole unit, and a padded last byte
            exp = B.expand_raw(data, n, order)
            assert _host(stream, n, order, BITS_BYTE_RLE).tolist() == exp

    @pytest.mark.parametrize("fmt", [BITS_RAW, BITS_BYTE_RLE])
    @pytest.mark.parametrize("out_shift", range(8))
    def test_every_output_alignment_and_width(self, out_shift, fmt):
        # the host mode walks the kernel's group geometry: the same values
        # at every residue of the first output element, 1- and 4-byte wide
        n = 513
        rng = np.random.default_rng(40 + out_shift)
        if fmt == BITS_RAW:
            vals = [int(x) for x in rng.integers(0, 2, n)]
            stream, order = B.pack(vals, BITS_LSB), BITS_LSB
        else:
            stream, data, _ = B.random_byte_rle(rng, n, (3, 9), (1, 5))
            vals, order = B.expand_raw(data, n, BITS_MSB), BITS_MSB
        for esize, dt in ((1, np.uint8), (4, np.int32)):
            got = _host(stream, n, order, fmt, out_esize=esize,
                        out_shift=out_shift)
            assert got.dtype == dt and got.tolist() == vals

    def test_truncated_streams_are_refused(self):
        with pytest.raises(RuntimeError, match="fewer bits than"):
            _host(b"\xff", 9, BITS_LSB, BITS_RAW)
        with pytest.raises(RuntimeError, match="fewer values than"):
            _host(S.byte_run(-1, 3), 25, BITS_MSB, BITS_BYTE_RLE)
        with pytest.raises(RuntimeError, match="run truncated"):
            _host(bytes([0x05]), 8, BITS_MSB, BITS_BYTE_RLE)
        with pytest.raises(RuntimeError, match="literal truncated"):
            _host(bytes([0xFE, 0x01]), 16, BITS_MSB, BITS_BYTE_RLE)
        # a literal group cut short by the value count needs only the bytes
        # its values occupy
        assert _host(bytes([0xFE, 0x80]), 8, BITS_MSB,
                     BITS_BYTE_RLE).tolist() == [1, 0, 0, 0, 0, 0, 0, 0]

    def test_bad_arguments(self):
        with pytest.raises(RuntimeError, match="bad arguments"):
            debug_bits(b"\x00", 8, BITS_LSB, BITS_RAW, BITS_HOST,
                       out_esize=2)
        with pytest.raises(RuntimeError, match="bad arguments"):
            debug_bits(b"\x00", 8, BITS_LSB, BITS_RAW, BITS_HOST,
                       out_shift=8)


UNITS = [ORC_TS_MILLIS, ORC_TS_MICROS]


class TestOrcTimestampHost:
    @pytest.mark.parametrize("unit", UNITS, ids=["millis", "micros"])
    def test_value_matrix(self, unit):
        pairs = T.positive_pairs(unit)
        exp = [T.value(s, v, unit) for s, v in pairs]
        data, sec = T.streams(pairs)
        got = debug_orc_timestamp(data, sec, len(pairs), unit, ORC_TS_HOST)
        assert got.tolist() == exp
        # the matrix holds what it says: every code, both limits
        assert {v & 7 for _, v in pairs} == set(range(8))
        assert max(exp) > (1 << 63) - 10 ** 6 and \
            min(exp) < -(1 << 63) + 10 ** 6

    def test_model_pins_the_formula(self):
        # the issue's own statement of the arithmetic, spelled out once
        assert T.decode_nanos((5 << 3) | 7) == 500_000_000
        assert T.decode_nanos(123 << 3) == 123
        assert T.value(0, 0, T.MICROS) == 1_420_070_400 * 10 ** 6
        assert T.value(T.unix(1), T.encode_nanos(1_999_999), T.MICROS) == \
            1_001_999
        assert T.value(T.unix(1), T.encode_nanos(1_999_999), T.MILLIS) == 1001

    @pytest.mark.parametrize("unit", UNITS, ids=["millis", "micros"])
    @pytest.mark.parametrize("case", range(7))
    def test_refusals(self, case, unit):
        name, pair, text = T.refusal_cases(unit)[case]
        with pytest.raises(T.Refused, match=re.escape(text)):
            T.value(pair[0], pair[1], unit)
        # the refused value sits among good ones
        pairs = T.positive_pairs(unit)[:5] + [pair] + \
            T.positive_pairs(unit)[5:8]
        data, sec = T.streams(pairs)
        with pytest.raises(RuntimeError,
                           match="ORC timestamp refused at value 5: .*" +
                                 re.escape(text)):
            debug_orc_timestamp(data, sec, len(pairs), unit, ORC_TS_HOST)

    def test_stream_lengths_must_agree(self):
        data, sec = T.streams([(0, 0)] * 10)
        with pytest.raises(RuntimeError, match="RLEv2 stream overrun"):
            debug_orc_timestamp(data, sec, 12, ORC_TS_MICROS, ORC_TS_HOST)

    @pytest.mark.parametrize("run", range(3))
    def test_pyarrow_written_values(self, golden_dir, run):
        """pyarrow-written streams (fixture) decode to pyarrow's own
        read-back, in both units."""
        path = os.path.join(golden_dir, f"orc_ts_run{run}.orc")
        exp = np.load(os.path.join(golden_dir, f"orc_ts_run{run}.npy"))
        valid = exp[4].astype(bool)
        fi = ol.parse_orc(path)
        assert len(fi.stripes) == 1
        cid = fi.column_names.index("v_ts") + 1
        raw = open(path, "rb").read()
        st = {k: ol.find_stream(fi.stripes[0], cid, k) for k in (1, 5)}
        data = raw[st[1].offset:st[1].offset + st[1].length]
        sec = raw[st[5].offset:st[5].offset + st[5].length]
        n = int(valid.sum())
        assert 1000 < n < 2000
        us = debug_orc_timestamp(data, sec, n, ORC_TS_MICROS, ORC_TS_HOST)
        assert (us == exp[3][valid]).all()
        ms = debug_orc_timestamp(data, sec, n, ORC_TS_MILLIS, ORC_TS_HOST)
        assert (ms == exp[3][valid] // 1000).all()


def _temporal_table(n=100):
    days = np.arange(n, dtype=np.int32) * 37 - 500
    ms_of_day = (np.arange(n, dtype=np.int64) * 864_001 % 86_400_000) \
        .astype(np.int32)
    ts = np.arange(n, dtype=np.int64) * 1_000_003 - 10 ** 9
    return pa.table({
        "d": pa.array(days, pa.date32()),
        "t": pa.array(ms_of_day, pa.time32("ms")),
        "ts_ms": pa.array(ts, pa.timestamp("ms")),
        "ts_us": pa.array(ts, pa.timestamp("us")),
        "ts_us_tz": pa.array(ts, pa.timestamp("us", tz="UTC")),
        "ts_ns": pa.array(ts, pa.timestamp("ns")),
        "plain64": pa.array(ts),
        "b": pa.array(np.arange(n) % 3 == 0),
    })


@pytest.fixture(scope="module")
def temporal_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("temporal") / "t.parquet")
    pq.write_table(_temporal_table(), path, compression=None,
                   use_dictionary=False, data_page_version="1.0",
                   store_schema=False, version="2.6")
    return path


class TestParquetFooter:
    def test_annotations_are_reported(self, temporal_file):
        cols = {c["name"]: c for c in debug_footer(temporal_file)["columns"]}
        assert cols["d"]["phys"] == 1 and cols["d"]["logical"] == 6 and \
            cols["d"]["converted"] == 6
        assert cols["t"]["phys"] == 1 and cols["t"]["logical"] == 7 and \
            cols["t"]["unit"] == "MILLIS"
        assert cols["ts_ms"]["phys"] == 2 and cols["ts_ms"]["logical"] == 8 \
            and cols["ts_ms"]["unit"] == "MILLIS" and \
            cols["ts_ms"]["utc"] is False
        assert cols["ts_us"]["unit"] == "MICROS" and \
            cols["ts_us"]["utc"] is False
        assert cols["ts_us_tz"]["unit"] == "MICROS" and \
            cols["ts_us_tz"]["utc"] is True and \
            cols["ts_us_tz"]["converted"] == 10
        assert cols["ts_ns"]["unit"] == "NANOS"
        assert cols["plain64"]["logical"] == 0 and \
            cols["plain64"]["converted"] == -1 and \
            cols["plain64"]["unit"] == "none"
        assert cols["b"]["phys"] == 0

    @pytest.mark.parametrize("column,typ", [
        ("d", "date"), ("t", "time"), ("ts_ms", "timestamp(3)"),
        ("ts_ms", "timestamp(0)"), ("ts_us", "timestamp(6)"),
        ("ts_us", "timestamp"), ("ts_us", "timestamp(4)"),
        ("ts_us_tz", "timestamp_ltz(6)"), ("b", "boolean")])
    def test_matching_declarations_pass(self, temporal_file, column, typ):
        debug_check_column(temporal_file, column, typ)

    @pytest.mark.parametrize("column,typ,text", [
        ("ts_us", "timestamp(3)",
         r"declared timestamp\(3\) \(MILLIS\) but the file's TIMESTAMP unit "
         r"is MICROS"),
        ("ts_ms", "timestamp(6)",
         r"declared timestamp\(6\) \(MICROS\) but the file's TIMESTAMP unit "
         r"is MILLIS"),
        ("ts_ns", "timestamp(6)", r"TIMESTAMP unit is NANOS"),
        ("plain64", "timestamp(6)", r"carries no TIMESTAMP annotation"),
        ("plain64", "timestamp_ltz(3)", r"carries no TIMESTAMP annotation"),
        ("ts_us", "date", r"declared date but the file's physical type is 2"),
        ("d", "time", r"carries no TIME annotation"),
        ("t", "date", r"carries no DATE annotation"),
        ("d", "boolean", r"declared boolean but the file's physical type"),
        ("ts_us", "timestamp(9)", r"timestamp precision 9 is not supported"),
        ("ts_us", "timestamp(7)", r"timestamp precision 7 is not supported"),
    ])
    def test_refusals(self, temporal_file, column, typ, text):
        with pytest.raises(RuntimeError, match=text):
            debug_check_column(temporal_file, column, typ)

    def test_time_in_microseconds_is_refused(self, tmp_path):
        path = str(tmp_path / "t64.parquet")
        pq.write_table(pa.table({"t": pa.array([1, 2], pa.time64("us"))}),
                       path, store_schema=False)
        with pytest.raises(RuntimeError, match="physical type is 2"):
            debug_check_column(path, "t", "time")

    def test_rle_boolean_pages_are_refused(self, tmp_path):
        path = str(tmp_path / "rle.parquet")
        pq.write_table(pa.table({"b": pa.array([True, False, True] * 50)}),
                       path, compression=None, use_dictionary=False,
                       data_page_version="1.0", store_schema=False,
                       column_encoding={"b": "RLE"})
        with pytest.raises(RuntimeError,
                           match="boolean pages in RLE encoding are not "
                                 "supported"):
            debug_check_column(path, "b", "boolean")


class TestOrcColumnCheck:
    def test_fixture_is_a_utc_timestamp_column(self, golden_dir):
        path = os.path.join(golden_dir, "orc_ts_run0.orc")
        debug_check_column(path, "v_ts", "timestamp(6)")
        debug_check_column(path, "v_ts", "timestamp(3)")

    @pytest.mark.parametrize("typ,text", [
        ("timestamp_ltz(6)", r"declared timestamp_ltz\(6\) but ORC kind is 9"),
        ("int64", "ORC TIMESTAMP column read as another type"),
        ("date", "declared date but ORC kind is 9"),
        ("boolean", "declared boolean but ORC kind is 9")])
    def test_kind_mismatches(self, golden_dir, typ, text):
        with pytest.raises(RuntimeError, match=text):
            debug_check_column(os.path.join(golden_dir, "orc_ts_run0.orc"),
                               "v_ts", typ)

    def test_non_utc_writer_timezone(self, golden_dir, tmp_path):
        # the stripe footer's writerTimezone, rewritten in place
        path = str(tmp_path / "pst.orc")
        raw = bytearray(open(os.path.join(golden_dir, "orc_ts_run0.orc"),
                             "rb").read())
        at = raw.rfind(b"\x1a\x03GMT")
        assert at > 0 and raw.count(b"\x1a\x03GMT") == 1
        raw[at + 2:at + 5] = b"PST"
        open(path, "wb").write(raw)
        with pytest.raises(RuntimeError,
                           match="ORC TIMESTAMP written in timezone 'PST' "
                                 "is not supported"):
            debug_check_column(path, "v_ts", "timestamp(6)")
        raw[at + 2:at + 5] = b"UTC"
        open(path, "wb").write(raw)
        debug_check_column(path, "v_ts", "timestamp(6)")


class TestWriter:
    N = 1003  # not a multiple of 8

    def _columns(self):
        rng = np.random.default_rng(5)
        n = self.N
        return {
            "b": rng.random(n) < 0.5,
            "bn": rng.random(n) < 0.5,
            "d": rng.integers(-30000, 60000, n).astype(np.int32),
            "t": rng.integers(0, 86_400_000, n).astype(np.int32),
            "ts3": rng.integers(-10 ** 12, 4 * 10 ** 12, n, dtype=np.int64),
            "ts6": rng.integers(-10 ** 15, 4 * 10 ** 15, n, dtype=np.int64),
            "ltz": rng.integers(0, 4 * 10 ** 15, n, dtype=np.int64),
        }, {nm: rng.random(n) >= 0.3 for nm in ("bn", "d", "ts6", "ltz")}

    LOGICALS = {"d": LT_DATE, "t": LT_TIME_MILLIS,
                "ts3": LT_TIMESTAMP_MILLIS, "ts6": LT_TIMESTAMP_MICROS,
                "ltz": LT_TIMESTAMP_LTZ_MICROS}
    TYPES = {"b": pa.bool_(), "bn": pa.bool_(), "d": pa.date32(),
             "t": pa.time32("ms"), "ts3": pa.timestamp("ms"),
             "ts6": pa.timestamp("us"),
             "ltz": pa.timestamp("us", tz="UTC")}

    @pytest.mark.parametrize("compression", ["NONE", "zstd"])
    def test_pyarrow_reads_types_and_values(self, tmp_path, compression):
        vals, valid = self._columns()
        path = str(tmp_path / "w.parquet")
        # pages of 77 rows: every page but the first starts at a row that is
        # no multiple of 8, and restarts its bit-packing on a byte boundary
        write_parquet(path, [(nm, v, valid.get(nm)) for nm, v in vals.items()],
                      page_rows=77, row_group_rows=500,
                      compression=compression, logicals=self.LOGICALS)
        tbl = pq.read_table(path)
        assert tbl.num_rows == self.N
        for nm, v in vals.items():
            col = tbl.column(nm).combine_chunks()
            assert col.type == self.TYPES[nm], nm
            m = valid.get(nm)
            got_valid = np.asarray(col.is_valid())
            assert (got_valid == (m if m is not None
                                  else np.ones(self.N, bool))).all(), nm
            store = pa.bool_() if v.dtype == np.bool_ else \
                pa.from_numpy_dtype(v.dtype)
            got = np.asarray(col.cast(store).fill_null(v.dtype.type(0)))
            sel = got_valid
            assert (got[sel] == v[sel]).all(), nm
        # the library's own footer parser sees what it wrote
        cols = {c["name"]: c for c in debug_footer(path)["columns"]}
        assert cols["b"]["phys"] == 0 and cols["bn"]["max_def"] == 1
        assert cols["ltz"]["utc"] is True and cols["ts6"]["utc"] is False
        for nm, typ in (("b", "boolean"), ("d", "date"), ("t", "time"),
                        ("ts3", "timestamp(3)"), ("ts6", "timestamp(6)"),
                        ("ltz", "timestamp_ltz(6)")):
            debug_check_column(path, nm, typ)

    def test_annotation_on_the_wrong_width_is_refused(self, tmp_path):
        with pytest.raises(RuntimeError, match="does not fit dtype"):
            write_parquet(str(tmp_path / "x.parquet"),
                          [("d", np.zeros(4, np.int64))],
                          logicals={"d": LT_DATE})
