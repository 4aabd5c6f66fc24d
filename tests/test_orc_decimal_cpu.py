"""ORC DECIMAL decode on the host: the staging prescan (prescan_varint) plus
the scalar core k_orc_varint shares (orc_decimal_core.h), through
pmh_debug_orc_decimal mode 0, against the independent Python decoder of
tests/orc_decimal_streams.py and against pyarrow-written ORC files. No GPU.

Precision 19 (ORC_DECIMAL_FULL_RANGE) stands for the whole int64 range: a
10-byte varint holds a zigzag code of 2^63 or more, a magnitude no
decimal(p <= 18) column admits, so the length and extreme-value cases run
under it."""

import decimal
import os

import numpy as np
import pyarrow as pa
import pytest
from pyarrow import orc as pa_orc

from oracle import orc_light as ol
from paimon_amd.reader import (ORC_DECIMAL_FULL_RANGE, ORC_DECIMAL_HOST,
                               debug_orc_decimal)
from tests import orc_decimal_streams as D

STREAM_SECONDARY = 5
FULL = ORC_DECIMAL_FULL_RANGE


def _host(values, precision, scale, scales=None, esize=8):
    """Encode, decode with the Python decoder and with the product's host
    mode; the two must agree element for element."""
    stream = D.encode(values)
    ref = D.decode(stream, len(values), precision, scale, scales,
                   out_bits=esize * 8)
    got = debug_orc_decimal(stream, len(values), precision, scale,
                            ORC_DECIMAL_HOST, scales=scales, out_esize=esize)
    assert got.dtype == (np.int32 if esize == 4 else np.int64)
    assert [int(x) for x in got] == ref
    return ref


class TestHostVsPythonDecoder:
    def test_every_length_both_signs(self):
        vals = [D.with_length(n, sg, salt)
                for n in range(1, 11) for sg in (1, -1) for salt in range(7)]
        lens = {n for _, n in D.value_starts(vals)}
        assert lens == set(range(1, 11))
        ref = _host(vals, FULL, 0)
        assert ref == vals  # the Python decoder inverts the encoder

    def test_extremes_at_column_scale(self):
        vals = [0, 1, -1, 10**18 - 1, -(10**18 - 1)]
        for s in (0, 2, 18):
            assert _host(vals, 18, s) == vals
        wide = vals + [D.INT64_MIN, D.INT64_MAX]
        for s in (0, 2, 18):
            assert _host(wide, FULL, s) == wide

    @pytest.mark.parametrize("n", [1, 511, 512, 513, 1025])
    def test_counts_across_unit_boundaries(self, n):
        rng = np.random.default_rng(500 + n)
        vals = [D.with_length(int(ln), 1 if sg else -1, i)
                for i, (ln, sg) in enumerate(zip(rng.integers(1, 11, n),
                                                 rng.integers(0, 2, n)))]
        _host(vals, FULL, 0)

    def test_per_value_scales_every_0_to_18(self):
        # one-digit magnitudes rescale by up to 10^17 inside decimal(18,18)
        # (data scale 0 leaves room for 0 only)...
        vals, scales = [], []
        for ds in range(19):
            for m in ((0, 1, -1, 9, -9) if ds else (0,)):
                vals.append(m)
                scales.append(ds)
        # ...and the largest magnitude each data scale leaves room for
        for ds in range(19):
            m = 10**ds - 1
            vals += [m, -m]
            scales += [ds, ds]
        ref = _host(vals, 18, 18, scales=scales)
        # spot checks against plain arithmetic
        assert ref[scales.index(3) + 3] == 9 * 10**15
        assert ref[-1] == -(10**18 - 1) and ref[-2] == 10**18 - 1

    def test_int32_output_precision_9(self):
        rng = np.random.default_rng(520)
        vals = [0, 1, -1, 10**9 - 1, -(10**9 - 1)]
        vals += [int(x) for x in rng.integers(-(10**9) + 1, 10**9, 600)]
        assert _host(vals, 9, 3, esize=4) == vals
        scales = [int(x) for x in rng.integers(0, 4, 300)]
        small = [int(x) for x in rng.integers(-(10**6) + 1, 10**6, 300)]
        _host(small, 9, 3, scales=scales, esize=4)


def _orc_decimal_streams(path, column):
    """(DATA bytes, SECONDARY bytes) of the column, per stripe."""
    fi = ol.parse_orc(path)
    cid = fi.column_names.index(column) + 1
    with open(path, "rb") as f:
        raw = f.read()
    out = []
    for st in fi.stripes:
        d = ol.find_stream(st, cid, ol.STREAM_DATA)
        s = ol.find_stream(st, cid, STREAM_SECONDARY)
        assert d is not None and s is not None
        out.append((raw[d.offset:d.offset + d.length],
                    raw[s.offset:s.offset + s.length]))
    return out


class TestHostVsPyarrow:
    @pytest.mark.parametrize("p,s", [(18, 2), (9, 3), (18, 0)])
    @pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
    def test_pyarrow_written_column(self, tmp_path, p, s, nulls):
        rng = np.random.default_rng(600 + p + s + nulls)
        n = 3000
        lim = 10**p
        unscaled = [int(x) for x in rng.integers(-lim + 1, lim, n)]
        unscaled[:5] = [0, 1, -1, lim - 1, -(lim - 1)]
        valid = (rng.random(n) > 0.3) if nulls else np.ones(n, bool)
        pyvals = [decimal.Decimal(u).scaleb(-s) if ok else None
                  for u, ok in zip(unscaled, valid)]
        tbl = pa.table({"d": pa.array(pyvals, pa.decimal128(p, s))})
        path = os.path.join(str(tmp_path), "dec.orc")
        pa_orc.write_table(tbl, path, compression="uncompressed")
        # pyarrow reads its own file back to the same decimals
        back = pa_orc.read_table(path).column("d")
        assert back.type == pa.decimal128(p, s)
        assert back.to_pylist() == pyvals
        streams = _orc_decimal_streams(path, "d")
        assert len(streams) == 1
        data, _secondary = streams[0]
        dense = [u for u, ok in zip(unscaled, valid) if ok]
        got = debug_orc_decimal(data, len(dense), p, s, ORC_DECIMAL_HOST,
                                out_esize=4 if p <= 9 else 8)
        assert [int(x) for x in got] == dense


class TestMalformed:
    def _rejected(self, stream, n, p, s, match, scales=None):
        with pytest.raises(RuntimeError, match=match):
            debug_orc_decimal(stream, n, p, s, ORC_DECIMAL_HOST,
                              scales=scales)

    def test_stream_ends_mid_value(self):
        stream = D.encode([5, 1 << 40])
        self._rejected(stream[:-1], 2, FULL, 0, "ends inside a value")
        with pytest.raises(ValueError):
            D.decode(stream[:-1], 2, FULL, 0)

    def test_eleven_byte_value(self):
        stream = D.encode([7]) + bytes([0x80] * 10 + [0x00])
        self._rejected(stream, 2, FULL, 0, "longer than 10 bytes")
        with pytest.raises(ValueError):
            D.decode(stream, 2, FULL, 0)

    def test_ten_byte_value_wider_than_64_bits(self):
        stream = bytes([0xFF] * 9 + [0x02])
        self._rejected(stream, 1, FULL, 0, "more than 64 bits")
        with pytest.raises(ValueError):
            D.decode(stream, 1, FULL, 0)

    def test_fewer_values_than_asked(self):
        stream = D.encode([1, 2, 3])
        self._rejected(stream, 4, 18, 2, "fewer values")
        with pytest.raises(ValueError):
            D.decode(stream, 4, 18, 2)

    def test_data_scale_above_column_scale(self):
        stream = D.encode([100, 200])
        self._rejected(stream, 2, 18, 2, "ORC decimal rescale.*above the "
                       "column scale", scales=[2, 3])
        with pytest.raises(D.DecimalRangeError):
            D.decode(stream, 2, 18, 2, scales=[2, 3])

    def test_negative_data_scale(self):
        stream = D.encode([100])
        self._rejected(stream, 1, 18, 2, "ORC decimal rescale.*negative",
                       scales=[-1])

    def test_rescale_overflows_precision(self):
        # 10^16 at data scale 0 needs 19 digits at scale 2
        stream = D.encode([10**16])
        self._rejected(stream, 1, 18, 2, "ORC decimal rescale.*precision",
                       scales=[0])
        with pytest.raises(D.DecimalRangeError):
            D.decode(stream, 1, 18, 2, scales=[0])
        # at the column scale: exactly 10^p is one too many
        self._rejected(D.encode([10**18]), 1, 18, 2,
                       "ORC decimal rescale.*precision")
        assert int(debug_orc_decimal(D.encode([10**18 - 1]), 1, 18, 2,
                                     ORC_DECIMAL_HOST)[0]) == 10**18 - 1
