"""k_orc_varint on the device, stream by stream: every varint length and sign,
counts around the 64-lane and 512-value edges, every byte alignment of the
aligned 8-byte loads, the fullest span table and the densest terminator
masks, per-value scales, both output widths and the extreme values, bit for
bit against the independent Python decoder of tests/orc_decimal_streams.py.

Every device call runs between two guard zones: a store outside the output
fails the call (AssertionError from debug_orc_decimal) instead of faulting,
and an element the kernel never wrote reads back as 0xA5A5..., which no
expected value here equals. Precision 19 (ORC_DECIMAL_FULL_RANGE) is the
whole int64 range, which 10-byte varints need."""

import numpy as np
import pytest

from paimon_amd.reader import (ORC_DECIMAL_DEVICE, ORC_DECIMAL_FULL_RANGE,
                               debug_orc_decimal)
from tests import orc_decimal_streams as D

pytestmark = pytest.mark.gpu

FULL = ORC_DECIMAL_FULL_RANGE
COUNTS = (1, 63, 64, 65, 511, 512, 513, 1024, 1025)
UNWRITTEN = (-0x5A5A5A5A5A5A5A5B, -0x5A5A5A5B)  # 0xA5.. as int64 / int32


def _device(values, precision, scale, scales=None, esize=8, src_shift=0):
    stream = D.encode(values)
    ref = D.decode(stream, len(values), precision, scale, scales,
                   out_bits=esize * 8)
    assert not set(ref) & set(UNWRITTEN)
    got = debug_orc_decimal(stream, len(values), precision, scale,
                            ORC_DECIMAL_DEVICE, scales=scales,
                            out_esize=esize, src_shift=src_shift)
    assert got.dtype == (np.int32 if esize == 4 else np.int64)
    exp = np.array(ref, dtype=got.dtype)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (bad[:5], got[bad[:5]], exp[bad[:5]])
    return ref


def _mixed_lengths(n, seed):
    """n values cycling through every (length, sign), salted."""
    combos = [(ln, sg) for ln in range(1, 11) for sg in (1, -1)]
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(combos))
    return [D.with_length(*combos[order[i % len(combos)]], salt=seed + i)
            for i in range(n)]


class TestLengths:
    @pytest.mark.parametrize("n", COUNTS)
    def test_every_length_and_sign_at_count(self, n):
        # one stream per (length, sign) at this count, then all mixed
        for ln in range(1, 11):
            for sg in (1, -1):
                vals = [D.with_length(ln, sg, salt) for salt in range(n)]
                assert {b for _, b in D.value_starts(vals)} == {ln}
                _device(vals, FULL, 0)
        _device(_mixed_lengths(n, 700 + n), FULL, 0)

    def test_fullest_span_table(self):
        # 512 values of 10 bytes: one unit of 5120 bytes, the largest end
        # offsets the 16-bit table holds; a 513th value opens a second unit
        for n in (512, 513):
            vals = [D.with_length(10, 1 if i % 3 else -1, i)
                    for i in range(n)]
            assert len(D.encode(vals)) == 10 * n
            _device(vals, FULL, 0)

    def test_densest_terminator_masks(self):
        # 1-byte values: every byte of every loaded word ends a value
        for n in (512, 513, 1024):
            vals = [D.with_length(1, 1 if i % 2 else -1, i)
                    for i in range(n)]
            assert len(D.encode(vals)) == n
            _device(vals, 18, 2)


class TestAlignment:
    def test_every_residue(self):
        body = _mixed_lengths(700, 800)
        seen = set()
        straddles = set()
        for shift in range(8):
            _device(body, FULL, 0, src_shift=shift)
            for off, ln in D.value_starts(body, lead=shift):
                seen.add(off % 8)
                if off // 8 != (off + ln - 1) // 8:
                    straddles.add(ln)
        # value starts on every residue mod 8, and at every length of 2 or
        # more a value that crosses an 8-byte load boundary
        assert seen == set(range(8))
        assert straddles == set(range(2, 11))


class TestScalesAndWidths:
    def test_extremes(self):
        vals = [0, 1, -1, 10**18 - 1, -(10**18 - 1)]
        assert _device(vals, 18, 2) == vals
        wide = vals + [D.INT64_MIN, D.INT64_MAX]
        assert _device(wide, FULL, 0) == wide

    @pytest.mark.parametrize("esize", [8, 4])
    def test_varying_scales(self, esize):
        p, s = (18, 18) if esize == 8 else (9, 9)
        rng = np.random.default_rng(900 + esize)
        n = 1100
        scales = [int(x) for x in rng.integers(0, s + 1, n)]
        # the largest magnitudes each data scale leaves room for, and small
        # ones
        vals = []
        for i, ds in enumerate(scales):
            top = 10**(p - s + ds) - 1
            m = top if i % 4 == 0 else int(rng.integers(0, top + 1))
            vals.append(-m if i % 2 else m)
        ref = _device(vals, p, s, scales=scales, esize=esize)
        assert ref == [v * 10**(s - ds) for v, ds in zip(vals, scales)]

    def test_int32_output_at_column_scale(self):
        rng = np.random.default_rng(910)
        vals = [0, 1, -1, 10**9 - 1, -(10**9 - 1)]
        vals += [int(x) for x in rng.integers(-(10**9) + 1, 10**9, 700)]
        assert _device(vals, 9, 3, esize=4) == vals

    def test_scale_too_large_sets_the_error_bit(self):
        # an ordinary launch whose result is the plan's error bit: the call
        # returns -1 with the rescale message, the guard zones stay intact
        vals = list(range(-300, 300))
        scales = [2] * len(vals)
        scales[517] = 3
        with pytest.raises(D.DecimalRangeError):
            D.decode(D.encode(vals), len(vals), 18, 2, scales)
        with pytest.raises(RuntimeError,
                           match="ORC decimal rescale.*above the column "
                                 "scale"):
            debug_orc_decimal(D.encode(vals), len(vals), 18, 2,
                              ORC_DECIMAL_DEVICE, scales=scales)

    def test_precision_overflow_sets_the_error_bit(self):
        vals = [5] * 100 + [10**18]
        with pytest.raises(RuntimeError,
                           match="ORC decimal rescale.*precision"):
            debug_orc_decimal(D.encode(vals), len(vals), 18, 2,
                              ORC_DECIMAL_DEVICE)
