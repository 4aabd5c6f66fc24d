"""k_bits_expand through the device mode of pmh_debug_bits: BOOLEAN value
streams of both framings (raw Parquet PLAIN bits, ORC boolean byte-RLE) and
both bit orders, bit for bit against the plain-Python model
(tests/bits_model.py). The entry puts the output between two guard zones and
pre-fills it with 0xA5, so a store outside the output raises AssertionError
and an element the kernel never wrote shows as 0xA5 (the values are 0/1)."""

import numpy as np
import pytest

from paimon_amd import debug_bits
from paimon_amd.reader import (BITS_BYTE_RLE, BITS_DEVICE, BITS_LSB, BITS_MSB,
                               BITS_RAW)
from tests import bits_model as B

pytestmark = pytest.mark.gpu

ORDERS = [BITS_LSB, BITS_MSB]
FORMATS = [BITS_RAW, BITS_BYTE_RLE]


def _stream(n, order, fmt, seed, **kw):
    rng = np.random.default_rng(seed)
    if fmt == BITS_RAW:
        vals = [int(x) for x in rng.integers(0, 2, n)]
        return B.pack(vals, order), vals
    stream, data, _ = B.random_byte_rle(rng, n, **kw)
    return stream, B.expand_raw(data, n, order)


def _device(stream, n, order, fmt, **kw):
    got = debug_bits(stream, n, order, fmt, BITS_DEVICE, **kw)
    assert len(got) == n
    return got.tolist()


@pytest.mark.parametrize("fmt", FORMATS, ids=["raw", "byte_rle"])
@pytest.mark.parametrize("order", ORDERS, ids=["lsb", "msb"])
@pytest.mark.parametrize("n", B.COUNTS)
def test_counts(n, order, fmt):
    stream, exp = _stream(n, order, fmt, 3000 + n)
    for esize in (1, 4):
        assert _device(stream, n, order, fmt, out_esize=esize) == exp, esize


@pytest.mark.parametrize("fmt", FORMATS, ids=["raw", "byte_rle"])
@pytest.mark.parametrize("order", ORDERS, ids=["lsb", "msb"])
@pytest.mark.parametrize("n", [65, 513])
def test_every_source_and_output_alignment(n, order, fmt):
    # short runs and literal groups: many units, their edges on every residue
    stream, exp = _stream(n, order, fmt, 3100 + n,
                          **({"run_lens": (3, 6), "lit_lens": (1, 4)}
                             if fmt == BITS_BYTE_RLE else {}))
    for src_shift in range(8):
        for out_shift in range(8):
            for esize in (1, 4):
                got = _device(stream, n, order, fmt, out_esize=esize,
                              src_shift=src_shift, out_shift=out_shift)
                assert got == exp, (src_shift, out_shift, esize)


@pytest.mark.parametrize("order", ORDERS, ids=["lsb", "msb"])
@pytest.mark.parametrize("plan", [[("run", 3)], [("run", 130)],
                                  [("lit", 1)], [("lit", 128)]],
                         ids=["run3", "run130", "lit1", "lit128"])
def test_extreme_units(plan, order):
    rng = np.random.default_rng(9)
    kind, k = plan[0]
    data = bytes([0xB1]) * k if kind == "run" else \
        bytes(int(x) for x in rng.integers(0, 256, k))
    stream = B.byte_rle_segments(data, plan)
    for n in (k * 8, k * 8 - 5):
        exp = B.expand_raw(data, n, order)
        for out_shift in (0, 3):
            assert _device(stream, n, order, BITS_BYTE_RLE,
                           out_shift=out_shift) == exp


def test_hundred_maximal_runs():
    # 100 runs of 130 bytes = 1040 values each: unit output indices step by
    # 1040 = 0 mod 8, so out_shift walks the residues
    data = b"".join(bytes([0x5A if i % 2 else 0xC3]) * 130
                    for i in range(100))
    stream = B.byte_rle_segments(data, [("run", 130)] * 100)
    n = 100 * 1040 - 3
    exp = B.expand_raw(data, n, BITS_MSB)
    for out_shift in (0, 5):
        for esize in (1, 4):
            assert _device(stream, n, BITS_MSB, BITS_BYTE_RLE,
                           out_esize=esize, out_shift=out_shift) == exp


def test_alternating_literals_and_runs_take_every_residue():
    # 1-byte literals (8 values) and 3-byte runs (24 values) alternate; with
    # the value count cutting the stream the unit starts stay multiples of
    # 8, so the residues come from out_shift: all eight, both widths
    rng = np.random.default_rng(11)
    plan, data = [], bytearray()
    for i in range(200):
        if i % 2 == 0:
            plan.append(("lit", 1))
            data += bytes([int(rng.integers(0, 256))])
        else:
            plan.append(("run", 3))
            data += bytes([int(rng.integers(0, 256))]) * 3
    stream = B.byte_rle_segments(bytes(data), plan)
    n = len(data) * 8 - 1
    exp = B.expand_raw(bytes(data), n, BITS_MSB)
    for out_shift in range(8):
        for esize in (1, 4):
            assert _device(stream, n, BITS_MSB, BITS_BYTE_RLE,
                           out_esize=esize, out_shift=out_shift) == exp


def test_truncated_stream_is_refused_before_any_launch():
    with pytest.raises(RuntimeError, match="literal truncated"):
        debug_bits(bytes([0xFE, 0x01]), 16, BITS_MSB, BITS_BYTE_RLE,
                   BITS_DEVICE)
