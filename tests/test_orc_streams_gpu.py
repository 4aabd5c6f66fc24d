"""k_rlev2 on the device, stream by stream: every RLEv2 sub-encoding and bit
width, byte-RLE, the 64-lane scan carry of DELTA, PATCHED_BASE patch lists
and every byte alignment the aligned-window bit reader distinguishes,
against the oracle, bit for bit. Streams come from the spec-level builders
in tests/orc_streams.py; each is first proved against the oracle (the
encoder's own check). Unsigned streams must also agree with the host LENGTH
decoder. Many runs are joined into one stream per call, so a call decodes
thousands of values over hundreds of chunks.

Every device call runs between two guard zones: a store outside the output
fails the call (AssertionError from debug_orc_ints) instead of faulting, and
an element the kernel never wrote reads back as 0xA5A5..., which no expected
value here equals."""

import numpy as np
import pytest

from paimon_amd.reader import (ORC_INTS_BYTE, ORC_INTS_DEVICE, ORC_INTS_HOST,
                               ORC_INTS_SIGNED, ORC_INTS_UNSIGNED,
                               debug_orc_ints)
from tests import orc_cases as C
from tests import orc_streams as S

pytestmark = pytest.mark.gpu

DIRECT_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 511, 512)
DELTA_COUNTS = (1, 2, 3, 65, 66, 67, 129, 130, 131, 512)
STRADDLE_WIDTHS = (3, 7, 13, 24, 30, 40, 56, 64)


def _device_matches_oracle(cases, signed, esize=8, src_shift=0):
    stream, ref = C.check_oracle(cases, signed)
    kind = ORC_INTS_SIGNED if signed else ORC_INTS_UNSIGNED
    got = debug_orc_ints(stream, len(ref), kind, ORC_INTS_DEVICE,
                         out_esize=esize, src_shift=src_shift)
    if esize == 4:
        ref64 = ref.view(np.int64)
        assert (ref64 == ref64.astype(np.int32)).all(), "case leaves int32"
        assert got.dtype == np.int32
        bad = np.flatnonzero(got != ref64.astype(np.int32))
    else:
        bad = np.flatnonzero(got.view(np.uint64) != ref)
    assert bad.size == 0, (bad[:5], got[bad[:5]], ref[bad[:5]])
    if not signed:
        host = debug_orc_ints(stream, len(ref), kind, ORC_INTS_HOST)
        assert (host == ref).all()
    return stream


class TestDirect:
    @pytest.mark.parametrize("signed", [True, False],
                             ids=["signed", "unsigned"])
    @pytest.mark.parametrize("esize", [8, 4])
    def test_every_width(self, signed, esize):
        rng = np.random.default_rng(100 + esize + signed)
        cases = []
        for w in S.WIDTHS:
            if esize == 4 and w > 32:
                continue
            cases += C.direct_cases(w, DIRECT_COUNTS, signed, rng,
                                    int32_only=esize == 4)
        # literals of 1..8 bytes; int32 output holds 4 zigzag / 3 plain bytes
        n_lit = 8 if esize == 8 else (4 if signed else 3)
        cases += C.short_repeat_cases(signed)[:2 * n_lit]
        _device_matches_oracle(cases, signed, esize)


def _alignment_cases(signed, rng):
    """DIRECT runs whose values straddle the reader's two 8-byte loads,
    then PATCHED_BASE runs whose patch lists start wherever the packed
    values before them end."""
    cases = []
    for w in STRADDLE_WIDTHS:
        cases += C.direct_cases(w, (65, 129), signed, rng)
    for w in STRADDLE_WIDTHS[:-1]:
        cases.append(C.patched_run(w, 8, 8, -77, 1, 63, [0, 31, 62], rng))
        cases.append(C.patched_run(w, 8, 5, 77, 2, 300, [0, 33, 299], rng))
    return cases


def _starts(lead_len, cases):
    """Stream offsets of every packed payload and every patch list."""
    payload, patch, off = [], [], lead_len
    for run, _ in cases:
        enc, count = run[0] >> 6, (((run[0] & 1) << 8) | run[1]) + 1
        width = S.WIDTHS[(run[0] >> 1) & 31]
        if enc == 1:
            payload.append(off + 2)
        else:
            assert enc == 2
            bb = (run[2] >> 5) + 1
            payload.append(off + 4 + bb)
            patch.append(off + 4 + bb + (count * width + 7) // 8)
        off += len(run)
    return payload, patch


class TestAlignment:
    @pytest.mark.parametrize("signed", [True, False],
                             ids=["signed", "unsigned"])
    def test_every_residue(self, signed):
        rng = np.random.default_rng(200 + signed)
        body = _alignment_cases(signed, rng)
        seen_payload, seen_patch = set(), set()
        for shift in range(8):
            _device_matches_oracle(body, signed, src_shift=shift)
            pay, pat = _starts(shift, body)
            seen_payload |= {p % 8 for p in pay}
            seen_patch |= {p % 8 for p in pat}
        first_payload, first_patch = set(), set()
        for wb in range(1, 9):
            lead = C.short_repeat_cases(signed, repeats=(3,))[wb - 1]
            assert len(lead[0]) == 1 + wb
            _device_matches_oracle([lead] + body, signed)
            pay, pat = _starts(1 + wb, body)
            first_payload.add(pay[0] % 8)
            first_patch.add(pat[0] % 8)
        # the shifts alone and the leading literals alone each put a payload
        # start and a patch-list start on every residue mod 8
        assert seen_payload == seen_patch == set(range(8))
        assert first_payload == first_patch == set(range(8))


class TestDelta:
    @pytest.mark.parametrize("signed", [True, False],
                             ids=["signed", "unsigned"])
    def test_fixed_and_every_packed_width(self, signed):
        rng = np.random.default_rng(300 + signed)
        cases = C.delta_fixed_cases(DELTA_COUNTS, signed)
        for w in S.WIDTHS[1:]:
            cases += C.delta_packed_cases(w, DELTA_COUNTS, signed, rng)
        _device_matches_oracle(cases, signed)

    def test_int32_output(self):
        rng = np.random.default_rng(310)
        cases = []
        for n in DELTA_COUNTS:
            m = max(n - 2, 0)
            for sign in (1, -1):
                mags = [int(x) for x in rng.integers(0, 1 << 16, m)]
                base = -sign * (1 << 30)
                vals = np.cumsum([base, sign * 3] + [sign * g for g in mags])
                cases.append((S.delta(base, sign * 3, mags, 16, count=n),
                              C._u64(vals[:n])))
        _device_matches_oracle(cases, True, esize=4)


class TestPatchedBase:
    # the CPU matrix (pw x pgw x base sign x base_bytes x patch list: one
    # entry, 31 entries from position 0, a gap-extension entry ending on
    # the last element) at a count below 64 and at 512; width + pw = 64 is
    # the width-56, pw-8 corner
    @pytest.mark.parametrize("widths", [C.PATCH_WIDTHS[i::4]
                                        for i in range(4)],
                             ids=lambda ws: "w" + "_".join(map(str, ws)))
    def test_matrix(self, widths):
        rng = np.random.default_rng(400 + widths[0])
        cases = []
        for w in widths:
            cases += C.patched_cases(w, (63, 512), rng)
        _device_matches_oracle(cases, False)

    def test_signed_stream_and_int32_output(self):
        rng = np.random.default_rng(450)
        cases = []
        for w in (1, 5, 12, 23):
            for pgw in (1, 5, 8):
                for count in (63, 512):
                    for pos in C.patch_lists(pgw, count):
                        cases.append(C.patched_run(w, 8, pgw, -77, 1, count,
                                                   pos, rng))
        _device_matches_oracle(cases, True, esize=4)
        _device_matches_oracle(cases, True, esize=8)


class TestByteRle:
    @pytest.mark.parametrize("esize", [4, 8])
    def test_runs_literals_and_final_clamp(self, esize):
        lit128 = [((i * 37) % 256) - 128 for i in range(128)]
        runs = [S.byte_run(-128, 3), S.byte_literal([-1]),
                S.byte_run(127, 130), S.byte_literal(lit128),
                S.byte_literal([5]), S.byte_run(-7, 130)]
        total = 3 + 1 + 130 + 128 + 1 + 130
        # whole stream; final run cut short; final literal cut short
        for stream, n in ((S.join(runs), total),
                          (S.join(runs), total - 129),
                          (S.join(runs[:4]), 3 + 1 + 130 + 1),
                          (S.join(runs[:4]), 3 + 1 + 130 + 127)):
            ref = C.byte_rle_decode(stream, n)
            got = debug_orc_ints(stream, n, ORC_INTS_BYTE, ORC_INTS_DEVICE,
                                 out_esize=esize)
            assert got.dtype == (np.int32 if esize == 4 else np.int64)
            assert (got == ref).all()
        # the reference decoder restates the builders' inputs
        exp = ([-128] * 3 + [-1] + [127] * 130 + lit128 + [5] + [-7] * 130)
        assert C.byte_rle_decode(S.join(runs), total).tolist() == exp
