"""ORC integer decode on the host, stream by stream: the host RLEv2 decoder
that reads string LENGTH streams (host_rlev2_u) against the oracle at every
sub-encoding and bit width, and the prescan walk (prescan_rlev2 /
prescan_byterle) on whole and truncated streams. Streams come from the
spec-level builders in tests/orc_streams.py, so the test and not a file
writer picks the sub-encoding, the width and the counts. Each case first
proves the built stream against the oracle, then compares the product with
the oracle bit for bit (uint64 views). No GPU."""

import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import pytest

from oracle import orc_light as ol
from oracle.oracle import orc_rlev2_decode
from paimon_amd.reader import (ORC_INTS_BYTE, ORC_INTS_HOST,
                               ORC_INTS_PRESCAN, ORC_INTS_SIGNED,
                               ORC_INTS_UNSIGNED, debug_orc_ints, last_error)
from tests import orc_cases as C
from tests import orc_streams as S


def _host_matches_oracle(cases):
    stream, ref = C.check_oracle(cases, signed=False)
    got = debug_orc_ints(stream, len(ref), ORC_INTS_UNSIGNED, ORC_INTS_HOST)
    assert got.dtype == np.uint64 and len(got) == len(ref)
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, (bad[:5], got[bad[:5]], ref[bad[:5]])
    return stream, ref


class TestHostTwin:
    @pytest.mark.parametrize("width", S.WIDTHS)
    def test_direct(self, width):
        rng = np.random.default_rng(1000 + width)
        _host_matches_oracle(C.direct_cases(
            width, (1, 2, 63, 64, 65, 511, 512), False, rng))

    def test_short_repeat(self):
        _host_matches_oracle(C.short_repeat_cases(False))

    def test_delta_fixed(self):
        _host_matches_oracle(C.delta_fixed_cases(
            (1, 2, 3, 66, 67, 130, 512), False))

    @pytest.mark.parametrize("width", S.WIDTHS[1:])
    def test_delta_packed(self, width):
        rng = np.random.default_rng(2000 + width)
        _host_matches_oracle(C.delta_packed_cases(
            width, (1, 2, 3, 66, 67, 130, 512), False, rng))

    @pytest.mark.parametrize("width", C.PATCH_WIDTHS)
    def test_patched_base(self, width):
        # counts: 63 holds the 31-entry list; 300 has room for the (255, 0)
        # extension entry at pgw = 8
        rng = np.random.default_rng(3000 + width)
        _host_matches_oracle(C.patched_cases(width, (63, 300), rng))

    def test_until_exhausted(self):
        # n_values < 0: the DICTIONARY_V2 LENGTH call, where the entry
        # count comes from the stream itself. Every sub-encoding, PATCHED
        # with an extension entry last so a wrong entry width is seen.
        rng = np.random.default_rng(4000)
        cases = (C.short_repeat_cases(False, repeats=(5,)) +
                 C.direct_cases(13, (65,), False, rng) +
                 C.delta_packed_cases(9, (67,), False, rng) +
                 C.delta_fixed_cases((3,), False) +
                 [C.patched_run(3, 7, 5, 1, 1, 300, [0, 40, 299], rng),
                  C.patched_run(11, 8, 8, -77, 2, 300, [0, 257, 299], rng)])
        stream, ref = C.check_oracle(cases, signed=False)
        got = debug_orc_ints(stream, -1, ORC_INTS_UNSIGNED, ORC_INTS_HOST)
        assert len(got) == len(ref)
        assert (got == ref).all()

    @pytest.mark.parametrize("dict_threshold", [0.0, 1.0],
                             ids=["direct_v2", "dictionary_v2"])
    def test_writer_length_stream_with_patched_base(self, tmp_path,
                                                    dict_threshold):
        # a LENGTH stream as the ORC writer emits it for mostly tiny strings
        # with a few long ones: PATCHED_BASE runs (w=3, pw=7, pgw=5 and the
        # like). DICTIONARY_V2 decodes it until exhausted.
        rng = np.random.default_rng(4100)
        lens = rng.integers(1, 6, 5000)
        big = rng.random(5000) < 0.02
        lens[big] = rng.integers(200, 901, int(big.sum()))
        alpha = np.array(list("abcdefghijklmnopqrstuvwxyz"))
        words = ["".join(alpha[rng.integers(0, 26, int(n))]) for n in lens]
        if dict_threshold:
            words = [words[i] for i in rng.integers(0, 5000, 15000)]
        path = str(tmp_path / "s.orc")
        orc.write_table(pa.table({"s": pa.array(words)}), path,
                        compression="uncompressed",
                        dictionary_key_size_threshold=dict_threshold)
        fi = ol.parse_orc(path)
        with open(path, "rb") as f:
            raw = f.read()
        n_patched = 0
        for st in fi.stripes:
            assert st.encodings[1] == (ol.ENC_DICTIONARY_V2 if dict_threshold
                                       else ol.ENC_DIRECT_V2)
            ln = ol.find_stream(st, 1, ol.STREAM_LENGTH)
            stream = raw[ln.offset:ln.offset + ln.length]
            heads = S.run_headers(stream)
            n_patched += sum(e == S.PATCHED_BASE for e, _ in heads)
            n = sum(c for _, c in heads)
            ref = orc_rlev2_decode(stream, n, signed=False).view(np.uint64)
            if not dict_threshold:
                assert n == st.num_rows
                assert (ref == np.array([len(w) for w in words],
                                        np.uint64)).all()
            got = debug_orc_ints(stream, -1 if dict_threshold else n,
                                 ORC_INTS_UNSIGNED, ORC_INTS_HOST)
            assert len(got) == n and (got == ref).all()
        assert n_patched >= 1, "the writer emitted no PATCHED_BASE run"

    def test_rejects_other_kinds(self):
        for kind in (ORC_INTS_SIGNED, ORC_INTS_BYTE):
            with pytest.raises(RuntimeError):
                debug_orc_ints(S.short_repeat(1, 1, 3), 3, kind,
                               ORC_INTS_HOST)


def _rlev2_last_runs(rng):
    """(name, run bytes, value count): one run of each RLEv2 sub-encoding."""
    return [
        ("short_repeat", S.short_repeat(0xA55A01, 3, 4), 4),
        ("direct", C.direct_cases(13, (67,), True, rng)[0][0], 67),
        ("patched_base",
         C.patched_run(7, 8, 8, -300, 2, 300, [0, 257, 299], rng)[0], 300),
        ("delta_fixed", S.delta(1 << 40, -(1 << 20), [], 0, count=9), 9),
        ("delta_packed", C.delta_packed_cases(17, (67,), True, rng)[0][0],
         67),
    ]


class TestPrescan:
    def test_chunk_count_is_run_count(self):
        rng = np.random.default_rng(5000)
        for signed in (True, False):
            kind = ORC_INTS_SIGNED if signed else ORC_INTS_UNSIGNED
            cases = (C.short_repeat_cases(signed) +
                     C.direct_cases(30, (1, 64, 512), signed, rng) +
                     C.delta_fixed_cases((1, 2, 130), signed) +
                     C.delta_packed_cases(24, (1, 2, 3, 131), signed, rng) +
                     C.patched_cases(13, (63, 300), rng))
            stream, ref = C.check_oracle(cases, signed)
            for esize in (4, 8):
                assert debug_orc_ints(stream, len(ref), kind,
                                      ORC_INTS_PRESCAN,
                                      out_esize=esize) == len(cases)

    def test_chunk_count_byte_rle(self):
        runs = [S.byte_run(-3, 3), S.byte_literal([1, -2, 3]),
                S.byte_run(7, 130), S.byte_literal(list(range(-64, 64)))]
        n = 3 + 3 + 130 + 128
        assert debug_orc_ints(S.join(runs), n, ORC_INTS_BYTE,
                              ORC_INTS_PRESCAN) == 4
        # a final run longer than the values wanted is still one chunk
        assert debug_orc_ints(S.join(runs), n - 100, ORC_INTS_BYTE,
                              ORC_INTS_PRESCAN) == 4

    @pytest.mark.parametrize("name", ["short_repeat", "direct",
                                      "patched_base", "delta_fixed",
                                      "delta_packed"])
    def test_truncated_rlev2_is_rejected(self, name):
        rng = np.random.default_rng(6000)
        last, n_last = next((r, n) for nm, r, n in _rlev2_last_runs(rng)
                            if nm == name)
        lead = S.direct([5, 6, 7], 9)
        stream = lead + last
        n = 3 + n_last
        assert debug_orc_ints(stream, n, ORC_INTS_SIGNED,
                              ORC_INTS_PRESCAN) == 2
        # every cut inside the last run: its header, its base / literal
        # bytes, its packed payload, its patch list
        for cut in range(len(lead), len(stream)):
            with pytest.raises(RuntimeError):
                debug_orc_ints(stream[:cut], n, ORC_INTS_SIGNED,
                               ORC_INTS_PRESCAN)
            assert last_error(), cut

    @pytest.mark.parametrize("last,n_last", [
        (S.byte_run(-5, 130), 130),
        (S.byte_literal(list(range(-100, 28))), 128)],
        ids=["run", "literal"])
    def test_truncated_byte_rle_is_rejected(self, last, n_last):
        lead = S.byte_run(1, 3)
        stream = lead + last
        n = 3 + n_last
        assert debug_orc_ints(stream, n, ORC_INTS_BYTE,
                              ORC_INTS_PRESCAN) == 2
        for cut in range(len(lead), len(stream)):
            with pytest.raises(RuntimeError):
                debug_orc_ints(stream[:cut], n, ORC_INTS_BYTE,
                               ORC_INTS_PRESCAN)
            assert last_error(), cut
