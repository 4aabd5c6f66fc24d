"""Key-domain edges, CPU side: the plan descriptor's JSON numbers over the
whole int64 range, the key-domain generators' own invariants, the C oracle
against an independent numpy model on every generator (so the oracle is
known to be right at INT64_MIN / INT64_MAX before the kernels are judged
against it), and the tile-algorithm simulation over full-span and clustered
keys. No GPU calls."""

import numpy as np
import pytest

from oracle import merge_dedup
from paimon_amd.reader import debug_json_i64
from tests import keydomain as kd
from tests.test_tile_algorithm import simulate_tiles

I64_MIN, I64_MAX = kd.I64_MIN, kd.I64_MAX


class TestPlanJsonNumbers:
    @pytest.mark.parametrize("v", [
        I64_MIN, I64_MAX, 2**53 + 1, -(2**53 + 1), 2**60 + 101,
        -(2**60 + 101), 0, -1, I64_MAX - 1, I64_MIN + 1, I64_MAX - 512])
    def test_integer_tokens_are_exact(self, v):
        assert debug_json_i64(str(v)) == v
        assert debug_json_i64(f"  {v} ") == v

    @pytest.mark.parametrize("text,exp", [
        ("2.5", 3), ("-2.5", -3), ("1.25", 1), ("1e3", 1000),
        ("12.0", 12), ("-0.4", 0), ("4.5E1", 45)])
    def test_fractional_tokens_round_as_before(self, text, exp):
        # llround of the double: half away from zero
        assert debug_json_i64(text) == exp

    @pytest.mark.parametrize("text", [
        str(I64_MAX + 1), str(I64_MIN - 1), "18446744073709551615",
        "1" + "0" * 30])
    def test_out_of_range_integer_rejected(self, text):
        with pytest.raises(RuntimeError, match="bad JSON number"):
            debug_json_i64(text)

    def test_not_a_number_rejected(self):
        for text in ('"12"', "[1]", "", "12 13", "--1"):
            with pytest.raises(RuntimeError):
                debug_json_i64(text)


# (name, builder) — small shapes: the properties are those of the GPU
# shapes, the row counts only need several groups per run
def _generators(seq_base):
    out = [
        ("neg_dense", lambda: kd.neg_dense(5, 700, 11, seq_base)),
        ("full_span", lambda: kd.full_span(5, 700, 12, seq_base)),
        ("full_span_k2", lambda: kd.full_span(2, 300, 13, seq_base)),
        ("clustered", lambda: kd.clustered(4, 1500, 14, seq_base)),
        ("identical", lambda: kd.identical(6, 400, 15, seq_base)),
        ("lopsided", lambda: kd.lopsided(3000, 16, seq_base)),
    ]
    for span in kd.THRESHOLD_SPANS:
        for bi in range(3):
            out.append((f"threshold_{span - 2**32}_{bi}",
                        lambda s=span, b=bi: kd.threshold(
                            s, kd.threshold_bases(s)[b], 17 + b, seq_base)))
        out.append((f"threshold_{span - 2**32}_pred",
                    lambda s=span: kd.threshold(s, I64_MAX - s, 20, seq_base,
                                                pred_tile=True)))
    return out


_CASES = [(name, sb, fn) for sb in kd.SEQ_BASES for name, fn in _generators(sb)]
_IDS = [f"{name}-seq{sb.bit_length() - 1 if sb else 0}" for name, sb, _ in _CASES]


@pytest.mark.parametrize("name,seq_base,build", _CASES, ids=_IDS)
def test_generator_invariants_and_oracle_pin(name, seq_base, build):
    runs = build()
    kd.check_invariants(runs)
    assert min(int(r["seq"].min()) for r in runs) >= seq_base
    assert max(int(r["seq"].max()) for r in runs) < seq_base + 2**20
    for r in runs:
        assert (r["values"][0] == r["key"]).all()
    for drop_delete, ignore_delete in ((True, False), (False, False),
                                       (True, True), (False, True)):
        er, ew = merge_dedup(runs, ignore_delete=ignore_delete,
                             drop_delete=drop_delete)
        mr, mw = kd.dedup_model(runs, drop_delete, ignore_delete)
        assert len(er) == len(mr), (drop_delete, ignore_delete)
        assert (er == mr).all() and (ew == mw).all(), \
            (drop_delete, ignore_delete)


def test_model_rules_on_literal_groups():
    # the model itself, on groups small enough to check by eye: keys at both
    # ends of the domain; (key, seq, kind)
    def run(*recs):
        return {"key": np.array([r[0] for r in recs], np.int64),
                "seq": np.array([r[1] for r in recs], np.int64),
                "kind": np.array([r[2] for r in recs], np.int8)}
    runs = [run((I64_MIN, 5, 3), (-1, 1, 3), (7, 2, 0), (I64_MAX, 9, 0)),
            run((I64_MIN, 4, 0), (0, 3, 3), (7, 8, 3), (I64_MAX, 6, 3))]

    def keys(**kw):
        r, w = kd.dedup_model(runs, **kw)
        return [int(runs[a]["key"][b]) for a, b in zip(r, w)]
    # last record per key; retract winners (MIN, -1, 0, 7) dropped
    assert keys(drop_delete=True) == [I64_MAX]
    assert keys(drop_delete=False) == [I64_MIN, -1, 0, 7, I64_MAX]
    # ignore-delete: MIN and 7 fall back to their add record; the lone
    # retracts -1 and 0 bypass the merge function and then drop / stay
    assert keys(drop_delete=True, ignore_delete=True) == [I64_MIN, 7, I64_MAX]
    assert keys(drop_delete=False, ignore_delete=True) == \
        [I64_MIN, -1, 0, 7, I64_MAX]


class TestGeneratorProperties:
    def test_neg_dense_crosses_zero(self):
        runs = kd.neg_dense(4, 16_000, 21)
        for r in runs:
            assert r["key"][0] < -32_000 and r["key"][-1] > 16_000
            assert r["key"][0] >= -64_000 and r["key"][-1] < 32_000

    @pytest.mark.parametrize("k,rows", [(2, 3000), (4, 16_000), (40, 1000)])
    def test_full_span_extremes(self, k, rows):
        runs = kd.full_span(k, rows, 22)
        assert all(len(r["key"]) == rows for r in runs)
        lo = [(i, r) for i, r in enumerate(runs) if r["key"][0] == I64_MIN]
        hi = [(i, r) for i, r in enumerate(runs) if r["key"][-1] == I64_MAX]
        assert len(lo) >= 2 and len(hi) >= 2
        # the DELETE at INT64_MIN wins its group, the one at INT64_MAX loses
        top = max(lo, key=lambda t: t[1]["seq"][0])[1]
        assert top["kind"][0] == 3
        assert sum(r["kind"][-1] == 3 for _, r in hi) == 1
        assert max(hi, key=lambda t: t[1]["seq"][-1])[1]["kind"][-1] == 0
        # every tile spans far more than 2^32: none takes the repack
        assert not any(narrow for narrow, _ in kd.tile_stats(runs))
        # runs collide: well under T distinct keys
        allk = np.concatenate([r["key"] for r in runs])
        assert len(np.unique(allk)) < 0.8 * len(allk)

    @pytest.mark.parametrize("k,rows", [(4, 16_000), (12, 6000)])
    def test_clustered_tiles_alternate(self, k, rows):
        runs = kd.clustered(k, rows, 23)
        st = kd.tile_stats(runs)
        assert all(len(r["key"]) == rows for r in runs)
        narrow = [n for n, _ in st]
        assert sum(narrow) >= 8 and sum(not n for n in narrow) >= 6
        # narrow and wide tiles alternate over the small clusters
        assert sum(a != b for a, b in zip(narrow, narrow[1:])) >= 5
        # predecessor key more than 2^32 below the tile minimum, on tiles
        # of both kinds
        assert sum(n and f for n, f in st) >= 3
        assert sum(f and not n for n, f in st) >= 2
        gaps = np.diff(np.unique(np.concatenate([r["key"] for r in runs])))
        assert (gaps >= 2**40).sum() >= 8
        dense = np.concatenate([r["key"] for r in runs])
        dense = dense[dense < -2**62 + k * rows // 2]
        assert abs(len(dense) - k * rows // 2) < kd.TILE_ROWS

    @pytest.mark.parametrize("span", kd.THRESHOLD_SPANS)
    def test_threshold_is_one_tile_of_exact_span(self, span):
        for base in kd.threshold_bases(span):
            runs = kd.threshold(span, base, 24)
            assert len(runs) == 2
            assert sum(len(r["key"]) for r in runs) <= 3000
            for r in runs:
                assert int(r["key"][0]) == base
                assert int(r["key"][-1]) == base + span
            (narrow, far), = kd.tile_stats(runs)
            assert narrow == (span < kd.REPACK_LIMIT) and not far
        assert kd.threshold_bases(span)[2] + span == I64_MAX

    @pytest.mark.parametrize("span", kd.THRESHOLD_SPANS)
    def test_threshold_behind_a_far_predecessor(self, span):
        for base in (0, I64_MAX - span):
            runs = kd.threshold(span, base, 24, pred_tile=True)
            kd.check_invariants(runs)
            first, second = kd.tile_stats(runs)
            assert second == (span < kd.REPACK_LIMIT, True)
            assert int(runs[0]["key"][kd.TILE_ROWS // 2]) == base
            assert int(runs[1]["key"][-1]) == base + span

    def test_identical_groups(self):
        runs = kd.identical(12, 6000, 25)
        for r in runs[1:]:
            assert (r["key"] == runs[0]["key"]).all()
        assert runs[0]["key"][0] == I64_MIN and runs[0]["key"][-1] == I64_MAX
        assert kd.TILE_ROWS % 12 != 0  # cuts land inside groups

    def test_lopsided_one_section(self):
        runs = kd.lopsided(64_000, 26)
        assert [len(r["key"]) for r in runs] == [64_000, 1, 2, 64]
        first, last = runs[0]["key"][0], runs[0]["key"][-1]
        assert first < 0 < last
        for r in runs[1:]:
            assert r["key"][0] in (first, last) and r["key"][-1] == last
        assert runs[2]["key"][0] == first and runs[3]["key"][0] == first


# the tile simulation takes arbitrary int64 keys (Python ints throughout)
@pytest.mark.parametrize("tile_rows", [16, 64, 256])
@pytest.mark.parametrize("gen", ["full_span", "clustered", "identical"])
def test_tile_sim_over_key_domain(gen, tile_rows):
    if gen == "full_span":
        runs = kd.full_span(5, 500, 31, delete_p=0.25)
    elif gen == "clustered":
        # clusters laid out against the simulated tile, as the GPU shapes
        # are against the 3584-row tile
        runs = kd.clustered(4, 1200, 32, delete_p=0.25, tile_rows=tile_rows)
        st = kd.tile_stats(runs, tile_rows)
        assert sum(f for _, f in st) >= 2
    else:
        runs = kd.identical(5, 300, 33, delete_p=0.25)
    for dd in (True, False):
        for ig in (True, False):
            got = simulate_tiles(runs, tile_rows, dd, ig)
            er, ew = merge_dedup(runs, ignore_delete=ig, drop_delete=dd)
            assert got == list(zip(er.tolist(), ew.tolist())), (dd, ig)
