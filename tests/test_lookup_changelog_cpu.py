"""CPU pins of the lookup changelog producer: the sequential model
(tests/lookup_model.py) against the literal vectors of the reference's
LookupChangelogMergeFunctionWrapperTest.testDeduplicate, and the host entry
of the lookup search core (pmh_debug_lookup_probe, the code k_lookup_probe
runs on the device) against numpy.searchsorted. No GPU calls."""

import os
import subprocess

import numpy as np
import pytest

from paimon_amd import LIB_PATH
from tests.lookup_model import lookup_changelog_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INSERT, UPDATE_BEFORE, UPDATE_AFTER, DELETE = 0, 1, 2, 3


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(LIB_PATH):
        subprocess.run(["make", "-C",
                        os.path.join(REPO, "paimon_amd", "csrc")],
                       check=True, capture_output=True)


def _rec(seq, kind, value):
    """One-record run with key 1 (the reference vectors all use row(1))."""
    return {"key": np.array([1], np.int64), "seq": np.array([seq], np.int64),
            "kind": np.array([kind], np.int8),
            "values": [np.array([value], np.int32)]}


# (name, members [(seq, kind, value, level)] in add() order,
#  lookup hit (seq, kind, value) or None,
#  expected changelog [(kind, value)] without the equaliser,
#  expected changelog with the equaliser, expected result (kind, value))
# — LookupChangelogMergeFunctionWrapperTest.java:65-212, in order.
REFERENCE_VECTORS = [
    ("without_level0",
     [(1, INSERT, 1, 2), (2, INSERT, 2, 1)], None,
     [], [], (INSERT, 2)),
    ("level0_with_level1",
     [(1, INSERT, 1, 1), (2, INSERT, 2, 0)], None,
     [(UPDATE_BEFORE, 1), (UPDATE_AFTER, 2)],
     [(UPDATE_BEFORE, 1), (UPDATE_AFTER, 2)], (INSERT, 2)),
    ("level0_lookup_miss",
     [(1, UPDATE_AFTER, 2, 0)], None,
     [(INSERT, 2)], [(INSERT, 2)], (UPDATE_AFTER, 2)),
    ("level0_lookup_hit_insert",
     [(2, INSERT, 2, 0)], (1, INSERT, 1),
     [(UPDATE_BEFORE, 1), (UPDATE_AFTER, 2)],
     [(UPDATE_BEFORE, 1), (UPDATE_AFTER, 2)], (INSERT, 2)),
    ("level0_lookup_hit_delete",
     [(2, INSERT, 2, 0)], (1, DELETE, 1),
     [(INSERT, 2)], [(INSERT, 2)], (INSERT, 2)),
    ("level0_retract_lookup_miss",
     [(1, UPDATE_BEFORE, 2, 0)], None,
     [], [], (UPDATE_BEFORE, 2)),
    ("level0_delete_lookup_hit_delete",
     [(2, DELETE, 2, 0)], (1, DELETE, 1),
     [], [], (DELETE, 2)),
    ("level0_and_level2_same_record",
     [(2, INSERT, 2, 0), (2, INSERT, 2, 2)], None,
     [(UPDATE_BEFORE, 2), (UPDATE_AFTER, 2)], [], (INSERT, 2)),
    ("level0_lookup_hit_same_record",
     [(2, INSERT, 2, 0)], (2, INSERT, 2),
     [(UPDATE_BEFORE, 2), (UPDATE_AFTER, 2)], [], (INSERT, 2)),
]


@pytest.mark.parametrize("row_dedup", [False, True])
@pytest.mark.parametrize("case", REFERENCE_VECTORS, ids=lambda c: c[0])
def test_model_matches_reference_vectors(case, row_dedup):
    _, members, hit, exp_plain, exp_dedup, exp_result = case
    runs = [_rec(s, k, v) for s, k, v, _ in members]
    levels = [lvl for _, _, _, lvl in members]
    lookup = [_rec(*hit)] if hit else []
    sources = runs + lookup
    # drop_delete off: the reference test reads the wrapper's raw result
    cl, res = lookup_changelog_model(runs, levels, lookup,
                                     row_dedup=row_dedup, drop_delete=False)
    got_cl = [(kind, int(sources[s]["values"][0][r])) for s, r, kind in cl]
    assert got_cl == (exp_dedup if row_dedup else exp_plain)
    assert len(res) == 1
    s, r = res[0]
    assert (int(sources[s]["kind"][r]),
            int(sources[s]["values"][0][r])) == exp_result


def test_model_changelog_rows_carry_source_sequence():
    # rule 5: a changelog row keeps the key/sequence/values of the record
    # it was built from — UPDATE_BEFORE comes from the lookup level
    runs = [_rec(7, INSERT, 70)]
    lookup = [_rec(3, INSERT, 30)]
    cl, res = lookup_changelog_model(runs, [0], lookup)
    assert cl == [(1, 0, UPDATE_BEFORE), (0, 0, UPDATE_AFTER)]
    assert res == [(0, 0)]


def test_model_lookup_result_when_sequence_not_below_members():
    # rule 4 consequence: a looked-up record with seq >= every member's is
    # the result (ties included); a smaller one is not
    runs = [_rec(5, INSERT, 50), _rec(4, INSERT, 40)]
    for lseq, exp_src in ((5, 2), (6, 2), (4, 0)):
        cl, res = lookup_changelog_model(runs, [0, 0],
                                         [_rec(lseq, INSERT, 99)])
        assert res == [(exp_src, 0)], lseq
        assert cl == [(2, 0, UPDATE_BEFORE), (exp_src, 0, UPDATE_AFTER)]


def test_model_drops_other_upper_members_and_first_level_wins():
    # members at levels 0, 1 and 2: the level-2 record is dropped even with
    # the highest sequence number; lookup levels are not consulted
    runs = [_rec(5, INSERT, 50), _rec(3, INSERT, 30), _rec(9, INSERT, 90)]
    cl, res = lookup_changelog_model(runs, [0, 1, 2], [_rec(1, INSERT, 10)])
    assert res == [(0, 0)]
    assert cl == [(1, 0, UPDATE_BEFORE), (0, 0, UPDATE_AFTER)]
    # lookup: the lowest level holding the key wins
    cl, res = lookup_changelog_model(
        [_rec(5, INSERT, 50)], [0],
        [_rec(1, DELETE, 10), _rec(2, INSERT, 20)])
    assert cl == [(0, 0, INSERT)]


def test_model_drop_delete_only_affects_result():
    runs = [_rec(5, DELETE, 50)]
    lookup = [_rec(1, INSERT, 10)]
    for dd in (True, False):
        cl, res = lookup_changelog_model(runs, [0], lookup, drop_delete=dd)
        assert cl == [(1, 0, DELETE)]
        assert res == ([] if dd else [(0, 0)])


# ------------------------------------------------------------ debug probe

def _expected_probe(levels, queries):
    exp_level = np.full(len(queries), -1, np.int32)
    exp_row = np.full(len(queries), -1, np.int64)
    for li in range(len(levels) - 1, -1, -1):  # lower level overwrites
        lv = levels[li]
        if len(lv) == 0:
            continue
        pos = np.searchsorted(lv, queries)
        ok = pos < len(lv)
        ok[ok] = lv[pos[ok]] == queries[ok]
        exp_level[ok] = li
        exp_row[ok] = pos[ok]
    return exp_level, exp_row


def _check_probe(levels, queries):
    from paimon_amd import debug_lookup_probe
    queries = np.asarray(queries, np.int64)
    got_level, got_row = debug_lookup_probe(levels, queries)
    exp_level, exp_row = _expected_probe(levels, queries)
    assert (got_level == exp_level).all(), \
        np.flatnonzero(got_level != exp_level)[:10]
    assert (got_row == exp_row).all(), np.flatnonzero(got_row != exp_row)[:10]
    return got_level


class TestDebugLookupProbe:
    I64 = np.iinfo(np.int64)

    @pytest.mark.parametrize("size", [0, 1, 63, 64, 65, 5000])
    def test_level_sizes(self, size):
        rng = np.random.default_rng(100 + size)
        lv = np.sort(rng.choice(20_000, size, replace=False)).astype(np.int64)
        # all keys of the level, their neighbours, and a random sweep that
        # is mostly absent; sorted (as the kernel's probes are) and shuffled
        q = np.concatenate([lv, lv - 1, lv + 1,
                            rng.integers(-100, 20_100, 3000)])
        if size:
            q = np.concatenate([q, [lv[0], lv[-1], lv[0] - 5, lv[-1] + 5]])
        _check_probe([lv], np.sort(q))
        _check_probe([lv], rng.permutation(q))

    def test_bounds_and_edges(self):
        lv = np.arange(10, 1010, 10, dtype=np.int64)
        got = _check_probe([lv], [9, 10, 1000, 1001, -5, 5000, 500, 505])
        assert got.tolist() == [-1, 0, 0, -1, -1, -1, 0, -1]

    def test_lower_level_wins(self):
        rng = np.random.default_rng(7)
        a = np.sort(rng.choice(10_000, 3000, replace=False)).astype(np.int64)
        b = np.sort(rng.choice(10_000, 4000, replace=False)).astype(np.int64)
        c = np.sort(rng.choice(10_000, 65, replace=False)).astype(np.int64)
        q = np.arange(-10, 10_010, dtype=np.int64)
        got = _check_probe([a, b, c], q)
        both = np.intersect1d(a, b)
        assert len(both) > 100
        assert (got[both + 10] == 0).all()
        only_b = np.setdiff1d(b, a)
        assert (got[only_b + 10] == 1).all()
        absent = np.setdiff1d(q, np.concatenate([a, b, c]))
        assert len(absent) > 100
        assert (got[absent + 10] == -1).all()

    def test_absent_everywhere_and_empty_levels(self):
        e = np.empty(0, np.int64)
        lv = np.arange(0, 2000, 2, dtype=np.int64)
        got = _check_probe([e, lv, e], np.arange(1, 2001, 2))
        assert (got == -1).all()
        got = _check_probe([e, lv, e], lv)
        assert (got == 1).all()
        got = _check_probe([], np.arange(50))
        assert (got == -1).all()
        _check_probe([lv], e)

    def test_int64_extremes(self):
        lo, hi = self.I64.min, self.I64.max
        lv = np.array([lo, lo + 1, -1, 0, 1, hi - 1, hi], np.int64)
        lv2 = np.array([lo, hi], np.int64)
        q = np.array([lo, lo + 1, lo + 2, -2, -1, 0, 1, 2, hi - 2, hi - 1,
                      hi], np.int64)
        _check_probe([lv], q)
        _check_probe([lv2, lv], q)
        _check_probe([np.array([5], np.int64)], q)

    def test_many_chunks(self):
        # more queries than one search chunk, windows far apart
        rng = np.random.default_rng(11)
        lv0 = np.sort(rng.choice(1 << 40, 5000, replace=False)
                      ).astype(np.int64)
        lv1 = np.sort(np.concatenate([lv0[::3], rng.choice(
            1 << 40, 3000, replace=False)]))
        lv1 = np.unique(lv1).astype(np.int64)
        q = np.sort(np.concatenate([lv0[::2], lv1[::2],
                                    rng.integers(0, 1 << 40, 4000)]))
        _check_probe([lv0, lv1], q)
