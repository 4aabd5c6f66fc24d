"""CPU pins of the full-compaction changelog for the folding engines
(partial-update / aggregation):
 - the decision table k_merge_tiles' folded walk runs (changelog_core.h,
   through the host entry pmh_debug_changelog_decide) over the nine INPUT_KVS
   groups of the reference's FullChangelogMergeFunctionWrapperTestBase;
 - the sequential wrapper port of tests/changelog_fold_model.py against
   oracle.full_changelog_model (itself pinned to the reference vectors in
   tests/test_changelog_cpu.py), with a deduplicate fold;
 - hand vectors for a partial-update and an aggregation fold.
No GPU calls."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import (aggregation_model, full_changelog_model,
                    partial_update_model)
from paimon_amd import LIB_PATH
from tests.changelog_fold_model import (dedup_fold, fold_changelog,
                                        rows_to_columns)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAX_LEVEL = 3
I, UB, UA, D = 0, 1, 2, 3


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(LIB_PATH):
        subprocess.run(["make", "-C",
                        os.path.join(REPO, "paimon_amd", "csrc")],
                       check=True, capture_output=True)


# FullChangelogMergeFunctionWrapperTestBase INPUT_KVS: per key group the
# records (seq, kind, value, level) in add() order
INPUT_KVS = [
    [(1, I, 1, 0)],
    [(2, D, 0, 0)],
    [(3, I, 3, MAX_LEVEL)],
    [(4, I, 3, 0), (5, I, -3, 0)],
    [(6, I, 3, 0), (7, D, 3, 0)],
    [(8, I, 3, MAX_LEVEL), (9, I, -3, 0)],
    [(10, I, 3, MAX_LEVEL), (11, D, 3, 0)],
    [(12, I, 3, MAX_LEVEL), (13, UB, 3, 0)],
    [(14, I, 3, MAX_LEVEL), (15, I, 3, 0)],
]
# changelog kinds per group (the deduplicate merge function of the reference
# test: merged = the last record); the row-deduplicate variant of the test
# base drops group 9's pair, whose values are equal
EXPECTED_KINDS = [[I], [], [], [I], [], [UB, UA], [D], [D], [UB, UA]]


def _decide(nlive, n_top, m_add, pending):
    lib = ctypes.CDLL(LIB_PATH)
    fn = lib.pmh_debug_changelog_decide
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 3 + \
        [ctypes.c_int] + [ctypes.c_void_p] * 4
    n = len(nlive)
    a = np.asarray(nlive, np.int32)
    b = np.asarray(n_top, np.int32)
    c = np.asarray(m_add, np.uint8)
    out_n = np.full(n, -7, np.int32)
    kinds = np.full(2 * n, -7, np.int8)
    after = np.full(n, 7, np.uint8)
    pend = np.full(n, 7, np.uint8)
    rc = fn(n, a.ctypes.data, b.ctypes.data, c.ctypes.data, int(pending),
            out_n.ctypes.data, kinds.ctypes.data, after.ctypes.data,
            pend.ctypes.data)
    assert rc == 0
    return out_n, kinds.reshape(n, 2), after, pend


class TestDecisionTable:
    def _inputs(self):
        nlive = [len(g) for g in INPUT_KVS]
        n_top = [sum(1 for m in g if m[3] == MAX_LEVEL) for g in INPUT_KVS]
        m_add = [g[-1][1] in (I, UA) for g in INPUT_KVS]
        return nlive, n_top, m_add

    @pytest.mark.parametrize("pending", [False, True])
    def test_reference_groups(self, pending):
        out_n, kinds, after, pend = _decide(*self._inputs(), pending)
        for g, exp in enumerate(EXPECTED_KINDS):
            assert out_n[g] == len(exp), g
            got = [int(k) for k in kinds[g][:len(exp)]]
            assert got == exp, g
            assert all(int(k) == -1 for k in kinds[g][len(exp):]), g
            # the last row carries the merged result unless it is DELETE(top)
            assert bool(after[g]) == (len(exp) > 0 and exp[-1] in (I, UA)), g
            # only an UPDATE_BEFORE / UPDATE_AFTER pair waits for the
            # row-deduplicate value comparison
            assert bool(pend[g]) == (pending and exp == [UB, UA]), g

    def test_exhaustive_small(self):
        # every (nlive, n_top, merged_is_add) up to four records against the
        # wrapper's getResult branches written out
        cases = [(n, t, a) for n in range(1, 5) for t in (0, 1)
                 for a in (False, True)]
        out_n, kinds, _, _ = _decide([c[0] for c in cases],
                                     [c[1] for c in cases],
                                     [c[2] for c in cases], False)
        for i, (n, t, a) in enumerate(cases):
            if n == 1:
                exp = [I] if (t == 0 and a) else []
            elif t == 0:
                exp = [I] if a else []
            else:
                exp = [UB, UA] if a else [D]
            assert [int(k) for k in kinds[i][:out_n[i]]] == exp, (n, t, a)

    def test_bad_arguments(self):
        lib = ctypes.CDLL(LIB_PATH)
        fn = lib.pmh_debug_changelog_decide
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 3 + \
            [ctypes.c_int] + [ctypes.c_void_p] * 4
        assert fn(1, None, None, None, 0, None, None, None, None) == -1
        a = np.array([0], np.int32)  # nlive 0 is not a group
        z = np.array([0], np.int32)
        m = np.array([1], np.uint8)
        o = np.zeros(1, np.int32)
        k = np.zeros(2, np.int8)
        assert fn(1, a.ctypes.data, z.ctypes.data, m.ctypes.data, 0,
                  o.ctypes.data, k.ctypes.data, None, None) == -1


def _flat(rows):
    return [(r[0], r[1], r[2]) + tuple(None if v is None else int(v)
                                       for v in r[3]) for r in rows]


class TestHelperVsPinnedModel:
    """The wrapper port with a deduplicate fold must reproduce
    full_changelog_model on test_changelog_cpu.py's random generator."""

    @pytest.mark.parametrize("row_dedup", [False, True])
    def test_random(self, row_dedup):
        rng = np.random.default_rng(97 + int(row_dedup))
        for trial in range(25):
            k = int(rng.integers(2, 6))
            levels = [0] * (k - 1) + [MAX_LEVEL]
            runs = []
            seqbase = 0
            for ri in range(k):
                nrows = int(rng.integers(1, 400))
                keys = np.sort(rng.choice(600, nrows, replace=False))
                kind = np.where(rng.random(nrows) < 0.25, D, I).astype(np.int8)
                if ri == k - 1:
                    kind[:] = I  # top level holds compaction results
                runs.append({
                    "key": keys.astype(np.int64),
                    "seq": np.arange(nrows, dtype=np.int64) + seqbase,
                    "kind": kind,
                    "values": [rng.integers(0, 3, nrows).astype(np.int32),
                               rng.integers(0, 3, nrows).astype(np.int32)],
                })
                seqbase += nrows
            (cr, cw, ck), (rr, rw) = full_changelog_model(
                runs, levels, MAX_LEVEL, row_dedup=row_dedup)
            exp_cl = [(int(runs[a]["key"][b]), int(runs[a]["seq"][b]),
                       int(kk), int(runs[a]["values"][0][b]),
                       int(runs[a]["values"][1][b]))
                      for a, b, kk in zip(cr, cw, ck)]
            exp_res = sorted((int(runs[a]["key"][b]), int(runs[a]["seq"][b]))
                             for a, b in zip(rr, rw))
            cl, res = fold_changelog(runs, levels, MAX_LEVEL, dedup_fold,
                                     row_dedup=row_dedup)
            assert _flat(cl) == exp_cl, trial
            assert sorted((r[0], r[1]) for r in res) == exp_res, trial

    def test_reference_vectors(self):
        # the nine groups through the port itself (deduplicate fold)
        runs, levels = [], []
        for key, g in enumerate(INPUT_KVS, start=1):
            for seq, kind, value, level in g:
                runs.append({"key": np.array([key], np.int64),
                             "seq": np.array([seq], np.int64),
                             "kind": np.array([kind], np.int8),
                             "values": [np.array([value], np.int32)]})
                levels.append(level)
        for row_dedup in (False, True):
            cl, _ = fold_changelog(runs, levels, MAX_LEVEL, dedup_fold,
                                   row_dedup=row_dedup)
            exp = [(k, kind) for k, kinds in enumerate(EXPECTED_KINDS, 1)
                   for kind in kinds if not (row_dedup and k == 9)]
            assert [(r[0], r[2]) for r in cl] == exp


def _one(key, seq, kind, values, valid):
    return {"key": np.array([key], np.int64),
            "seq": np.array([seq], np.int64),
            "kind": np.array([kind], np.int8),
            "values": [np.array([v], np.int32) for v in values],
            "valid": [np.array([ok], bool) for ok in valid]}


class TestHandVectors:
    def _pu(self, runs, levels, row_dedup):
        cl, res = fold_changelog(
            runs, levels, MAX_LEVEL,
            lambda r: partial_update_model(r, drop_delete=False),
            row_dedup=row_dedup)
        return _flat(cl), _flat(res)

    def test_partial_update_all_null_update(self):
        # top (k, seq 1, a=1, b=2); the update sets nothing: merged values
        # equal top's, only the sequence number moves
        runs = [_one(7, 1, I, [1, 2], [True, True]),
                _one(7, 2, I, [0, 0], [False, False])]
        levels = [MAX_LEVEL, 0]
        cl, res = self._pu(runs, levels, row_dedup=False)
        assert cl == [(7, 1, UB, 1, 2), (7, 2, UA, 1, 2)]
        assert res == [(7, 2, I, 1, 2)]
        cl, res = self._pu(runs, levels, row_dedup=True)
        assert cl == []
        assert res == [(7, 2, I, 1, 2)]  # the main row does not depend on it

    def test_partial_update_one_field(self):
        runs = [_one(7, 1, I, [1, 2], [True, True]),
                _one(7, 2, I, [0, 5], [False, True])]
        for row_dedup in (False, True):
            cl, res = self._pu(runs, [MAX_LEVEL, 0], row_dedup)
            assert cl == [(7, 1, UB, 1, 2), (7, 2, UA, 1, 5)]
            assert res == [(7, 2, I, 1, 5)]

    def test_partial_update_null_is_not_a_value(self):
        # top's b is null, merged's b is 0: validity differs, so the pair
        # stays under row-deduplicate although a null is stored as 0
        runs = [_one(7, 1, I, [1, 0], [True, False]),
                _one(7, 2, I, [0, 0], [False, True])]
        cl, _ = self._pu(runs, [MAX_LEVEL, 0], row_dedup=True)
        assert cl == [(7, 1, UB, 1, None), (7, 2, UA, 1, 0)]

    def _agg(self, runs, levels, row_dedup):
        cl, res = fold_changelog(
            runs, levels, MAX_LEVEL,
            lambda r: aggregation_model(r, ["sum"], drop_delete=False),
            row_dedup=row_dedup)
        return _flat(cl), _flat(res)

    def test_aggregation_sum(self):
        runs = [_one(3, 1, I, [10], [True]), _one(3, 2, I, [5], [True])]
        for row_dedup in (False, True):
            cl, res = self._agg(runs, [MAX_LEVEL, 0], row_dedup)
            assert cl == [(3, 1, UB, 10), (3, 2, UA, 15)]
            assert res == [(3, 2, I, 15)]

    def test_aggregation_sum_of_zero(self):
        runs = [_one(3, 1, I, [10], [True]), _one(3, 2, I, [0], [True])]
        cl, _ = self._agg(runs, [MAX_LEVEL, 0], row_dedup=False)
        assert cl == [(3, 1, UB, 10), (3, 2, UA, 10)]
        cl, res = self._agg(runs, [MAX_LEVEL, 0], row_dedup=True)
        assert cl == []
        assert res == [(3, 2, I, 10)]

    def test_no_top_inserts_the_fold(self):
        runs = [_one(3, 1, I, [10], [True]), _one(3, 2, I, [5], [True]),
                _one(4, 3, D, [1], [True])]
        cl, res = self._agg(runs, [0, 0, 0], row_dedup=False)
        assert cl == [(3, 2, I, 15)]
        assert res == [(3, 2, I, 15)]  # the lone DELETE of key 4 is no row

    def test_rows_to_columns_roundtrip(self):
        runs = [_one(7, 1, I, [1, 2], [True, True]),
                _one(7, 2, I, [0, 5], [False, True])]
        cl, _ = fold_changelog(
            runs, [MAX_LEVEL, 0], MAX_LEVEL,
            lambda r: partial_update_model(r, drop_delete=False))
        cols = rows_to_columns(cl, [np.dtype(np.int32)] * 2)
        assert cols["kind"].tolist() == [UB, UA]
        assert cols["values"][1].tolist() == [2, 5]
        assert cols["valid"][0].tolist() == [True, True]
