"""The partition's shared search core (paimon_amd/csrc/partition_core.h: the
lockstep multi-run search and the per-bound refine routine that
k_partition_refine runs) through the host mode of pmh_debug_partition,
against the numpy model of tests/partition_cases.py. Every case asserts the
whole cuts array. No GPU calls."""

import os
import subprocess

import numpy as np
import pytest

from paimon_amd import LIB_PATH
from paimon_amd.reader import PARTITION_HOST, debug_partition
from tests import partition_cases as pc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(LIB_PATH):
        subprocess.run(["make", "-C",
                        os.path.join(REPO, "paimon_amd", "csrc")],
                       check=True, capture_output=True)


def test_model_on_a_hand_case():
    # merged order (key, run): 1a 2a 2b 3b 5a 5b 5c 9c
    runs = [np.array([1, 2, 5], np.int64), np.array([2, 3, 5], np.int64),
            np.array([5, 9], np.int64)]
    want = [[0, 0, 0], [2, 1, 0], [3, 3, 0], [3, 3, 2]]
    assert pc.model_cuts(runs, 3).tolist() == want


def test_model_orders_negative_keys_first():
    runs = [np.array([-2**63, 0], np.int64), np.array([-1, 2**63 - 1],
                                                      np.int64)]
    assert pc.model_cuts(runs, 1).tolist() == [
        [0, 0], [1, 0], [1, 1], [2, 1], [2, 2]]


def test_case_list_covers_every_template_bound_and_width():
    ks = {(len(pc.case(n)[0]), pc.case(n)[0][0].dtype.itemsize)
          for n in pc.CASE_IDS if n.startswith("dense_")}
    assert ks == {(k, w) for k in pc.RUN_COUNTS for w in (4, 8)}


@pytest.mark.parametrize("name", pc.CASE_IDS)
def test_host_core_matches_model(name):
    runs, tile_rows, want = pc.case(name)
    got = debug_partition(runs, tile_rows, PARTITION_HOST)
    pc.check_cuts(got, runs, tile_rows, want)


def test_no_rows():
    runs = [np.empty(0, np.int64)] * 3
    got = debug_partition(runs, 64, PARTITION_HOST)
    assert got.tolist() == [[0, 0, 0]]


def test_too_many_runs_are_refused():
    with pytest.raises(RuntimeError, match="pmh_debug_partition"):
        debug_partition([np.arange(4, dtype=np.int64)] * 33, 64,
                        PARTITION_HOST)
