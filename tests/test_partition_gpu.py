"""k_partition_wave / k_partition_refine on their own, through the device
mode of pmh_debug_partition (pmh_launch_partition exactly as pmh_read_next
calls it, nothing downstream), against the numpy model of
tests/partition_cases.py — the CPU suite's case list. Every case asserts the
whole cuts array."""

import numpy as np
import pytest

from paimon_amd.reader import (PARTITION_DEVICE, PARTITION_HOST,
                               debug_partition)
from tests import partition_cases as pc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", pc.CASE_IDS)
def test_kernels_match_model(name):
    runs, tile_rows, want = pc.case(name)
    got = debug_partition(runs, tile_rows, PARTITION_DEVICE)
    pc.check_cuts(got, runs, tile_rows, want)


@pytest.mark.parametrize("name", ["tile3584_x9p1_k8_i64",
                                  "tile3584_x20p1_k8_i64",
                                  "tile3584_x9p1_k16_i64",
                                  "tile3584_x9_k16_i32"])
def test_production_path_equals_host_core(name):
    """k = 8 (two-level) and k = 16 (single-level) at the production tile:
    the kernels and the host walk of the same core agree bit for bit."""
    runs, tile_rows, _ = pc.case(name)
    assert tile_rows == pc.TILE and len(runs) in (8, 16)
    dev = debug_partition(runs, tile_rows, PARTITION_DEVICE)
    host = debug_partition(runs, tile_rows, PARTITION_HOST)
    assert dev.dtype == host.dtype == np.int32
    assert dev.tobytes() == host.tobytes()


def test_no_rows():
    runs = [np.empty(0, np.int64)] * 3
    got = debug_partition(runs, 64, PARTITION_DEVICE)
    assert got.tolist() == [[0, 0, 0]]
