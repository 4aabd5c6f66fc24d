"""k_rlev2 + k_orc_timestamp through the device mode of
pmh_debug_orc_timestamp: the CPU suite's value matrix
(tests/orc_timestamp_model.py), repeated out to each count so values cross
the 512-value RLEv2 runs, the 256-thread steps and the 4096-value units of
the combine kernel, in both units, and each refusal."""

import re

import numpy as np
import pytest

from paimon_amd import debug_orc_timestamp
from paimon_amd.reader import ORC_TS_DEVICE, ORC_TS_MICROS, ORC_TS_MILLIS
from tests import orc_timestamp_model as T

pytestmark = pytest.mark.gpu

COUNTS = [1, 64, 65, 512, 513, 1025]
UNITS = [ORC_TS_MILLIS, ORC_TS_MICROS]


def _tiled(pairs, n):
    return [pairs[i % len(pairs)] for i in range(n)]


@pytest.mark.parametrize("unit", UNITS, ids=["millis", "micros"])
@pytest.mark.parametrize("n", COUNTS + [4097])
def test_value_matrix(n, unit):
    pairs = _tiled(T.positive_pairs(unit), n)
    exp = [T.value(s, v, unit) for s, v in pairs]
    data, sec = T.streams(pairs)
    got = debug_orc_timestamp(data, sec, n, unit, ORC_TS_DEVICE)
    assert got.dtype == np.int64 and got.tolist() == exp


@pytest.mark.parametrize("unit", UNITS, ids=["millis", "micros"])
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("case", range(7))
def test_refusals(case, n, unit):
    name, pair, text = T.refusal_cases(unit)[case]
    pairs = _tiled(T.positive_pairs(unit), n)
    pairs[n - 1] = pair  # the last value: the ragged end of the last step
    data, sec = T.streams(pairs)
    with pytest.raises(RuntimeError,
                       match="ORC timestamp refused: .*" + re.escape(text)):
        debug_orc_timestamp(data, sec, n, unit, ORC_TS_DEVICE)
