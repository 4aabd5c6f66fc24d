"""Plain-Python model of ORC TIMESTAMP values (ORC v1 spec, "Timestamp
Columns") and stream builders for them, independent of the product's decoder.

DATA holds signed seconds relative to 2015-01-01T00:00:00 UTC, SECONDARY the
nanoseconds with trailing decimal zeros removed: stored v, z = v & 7,
r = v >> 3, nanos = r if z == 0 else r * 10**(z + 1). The reader's column is
milliseconds or microseconds since the Unix epoch, truncated; values before
1970 with a fraction, nanos of 10**9 or more and results outside int64 are
refused (python ints do not overflow, so the model checks the range itself).
"""

from tests import orc_streams as S

BASE = 1_420_070_400  # 2015-01-01T00:00:00Z in Unix seconds
MILLIS, MICROS = 0, 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

NEG_FRACTION = "before 1970 with a fractional second"
NANOS = "nanoseconds of 10^9 or more"
RANGE = "outside the int64 range"


class Refused(Exception):
    def __init__(self, text):
        super().__init__(text)
        self.text = text


def encode_nanos(nanos, zeros=None):
    """nanos -> the stored SECONDARY value. zeros = how many trailing decimal
    zeros to strip (2..8 -> code 1..7; None = as many as the writer would:
    all of them when there are at least two)."""
    if zeros is None:
        zeros = 0
        if nanos:
            while zeros < 8 and nanos % 10 ** (zeros + 1) == 0:
                zeros += 1
        if zeros < 2:
            zeros = 0
    if zeros == 0:
        return nanos << 3
    assert 2 <= zeros <= 8 and nanos % 10 ** zeros == 0
    return ((nanos // 10 ** zeros) << 3) | (zeros - 1)


def decode_nanos(v):
    z, r = v & 7, v >> 3
    return r if z == 0 else r * 10 ** (z + 1)


def value(secs, stored, unit):
    """One (DATA, SECONDARY) pair -> column value, or Refused."""
    nanos = decode_nanos(stored)
    if nanos >= 10 ** 9:
        raise Refused(NANOS)
    s = secs + BASE
    if not I64_MIN <= s <= I64_MAX:
        raise Refused(RANGE)
    if s < 0 and nanos:
        raise Refused(NEG_FRACTION)
    v = s * 10 ** 6 + nanos // 1000 if unit == MICROS \
        else s * 10 ** 3 + nanos // 10 ** 6
    if not I64_MIN <= v <= I64_MAX:
        raise Refused(RANGE)
    return v


def _runs(raws, width):
    return S.join([S.direct(raws[i:i + 512], width)
                   for i in range(0, len(raws), 512)])


def streams(pairs):
    """[(secs relative to 2015, stored nanos)] -> (DATA, SECONDARY) streams:
    DIRECT runs of 64-bit values (zigzag seconds / raw stored nanos), so any
    int64 second and any stored value, wrapped negatives included, fits."""
    data = _runs([S.zigzag(s) for s, _ in pairs], 64)
    sec = _runs([v & ((1 << 64) - 1) for _, v in pairs], 64)
    return data, sec


def unix(secs_since_epoch):
    """Unix seconds -> the DATA stream's 2015-relative seconds."""
    return secs_since_epoch - BASE


def unit_limits(unit):
    """(largest Unix second, largest fraction in nanos at that second,
    smallest Unix second) whose value still fits int64 in `unit`."""
    per = 10 ** 6 if unit == MICROS else 10 ** 3
    s_max = I64_MAX // per
    frac_nanos = (I64_MAX - s_max * per) * (10 ** 9 // per)
    s_min = -((1 << 63) // per)
    return s_max, frac_nanos, s_min


def positive_pairs(unit):
    """The value matrix both suites decode: every trailing-zero code, the
    nanos edges, digits below the unit, the epoch, whole seconds before it
    and both int64 limits of the unit."""
    now = 1_700_000_000
    pairs = []
    for zeros in (0, 2, 3, 4, 5, 6, 7, 8):  # stored code z = 0..7
        pairs.append((unix(now), encode_nanos(7 * 10 ** zeros, zeros)))
    pairs.append((unix(now), encode_nanos(123_400_000, 5)))
    for nanos in (0, 1000, 999_999_000, 999_999_999, 1, 999, 1_999_999,
                  500_000_000, 123_456_789):
        pairs.append((unix(now + 1), encode_nanos(nanos)))
    pairs.append((unix(0), encode_nanos(0)))            # S = 0
    pairs.append((unix(0), encode_nanos(999_999_999)))  # ... plus a fraction
    pairs.append((unix(-1), encode_nanos(0)))           # S = -1, whole
    pairs.append((unix(-2_208_988_800), encode_nanos(0)))  # 1900-01-01
    pairs.append((0, encode_nanos(0)))                  # 2015-01-01 itself
    s_max, frac, s_min = unit_limits(unit)
    pairs.append((unix(s_max), encode_nanos(frac)))
    pairs.append((unix(s_min), encode_nanos(0)))
    return pairs


def refusal_cases(unit):
    """[(name, (secs, stored), refusal text)]: one value each that the
    reader must refuse."""
    s_max, frac, _ = unit_limits(unit)
    step = 10 ** 3 if unit == MICROS else 10 ** 6  # nanos per unit
    return [
        ("negative_second_with_nanos",
         (unix(-1), encode_nanos(500_000_000)), NEG_FRACTION),
        ("nanos_1e9_plain", (unix(5), 10 ** 9 << 3), NANOS),
        ("nanos_1e9_scaled", (unix(5), (10 << 3) | 7), NANOS),
        # what a writer that keeps negative nanos leaves in the unsigned
        # stream: -500 000 000 ns as (-5 << 3 | 7), two's complement
        ("wrapped_negative_nanos",
         (unix(-2), ((-5 << 3) | 7) & ((1 << 64) - 1)), NANOS),
        ("overflow_multiply", (unix(s_max + 1), encode_nanos(0)), RANGE),
        ("overflow_fraction",
         (unix(s_max), encode_nanos(frac + step)), RANGE),
        ("overflow_base_add", (I64_MAX, encode_nanos(0)), RANGE),
    ]
