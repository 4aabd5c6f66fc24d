"""Spec-level ORC integer stream builders for tests: RLEv2 (all four
sub-encodings) and byte-RLE, written from the ORC v1 specification ("Run
Length Encoding version 2", "Byte Run Length Encoding"). Unlike a file
writer, the caller picks the sub-encoding, the bit width and the counts.

Every builder returns the bytes of ONE run; join() concatenates runs into a
stream. Values are passed RAW: the builders neither zigzag nor subtract a
base (zigzag() below does the former for signed DIRECT/SHORT_REPEAT data).
"""

import numpy as np

# 5-bit width code -> bit width ("fixed bit sizes" table of the spec)
WIDTHS = list(range(1, 25)) + [26, 28, 30, 32, 40, 48, 56, 64]
_CODE = {w: c for c, w in enumerate(WIDTHS)}


def closest_fixed_bits(n):
    return next(w for w in WIDTHS if w >= n)


def zigzag(v):
    """Signed -> unsigned zigzag of one Python int (64-bit range)."""
    return ((v << 1) ^ (v >> 63)) & ((1 << 64) - 1)


def _uvarint(v):
    out = bytearray()
    while True:
        if v < 0x80:
            out.append(v)
            return bytes(out)
        out.append((v & 0x7F) | 0x80)
        v >>= 7


def _svarint(v):
    return _uvarint(zigzag(v))


def _pack(values, width):
    """Big-endian, MSB-first bit packing, zero-padded to a whole byte."""
    v = np.asarray(values, dtype=np.uint64)
    if width < 64 and len(v):
        assert int(v.max()) < (1 << width), (int(v.max()), width)
    bits = np.unpackbits(v.astype(">u8").view(np.uint8).reshape(-1, 8),
                         axis=1)[:, 64 - width:]
    return np.packbits(bits.reshape(-1)).tobytes()


def _head(enc, width_code, count):
    assert 1 <= count <= 512
    n = count - 1
    return bytes([(enc << 6) | (width_code << 1) | (n >> 8), n & 0xFF])


def short_repeat(raw, width_bytes, repeat):
    assert 1 <= width_bytes <= 8 and 3 <= repeat <= 10
    assert 0 <= raw < (1 << (8 * width_bytes))
    return bytes([((width_bytes - 1) << 3) | (repeat - 3)]) + \
        raw.to_bytes(width_bytes, "big")


def direct(raws, width):
    return _head(1, _CODE[width], len(raws)) + _pack(raws, width)


def delta(base, delta0, magnitudes, width, signed=True, count=None):
    """base, base+delta0, then +-magnitudes (direction = sign of delta0).
    width 0 = fixed delta: no packed payload, every step is delta0, and
    `count` gives the run length. Otherwise width is the bit width of the
    packed magnitudes (2 at the least: width code 1 means 2 bits in a DELTA
    header) and the run holds 2 + len(magnitudes) values; count=1 or 2 with
    no magnitudes writes the shorter runs a header can still express."""
    if count is None:
        count = 2 + len(magnitudes)
    if width == 0:
        assert not magnitudes
        code, payload = 0, b""
    else:
        assert width >= 2 and len(magnitudes) == max(count - 2, 0)
        code, payload = _CODE[width], _pack(magnitudes, width)
    return (_head(3, code, count) +
            (_svarint(base) if signed else _uvarint(base)) +
            _svarint(delta0) + payload)


def patched_base(base, base_bytes, reduced, width, patches, pw, pgw):
    """reduced: the low `width` bits of (value - base) per element;
    patches: [(gap, patch)] packed at closest_fixed_bits(pw + pgw) bits
    each, gap in the high bits; base is sign-magnitude in base_bytes."""
    assert 1 <= base_bytes <= 8 and 1 <= pgw <= 8 and len(patches) <= 31
    mag = abs(base)
    assert mag < (1 << (8 * base_bytes - 1))
    braw = mag | ((1 << (8 * base_bytes - 1)) if base < 0 else 0)
    for g, p in patches:
        assert 0 <= g < (1 << pgw) and 0 <= p < (1 << pw)
    cfb = closest_fixed_bits(pw + pgw)
    return (_head(2, _CODE[width], len(reduced)) +
            bytes([((base_bytes - 1) << 5) | _CODE[pw],
                   ((pgw - 1) << 5) | len(patches)]) +
            braw.to_bytes(base_bytes, "big") +
            _pack(reduced, width) +
            _pack([(g << pw) | p for g, p in patches], cfb))


def byte_run(value, count):
    assert 3 <= count <= 130 and -128 <= value <= 127
    return bytes([count - 3, value & 0xFF])


def byte_literal(values):
    assert 1 <= len(values) <= 128
    return bytes([256 - len(values)]) + bytes(v & 0xFF for v in values)


def join(runs):
    return b"".join(runs)


SHORT_REPEAT, DIRECT, PATCHED_BASE, DELTA = range(4)


def run_headers(stream):
    """Walk a whole RLEv2 stream (a writer's, say) and return one
    (sub-encoding, count) per run, to assert what a file really holds."""
    out, p = [], 0
    while p < len(stream):
        h = stream[p]
        enc = h >> 6
        if enc == SHORT_REPEAT:
            out.append((enc, (h & 7) + 3))
            p += 2 + ((h >> 3) & 7)
            continue
        count = (((h & 1) << 8) | stream[p + 1]) + 1
        width = WIDTHS[(h >> 1) & 31]
        out.append((enc, count))
        if enc == DIRECT:
            p += 2 + (count * width + 7) // 8
        elif enc == PATCHED_BASE:
            bb = (stream[p + 2] >> 5) + 1
            pw = WIDTHS[stream[p + 2] & 31]
            pgw = (stream[p + 3] >> 5) + 1
            pl = stream[p + 3] & 31
            p += (4 + bb + (count * width + 7) // 8 +
                  (pl * closest_fixed_bits(pw + pgw) + 7) // 8)
        else:
            p += 2
            for _ in range(2):  # base and delta varints
                while stream[p] & 0x80:
                    p += 1
                p += 1
            if (h >> 1) & 31 and count > 2:
                p += ((count - 2) * width + 7) // 8
    assert p == len(stream), "stream does not end on a run boundary"
    return out
