"""Spec-level ORC DECIMAL stream tools for the tests: a varint encoder and an
independent pure-Python decoder over Python ints (ORC v1 spec, "Decimal
Columns": the DATA stream holds each unscaled value as a zigzag base-128
varint, least-significant group first; SECONDARY holds each value's scale).
Shares no code with the product."""

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
FULL_RANGE = 19  # "precision" under which every int64 is in range


class DecimalRangeError(ValueError):
    """A value the column cannot hold (what the product must refuse)."""


def zigzag(v):
    assert INT64_MIN <= v <= INT64_MAX
    return (v << 1) if v >= 0 else ((-v << 1) - 1)


def encode_value(v):
    u = zigzag(v)
    out = bytearray()
    while True:
        if u < 0x80:
            out.append(u)
            return bytes(out)
        out.append(0x80 | (u & 0x7F))
        u >>= 7


def encode(values):
    return b"".join(encode_value(int(v)) for v in values)


def value_starts(values, lead=0):
    """(start offset, byte length) of every value of encode(values), the
    stream beginning at offset `lead`."""
    out, off = [], lead
    for v in values:
        n = len(encode_value(int(v)))
        out.append((off, n))
        off += n
    return out


def with_length(nbytes, sign, salt=0):
    """A value whose varint takes exactly nbytes (1..10) bytes: zigzag codes
    of nbytes bytes span [2^(7(n-1)), 2^(7n)) (10 bytes: up to 2^64)."""
    lo = 0 if nbytes == 1 else 1 << (7 * (nbytes - 1))
    hi = min(1 << (7 * nbytes), 1 << 64)
    u = lo + (salt * 0x9E3779B97F4A7C15 + 12345) % (hi - lo)
    u = (u & ~1) | (1 if sign < 0 else 0)  # zigzag: odd codes are negative
    if u < lo:
        u += 2
    v = (u >> 1) if not (u & 1) else -((u + 1) >> 1)
    assert len(encode_value(v)) == nbytes, (nbytes, sign, v)
    assert (v < 0) == (sign < 0) or v == 0
    return v


def decode(stream, n_values, precision, scale, scales=None, out_bits=64):
    """n_values unscaled ints at the column scale. Raises ValueError on a
    malformed stream and DecimalRangeError on a value outside the column."""
    out, p = [], 0
    for j in range(n_values):
        if p >= len(stream):
            raise ValueError("fewer values than asked")
        u, shift, n = 0, 0, 0
        while True:
            if p >= len(stream):
                raise ValueError("stream ends inside a value")
            b = stream[p]
            p += 1
            n += 1
            if n > 10:
                raise ValueError("value longer than 10 bytes")
            u |= (b & 0x7F) << shift
            shift += 7
            if not (b & 0x80):
                break
        if u >= 1 << 64:
            raise ValueError("value wider than 64 bits")
        v = (u >> 1) if not (u & 1) else -((u + 1) >> 1)
        ds = scale if scales is None else int(scales[j])
        if ds < 0:
            raise DecimalRangeError("negative data scale")
        if ds > scale:
            raise DecimalRangeError("data scale above the column scale")
        v *= 10 ** (scale - ds)
        if precision >= FULL_RANGE:
            if not INT64_MIN <= v <= INT64_MAX:
                raise DecimalRangeError("outside int64")
        elif abs(v) >= 10 ** precision:
            raise DecimalRangeError("10^precision or more")
        if out_bits == 32 and not -(1 << 31) <= v < (1 << 31):
            raise DecimalRangeError("outside int32")
        out.append(v)
    return out
