"""Plain-Python model of the BOOLEAN value streams and builders for them,
written from the format specifications, independent of the product's decoder:
Parquet PLAIN booleans (1 bit per value, LSB first) and ORC boolean streams
(byte-RLE over bytes that hold 8 values each, MSB first).

The product accepts either bit order with either framing, so the model does
too: `msb` says how the 8 values of a byte are ordered, `raw`/`byte_rle` how
the bytes are framed."""

from tests import orc_streams as S

# value counts every suite walks: around one byte, one wave (64 source bytes
# = 512 values), the largest ORC literal group (1024) and run (1040), and a
# count that takes several units of either format
COUNTS = [1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1039, 1040, 1041, 4099]


def pack(values, msb):
    """0/1 values -> bytes, 8 per byte in the given bit order, zero-padded."""
    out = bytearray((len(values) + 7) // 8)
    for i, v in enumerate(values):
        if v:
            out[i >> 3] |= (0x80 >> (i & 7)) if msb else (1 << (i & 7))
    return bytes(out)


def expand_raw(data, n, msb):
    """The first n values of raw packed bytes."""
    out = []
    for i in range(n):
        b = data[i >> 3]
        out.append((b >> (7 - (i & 7))) & 1 if msb else (b >> (i & 7)) & 1)
    return out


def byte_rle_decode(stream, n_bytes):
    """ORC byte-RLE -> at least n_bytes decoded bytes (the spec's "Byte Run
    Length Encoding": header 0..127 = run of header + 3 copies, header
    -1..-128 = -header literals)."""
    out = bytearray()
    p = 0
    while len(out) < n_bytes:
        h = stream[p]
        p += 1
        if h < 128:
            out += bytes([stream[p]]) * (h + 3)
            p += 1
        else:
            lit = 256 - h
            out += stream[p:p + lit]
            p += lit
    return bytes(out)


def expand_byte_rle(stream, n, msb):
    return expand_raw(byte_rle_decode(stream, (n + 7) // 8), n, msb)


def byte_rle_segments(data, plan):
    """Frame `data` as byte-RLE following `plan`, a list of ("run", k) /
    ("lit", k) byte counts that sum to len(data). A run's bytes must all be
    equal (the caller builds data that way)."""
    out, p = [], 0
    for kind, k in plan:
        seg = data[p:p + k]
        if kind == "run":
            assert len(set(seg)) == 1 and 3 <= k <= 130
            v = seg[0] - 256 if seg[0] > 127 else seg[0]
            out.append(S.byte_run(v, k))
        else:
            out.append(S.byte_literal(list(seg)))
        p += k
    assert p == len(data)
    return S.join(out)


def random_byte_rle(rng, n_values, run_lens=(3, 130), lit_lens=(1, 128)):
    """A byte-RLE stream of n_values random booleans mixing runs and literal
    groups of random sizes within the given bounds; the last segment may
    carry more bytes than the values need (a stripe's padding only pads the
    last BYTE, but a decoder has to stop at the value count either way).
    Returns (stream, values, plan)."""
    n_bytes = (n_values + 7) // 8
    data, plan = bytearray(), []
    while len(data) < n_bytes:
        if rng.random() < 0.5:
            k = int(rng.integers(run_lens[0], run_lens[1] + 1))
            b = int(rng.choice([0x00, 0xFF, int(rng.integers(0, 256))]))
            data += bytes([b]) * k
            plan.append(("run", k))
        else:
            k = int(rng.integers(lit_lens[0], lit_lens[1] + 1))
            data += bytes(int(x) for x in rng.integers(0, 256, k))
            plan.append(("lit", k))
    return byte_rle_segments(bytes(data), plan), bytes(data), plan
