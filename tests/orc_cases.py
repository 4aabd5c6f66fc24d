"""Case generators shared by the CPU and GPU ORC integer stream tests.

Each generator returns a list of (run_bytes, intended) pairs, one per run:
`intended` is the uint64 view of the values the run was built to hold,
computed here with plain modular arithmetic. check_oracle() asserts that the
oracle decodes the joined stream to exactly those values (the encoder's own
check) and returns the oracle's result, which is what the product is then
compared with.
"""

import numpy as np

from oracle.oracle import orc_rlev2_decode
from tests import orc_streams as S

M64 = (1 << 64) - 1
PATCH_WIDTHS = [w for w in S.WIDTHS if w <= 56]


def _u64(ints):
    return np.array([int(v) & M64 for v in ints], dtype=np.uint64)


def _rand_raws(rng, width, n):
    """n raw values below 2^width as Python ints."""
    hi = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(object)
    lo = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(object)
    return [int((h << 32) | l) & ((1 << width) - 1) for h, l in zip(hi, lo)]


def _zz_dec(raw):
    return (raw >> 1) ^ -(raw & 1)


def stream_of(cases):
    return S.join(r for r, _ in cases), np.concatenate([v for _, v in cases])


def check_oracle(cases, signed):
    """Encoder self-check; returns (stream, oracle values as uint64)."""
    stream, intended = stream_of(cases)
    ref = orc_rlev2_decode(stream, len(intended), signed=signed)
    ref = ref.view(np.uint64)
    bad = np.flatnonzero(ref != intended)
    assert bad.size == 0, (
        f"encoder/oracle disagree at {bad[:5]}: "
        f"{ref[bad[:5]]} != {intended[bad[:5]]}")
    return stream, ref


# ----------------------------------------------------------------- DIRECT

def direct_cases(width, counts, signed, rng, int32_only=False):
    """One DIRECT run per count. Every run starts with the all-ones raw
    value (unsigned maximum; zigzag: the most negative value the width can
    hold), raw 0 and the largest even raw (zigzag: the most positive)."""
    top = (1 << width) - 1
    if int32_only and not signed:
        top = min(top, (1 << 31) - 1)
    out = []
    for n in counts:
        raws = ([top, 0, top - 1] +
                [r & top for r in _rand_raws(rng, width, n)])[:n]
        vals = [_zz_dec(r) for r in raws] if signed else raws
        out.append((S.direct(raws, width), _u64(vals)))
    return out


def short_repeat_cases(signed, repeats=(3, 10)):
    """Byte widths 1..8, top bit of the literal set."""
    out = []
    for wb in range(1, 9):
        raw = int.from_bytes(bytes([0xA5] + [0x5A] * (wb - 1)), "big")
        for rep in repeats:
            v = _zz_dec(raw) if signed else raw
            out.append((S.short_repeat(raw, wb, rep), _u64([v] * rep)))
    return out


# ------------------------------------------------------------------ DELTA

def delta_fixed_cases(counts, signed):
    """Width code 0: positive, negative and zero fixed delta."""
    out = []
    for n in counts:
        for base, d in ((5, 7), ((1 << 40) + 3, -7), (1 << 33, 0)):
            if signed:
                base = -base if d >= 0 else base
            vals = [base + i * d for i in range(n)]
            out.append((S.delta(base, d, [], 0, signed=signed, count=n),
                        _u64(vals)))
    return out


def delta_packed_cases(width, counts, signed, rng):
    """Both directions per count. Magnitudes reach 2^w-1 for w <= 48; from
    56 bits on a run holds ONE full-range magnitude and small ones
    otherwise, so the running value stays inside int64 and the result is
    well defined. Unsigned streams keep every value in [0, 2^63)."""
    top = (1 << width) - 1
    out = []
    for n in counts:
        for sign in (1, -1):
            m = max(n - 2, 0)
            if width <= 48:
                mags = [r for r in _rand_raws(rng, width, m)]
                if m:
                    mags[0] = top
                    mags[-1] = top
            else:
                mags = [int(x) for x in rng.integers(0, 1000, m)]
                if m:
                    mags[(n * 7) % m] = top
            d0 = sign * (width + 1)
            if signed:
                base = -(1 << 61) - 3 if sign > 0 else (1 << 61) + 12345
            else:
                base = 5 if sign > 0 else (1 << 62) + 12345
            vals, cur = [base], base
            if n > 1:
                cur += d0
                vals.append(cur)
            for g in mags:
                g = g - (1 << 64) if g >> 63 else g  # the int64 the bits hold
                cur += sign * g
                vals.append(cur)
            assert all(-(1 << 63) <= v < (1 << 63) for v in vals)
            if not signed:
                assert all(v >= 0 for v in vals)
            out.append((S.delta(base, d0, mags, width, signed=signed,
                                count=n), _u64(vals)))
    return out


# ----------------------------------------------------------- PATCHED_BASE

def patch_entries(positions, patches, pgw):
    """(gap, patch) entries reaching `positions`: a gap too wide for pgw
    bits is carried by (2^pgw-1, 0) extension entries, the spec's (255, 0)
    at pgw = 8."""
    maxgap = (1 << pgw) - 1
    out, prev = [], 0
    for pos, pv in zip(positions, patches):
        d = pos - prev
        while d > maxgap:
            out.append((maxgap, 0))
            d -= maxgap
        out.append((d, pv))
        prev = pos
    assert len(out) <= 31, len(out)
    return out


def base_for(base_bytes, negative):
    """A base whose magnitude needs the top byte of base_bytes (the sign
    bit sits in that byte too)."""
    mag = 77 if base_bytes == 1 else (1 << (8 * base_bytes - 2)) | 77
    return -mag if negative else mag


def patched_run(width, pw, pgw, base, base_bytes, count, positions, rng):
    """One PATCHED_BASE run with a patch at each position. Patch values are
    as wide as pw allows (all ones, or all ones but the lowest bit) unless
    base + value would leave int64, where the oracle's arithmetic stops
    being defined; then the widest patch that stays inside is used. The
    unpatched elements are below 2^56 and the base below 2^63 - 2^56, so
    they cannot leave it."""
    assert width <= 56 and abs(base) < (1 << 63) - (1 << 56)
    reduced = rng.integers(0, 1 << width, count, dtype=np.uint64)
    reduced[0] = (1 << width) - 1
    full = reduced.copy()
    patches = []
    for k, pos in enumerate(positions):
        cands = [(1 << pw) - 1 - (k % 2 if pw > 1 else 0)]
        while cands[-1] > 1:
            cands.append(cands[-1] >> 1)
        for pv in cands:
            raw = int(reduced[pos]) | (pv << width)
            as_i64 = raw - (1 << 64) if raw >> 63 else raw
            if -(1 << 63) <= base + as_i64 < (1 << 63):
                break
        else:
            raise AssertionError("no patch value fits")
        patches.append(pv)
        full[pos] = raw
    run = S.patched_base(base, base_bytes, reduced, width,
                         patch_entries(positions, patches, pgw), pw, pgw)
    return run, full + np.uint64(base & M64)  # wraps mod 2^64


def patch_lists(pgw, count):
    """The patch position lists every (width, pw, pgw, base) runs with:
      - one entry;
      - 31 entries, the first at position 0;
      - a list with a gap wider than pgw bits hold, which takes a
        (2^pgw-1, 0) extension entry: the spec's (255, 0) at pgw = 8. It
        starts at position 0 and ends on the last element where 31 entries
        reach that far (they cannot at pgw = 1: see patched_cases)."""
    maxgap = (1 << pgw) - 1
    step = [1 + (i % min(3, maxgap)) for i in range(30)]
    pos31 = [0] + [int(p) for p in np.cumsum(step)]
    assert pos31[-1] < count
    lists = [[min(17, maxgap, count - 1)], pos31]
    far = maxgap + 2
    if far < count:
        ext = [0, far] + ([count - 1] if far < count - 1 else [])
        lists.append(ext if _fits(ext, pgw) else [0, far])
    return lists


def _fits(positions, pgw):
    maxgap = (1 << pgw) - 1
    n, prev = 0, 0
    for p in positions:
        n += 1 + max(p - prev - 1, 0) // maxgap
        prev = p
    return n <= 31


def patched_cases(width, counts, rng):
    """The PATCHED_BASE matrix for one packed width: pw x pgw x base sign x
    base_bytes x patch list, at each count. At pgw = 1 a gap is at most 1,
    so 31 entries end at position 30: there a run of exactly 31 values,
    every one patched, puts a patch on the first and the last element."""
    out = []
    for pw in (1, 8):
        if width + pw > 64:
            continue
        for pgw in (1, 5, 8):
            for bb in range(1, 9):
                for neg in (False, True):
                    base = base_for(bb, neg)
                    for count in counts:
                        for positions in patch_lists(pgw, count):
                            out.append(patched_run(
                                width, pw, pgw, base, bb, count,
                                positions, rng))
                    if pgw == 1:
                        out.append(patched_run(width, pw, pgw, base, bb, 31,
                                               list(range(31)), rng))
    return out


# --------------------------------------------------------------- byte-RLE

def byte_rle_decode(stream, n):
    """Plain restatement of the spec's byte-RLE, the reference for kind 2
    (the oracle library has no tinyint decoder)."""
    out, p = [], 0
    while len(out) < n:
        h = stream[p]
        p += 1
        if h < 128:
            v = stream[p] - 256 if stream[p] > 127 else stream[p]
            out += [v] * (h + 3)
            p += 1
        else:
            k = 256 - h
            out += [b - 256 if b > 127 else b for b in stream[p:p + k]]
            p += k
    return np.array(out[:n], dtype=np.int64)
