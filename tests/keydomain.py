"""Key-domain edge generators shared by tests/test_keydomain_cpu.py and
tests/test_keydomain_gpu.py, plus the independent numpy model the CPU file
pins the C oracle against.

Every other generator in the suite draws non-negative keys dense in
[0, 1.5 * rows); these place the keys where the int64 domain itself matters:
across zero, at INT64_MIN / INT64_MAX, spread over the whole range, in
clusters separated by 2^40 gaps, and exactly at the 2^32-2 tile-span limit of
the fused kernel's 32-bit key repack.

Each generator is seeded and returns runs in the tests/util.random_runs
shape ({key, seq, kind, values[, valid]}; keys ascending and unique per run,
sequence numbers unique across runs, values[0] a copy of the key). `seq_base`
is added to every sequence number (SEQ_BASES; 2^60 is inside both packed
sequence words, (seq << 1) | isAdd and seq << 2)."""

import numpy as np

I64_MIN = -2**63
I64_MAX = 2**63 - 1
TILE_ROWS = 3584  # PMH_TILE_ROWS
REPACK_LIMIT = 0xfffffffe  # k_merge_emit repacks a tile iff max-min < this
SEQ_BASES = (0, 2**40, 2**60)
THRESHOLD_SPANS = (2**32 - 3, 2**32 - 2, 2**32 - 1, 2**32)


def threshold_bases(span):
    return (0, I64_MIN, I64_MAX - span)


def finish_runs(rng, key_lists, seq_base=0, delete_p=0.2, n_value_cols=2,
            null_p=0.0):
    """Attach seq / kind / values to per-run sorted unique key arrays."""
    total = sum(len(k) for k in key_lists)
    seqpool = rng.permutation(total).astype(np.int64) + np.int64(seq_base)
    runs, off = [], 0
    for keys in key_lists:
        keys = np.asarray(keys, np.int64)
        n = len(keys)
        assert n == 0 or (keys[1:] > keys[:-1]).all()
        r = {"key": keys, "seq": seqpool[off:off + n].copy(),
             "kind": np.where(rng.random(n) < delete_p, 3, 0).astype(np.int8),
             "values": [keys.copy()] + [
                 rng.integers(-2**31, 2**31, n).astype(np.int32)
                 for _ in range(n_value_cols)]}
        if null_p > 0:
            r["valid"] = [np.ones(n, bool)] + [
                rng.random(n) >= null_p for _ in range(n_value_cols)]
        off += n
        runs.append(r)
    return runs


def _choose_sorted(rng, universe, n):
    return np.sort(rng.choice(universe, size=n, replace=False))


def _full_span_universe(rng, n):
    """n unique keys uniform over the whole int64 range, INT64_MIN and
    INT64_MAX included."""
    u = np.unique(rng.integers(I64_MIN, I64_MAX, size=n + 64, dtype=np.int64,
                               endpoint=True))
    u = u[(u != I64_MIN) & (u != I64_MAX)]
    u = rng.permutation(u)[:n - 2]
    return np.sort(np.concatenate([u, np.array([I64_MIN, I64_MAX],
                                               np.int64)]))


def neg_dense(n_runs, rows, seed, seq_base=0, **kw):
    """A: keys uniform in [-T, T/2), T = n_runs * rows — dense, crossing
    zero."""
    rng = np.random.default_rng(seed)
    total = n_runs * rows
    dom = np.arange(-total, total // 2, dtype=np.int64)
    return finish_runs(rng, [_choose_sorted(rng, dom, rows)
                         for _ in range(n_runs)], seq_base, **kw)


def _rank_seq(runs, members, top):
    """Permute the sequence numbers of one key group's members (run, row)
    so that member `top` holds the largest (top >= 0) or, for top = ~i,
    member i holds the smallest."""
    seqs = sorted(int(runs[r]["seq"][w]) for r, w in members)
    if top >= 0:
        order = [m for i, m in enumerate(members) if i != top] + [members[top]]
    else:
        order = [members[~top]] + [m for i, m in enumerate(members)
                                   if i != ~top]
    for (r, w), s in zip(order, seqs):
        runs[r]["seq"][w] = s


def full_span(n_runs, rows, seed, seq_base=0, **kw):
    """B: keys uniform over the whole int64 range, drawn from a shared pool
    of ~0.75 * T keys so runs collide. INT64_MIN and INT64_MAX sit in runs
    0, 1 and the last run. Run 0's INT64_MIN record is a DELETE carrying the
    group's HIGHEST sequence number (the key vanishes under drop-delete);
    run 1's INT64_MAX record is a DELETE carrying the group's LOWEST (an
    INSERT wins). A 3584-row tile spans ~2^64 * 3584 / T >> 2^32."""
    rng = np.random.default_rng(seed)
    total = n_runs * rows
    pool = _full_span_universe(rng, max(total * 3 // 4, rows + rows // 2))
    inner = pool[1:-1]
    forced = sorted({0, min(1, n_runs - 1), n_runs - 1})
    lists = []
    for r in range(n_runs):
        if r in forced:
            k = _choose_sorted(rng, inner, rows - 2)
            k = np.concatenate([[I64_MIN], k, [I64_MAX]]).astype(np.int64)
        else:
            k = _choose_sorted(rng, inner, rows)
        lists.append(k)
    runs = finish_runs(rng, lists, seq_base, **kw)
    for r in forced:
        runs[r]["kind"][0] = 0
        runs[r]["kind"][-1] = 0
    runs[forced[0]]["kind"][0] = 3
    runs[forced[min(1, len(forced) - 1)]]["kind"][-1] = 3
    if len(forced) > 1:
        _rank_seq(runs, [(r, 0) for r in forced], top=0)
        _rank_seq(runs, [(r, rows - 1) for r in forced], top=~1)
    return runs


def clustered(n_runs, rows, seed, seq_base=0, tile_rows=TILE_ROWS, **kw):
    """C: one dense cluster of T/2 keys at -2^62, then clusters of 500..1500
    dense keys separated by gaps of 2^40. Row counts are laid out against
    the tile: the first cluster holds a whole number of tiles (narrow ones,
    they take the 32-bit repack), the small clusters then repeat 1.5, 1.5,
    0.5 and 0.5 tiles of rows, so per four tiles
      - one starts on a cluster's first key and ends inside it: narrow, with
        its predecessor key 2^40 below its minimum (no 32-bit predecessor),
      - one straddles a gap: wide (int64 fallback), predecessor adjacent,
      - one ends on a cluster's last key: wide only through its per-run
        extras, which belong to the next cluster,
      - one covers two whole clusters: wide, predecessor 2^40 below.
    Every run gets exactly `rows` rows (n_runs >= 4)."""
    rng = np.random.default_rng(seed)
    total = n_runs * rows
    half = tile_rows // 2
    dense_rows = min(max(1, round(total / 2 / tile_rows)) * tile_rows, total)
    segs = [(total // 2, dense_rows)]  # (keys in the cluster, rows drawn)
    left, i = total - dense_rows, 0
    while left > 0:
        s = min((3, 3, 1, 1)[i % 4] * half, left)
        lo = max(500, -(-s // n_runs) + 1)
        assert lo <= 1500, "clustered() needs n_runs >= 4"
        segs.append((int(rng.integers(lo, 1501)), s))
        left -= s
        i += 1
    lists = [[] for _ in range(n_runs)]
    start, done = -2**62, 0
    for m, s in segs:
        cluster = np.arange(m, dtype=np.int64) + start
        for r in range(n_runs):
            # sum over r of floor((c + r) / k) == c: exact row totals
            n = (done + s + r) // n_runs - (done + r) // n_runs
            lists[r].append(_choose_sorted(rng, cluster, n))
        start += m - 1 + 2**40
        done += s
    return finish_runs(rng, [np.concatenate(ks) for ks in lists], seq_base, **kw)


def threshold(span, base, seed, seq_base=0, pred_tile=False,
              tile_rows=TILE_ROWS, **kw):
    """D: one tile — 2 runs, < 3000 rows. Keys base + {0..1399} plus three
    keys ending at base + span; both runs hold base and base + span, so the
    tile's key range is exactly `span` (repacked iff span < 2^32 - 2).

    pred_tile=True puts exactly one tile of rows (tile_rows / 2 per run)
    2^40 below `base` in front, so the threshold tile also has a
    predecessor key that no 32-bit offset can express — the case the
    repack's reserved offset 0xffffffff stands for."""
    rng = np.random.default_rng(seed)
    low = [base + i for i in range(1400)]
    high = [base + span - 2, base + span - 1, base + span]
    front = [base - 2**40 - 2500 + i for i in range(2500)]
    lists = []
    for _ in range(2):
        mid = rng.choice(len(low) - 1, 1100, replace=False) + 1
        ks = [low[0]] + [low[i] for i in np.sort(mid)]
        ks += [h for h in high[:2] if rng.random() < 0.5] + [high[2]]
        if pred_tile:
            pick = np.sort(rng.choice(len(front), tile_rows // 2,
                                      replace=False))
            ks = [front[i] for i in pick] + ks
        lists.append(np.array(ks, dtype=np.int64))
    return finish_runs(rng, lists, seq_base, **kw)


def identical(n_runs, rows, seed, seq_base=0, **kw):
    """E: all runs hold the same `rows` keys (a subset of B's key pool,
    INT64_MIN and INT64_MAX included): every group has n_runs members. A
    tile cut lands inside a group whenever n_runs does not divide the tile
    (12 runs); for 4, 8 and 32 runs every cut falls exactly between two
    groups, so each run's extra element opens the next tile's first group."""
    rng = np.random.default_rng(seed)
    keys = _full_span_universe(rng, rows)
    return finish_runs(rng, [keys.copy() for _ in range(n_runs)], seq_base, **kw)


def lopsided(total, seed, seq_base=0, **kw):
    """F: one run of `total` rows with A's keys plus runs of 1, 2 and 64
    rows that hold the big run's first and last key (one section)."""
    rng = np.random.default_rng(seed)
    dom = np.arange(-total, total // 2, dtype=np.int64)
    big = _choose_sorted(rng, dom, total)
    first, last = big[0], big[-1]
    inner = dom[(dom > first) & (dom < last)]
    r64 = np.concatenate([[first], _choose_sorted(rng, inner, 62), [last]])
    return finish_runs(rng, [big, np.array([last], np.int64),
                         np.array([first, last], np.int64),
                         r64.astype(np.int64)], seq_base, **kw)


def check_invariants(runs):
    """Sorted unique keys per run, globally unique sequence numbers."""
    for r in runs:
        k = r["key"]
        assert k.dtype == np.int64 and r["seq"].dtype == np.int64
        assert (k[1:] > k[:-1]).all()
        assert len(k) == len(r["seq"]) == len(r["kind"])
    seq = np.concatenate([r["seq"] for r in runs])
    assert len(np.unique(seq)) == len(seq)


def dedup_model(runs, drop_delete=True, ignore_delete=False):
    """Deduplicate merge-on-read as DESIGN.md §2 states it, in plain numpy:
    concatenate, stable lexsort by (key, seq, isAdd), keep the last record
    per key; with ignore-delete the last ADD record, a group without one
    yields nothing — except a one-record group, which bypasses the merge
    function and is returned untouched; drop-delete then removes retract
    results. Returns (run, row) in key order."""
    key = np.concatenate([r["key"] for r in runs])
    seq = np.concatenate([r["seq"] for r in runs])
    kind = np.concatenate([r["kind"] for r in runs])
    run = np.concatenate([np.full(len(r["key"]), i, np.int32)
                          for i, r in enumerate(runs)])
    row = np.concatenate([np.arange(len(r["key"]), dtype=np.int64)
                          for r in runs])
    n = len(key)
    if n == 0:
        return np.empty(0, np.int32), np.empty(0, np.int64)
    add = (kind == 0) | (kind == 2)
    order = np.lexsort((add, seq, key))
    key, add, run, row = key[order], add[order], run[order], row[order]
    starts = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    ends = np.r_[starts[1:], n]
    if ignore_delete:
        last = np.maximum.reduceat(np.where(add, np.arange(n), -1), starts)
        last = np.where(ends - starts == 1, starts, last)
    else:
        last = ends - 1
    sel = last[last >= 0]
    if drop_delete:
        sel = sel[add[sel]]
    return run[sel], row[sel]


def tile_stats(runs, tile_rows=TILE_ROWS):
    """Per tile of the (key, run) merge order: (narrow, far_pred) — whether
    the tile's key range (its per-run extras included) takes the 32-bit
    repack, and whether its predecessor key lies more than 2^32 below the
    tile minimum."""
    key = np.concatenate([r["key"] for r in runs])
    run = np.concatenate([np.full(len(r["key"]), i) for i, r in
                          enumerate(runs)])
    order = np.lexsort((run, key))
    key, run = key[order], run[order]
    out = []
    for lo in range(0, len(key), tile_rows):
        hi = min(lo + tile_rows, len(key))
        kmin, kmax = int(key[lo]), int(key[hi - 1])
        for r in np.unique(run):
            nxt = np.flatnonzero(run[hi:] == r)
            if len(nxt):
                kmax = max(kmax, int(key[hi + nxt[0]]))
        far = lo > 0 and kmin - int(key[lo - 1]) > 2**32
        out.append((kmax - kmin < REPACK_LIMIT, far))
    return out
