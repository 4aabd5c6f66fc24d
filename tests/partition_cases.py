"""Case list and numpy model shared by tests/test_partition_cpu.py and
tests/test_partition_gpu.py.

A case is (id, builder, tile_rows); the builder returns the per-run key
arrays (ascending and unique within a run, all int64 or all int32). Cases and
their expected cuts are built once per process and never modified.

The model is independent of the code under test: concatenate
(key ^ 2^63 as uint64, run) over all rows, lexsort by (key, run), and for each
bound count the runs in the prefix of min(b * tile_rows, total) rows."""

import functools

import numpy as np

from tests import keydomain

TILE = 3584  # PMH_TILE_ROWS
RUN_COUNTS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)  # template bounds, +1, below


def model_cuts(key_lists, tile_rows):
    k = len(key_lists)
    key = np.concatenate([
        np.asarray(a).astype(np.int64).view(np.uint64) ^ np.uint64(2**63)
        for a in key_lists])
    run = np.concatenate([np.full(len(a), r, np.int64)
                          for r, a in enumerate(key_lists)])
    run = run[np.lexsort((run, key))]
    total = len(run)
    n_bounds = (total + tile_rows - 1) // tile_rows + 1
    cuts = np.empty((n_bounds, k), np.int32)
    for b in range(n_bounds):
        cuts[b] = np.bincount(run[:min(b * tile_rows, total)], minlength=k)
    return cuts


def _draw(rng, lo, hi, n, dtype):
    """n sorted unique keys from [lo, hi)."""
    return np.sort(rng.choice(np.arange(lo, hi, dtype=np.int64), size=n,
                              replace=False)).astype(dtype)


def _split(total, k):
    """k run lengths summing to total, as even as possible."""
    return [(total + r) // k for r in range(k)]


def dense(k, dtype, seed, lens=None):
    """Keys dense in [0, 1.5 * total): runs collide often."""
    rng = np.random.default_rng(seed)
    if lens is None:
        lens = [int(x) for x in rng.integers(250, 401, k)]
    total = max(sum(lens), 1)
    return [_draw(rng, 0, total * 3 // 2 + 2, n, dtype) for n in lens]


def same_keys(k, rows, dtype, seed):
    rng = np.random.default_rng(seed)
    keys = _draw(rng, -rows, rows * 2, rows, dtype)
    return [keys.copy() for _ in range(k)]


def half_shared(k, rows, dtype, seed):
    """Half of every run's keys come from a pool all runs hold."""
    rng = np.random.default_rng(seed)
    shared = _draw(rng, 0, rows * 4, rows // 2, np.int64) * 2  # even
    out = []
    for _ in range(k):
        own = _draw(rng, 0, rows * 4 * k, rows - rows // 2, np.int64) * 2 + 1
        out.append(np.sort(np.concatenate([shared, own])).astype(dtype))
    return out


def disjoint(k, rows, dtype, seed):
    """Run r lies entirely below run r + 1."""
    rng = np.random.default_rng(seed)
    return [_draw(rng, r * rows * 3, r * rows * 3 + rows * 2, rows, dtype)
            for r in range(k)]


def long_run(k, dtype, seed):
    """One run 100x longer than the others."""
    return dense(k, dtype, seed, lens=[30000] + [300] * (k - 1))


def int32_full_range(k, rows, seed):
    rng = np.random.default_rng(seed)
    out = []
    for r in range(k):
        u = np.unique(rng.integers(-2**31, 2**31, rows * 2, dtype=np.int64))
        u = rng.permutation(u[(u != -2**31) & (u != 2**31 - 1)])[:rows - 2]
        out.append(np.sort(np.concatenate(
            [u, [-2**31, 2**31 - 1]])).astype(np.int32))
    return out


def _keys(runs):
    return [r["key"] for r in runs]


def _cases():
    c = []

    def add(name, builder, tile_rows=64):
        c.append((name, builder, tile_rows))

    for dt, tag in ((np.int64, "i64"), (np.int32, "i32")):
        # many bounds: coarse and refine levels, several coarse windows
        for k in RUN_COUNTS:
            add(f"dense_k{k}_{tag}",
                functools.partial(dense, k, dt, 100 + k))
        # the n_bounds > G + 1 edge (17 | 18 bounds): an exact multiple of
        # the tile, and one row more
        for k in (4, 8):
            add(f"bounds17_k{k}_{tag}", functools.partial(
                dense, k, dt, 200 + k, _split(1024, k)))
            add(f"bounds18_k{k}_{tag}", functools.partial(
                dense, k, dt, 210 + k, _split(1025, k)))
        add(f"bounds3_k5_{tag}",
            functools.partial(dense, 5, dt, 220, _split(100, 5)))
        add(f"bounds2_k3_{tag}",
            functools.partial(dense, 3, dt, 221, _split(64, 3)))
        # the production tile: 9 tiles exactly, and one row more
        for k in (5, 8, 16):
            add(f"tile3584_x9_k{k}_{tag}", functools.partial(
                dense, k, dt, 300 + k, _split(9 * TILE, k)), TILE)
            add(f"tile3584_x9p1_k{k}_{tag}", functools.partial(
                dense, k, dt, 310 + k, _split(9 * TILE + 1, k)), TILE)
        # ties
        for k in (3, 8, 17):
            add(f"same_keys_k{k}_{tag}",
                functools.partial(same_keys, k, 300, dt, 400 + k))
        add(f"half_shared_k8_{tag}",
            functools.partial(half_shared, 8, 300, dt, 410))
        add(f"half_shared_k9_{tag}",
            functools.partial(half_shared, 9, 300, dt, 411))
        # disjoint runs: empty refine windows, the all-windows-empty exit
        add(f"disjoint_k2_{tag}", functools.partial(disjoint, 2, 640, dt, 500))
        add(f"disjoint_k8_{tag}", functools.partial(disjoint, 8, 256, dt, 501))
        add(f"disjoint_k16_{tag}",
            functools.partial(disjoint, 16, 100, dt, 502))
        add(f"long_run_k4_{tag}", functools.partial(long_run, 4, dt, 510))
        add(f"long_run_k9_{tag}", functools.partial(long_run, 9, dt, 511))
        # empty runs and runs of length 1
        for k in (4, 5, 9, 17):
            n = 330
            add(f"empty_first_k{k}_{tag}", functools.partial(
                dense, k, dt, 600 + k, [0] + [n] * (k - 1)))
            add(f"empty_last_k{k}_{tag}", functools.partial(
                dense, k, dt, 610 + k, [n] * (k - 1) + [0]))
            add(f"empty_middle_k{k}_{tag}", functools.partial(
                dense, k, dt, 620 + k,
                [n] * (k // 2) + [0] + [n] * (k - k // 2 - 1)))
            add(f"only_last_k{k}_{tag}", functools.partial(
                dense, k, dt, 630 + k, [0] * (k - 1) + [1500]))
            add(f"only_first_k{k}_{tag}", functools.partial(
                dense, k, dt, 640 + k, [1500] + [0] * (k - 1)))
            add(f"len1_k{k}_{tag}", functools.partial(
                dense, k, dt, 650 + k, [1, n, 1] + [n] * (k - 3)
                if k >= 3 else [1] * k))
        add(f"all_len1_k32_{tag}",
            functools.partial(dense, 32, dt, 660, [1] * 32), 3)

    # key-domain edges (tests/keydomain.py)
    add("neg_dense_k8", lambda: _keys(keydomain.neg_dense(8, 300, 700)))
    add("neg_dense_k17", lambda: _keys(keydomain.neg_dense(17, 150, 701)))
    add("full_span_k8", lambda: _keys(keydomain.full_span(8, 300, 710)))
    add("full_span_k3", lambda: _keys(keydomain.full_span(3, 400, 711)))
    add("full_span_k16", lambda: _keys(keydomain.full_span(16, 200, 712)))
    add("full_span_same_keys_k12",
        lambda: _keys(keydomain.identical(12, 300, 713)))
    add("clustered_k8",
        lambda: _keys(keydomain.clustered(8, 300, 720, tile_rows=64)))
    add("clustered_k4_tile3584",
        lambda: _keys(keydomain.clustered(4, 9 * TILE // 4, 721)), TILE)
    add("lopsided", lambda: _keys(keydomain.lopsided(3000, 730)))
    add("i32_full_range_k8", functools.partial(int32_full_range, 8, 300, 740))
    add("i32_full_range_k5", functools.partial(int32_full_range, 5, 300, 741))
    # two-level scheme at the production tile (20 tiles and one row)
    add("tile3584_x20p1_k8_i64", functools.partial(
        dense, 8, np.int64, 800, _split(20 * TILE + 1, 8)), TILE)
    return c


CASES = _cases()
CASE_IDS = [c[0] for c in CASES]
_BY_ID = {c[0]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def case(name):
    """(runs, tile_rows, expected cuts) of one case, built once."""
    _, builder, tile_rows = _BY_ID[name]
    runs = builder()
    for a in runs:
        assert len(a) < 2 or (a[1:] > a[:-1]).all()
        a.setflags(write=False)
    want = model_cuts(runs, tile_rows)
    want.setflags(write=False)
    return runs, tile_rows, want


def check_cuts(got, runs, tile_rows, want):
    total = sum(len(a) for a in runs)
    n_bounds = (total + tile_rows - 1) // tile_rows + 1
    assert got.shape == (n_bounds, len(runs))
    sums = np.minimum(np.arange(n_bounds, dtype=np.int64) * tile_rows, total)
    assert (got.sum(axis=1, dtype=np.int64) == sums).all()
    assert np.array_equal(got, want)
