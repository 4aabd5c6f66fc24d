"""One small shape that puts every column dtype through an emit kernel, for
the GPU tests of the kernels that share the column-access helpers of
kernels.hip (col_valid, member_col, col_load_wide, out_store, the slice and
tile-cursor helpers).

Shape: 3 runs x 2 500 rows over 3 500 keys: 7 500 rows in three merge tiles of
3 584, the last one ragged, with key groups of one to three members. Columns:
v_k (the key again), one non-null column of each of the seven dtype codes
(int8, int16, int32, int64, float32, float64, string) and one nullable column
of each of the four output widths (1, 2, 4, 8 bytes; 30 % nulls). Integers
span their whole range, so a store of the wrong width or a lost sign shows.

A test reads once at the default emit grid and once with PMH_EMIT_BLOCKS=7:
seven slices of about a thousand rows, whose edges fall inside tiles and which
cross the tile boundaries, so both the tile search and the forward walk of the
cursor run.

Runs are in the oracle models' layout: key / seq / kind, values[c] and
valid[c] by column index, values[0] = v_k. String values are ids into
STR_DICT."""

import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

N_RUNS, ROWS, KEYSPACE = 3, 2_500, 3_500
EMIT_BLOCKS = (None, "7")  # None = variable unset (the default grid)
NULL_FRAC = 0.3
STR_DICT = [f"s{i:03d}" for i in range(200)]

# (name, plan type, numpy dtype of the values, has nulls)
COLS = [
    ("v_i8", "int8", np.int8, False),
    ("v_i16", "int16", np.int16, False),
    ("v_i32", "int32", np.int32, False),
    ("v_i64", "int64", np.int64, False),
    ("v_f32", "float32", np.float32, False),
    ("v_f64", "float64", np.float64, False),
    ("v_s", "string", np.int32, False),
    ("n_i8", "int8", np.int8, True),
    ("n_i16", "int16", np.int16, True),
    ("n_i32", "int32", np.int32, True),
    ("n_i64", "int64", np.int64, True),
]
NAMES = ["v_k"] + [c[0] for c in COLS]
KEY_COLS = [{"name": "_KEY_k", "type": "int64"}]
VALUE_COLS = ([{"name": "v_k", "type": "int64"}] +
              [{"name": nm, "type": pt} for nm, pt, _, _ in COLS])


def index_of(name):
    """Index of a column in the runs' values / valid lists."""
    return NAMES.index(name)


def _column(rng, name, dt, n):
    if name == "v_s":
        return rng.integers(0, len(STR_DICT), n).astype(np.int32)
    if np.issubdtype(dt, np.floating):
        return rng.standard_normal(n).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)


def gen(seed, kinds=(0,), kind_p=None, top=False, nulls=True):
    """N_RUNS runs, kinds drawn from `kinds`. Sequence numbers are a
    permutation, so every total order is strict. top: the last run holds the
    oldest sequence numbers and INSERTs only (a max-level run of a
    full-compaction changelog case). nulls=False: no column holds a null, so
    no validity array is staged (the folding engines then run without their
    packed row masks)."""
    rng = np.random.default_rng(seed)
    seqs = rng.permutation(N_RUNS * ROWS).astype(np.int64)
    runs = []
    for r in range(N_RUNS):
        key = np.sort(rng.choice(KEYSPACE, ROWS, replace=False)
                      ).astype(np.int64)
        vals, msks = [key.copy()], [np.ones(ROWS, bool)]
        for name, _, dt, has_nulls in COLS:
            vals.append(_column(rng, name, dt, ROWS))
            msks.append(rng.random(ROWS) >= NULL_FRAC if nulls and has_nulls
                        else np.ones(ROWS, bool))
        seq = seqs[r * ROWS:(r + 1) * ROWS]
        kind = rng.choice(kinds, ROWS, p=kind_p).astype(np.int8)
        if top and r == N_RUNS - 1:
            seq = np.arange(ROWS, dtype=np.int64) - ROWS
            kind = np.zeros(ROWS, np.int8)
        runs.append({"key": key, "seq": seq, "kind": kind, "values": vals,
                     "valid": msks})
    return runs


def write(runs, out_dir, levels=None):
    """Parquet files of the runs (every value column an optional field, the
    string column dictionary-encoded); returns their metas."""
    os.makedirs(out_dir, exist_ok=True)
    metas = []
    for i, run in enumerate(runs):
        fields = [pa.field("_KEY_k", pa.int64(), nullable=False),
                  pa.field("_SEQUENCE_NUMBER", pa.int64(), nullable=False),
                  pa.field("_VALUE_KIND", pa.int8(), nullable=False)]
        arrays = [pa.array(run["key"]), pa.array(run["seq"]),
                  pa.array(run["kind"])]
        for c, name in enumerate(NAMES):
            v, mask = run["values"][c], ~run["valid"][c]
            if name == "v_s":
                arr = pa.DictionaryArray.from_arrays(pa.array(v, mask=mask),
                                                     pa.array(STR_DICT))
            else:
                arr = pa.array(v, mask=mask)
            fields.append(pa.field(name, arr.type, nullable=True))
            arrays.append(arr)
        path = os.path.join(out_dir, f"run-{i}.parquet")
        pq.write_table(pa.Table.from_arrays(arrays, schema=pa.schema(fields)),
                       path, compression=None, use_dictionary=["v_s"],
                       data_page_version="1.0", store_schema=False)
        metas.append({"path": path, "rowCount": len(run["key"]),
                      "minKey": int(run["key"][0]),
                      "maxKey": int(run["key"][-1]),
                      "level": levels[i] if levels else 0})
    return metas


def gather(runs, r, w, kind=None):
    """The records (run r[i], row w[i]) as a model-style output dict."""
    pick = lambda src: np.array([src(a)[b] for a, b in zip(r, w)],
                                dtype=src(0).dtype)
    return {"key": pick(lambda a: runs[a]["key"]),
            "seq": pick(lambda a: runs[a]["seq"]),
            "kind": (pick(lambda a: runs[a]["kind"]) if kind is None
                     else np.asarray(kind, np.int8)),
            "values": [pick(lambda a, c=c: runs[a]["values"][c])
                       for c in range(len(NAMES))],
            "valid": [pick(lambda a, c=c: runs[a]["valid"][c])
                      for c in range(len(NAMES))]}


def read_all(plan, changelog=False):
    """The plan's batches, concatenated (and its changelog batches)."""
    main, cl = {}, {}
    while True:
        b = plan.read_next()
        if b is None:
            break
        for k, v in b.items():
            main.setdefault(k, []).append(v.copy())
        if changelog:
            for k, v in plan.read_changelog().items():
                cl.setdefault(k, []).append(v.copy())
    cat = lambda d: {k: v[0] if k.endswith("#dict") else np.concatenate(v)
                     for k, v in d.items()}
    return (cat(main), cat(cl)) if changelog else cat(main)


def check(got, exp, what, dicts=None):
    """Every column of `got` against the model-style dict `exp`: key,
    sequence number, kind, validity, dtype, and the bytes of every non-null
    value (strings through the dictionary of `got`, or of `dicts`)."""
    n = len(exp["key"])
    assert n > 0, what
    assert len(got["_KEY_k"]) == n, (what, len(got["_KEY_k"]), n)
    assert (got["_KEY_k"] == exp["key"]).all(), what
    assert (got["_SEQUENCE_NUMBER"] == exp["seq"]).all(), what
    assert (got["_VALUE_KIND"] == exp["kind"]).all(), what
    for c, nm in enumerate(NAMES):
        ev, em = np.asarray(exp["values"][c]), np.asarray(exp["valid"][c], bool)
        gm = got.get(nm + "#valid")
        if gm is None:
            gm = np.ones(n, bool)
        assert (gm.astype(bool) == em).all(), (what, nm, "validity")
        g = got[nm]
        assert len(g) == n, (what, nm)
        if nm == "v_s":
            d = got.get("v_s#dict", (dicts or {}).get("v_s#dict"))
            e = np.array([s.encode() for s in STR_DICT], object)[ev[em]]
            assert (d[g[em]] == e).all(), (what, nm)
            continue
        assert g.dtype == ev.dtype, (what, nm, g.dtype, ev.dtype)
        assert g[em].tobytes() == ev[em].tobytes(), \
            f"{what} {nm}: rows {np.flatnonzero((g != ev) & em)[:8]}"
