"""Key-domain edges on the GPU: the product path (plan create + read over
real Parquet / ORC files) against the CPU oracle with keys the rest of the
suite never produces — negative, at INT64_MIN / INT64_MAX, spread over the
whole int64 range, clustered around 2^40 gaps, and exactly at the 2^32-2
tile-span limit of the fused kernel's 32-bit key repack (generators and
their properties: tests/keydomain.py, pinned in tests/test_keydomain_cpu.py).

Every comparison is bit-exact on every key column, _SEQUENCE_NUMBER,
_VALUE_KIND and every value column. Shapes (tile = 3584 rows; the two-level
partition needs > 17 tiles):

  S1  2 x  3000   single-level wave partition, ~2 tiles
  S2  4 x 16000   two-level wave + refine, KM=4 (18 tiles)
  S3  8 x  8000   two-level, KM=8
  S4 12 x  6000   k > 8 seeded refine, KM=16
  S5 20 x  3500   KM=32
  S6 40 x  1000   hierarchical virtual runs
"""

import os

import numpy as np
import pytest

from oracle import (merge_dedup, merge_dedup_useq_model,
                    merge_first_row_model, partial_update_model)
from paimon_amd import Session, MergeReadPlan, file_descs_from_metas
from paimon_amd.datagen import write_runs
from tests import keydomain as kd
from tests import test_lookup_changelog_gpu as tlc
from tests import test_merge_gpu as tmg

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = kd.I64_MIN, kd.I64_MAX
I32_MIN, I32_MAX = -2**31, 2**31 - 1
S1, S2, S3, S4, S5, S6 = ((2, 3000), (4, 16_000), (8, 8000), (12, 6000),
                          (20, 3500), (40, 1000))
SHAPES = {"S1": S1, "S2": S2, "S3": S3, "S4": S4, "S5": S5, "S6": S6,
          "k32": (32, 2500)}

# path_mode in the plan stats: 0 = chain, 1 = fused in-kernel emit,
# 2 = fused split pair
PATHS = {"chain": ({}, 0),
         "fused_split": ({"PMH_FUSED": "1"}, 2),
         "fused_inkernel": ({"PMH_FUSED": "1", "PMH_FSPLIT": "0"}, 1)}


def _select_path(monkeypatch, path):
    env, mode = PATHS[path]
    monkeypatch.delenv("PMH_FUSED", raising=False)
    monkeypatch.delenv("PMH_FSPLIT", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return mode


def _build(gen, shape, seed, **kw):
    k, rows = SHAPES[shape]
    if gen == "A":
        return kd.neg_dense(k, rows, seed, **kw)
    if gen == "B":
        return kd.full_span(k, rows, seed, **kw)
    if gen == "C":
        return kd.clustered(k, rows, seed, **kw)
    if gen == "E":
        return kd.identical(k, rows, seed, **kw)
    assert gen == "F"
    return kd.lopsided(k * rows, seed, **kw)


def _value_cols(runs):
    n = len(runs[0]["values"])
    names = ["v_k"] + [f"v_c{i}" for i in range(n - 1)]
    return [{"name": nm, "type": str(v.dtype)}
            for nm, v in zip(names, runs[0]["values"])]


def _gather(runs, r, w, get):
    """Column of the records (run r[i], row w[i])."""
    r = np.asarray(r, np.int64)
    w = np.asarray(w, np.int64)
    out = np.zeros(len(r), get(runs[0]).dtype)
    for i in np.unique(r):
        sel = r == i
        out[sel] = get(runs[i])[w[sel]]
    return out


def _read_batches(plan):
    batches = []
    while True:
        b = plan.read_next()
        if b is None:
            break
        batches.append({k: v.copy() for k, v in b.items()})
    got = {k: np.concatenate([b[k] for b in batches])
           for k in (batches[0] if batches else {})}
    return got, len(batches)


def _expected(runs, r, w, key_fields=None):
    """Expected output columns of the winner records (r, w). key_fields:
    {column name: run field} of the key columns (default the single
    _KEY_k = run["key"])."""
    exp = {}
    for name, field in (key_fields or {"_KEY_k": "key"}).items():
        exp[name] = _gather(runs, r, w, lambda run, f=field: run[f])
    exp["_SEQUENCE_NUMBER"] = _gather(runs, r, w, lambda run: run["seq"])
    exp["_VALUE_KIND"] = _gather(runs, r, w, lambda run: run["kind"])
    for c, col in enumerate(_value_cols(runs)):
        exp[col["name"]] = _gather(runs, r, w,
                                   lambda run, c=c: run["values"][c])
    return exp


def _assert_columns(got, exp):
    n = len(exp["_SEQUENCE_NUMBER"])
    assert len(got["_SEQUENCE_NUMBER"]) == n, \
        (len(got["_SEQUENCE_NUMBER"]), n)
    for name, e in exp.items():
        g = got[name]
        assert g.dtype == e.dtype, (name, g.dtype, e.dtype)
        assert (g == e).all(), \
            f"column {name} mismatch at {np.flatnonzero(g != e)[:10]}"


def _run_plan(metas, key_cols, value_cols, expect_mode=None, **plan_kw):
    with Session(0) as s:
        with MergeReadPlan(s, file_descs_from_metas(metas), key_cols,
                           value_cols, **plan_kw) as plan:
            got, n_batches = _read_batches(plan)
            mode = plan.stats().get("path_mode", 0)
    if expect_mode is not None:
        assert mode == expect_mode, (mode, expect_mode)
    return got, n_batches


def _dedup_case(tmp_path, runs, expect_mode=0, drop_delete=True,
                ignore_delete=False, file_format="parquet"):
    """Deduplicate over `runs` vs oracle.merge_dedup; returns the batch
    count."""
    metas = write_runs(runs, str(tmp_path), compression="NONE",
                       file_format=file_format)
    r, w = merge_dedup(runs, ignore_delete=ignore_delete,
                       drop_delete=drop_delete)
    key_type = str(runs[0]["key"].dtype)
    got, n_batches = _run_plan(
        metas, [{"name": "_KEY_k", "type": key_type}], _value_cols(runs),
        expect_mode, drop_delete=drop_delete, ignore_delete=ignore_delete)
    _assert_columns(got, _expected(runs, r, w))
    return n_batches


# ------------------------------------------------------- deduplicate, chain

_CHAIN = ([(g, s) for g in "ABCEF" for s in ("S2", "S4")] +
          [("B", s) for s in ("S1", "S3", "S5", "S6")] +
          [("E", "S3"), ("E", "k32")])


class TestChain:
    @pytest.mark.parametrize("gen,shape", _CHAIN)
    def test_dedup(self, tmp_path, monkeypatch, gen, shape):
        mode = _select_path(monkeypatch, "chain")
        runs = _build(gen, shape, seed=1100 + len(shape) + ord(gen))
        assert _dedup_case(tmp_path, runs, mode) == 1  # one section

    @pytest.mark.parametrize("gen", ["B", "C"])
    @pytest.mark.parametrize("flags", ["keep_delete", "ignore_delete"])
    def test_delete_flags(self, tmp_path, monkeypatch, gen, flags):
        mode = _select_path(monkeypatch, "chain")
        runs = _build(gen, "S2", seed=1200, delete_p=0.3)
        _dedup_case(tmp_path, runs, mode,
                    drop_delete=flags != "keep_delete",
                    ignore_delete=flags == "ignore_delete")

    @pytest.mark.parametrize("seq_base", [2**40, 2**60])
    def test_sequence_offsets(self, tmp_path, monkeypatch, seq_base):
        # (seq << 1) | isAdd near its width
        mode = _select_path(monkeypatch, "chain")
        runs = _build("B", "S2", seed=1210, seq_base=seq_base)
        _dedup_case(tmp_path, runs, mode)


# ------------------------------------------------------- deduplicate, fused

@pytest.mark.parametrize("path", ["fused_split", "fused_inkernel"])
class TestFused:
    @pytest.mark.parametrize("gen,shape", [("A", "S2"), ("B", "S2"),
                                           ("C", "S2"), ("E", "S2"),
                                           ("B", "S4")])
    def test_dedup(self, tmp_path, monkeypatch, path, gen, shape):
        mode = _select_path(monkeypatch, path)
        runs = _build(gen, shape, seed=1300 + len(shape) + ord(gen))
        _dedup_case(tmp_path, runs, mode)

    @pytest.mark.parametrize("base_i", [0, 1, 2])
    @pytest.mark.parametrize("span", kd.THRESHOLD_SPANS)
    def test_repack_threshold(self, tmp_path, monkeypatch, path, span,
                              base_i):
        # one tile whose key range is exactly `span`: 2^32-3 is the last
        # one repacked to 32-bit offsets, 2^32-2 the first on the int64
        # fallback; bases put the tile at 0, INT64_MIN and INT64_MAX
        mode = _select_path(monkeypatch, path)
        base = kd.threshold_bases(span)[base_i]
        runs = kd.threshold(span, base, seed=1400 + base_i)
        _dedup_case(tmp_path, runs, mode)

    @pytest.mark.parametrize("top", [False, True])
    @pytest.mark.parametrize("span", kd.THRESHOLD_SPANS)
    def test_repack_threshold_far_predecessor(self, tmp_path, monkeypatch,
                                              path, span, top):
        # the same tile behind one whole tile of keys 2^40 below it: its
        # predecessor key has no 32-bit offset, and at span 2^32-1 the
        # tile's largest key would sit on the offset reserved for that
        mode = _select_path(monkeypatch, path)
        base = I64_MAX - span if top else 0
        runs = kd.threshold(span, base, seed=1410, pred_tile=True)
        _dedup_case(tmp_path, runs, mode)

    def test_sequence_offset_2_60(self, tmp_path, monkeypatch, path):
        # ps2_pack (seq << 2) near its width
        mode = _select_path(monkeypatch, path)
        runs = _build("B", "S2", seed=1310, seq_base=2**60)
        _dedup_case(tmp_path, runs, mode)


# ----------------------------------------------------------- other engines

class TestFirstRow:
    @pytest.mark.parametrize("path", ["chain", "fused_split"])
    @pytest.mark.parametrize("gen", ["B", "C"])
    def test_first_row(self, tmp_path, monkeypatch, gen, path):
        mode = _select_path(monkeypatch, path)
        runs = _build(gen, "S2", seed=1500, delete_p=0.0)
        for r in runs:
            r["kind"][:] = 0  # insert-only (B forces two DELETEs)
        metas = write_runs(runs, str(tmp_path), compression="NONE")
        r, w = merge_first_row_model(runs)
        got, _ = _run_plan(metas, tmg.KEY_COLS, _value_cols(runs), mode,
                           merge_engine="first-row")
        _assert_columns(got, _expected(runs, r, w))


class TestSequenceField:
    def test_full_span_int32_sequence_field(self, tmp_path, monkeypatch):
        # sequence fields run the fused walk by construction
        monkeypatch.delenv("PMH_FUSED", raising=False)
        monkeypatch.delenv("PMH_FSPLIT", raising=False)
        runs = _build("B", "S2", seed=1600)
        rng = np.random.default_rng(1600)
        for r in runs:
            # low cardinality: ties fall through to (seq, isAdd)
            r["values"][1] = rng.integers(-2, 2, len(r["key"])).astype(
                np.int32)
        metas = write_runs(runs, str(tmp_path), compression="NONE")
        r, w = merge_dedup_useq_model(runs, [1])
        with Session(0) as s:
            with MergeReadPlan(s, file_descs_from_metas(metas), tmg.KEY_COLS,
                               _value_cols(runs),
                               sequence_fields=["v_c0"]) as plan:
                got, _ = _read_batches(plan)
                assert plan.stats()["path_mode"] != 0
        _assert_columns(got, _expected(runs, r, w))


class TestPartialUpdate:
    @pytest.mark.parametrize("gen", ["B", "E"])
    def test_nullable_columns(self, tmp_path, monkeypatch, gen):
        _select_path(monkeypatch, "chain")
        runs = _build(gen, "S3", seed=1700, delete_p=0.0, n_value_cols=3,
                      null_p=0.4)
        for r in runs:
            r["kind"][:] = 0  # partial-update takes insert-only streams
        metas = write_runs(runs, str(tmp_path), compression="NONE")
        exp = partial_update_model(runs)
        got, _ = _run_plan(metas, tmg.KEY_COLS, _value_cols(runs),
                           merge_engine="partial-update")
        assert len(got["_KEY_k"]) == len(exp["key"])
        assert (got["_KEY_k"] == exp["key"]).all()
        assert (got["_SEQUENCE_NUMBER"] == exp["seq"]).all()
        assert (got["_VALUE_KIND"] == exp["kind"]).all()
        for c, col in enumerate(_value_cols(runs)):
            nm = col["name"]
            ev, evalid = exp["values"][c], exp["valid"][c]
            gvalid = got.get(nm + "#valid")
            if gvalid is None:
                gvalid = np.ones(len(got[nm]), dtype=bool)
            assert (gvalid == evalid).all(), nm
            assert got[nm].dtype == ev.dtype, nm
            assert (got[nm][evalid] == ev[evalid]).all(), nm


# -------------------------------------------------------------- narrow keys

def _narrow_runs(dtype, rows, seed):
    """4 runs of `rows` keys uniform over the whole domain of `dtype`, its
    minimum and maximum present in two runs each."""
    info = np.iinfo(dtype)
    rng = np.random.default_rng(seed)
    lists = []
    for i in range(4):
        if info.bits <= 16:
            dom = np.arange(info.min + 1, info.max, dtype=np.int64)
            k = rng.choice(dom, rows - 2, replace=False)
        else:
            k = np.unique(rng.integers(info.min + 1, info.max, rows + 64,
                                       dtype=np.int64))
            k = rng.permutation(k)[:rows - 2]
            if i:  # collide with the previous run
                k[:rows // 2] = lists[-1][1:1 + rows // 2]
                k = np.unique(k)
        if i < 2:
            k = np.concatenate([k, [info.min, info.max]])
        lists.append(np.sort(k))
    runs = kd.finish_runs(rng, lists, n_value_cols=1)
    for r in runs:
        r["key"] = r["key"].astype(dtype)
        r["values"][0] = r["key"].astype(np.int32)
    runs[0]["kind"][0] = 3
    runs[1]["kind"][-1] = 3
    return runs


class TestNarrowKeys:
    @pytest.mark.parametrize("file_format", ["parquet", "orc"])
    @pytest.mark.parametrize("dtype,rows", [(np.int32, 16_000),
                                            (np.int16, 20_000),
                                            (np.int8, 200)])
    def test_signed_extremes(self, tmp_path, monkeypatch, dtype, rows,
                             file_format):
        mode = _select_path(monkeypatch, "chain")
        runs = _narrow_runs(dtype, rows, seed=1800)
        info = np.iinfo(dtype)
        assert runs[0]["key"][0] == info.min and runs[1]["key"][-1] == info.max
        _dedup_case(tmp_path, runs, mode, file_format=file_format)
        _dedup_case(tmp_path / "keep", runs, mode, drop_delete=False,
                    file_format=file_format)


# ----------------------------------------------------------- composite keys

def _pack2(k1, k2):
    """TestCompositeKeys._comp over arrays: the order-preserving pack of the
    biased sub-keys, as the signed int64 the plan's minKey/maxKey carry."""
    u = ((k1.astype(np.int64) + 2**31).astype(np.uint64) << np.uint64(32)) \
        | (k2.astype(np.int64) + 2**31).astype(np.uint64)
    return (u ^ np.uint64(2**63)).view(np.int64)


class TestCompositeKeys:
    def test_two_int32_columns_full_range(self, tmp_path, monkeypatch):
        import pyarrow as pa
        import pyarrow.parquet as pq
        _select_path(monkeypatch, "chain")
        comp = tmg.TestCompositeKeys._comp
        k, rows = S2
        rng = np.random.default_rng(1900)
        # k1: 300 distinct values over the whole int32 range, both ends
        # included, so k2 decides the order inside equal k1; k2 uniform
        k1_vals = np.concatenate([rng.integers(I32_MIN, I32_MAX, 298),
                                  [I32_MIN, I32_MAX]])
        pool = np.unique(_pack2(
            rng.choice(k1_vals, 48_000),
            np.concatenate([rng.integers(I32_MIN, I32_MAX, 47_000),
                            rng.choice([I32_MIN, I32_MAX, -1, 0], 1000)])))
        pool = pool[(pool != I64_MIN) & (pool != I64_MAX)]
        lists = []
        for i in range(k):
            ks = np.sort(rng.choice(pool, rows - 2, replace=False))
            ends = [I64_MIN, I64_MAX] if i < 2 else \
                rng.choice(np.setdiff1d(pool, ks), 2, replace=False)
            lists.append(np.sort(np.concatenate([ks, ends])))
        runs = kd.finish_runs(rng, lists, n_value_cols=1)
        metas = []
        for i, r in enumerate(runs):
            u = r["key"].view(np.uint64) ^ np.uint64(2**63)
            r["k1"] = ((u >> np.uint64(32)).astype(np.int64)
                       - 2**31).astype(np.int32)
            r["k2"] = ((u & np.uint64(0xffffffff)).astype(np.int64)
                       - 2**31).astype(np.int32)
            assert (_pack2(r["k1"], r["k2"]) == r["key"]).all()
            r["values"] = [r["values"][1]]
            fields = [pa.field("_KEY_k1", pa.int32(), nullable=False),
                      pa.field("_KEY_k2", pa.int32(), nullable=False),
                      pa.field("_SEQUENCE_NUMBER", pa.int64(),
                               nullable=False),
                      pa.field("_VALUE_KIND", pa.int8(), nullable=False),
                      pa.field("v_k", pa.int32())]
            tbl = pa.Table.from_arrays(
                [pa.array(r["k1"]), pa.array(r["k2"]), pa.array(r["seq"]),
                 pa.array(r["kind"]), pa.array(r["values"][0])],
                schema=pa.schema(fields))
            path = os.path.join(str(tmp_path), f"run-{i}.parquet")
            pq.write_table(tbl, path, compression=None, use_dictionary=False,
                           data_page_version="1.0", store_schema=False)
            metas.append({"path": path, "rowCount": rows,
                          "minKey": comp(r["k1"][0], r["k2"][0]),
                          "maxKey": comp(r["k1"][-1], r["k2"][-1]),
                          "level": 0})
            assert metas[-1]["minKey"] == int(r["key"][0])
            assert metas[-1]["maxKey"] == int(r["key"][-1])
        # the packed comparand touches both ends of the 64-bit range
        assert metas[0]["minKey"] == I64_MIN and metas[0]["maxKey"] == I64_MAX
        assert (runs[0]["k1"][0], runs[0]["k2"][0]) == (I32_MIN, I32_MIN)
        assert (runs[0]["k1"][-1], runs[0]["k2"][-1]) == (I32_MAX, I32_MAX)
        r_, w_ = merge_dedup(runs)
        got, n_batches = _run_plan(
            metas, [{"name": "_KEY_k1", "type": "int32"},
                    {"name": "_KEY_k2", "type": "int32"}],
            [{"name": "v_k", "type": "int32"}])
        assert n_batches == 1
        _assert_columns(got, _expected(
            runs, r_, w_, key_fields={"_KEY_k1": "k1", "_KEY_k2": "k2"}))


# -------------------------------------------------- plan JSON, end to end

def _half_domain_runs(seed, top):
    """3 overlapping runs x 2000 keys in the top (or bottom) quarter of the
    int64 range; run 0 holds INT64_MAX (INT64_MIN)."""
    rng = np.random.default_rng(seed)
    lo, hi = (2**62, I64_MAX - 1) if top else (I64_MIN + 1, -2**62)
    pool = np.unique(rng.integers(lo, hi, 4500, dtype=np.int64))
    lists = [np.sort(rng.choice(pool, 2000, replace=False))
             for _ in range(3)]
    lists[0][-1 if top else 0] = I64_MAX if top else I64_MIN
    return kd.finish_runs(rng, lists)


class TestPlanJsonEndToEnd:
    @pytest.mark.parametrize("end", ["max", "min"])
    def test_file_bound_at_int64_end(self, tmp_path, monkeypatch, end):
        # minKey/maxKey travel through the plan JSON. A maxKey of INT64_MAX
        # parsed through a double came back as INT64_MIN: the section was
        # cut after the first file and overlapping files were served as
        # separate batches with their duplicate keys unmerged
        mode = _select_path(monkeypatch, "chain")
        runs = _half_domain_runs(2000, top=end == "max")
        mins = [int(r["key"][0]) for r in runs]
        maxs = [int(r["key"][-1]) for r in runs]
        assert max(mins) < min(maxs)  # the three ranges overlap
        assert (maxs[0] == I64_MAX) if end == "max" else (mins[0] == I64_MIN)
        assert _dedup_case(tmp_path, runs, mode) == 1

    def test_int64_filter_literal_above_2_53(self, tmp_path):
        n = 3000
        rng = np.random.default_rng(2001)
        keys = np.arange(n, dtype=np.int64) - n // 2
        vals = (2**53 + rng.integers(0, 3, n)).astype(np.int64)
        assert set(vals.tolist()) == {2**53, 2**53 + 1, 2**53 + 2}
        run = {"key": keys, "seq": np.arange(n, dtype=np.int64),
               "kind": np.zeros(n, np.int8),
               "values": [vals, np.arange(n, dtype=np.int32)]}
        metas = write_runs([run], str(tmp_path), compression="NONE")
        for op, keep in (("eq", vals == 2**53 + 1), ("lt", vals == 2**53),
                         ("ge", vals >= 2**53 + 1)):
            got, _ = _run_plan(
                metas, tmg.KEY_COLS, _value_cols([run]),
                filters=[{"field": "v_k", "op": op,
                          "literal": 2**53 + 1}])
            assert 0 < keep.sum() < n
            assert len(got["_KEY_k"]) == keep.sum(), op
            assert (got["_KEY_k"] == keys[keep]).all(), op
            assert (got["v_k"] == vals[keep]).all(), op


# --------------------------------------------------------- lookup changelog

class TestLookupChangelog:
    @pytest.mark.parametrize("extremes", ["hit", "miss"])
    def test_full_span_levels(self, tmp_path, extremes):
        # level-0 runs and both lookup levels hold full-span keys;
        # INT64_MIN / INT64_MAX are probe keys (runs 0..2 hold them) that
        # hit — INT64_MAX in level 3, INT64_MIN only in level 5, after
        # missing level 3 — or miss both levels, whose nearest keys are
        # then INT64_MIN + 1 and INT64_MAX - 1
        runs = kd.full_span(3, tlc.ROWS, seed=2100, seq_base=100_000,
                            n_value_cols=3)
        rng = np.random.default_rng(2100)
        probe = np.unique(np.concatenate([r["key"] for r in runs]))
        inner = probe[1:-1]
        assert probe[0] == I64_MIN and probe[-1] == I64_MAX

        def level_keys(n_hit, n_other, extra):
            other = rng.integers(I64_MIN + 2, I64_MAX - 2, n_other,
                                 dtype=np.int64)
            return np.unique(np.concatenate(
                [rng.choice(inner, n_hit, replace=False), other,
                 np.array(extra, np.int64)]))
        if extremes == "hit":
            k3 = level_keys(12_000, 8000, [I64_MAX])
            k5 = level_keys(9000, 6000, [I64_MIN])
        else:
            k3 = level_keys(12_000, 8000, [I64_MIN + 1, I64_MAX - 1])
            k5 = level_keys(9000, 6000, [I64_MIN + 1, I64_MAX - 1])
        lookup = [(3, tlc._make_level(rng, k3, 50_000), 2),
                  (5, tlc._make_level(rng, k5, 0), 1)]
        assert len(np.intersect1d(k3, k5)) > 1000
        cl, res, _ = tlc._run_case(tmp_path, runs, [0, 0, 0], lookup)
        n_runs = len(runs)
        assert (tlc._kind_counts(cl) > 100).all()
        assert sum(1 for s, _, _ in cl if s == n_runs) > 100
        assert sum(1 for s, _, _ in cl if s == n_runs + 1) > 100
        # what the model says about the two extreme keys, so a change of
        # the fixture cannot quietly stop covering them: INT64_MIN's group
        # winner is a DELETE (-D of the level-5 record on a hit, nothing on
        # a miss); INT64_MAX's is an INSERT (-U/+U on a hit, +I on a miss)
        src = list(runs) + [lv for _, lv, _ in lookup]
        ext = {(int(src[s]["key"][r]), kind) for s, r, kind in cl
               if int(src[s]["key"][r]) in (I64_MIN, I64_MAX)}
        if extremes == "hit":
            assert ext == {(I64_MIN, 3), (I64_MAX, 1), (I64_MAX, 2)}
        else:
            assert ext == {(I64_MAX, 0)}
