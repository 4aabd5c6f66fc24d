"""Lookup changelog producer on the GPU (changelog_producer = "lookup":
k_lookup_probe + the lookup walk of k_merge_tiles + k_cl_finalize +
k_cl_emit) against the sequential model (tests/lookup_model.py), which is
itself pinned to the reference's LookupChangelogMergeFunctionWrapperTest
vectors (tests/test_lookup_changelog_cpu.py).

Every case compares the WHOLE main stream and the WHOLE changelog stream
bit-exactly: key, sequence number, kind and every value column (plus
validity where columns are nullable). Shapes stay around 3 runs x 12 000
rows: ~10 tiles of 3584 rows, so key groups cross tile cuts."""
import os

import numpy as np
import pytest

from paimon_amd import Session, MergeReadPlan, file_descs_from_metas
from paimon_amd.datagen import gen_runs_dedup, write_runs
from tests.lookup_model import lookup_changelog_model

pytestmark = pytest.mark.gpu

ROWS = 12_000


def _key_cols(key_type="int64"):
    return [{"name": "_KEY_k", "type": key_type}]


def _value_cols(n):
    return ([{"name": "v_k", "type": "int64"}] +
            [{"name": f"v_c{i}", "type": "int32"} for i in range(n)])


def _read_all(plan):
    main, cl = [], []
    while True:
        b = plan.read_next()
        if b is None:
            break
        main.append({k: v.copy() for k, v in b.items()})
        cl.append({k: v.copy() for k, v in plan.read_changelog().items()})
    keys = set().union(*[set(p) for p in main + cl])

    def cat(parts):
        out = {}
        for k in keys:
            if k.endswith("#valid"):
                # a batch without rows carries no validity array
                out[k] = np.concatenate(
                    [p[k] if k in p else np.ones(len(p["_KEY_k"]), bool)
                     for p in parts])
            elif all(k in p for p in parts):
                out[k] = np.concatenate([p[k] for p in parts])
        return out
    return cat(main), cat(cl), len(main)


def _make_level(rng, keys, seq_lo, delete_frac=0.0, n_value_cols=3,
                value_card=None):
    """One lookup level: ascending unique keys, sequence numbers from
    seq_lo upwards in random order."""
    n = len(keys)
    card = value_card or (1 << 30)
    return {
        "key": np.asarray(keys, np.int64),
        "seq": (seq_lo + rng.permutation(n)).astype(np.int64),
        "kind": np.where(rng.random(n) < delete_frac, 3, 0).astype(np.int8),
        "values": [rng.integers(0, card, n).astype(np.int64)] +
                  [rng.integers(0, card, n).astype(np.int32)
                   for _ in range(n_value_cols)],
    }


def _slice(run, lo, hi):
    out = {"key": run["key"][lo:hi], "seq": run["seq"][lo:hi],
           "kind": run["kind"][lo:hi],
           "values": [v[lo:hi] for v in run["values"]]}
    if "valid" in run:
        out["valid"] = [m[lo:hi] for m in run["valid"]]
    return out


def _write_dictionary_runs(parts, out_dir):
    """Like write_runs, with dictionary pages + RLE_DICTIONARY ids for the
    int32 value columns (decoded on the device at staging time)."""
    import pyarrow.parquet as pq
    from paimon_amd.datagen import run_to_arrow
    os.makedirs(out_dir, exist_ok=True)
    metas = []
    for i, part in enumerate(parts):
        path = os.path.join(out_dir, f"run-{i}.parquet")
        n_vals = len(part["values"])
        pq.write_table(run_to_arrow(part), path, compression=None,
                       use_dictionary=[f"v_c{c}" for c in range(n_vals - 1)],
                       data_page_version="1.0", store_schema=False)
        metas.append({"path": path, "rowCount": len(part["key"]),
                      "minKey": int(part["key"][0]),
                      "maxKey": int(part["key"][-1])})
    return metas


def _write_lookup(tmp_path, lookup, compression="NONE"):
    """lookup: [(level, level_run, n_files)] -> lookup_files descriptors;
    a level is cut into n_files key-disjoint files, listed in REVERSE key
    order so the plan has to sort them. compression "dictionary" writes
    uncompressed dictionary-encoded value columns."""
    descs = []
    for level, run, n_files in lookup:
        n = len(run["key"])
        cuts = [n * i // n_files for i in range(n_files + 1)]
        parts = [_slice(run, cuts[i], cuts[i + 1]) for i in range(n_files)]
        out_dir = os.path.join(str(tmp_path), f"L{level}")
        if compression == "dictionary":
            metas = _write_dictionary_runs(parts, out_dir)
        else:
            metas = write_runs(parts, out_dir, compression=compression)
        for m in metas:
            m["level"] = level
        descs += file_descs_from_metas(metas)[::-1]
    return descs


def _gather(sources, stream, field, dtype, col=None):
    src = np.array([s[0] for s in stream], np.int64)
    row = np.array([s[1] for s in stream], np.int64)
    out = np.zeros(len(stream), dtype)
    for s in np.unique(src):
        sel = src == s
        arr = sources[s][field] if col is None else sources[s][field][col]
        out[sel] = arr[row[sel]]
    return out


def _assert_stream(got, sources, stream, n_vals, what, kinds=None,
                   key_dtype=np.int64):
    n = len(stream)
    assert len(got["_KEY_k"]) == n, (what, len(got["_KEY_k"]), n)
    exp = {"_KEY_k": _gather(sources, stream, "key", key_dtype),
           "_SEQUENCE_NUMBER": _gather(sources, stream, "seq", np.int64),
           "_VALUE_KIND": (np.asarray(kinds, np.int8) if kinds is not None
                           else _gather(sources, stream, "kind", np.int8))}
    for name, e in exp.items():
        assert got[name].dtype == e.dtype, (what, name)
        assert (got[name] == e).all(), \
            f"{what} {name}: first diffs {np.flatnonzero(got[name] != e)[:10]}"
    for c in range(n_vals):
        name = "v_k" if c == 0 else f"v_c{c - 1}"
        e = _gather(sources, stream, "values",
                    sources[0]["values"][c].dtype, col=c)
        valid = np.ones(n, bool)
        if any("valid" in s for s in sources):
            valid = _gather([{"valid": s.get(
                "valid", [np.ones(len(s["key"]), bool)] * n_vals)}
                for s in sources], stream, "valid", bool, col=c)
        gv = got.get(name + "#valid")
        if gv is None:
            assert valid.all(), (what, name, "validity array missing")
        else:
            assert (gv == valid).all(), \
                f"{what} {name} validity: {np.flatnonzero(gv != valid)[:10]}"
        g = got[name]
        assert (g[valid] == e[valid]).all(), \
            f"{what} {name}: first diffs " \
            f"{np.flatnonzero((g != e) & valid)[:10]}"


def _run_case(tmp_path, runs, levels, lookup, row_dedup=False,
              drop_delete=True, key_type="int64", compression="NONE",
              min_sections=1):
    """Writes the files, runs the plan, compares both streams with the
    model. Returns (model changelog, model result, stats)."""
    metas = write_runs(runs, os.path.join(str(tmp_path), "merge"),
                       compression="NONE")
    for m, lvl in zip(metas, levels):
        m["level"] = lvl
    lookup_descs = _write_lookup(tmp_path, lookup, compression)
    lookup_runs = [run for _, run, _ in lookup]
    n_vals = len(runs[0]["values"])

    def null_masks(rs):
        if not any("valid" in r for r in rs):
            return None
        return [[~m for m in r["valid"]] if "valid" in r else None
                for r in rs]
    exp_cl, exp_res = lookup_changelog_model(
        runs, levels, lookup_runs, row_dedup=row_dedup,
        drop_delete=drop_delete, masks=null_masks(runs),
        lookup_masks=null_masks(lookup_runs))
    with Session(0) as s:
        with MergeReadPlan(s, file_descs_from_metas(metas),
                           _key_cols(key_type), _value_cols(n_vals - 1),
                           drop_delete=drop_delete,
                           changelog_producer="lookup",
                           changelog_row_dedup=row_dedup,
                           lookup_files=lookup_descs) as plan:
            main, cl, n_sections = _read_all(plan)
            stats = plan.stats()
    assert n_sections >= min_sections
    sources = list(runs) + lookup_runs
    key_dtype = np.dtype(key_type)
    _assert_stream(main, sources, exp_res, n_vals, "main",
                   key_dtype=key_dtype)
    _assert_stream(cl, sources, [(s_, r_) for s_, r_, _ in exp_cl], n_vals,
                   "changelog", kinds=[k for _, _, k in exp_cl],
                   key_dtype=key_dtype)
    return exp_cl, exp_res, stats


def _level0_runs(seed, n_runs=3, rows=ROWS, delete_frac=0.2, n_value_cols=3,
                 seq_base=100_000, value_card=None):
    runs = gen_runs_dedup(n_runs, rows, n_value_cols=n_value_cols, seed=seed,
                          delete_frac=delete_frac)
    for r in runs:
        r["seq"] = r["seq"] + seq_base  # newer than the lookup levels
        if value_card:
            r["values"] = [(v % value_card).astype(v.dtype)
                           for v in r["values"]]
    return runs


def _two_lookup_levels(rng, keyspace, n3=20_000, n5=15_000, delete_frac=0.0,
                       n_value_cols=3, value_card=None):
    """Levels 3 (two files) and 5 (one file), random keys: about
    n3 * n5 / keyspace keys sit in both."""
    k3 = np.sort(rng.choice(keyspace, n3, replace=False))
    k5 = np.sort(rng.choice(keyspace, n5, replace=False))
    l3 = _make_level(rng, k3, 50_000, delete_frac, n_value_cols, value_card)
    l5 = _make_level(rng, k5, 0, delete_frac, n_value_cols, value_card)
    return [(3, l3, 2), (5, l5, 1)]


def _keyspace(runs):
    return int(max(r["key"].max() for r in runs)) + 1


def _kind_counts(cl):
    return np.bincount([k for _, _, k in cl], minlength=4)


class TestLookupChangelog:
    @pytest.mark.parametrize("drop_delete", [True, False])
    def test_basic(self, tmp_path, drop_delete):
        runs = _level0_runs(seed=601)
        rng = np.random.default_rng(601)
        lookup = _two_lookup_levels(rng, _keyspace(runs))
        both = np.intersect1d(lookup[0][1]["key"], lookup[1][1]["key"])
        assert len(both) > 1000  # keys held by both lookup levels
        cl, res, _ = _run_case(tmp_path, runs, [0, 0, 0], lookup,
                               drop_delete=drop_delete)
        n_runs = len(runs)
        assert (_kind_counts(cl) > 100).all()  # +I, -U, +U, -D all occur
        assert sum(1 for s, _, _ in cl if s == n_runs) > 100      # level 3
        assert sum(1 for s, _, _ in cl if s == n_runs + 1) > 100  # level 5

    def test_upper_level_members(self, tmp_path):
        # compaction members at levels 1 and 2 next to level 0: only the
        # level-1 record joins the merge when both hold a key, even where
        # the dropped level-2 record carries the highest sequence number
        runs = _level0_runs(seed=602, n_runs=4, rows=9_000)
        levels = [0, 0, 1, 2]
        rng = np.random.default_rng(602)
        lookup = _two_lookup_levels(rng, _keyspace(runs))
        k1, k2 = runs[2]["key"], runs[3]["key"]
        both = np.intersect1d(k1, k2)
        assert len(both) > 500
        # keys of both upper members where the level-2 record is newest
        seq_of = [dict(zip(r["key"].tolist(), r["seq"].tolist()))
                  for r in runs]
        top_is_l2 = [k for k in both.tolist()
                     if seq_of[3][k] > max(seq_of[i].get(k, -1)
                                           for i in range(3))]
        assert len(top_is_l2) > 50
        cl, res, _ = _run_case(tmp_path, runs, levels, lookup,
                               drop_delete=False)
        res_keys = {int(runs[s]["key"][r]): s for s, r in res if s < 4}
        # the exclusion rule shows: none of those results is the level-2 row
        assert all(res_keys[k] != 3 for k in top_is_l2)

    @pytest.mark.parametrize("row_dedup", [False, True])
    def test_lookup_record_wins(self, tmp_path, row_dedup):
        # lookup hits whose sequence number is >= the group's maximum
        # (exact ties included): the main row is a copy of the lookup
        # record, and the UPDATE_BEFORE/UPDATE_AFTER pair is the same record
        # twice — row-deduplicate drops it, otherwise both rows appear
        runs = _level0_runs(seed=603)
        rng = np.random.default_rng(603)
        lookup = _two_lookup_levels(rng, _keyspace(runs))
        gmax = {}
        for r in runs:
            for k, s in zip(r["key"].tolist(), r["seq"].tolist()):
                gmax[k] = max(gmax.get(k, -1), s)
        n_tie = n_above = 0
        for _, lv, _ in lookup:
            for i, k in enumerate(lv["key"].tolist()):
                if k in gmax and k % 3 == 0:
                    lv["seq"][i] = gmax[k]            # exact tie
                    n_tie += 1
                elif k in gmax and k % 3 == 1:
                    lv["seq"][i] = gmax[k] + 1 + k % 5  # strictly newer
                    n_above += 1
        assert n_tie > 500 and n_above > 500
        cl, res, _ = _run_case(tmp_path, runs, [0, 0, 0], lookup,
                               row_dedup=row_dedup)
        n_runs = len(runs)
        assert sum(1 for s, _ in res if s >= n_runs) > 500
        same_pairs = sum(1 for a, b in zip(cl, cl[1:])
                         if a[2] == 1 and b[2] == 2 and a[:2] == b[:2])
        if row_dedup:
            assert same_pairs == 0
        else:
            assert same_pairs > 500

    def test_kinds(self, tmp_path):
        # lookup hits of kind DELETE, level-0 groups that end in DELETE
        runs = _level0_runs(seed=604, delete_frac=0.5)
        rng = np.random.default_rng(604)
        lookup = _two_lookup_levels(rng, _keyspace(runs), delete_frac=0.5)
        cl, _, _ = _run_case(tmp_path, runs, [0, 0, 0], lookup)
        assert (_kind_counts(cl) > 100).all()

    @pytest.mark.parametrize("row_dedup", [True, False])
    def test_row_dedup_low_cardinality(self, tmp_path, row_dedup):
        runs = _level0_runs(seed=605, n_value_cols=2, delete_frac=0.1,
                            value_card=2)
        rng = np.random.default_rng(605)
        lookup = _two_lookup_levels(rng, _keyspace(runs), n_value_cols=2,
                                    value_card=2)
        plain, _ = lookup_changelog_model(
            runs, [0, 0, 0], [lv for _, lv, _ in lookup], row_dedup=False)
        cl, _, _ = _run_case(tmp_path, runs, [0, 0, 0], lookup,
                             row_dedup=row_dedup)
        if row_dedup:  # the equaliser really removes pairs at this shape
            assert len(plain) - len(cl) > 500

    def test_row_dedup_nullable(self, tmp_path):
        # null == null, null != value (k_cl_finalize compares validity
        # bytes before values), across merge runs and lookup levels
        runs = _level0_runs(seed=606, n_value_cols=2, delete_frac=0.05,
                            value_card=3)
        rng = np.random.default_rng(606)
        lookup = _two_lookup_levels(rng, _keyspace(runs), n_value_cols=2,
                                    value_card=3)
        for r in runs + [lv for _, lv, _ in lookup]:
            n = len(r["key"])
            r["valid"] = [np.ones(n, bool)] + \
                [rng.random(n) >= 0.4 for _ in range(2)]
        plain, _ = lookup_changelog_model(
            runs, [0, 0, 0], [lv for _, lv, _ in lookup], row_dedup=False)
        cl, _, _ = _run_case(tmp_path, runs, [0, 0, 0], lookup,
                             row_dedup=True)
        assert len(plain) - len(cl) > 200

    def test_no_lookup_files(self, tmp_path):
        # first compaction under an empty upper tree
        runs = _level0_runs(seed=607)
        cl, _, stats = _run_case(tmp_path, runs, [0, 0, 0], [])
        assert set(k for _, _, k in cl) == {0}  # INSERT only

    def test_two_sections(self, tmp_path):
        # two disjoint key ranges -> two sections sharing the lookup levels
        a = _level0_runs(seed=608, rows=6_000)
        b = _level0_runs(seed=609, rows=6_000, seq_base=200_000)
        off = _keyspace(a) + 1_000
        for r in b:
            r["key"] = r["key"] + off
            r["values"][0] = r["values"][0] + off
        rng = np.random.default_rng(608)
        lookup = _two_lookup_levels(rng, off + _keyspace(a), n3=30_000,
                                    n5=24_000)
        cl, _, _ = _run_case(tmp_path, a + b, [0] * 6, lookup,
                             min_sections=2)
        hit_keys = np.array([lookup[s - 6][1]["key"][r]
                             for s, r, _ in cl if s >= 6])
        assert (hit_keys < off).sum() > 100 and (hit_keys >= off).sum() > 100

    def test_int32_key(self, tmp_path):
        runs = _level0_runs(seed=610)
        rng = np.random.default_rng(610)
        lookup = _two_lookup_levels(rng, _keyspace(runs))
        for r in runs + [lv for _, lv, _ in lookup]:
            r["key"] = (r["key"] - 20_000).astype(np.int32)  # signed keys
        _run_case(tmp_path, runs, [0, 0, 0], lookup, key_type="int32")

    def test_zstd_lookup_files(self, tmp_path):
        runs = _level0_runs(seed=611)
        rng = np.random.default_rng(611)
        lookup = _two_lookup_levels(rng, _keyspace(runs))
        _run_case(tmp_path, runs, [0, 0, 0], lookup, compression="zstd")

    def test_dictionary_encoded_lookup_files(self, tmp_path):
        # lookup levels whose value columns need the read-time dictionary
        # decode: it runs once, when the plan stages them
        runs = _level0_runs(seed=613, value_card=50)
        rng = np.random.default_rng(613)
        lookup = _two_lookup_levels(rng, _keyspace(runs), value_card=50)
        _run_case(tmp_path, runs, [0, 0, 0], lookup,
                  compression="dictionary")

    def test_stats_and_reset(self, tmp_path):
        # lookup_ms is reported, and the lookup levels stay resident across
        # pmh_plan_reset: a second pass gives the same streams
        runs = _level0_runs(seed=612, rows=6_000)
        rng = np.random.default_rng(612)
        lookup = _two_lookup_levels(rng, _keyspace(runs))
        metas = write_runs(runs, os.path.join(str(tmp_path), "merge"),
                           compression="NONE")
        for m in metas:
            m["level"] = 0
        descs = _write_lookup(tmp_path, lookup)
        with Session(0) as s:
            with MergeReadPlan(s, file_descs_from_metas(metas), _key_cols(),
                               _value_cols(3), changelog_producer="lookup",
                               lookup_files=descs) as plan:
                main1, cl1, _ = _read_all(plan)
                st = plan.stats()
                assert st["lookup_ms"] > 0
                plan.reset()
                main2, cl2, _ = _read_all(plan)
                assert plan.stats()["lookup_ms"] > st["lookup_ms"]
        for a, b in ((main1, main2), (cl1, cl2)):
            assert a.keys() == b.keys()
            for k in a:
                assert (a[k] == b[k]).all(), k


class TestLookupRejections:
    """One pytest.raises per plan-create error."""

    @pytest.fixture()
    def files(self, tmp_path):
        runs = _level0_runs(seed=620, n_runs=2, rows=500)
        metas = write_runs(runs, os.path.join(str(tmp_path), "merge"),
                           compression="NONE")
        for m in metas:
            m["level"] = 0
        rng = np.random.default_rng(620)
        lv = _make_level(rng, np.arange(0, 2000, 2), 0)
        return (file_descs_from_metas(metas),
                _write_lookup(tmp_path, [(3, lv, 2)]))

    def _create(self, files, lookup_files, key_cols=None, **kw):
        with Session(0) as s:
            MergeReadPlan(s, files, key_cols or _key_cols(), _value_cols(3),
                          changelog_producer="lookup",
                          lookup_files=lookup_files, **kw).close()

    def test_accepts_the_baseline(self, files):
        self._create(*files)  # the fixture itself is a legal plan

    def test_too_many_slots(self, files):
        merge, lookup = files
        many = [dict(lookup[0], level=3 + i, minKey=0, maxKey=1)
                for i in range(31)]
        with pytest.raises(RuntimeError, match="lookup levels exceed"):
            self._create(merge, many)

    def test_level_too_large(self, files):
        merge, lookup = files
        big = [dict(lookup[0], rowCount=1 << 27)]
        with pytest.raises(RuntimeError, match="rows-per-run limit"):
            self._create(merge, big)

    def test_level_not_above_merge_levels(self, files):
        merge, lookup = files
        merge = [dict(merge[0], level=0), dict(merge[1], level=3)]
        with pytest.raises(RuntimeError, match="must be above every level"):
            self._create(merge, lookup)

    def test_overlapping_files_in_level(self, files):
        merge, lookup = files
        a, b = sorted(lookup, key=lambda d: d["minKey"])
        clash = [a, dict(b, minKey=a["maxKey"])]
        with pytest.raises(RuntimeError, match="overlap"):
            self._create(merge, clash)

    @pytest.mark.parametrize("engine", ["first-row", "partial-update",
                                        "aggregation"])
    def test_other_engines(self, files, engine):
        with pytest.raises(RuntimeError, match="deduplicate engine"):
            self._create(*files, merge_engine=engine)

    def test_ignore_delete(self, files):
        with pytest.raises(RuntimeError, match="ignore_delete"):
            self._create(*files, ignore_delete=True)

    def test_sequence_field(self, files):
        with pytest.raises(RuntimeError, match="sequence.field"):
            self._create(*files, sequence_fields=["v_c0"])

    def test_fused_path(self, files, monkeypatch):
        monkeypatch.setenv("PMH_FUSED", "1")
        with pytest.raises(RuntimeError, match="PMH_FUSED"):
            self._create(*files)

    def test_composite_key(self, files):
        with pytest.raises(RuntimeError, match="single integer key"):
            self._create(*files, key_cols=[
                {"name": "_KEY_k", "type": "int32"},
                {"name": "_KEY_j", "type": "int32"}])

    def test_deletion_vector_on_lookup_file(self, files, tmp_path):
        merge, lookup = files
        dv = [dict(lookup[0], deletionVector={
            "file": str(tmp_path / "index.dv"), "offset": 0, "length": 8})]
        with pytest.raises(RuntimeError, match="deletionVector"):
            self._create(merge, dv + lookup[1:])
