"""Decode-stage comparison for BOOLEAN and ORC TIMESTAMP columns (DESIGN.md
§7): an 8 x 1M-row uncompressed deduplicate plan with ONE value column, in
five variants:

    orc_boolean      ORC BOOLEAN (byte-RLE units -> k_bits_expand)
    orc_timestamp    ORC TIMESTAMP as timestamp(6) (k_rlev2 twice +
                     k_orc_timestamp)
    orc_long         the same microsecond integers as ORC LONG (k_rlev2)
    parquet_boolean  Parquet BOOLEAN, PLAIN (k_bits_expand)
    parquet_int32    Parquet INT32, PLAIN (staged as the column itself: no
                     decode kernel)

HIP-event decode_ms per step, 3 warm-up + 10 timed steps, medians; the plans
alternate twice in one process on one device. What k_bits_expand and
k_orc_timestamp cost is the difference to the neighbouring variant.

pyarrow's ORC writer needs an IANA zoneinfo directory for TIMESTAMP columns:
TZDIR is pointed at the `tzdata` package's when that is installed, and the
orc_timestamp variant is left out (and said so) when the write fails.

    python -m scripts.bench_bool_temporal [--runs 8] [--rows 1000000]
prints one JSON line."""

import argparse
import importlib.util
import json
import os
import tempfile

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

from paimon_amd import MergeReadPlan, Session, file_descs_from_metas
from paimon_amd.datagen import gen_runs_dedup

KEY_COLS = [{"name": "_KEY_k", "type": "int64"}]

VARIANTS = {  # name -> (file format, plan type)
    "orc_boolean": ("orc", "boolean"),
    "orc_timestamp": ("orc", "timestamp(6)"),
    "orc_long": ("orc", "int64"),
    "parquet_boolean": ("parquet", "boolean"),
    "parquet_int32": ("parquet", "int32"),
}


def _value(r, name):
    if name.endswith("boolean"):
        return pa.array(r["flag"])
    if name == "orc_timestamp":
        return pa.array(r["ts"], pa.timestamp("us"))
    if name == "orc_long":
        return pa.array(r["ts"])
    return pa.array(r["i32"])


def _write(runs, out_dir, name):
    from pyarrow import orc as pa_orc
    os.makedirs(out_dir, exist_ok=True)
    fmt = VARIANTS[name][0]
    metas = []
    for i, r in enumerate(runs):
        tbl = pa.table({"_KEY_k": pa.array(r["key"]),
                        "_SEQUENCE_NUMBER": pa.array(r["seq"]),
                        "_VALUE_KIND": pa.array(r["kind"]),
                        "v": _value(r, name)})
        path = os.path.join(out_dir, f"run-{i}.{fmt}")
        if fmt == "orc":
            pa_orc.write_table(tbl, path, compression="uncompressed")
        else:
            pq.write_table(tbl, path, compression=None, use_dictionary=False,
                           data_page_version="1.0", write_statistics=False,
                           store_schema=False)
        metas.append({"path": path, "rowCount": len(r["key"]),
                      "minKey": int(r["key"][0]),
                      "maxKey": int(r["key"][-1]), "level": 0})
    return metas


def _steps(plan, warmup, steps):
    """Per-step (decode_ms, total_device_ms) medians."""
    dec, tot = [], []
    rows = 0
    for i in range(warmup + steps):
        plan.reset()
        s0 = plan.stats()
        rows = 0
        while True:
            b = plan.read_next()
            if b is None:
                break
            rows += b.n_rows
        s1 = plan.stats()
        if i >= warmup:
            dec.append(s1["decode_ms"] - s0["decode_ms"])
            tot.append(s1["total_device_ms"] - s0["total_device_ms"])
    return float(np.median(dec)), float(np.median(tot)), rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()

    spec = importlib.util.find_spec("tzdata")
    if spec is not None and "TZDIR" not in os.environ:
        os.environ["TZDIR"] = os.path.join(os.path.dirname(spec.origin),
                                           "zoneinfo")
    runs = gen_runs_dedup(args.runs, args.rows, n_value_cols=0, seed=87,
                          delete_frac=0.05)
    rng = np.random.default_rng(88)
    for r in runs:
        n = len(r["key"])
        r["flag"] = rng.random(n) < 0.5
        r["ts"] = (rng.integers(0, 4_000_000_000, n, dtype=np.int64) * 10**6
                   + rng.integers(0, 10**6, n, dtype=np.int64))
        r["i32"] = r["flag"].astype(np.int32)
    skipped = {}
    with tempfile.TemporaryDirectory() as d:
        metas = {}
        for name in VARIANTS:
            try:
                metas[name] = _write(runs, os.path.join(d, name), name)
            except Exception as e:  # no zoneinfo for the ORC writer
                if name != "orc_timestamp":
                    raise
                skipped[name] = str(e)
        enc = {k: sum(os.path.getsize(m["path"]) for m in ms)
               for k, ms in metas.items()}
        with Session(0) as s:
            plans = {name: MergeReadPlan(
                s, file_descs_from_metas(ms), KEY_COLS,
                [{"name": "v", "type": VARIANTS[name][1]}], output="device")
                for name, ms in metas.items()}
            res = {k: [] for k in plans}
            for _ in range(2):
                for k, p in plans.items():
                    d_ms, t_ms, rows = _steps(p, args.warmup, args.steps)
                    res[k].append({"decode_ms": round(d_ms, 4),
                                   "total_device_ms": round(t_ms, 4),
                                   "rows_out": rows})
            for p in plans.values():
                p.close()
    print(json.dumps({"bench": "bool_temporal_decode", "runs": args.runs,
                      "rows_per_run": args.rows, "file_bytes": enc,
                      "skipped": skipped, "passes": res}))


if __name__ == "__main__":
    main()
