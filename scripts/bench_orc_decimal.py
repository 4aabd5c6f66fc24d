"""Decode-stage comparison for ORC DECIMAL: an 8 x 1M-row ORC
deduplicate plan whose one value column is decimal(18,2) (k_orc_varint)
beside the same plan with the same integers stored as ORC LONG (k_rlev2),
and with an all-zero INT value column, whose decode is a handful of constant
runs (what the key / sequence / kind streams cost alone). HIP-event decode_ms
per step, 3 warm-up + 10 timed steps, medians; the three plans alternate
twice in one process on one device.

    python -m scripts.bench_orc_decimal [--runs 8] [--rows 1000000]
prints one JSON line."""

import argparse
import json
import os
import tempfile

import numpy as np
import pyarrow as pa
from pyarrow import orc as pa_orc

from paimon_amd import MergeReadPlan, Session, file_descs_from_metas
from paimon_amd.datagen import gen_runs_dedup

KEY_COLS = [{"name": "_KEY_k", "type": "int64"}]


def _decimal128(unscaled, precision, scale):
    """decimal128 array straight from int64 unscaled values (two's
    complement, little-endian 16-byte words) — no Python Decimal objects."""
    n = len(unscaled)
    words = np.empty((n, 2), dtype=np.int64)
    words[:, 0] = unscaled
    words[:, 1] = unscaled >> 63
    return pa.Array.from_buffers(pa.decimal128(precision, scale), n,
                                 [None, pa.py_buffer(words.tobytes())])


def _write(runs, out_dir, kind):
    os.makedirs(out_dir, exist_ok=True)
    metas = []
    for i, r in enumerate(runs):
        if kind == "decimal":
            v = _decimal128(r["v"], 18, 2)
        elif kind == "long":
            v = pa.array(r["v"])
        else:
            v = pa.array(np.zeros(len(r["key"]), dtype=np.int32))
        tbl = pa.table({"_KEY_k": pa.array(r["key"]),
                        "_SEQUENCE_NUMBER": pa.array(r["seq"]),
                        "_VALUE_KIND": pa.array(r["kind"]),
                        "v": v})
        path = os.path.join(out_dir, f"run-{i}.orc")
        pa_orc.write_table(tbl, path, compression="uncompressed")
        metas.append({"path": path, "rowCount": len(r["key"]),
                      "minKey": int(r["key"][0]),
                      "maxKey": int(r["key"][-1]), "level": 0})
    return metas


def _steps(plan, warmup, steps):
    """Per-step (decode_ms, total_device_ms) medians."""
    dec, tot = [], []
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

    runs = gen_runs_dedup(args.runs, args.rows, n_value_cols=0, seed=77,
                          delete_frac=0.05)
    rng = np.random.default_rng(78)
    for r in runs:
        r["v"] = rng.integers(-10**12, 10**12, len(r["key"]), dtype=np.int64)
    with tempfile.TemporaryDirectory() as d:
        m_dec = _write(runs, os.path.join(d, "dec"), "decimal")
        m_long = _write(runs, os.path.join(d, "long"), "long")
        m_zero = _write(runs, os.path.join(d, "zero"), "zero")
        enc = {k: sum(os.path.getsize(m["path"]) for m in ms)
               for k, ms in (("decimal", m_dec), ("long", m_long))}
        with Session(0) as s:
            plans = {
                "decimal": MergeReadPlan(
                    s, file_descs_from_metas(m_dec), KEY_COLS,
                    [{"name": "v", "type": "decimal(18,2)"}],
                    output="device"),
                "long": MergeReadPlan(
                    s, file_descs_from_metas(m_long), KEY_COLS,
                    [{"name": "v", "type": "int64"}], output="device"),
                "zero_int": MergeReadPlan(
                    s, file_descs_from_metas(m_zero), KEY_COLS,
                    [{"name": "v", "type": "int32"}], output="device"),
            }
            res = {k: [] for k in plans}
            for _ in range(2):
                for k, p in plans.items():
                    d_ms, t_ms, rows = _steps(p, args.warmup, args.steps)
                    res[k].append({"decode_ms": round(d_ms, 4),
                                   "total_device_ms": round(t_ms, 4),
                                   "rows_out": rows})
            for p in plans.values():
                p.close()
    print(json.dumps({"bench": "orc_decimal_decode", "runs": args.runs,
                      "rows_per_run": args.rows, "file_bytes": enc,
                      "passes": res}))


if __name__ == "__main__":
    main()
