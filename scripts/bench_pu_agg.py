"""Emit-stage comparison for partial-update aggregate functions inside
sequence groups: an 8 x 1M-row plan over int64 v_k + 6
nullable int32 columns in two sequence groups, read without aggregate
functions (plan A: k_emit_pu_sg) and with a mixed set of them (plan B:
k_emit_pu_sga: sum, last_value, first_value under ignore-retract, max under
ignore-retract). HIP-event emit_ms and total device ms per step, 3 warm-up +
10 timed steps with a plan reset between steps, medians; the two plans
alternate twice in one process on one device.

    python -m scripts.bench_pu_agg [--runs 8] [--rows 1000000]
prints one JSON line."""

import argparse
import json
import tempfile

import numpy as np

from paimon_amd import MergeReadPlan, Session, file_descs_from_metas
from paimon_amd.datagen import write_runs

KEY_COLS = [{"name": "_KEY_k", "type": "int64"}]
VALUE_COLS = ([{"name": "v_k", "type": "int64"}] +
              [{"name": f"v_c{i}", "type": "int32"} for i in range(6)])
# group A: v_c0 orders v_c1, v_c2; group B: v_c3 orders v_c4, v_c5
GROUPS = [{"sequence_fields": ["v_c0"], "group_fields": ["v_c1", "v_c2"]},
          {"sequence_fields": ["v_c3"], "group_fields": ["v_c4", "v_c5"]}]
AGGS = {"v_c1": "sum", "v_c2": "last_value", "v_c4": "first_value",
        "v_c5": "max"}
IGNORE = ["v_c4", "v_c5"]


def _gen(n_runs, rows, seed):
    """All four row kinds, 35% nulls, values in 0..50, key space 0.6 x the
    total (key groups of 1..n_runs members)."""
    rng = np.random.default_rng(seed)
    total = n_runs * rows
    seqs = rng.permutation(total).astype(np.int64)
    runs = []
    for r in range(n_runs):
        key = np.sort(rng.choice(int(total * 0.6), rows, replace=False)
                      ).astype(np.int64)
        kind = rng.choice([0, 2, 1, 3], rows,
                          p=[.45, .2, .15, .2]).astype(np.int8)
        vals, msks = [key.copy()], [np.ones(rows, bool)]
        for _ in range(6):
            vals.append(rng.integers(0, 50, rows).astype(np.int32))
            msks.append(rng.random(rows) >= 0.35)
        runs.append({"key": key, "seq": seqs[r * rows:(r + 1) * rows],
                     "kind": kind, "values": vals, "valid": msks})
    return runs


def _steps(plan, warmup, steps):
    """Per-step (emit_ms, total_device_ms) medians."""
    emit, tot = [], []
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
            emit.append(s1["emit_ms"] - s0["emit_ms"])
            tot.append(s1["total_device_ms"] - s0["total_device_ms"])
    return float(np.median(emit)), float(np.median(tot)), rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()

    runs = _gen(args.runs, args.rows, seed=91)
    with tempfile.TemporaryDirectory() as d:
        metas = write_runs(runs, d, compression="NONE")
        with Session(0) as s:
            common = dict(merge_engine="partial-update",
                          sequence_groups=GROUPS, output="device")
            plans = {
                "A_no_aggregators": MergeReadPlan(
                    s, file_descs_from_metas(metas), KEY_COLS, VALUE_COLS,
                    **common),
                "B_aggregators": MergeReadPlan(
                    s, file_descs_from_metas(metas), KEY_COLS, VALUE_COLS,
                    aggregations=AGGS, ignore_retract=IGNORE, **common),
            }
            res = {k: [] for k in plans}
            for _ in range(2):
                for k, p in plans.items():
                    e_ms, t_ms, rows = _steps(p, args.warmup, args.steps)
                    res[k].append({"emit_ms": round(e_ms, 4),
                                   "total_device_ms": round(t_ms, 4),
                                   "rows_out": rows})
            for p in plans.values():
                p.close()
    print(json.dumps({"bench": "pu_agg_emit", "runs": args.runs,
                      "rows_per_run": args.rows, "value_cols": 7,
                      "passes": res}))


if __name__ == "__main__":
    main()
