"""bench.py's command line at a tiny shape: the result line, `--full`, and
`--dump-outputs` checked value for value against the host-output reader
path over the same generated files."""

import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from paimon_amd import Session, MergeReadPlan, file_descs_from_metas

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS, ROWS, VALS = 4, 30_000, 8  # partial-update sets 6-column subsets


def _bench(data_dir, *extra):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
           "--steps", "2", "--warmup", "1", "--runs", str(RUNS),
           "--rows", str(ROWS), "--vals", str(VALS),
           "--data-dir", str(data_dir)] + list(extra)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("engine", ["deduplicate", "partial-update"])
def test_dump_outputs_match_host_reader(tmp_path, engine):
    out = tmp_path / "dump"
    res = _bench(tmp_path, "--engine", engine, "--dump-outputs", str(out))
    assert res["steps"] == 2 and res["warmup"] == 1
    assert res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(
        RUNS * ROWS / (res["ms_per_step"] / 1e3))
    assert "cpu_baseline" not in res  # only with --full

    files = sorted(glob.glob(str(out / "*.npy")))
    dump = {os.path.basename(f)[:-4]: np.load(f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in dump.values())
    assert sum(os.path.getsize(f) for f in files) <= 64_000_000

    (manifest,) = glob.glob(str(tmp_path / "*" / "files.json"))
    metas = json.load(open(manifest))
    got, batch_rows = {}, []
    with Session(0) as s:
        with MergeReadPlan(
                s, file_descs_from_metas(metas),
                [{"name": "_KEY_k", "type": "int64"}],
                [{"name": "v_k", "type": "int64"}] +
                [{"name": f"v_c{i}", "type": "int32"} for i in range(VALS)],
                merge_engine=engine, drop_delete=True,
                output="host") as plan:
            while (b := plan.read_next()) is not None:
                batch_rows.append(len(b["_KEY_k"]))
                for k, v in b.items():
                    got.setdefault(k, []).append(v.copy())
    got = {k: np.concatenate(v) for k, v in got.items()}
    n = len(got["_KEY_k"])
    assert n == res["config"]["rows_out_per_step"]
    assert dump["batch_rows"].tolist() == batch_rows

    # the shape is small enough that the "sample" is every row
    assert dump["sample_rows"].tolist() == list(range(n))
    expect = {"sample_rows", "batch_rows"}
    for k, v in got.items():
        if k.endswith("#valid"):
            name = k[:-6] + "__valid"
            assert (dump[name] == v).all(), k
            expect.add(name)
            continue
        vv = v.astype(np.int64)
        if k + "#valid" in got:
            vv = np.where(got[k + "#valid"], vv, 0)
        assert (dump[k] == vv).all(), k
        s = int(vv.sum(dtype=np.int64)) & (2**64 - 1)
        assert dump[k + "__sum"].tolist() == [s >> 32, s & 0xFFFFFFFF], k
        expect |= {k, k + "__sum"}
    assert set(dump) == expect
    if engine == "partial-update":
        assert any(k.endswith("__valid") for k in dump)


def test_full_adds_cpu_baseline(tmp_path):
    res = _bench(tmp_path, "--full", "--cpu-baseline-rows", "10000")
    assert res["cpu_baseline"]["unit"] == "rows/s"
    assert res["cpu_baseline"]["value"] > 0
    for k in ("metric", "value", "unit", "higher_is_better", "dtype",
              "ms_per_step"):
        assert k in res
