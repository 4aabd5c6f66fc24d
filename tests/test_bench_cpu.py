"""bench.py pieces that need no GPU: option defaults and the writer side of
--dump-outputs (file set, checksum split, the size cap)."""

import os
import sys

import numpy as np

import bench


def test_option_defaults(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps",
                                      "7", "--warmup", "2"])
    a = bench.get_args()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs",
                                      "d"])
    a = bench.get_args()
    assert a.full is True and a.dump_outputs == "d"


def test_data_dir_falls_back_when_checkout_is_not_writable(tmp_path,
                                                          monkeypatch):
    # a path below a regular file cannot be created, whoever runs the test
    blocker = tmp_path / "blocker"
    blocker.write_text("")
    home = tmp_path / "home"
    monkeypatch.setenv("HOME", str(home))

    monkeypatch.setattr(bench, "REPO", str(tmp_path / "repo"))
    assert bench.default_data_dir() == str(tmp_path / "repo" / "data")

    monkeypatch.setattr(bench, "REPO", str(blocker))
    d = bench.default_data_dir()
    assert d == str(home / ".cache" / "paimon_hip" / "bench_data")
    assert os.path.isdir(d)

    monkeypatch.setenv("HOME", str(blocker))
    d = bench.default_data_dir()
    assert os.path.isdir(d) and not d.startswith(str(tmp_path))
    os.rmdir(d)  # else removed when the interpreter exits


def _filled(n_batches, rows_each):
    d = bench.OutputDump(0)
    d.names = ["a"]
    d.parts = {"a": [], "a__valid": []}
    d.sums = {"a": (-3) & (2**64 - 1)}
    for i in range(n_batches):
        d.parts["a"].append(np.arange(rows_each, dtype=np.float64) + i)
        d.parts["a__valid"].append(np.ones(rows_each, np.float32))
        d.sample_rows.append(np.arange(rows_each) + i * rows_each)
        d.batch_rows.append(rows_each)
    return d


def test_dump_write_files(tmp_path):
    _filled(2, 5).write(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == [
        "a.npy", "a__sum.npy", "a__valid.npy", "batch_rows.npy",
        "sample_rows.npy"]
    assert np.load(tmp_path / "a.npy").tolist() == [0, 1, 2, 3, 4,
                                                    1, 2, 3, 4, 5]
    assert np.load(tmp_path / "a__sum.npy").tolist() == [2**32 - 1,
                                                         2**32 - 3]
    assert np.load(tmp_path / "sample_rows.npy").tolist() == list(range(10))
    assert np.load(tmp_path / "batch_rows.npy").tolist() == [5, 5]


def test_dump_write_thins_to_budget(tmp_path, monkeypatch):
    # 3 arrays of 8 B/row budgeted at 100 rows; 4 batches brought 400
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 8 * 3 * 100)
    _filled(4, 100).write(str(tmp_path))
    rows = np.load(tmp_path / "sample_rows.npy")
    a = np.load(tmp_path / "a.npy")
    assert len(rows) == len(a) == len(np.load(tmp_path / "a__valid.npy")) == 100
    assert (np.diff(rows) > 0).all()
    assert (a == rows % 100 + rows // 100).all()  # same rows in every array
    # the thinning is seeded: a second writer keeps the same rows
    other = tmp_path / "again"
    _filled(4, 100).write(str(other))
    assert (np.load(other / "sample_rows.npy") == rows).all()
