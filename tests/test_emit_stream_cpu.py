"""k_emit_stream's slot mapping and column-group plan
(paimon_amd/csrc/emit_stream_core.h, the code the kernel runs) through the
stand-alone host check: slot -> (run, row) -> slot over generated tiles
(k = 1, 2, 3, 8, 32, empty slices, runs ending inside a tile, single-row runs,
the last partial tile, a tile at PMH_TILE_MAX) and the group planner over 1,
12, 13 and 256 columns. Built with ASan + UBSan; no GPU calls."""

import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "paimon_amd", "csrc")


def test_hostcheck_builds_and_passes():
    b = subprocess.run(["make", "-C", CSRC, "build/emit_stream_hostcheck"],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([os.path.join(CSRC, "build", "emit_stream_hostcheck")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "emit_stream_hostcheck OK" in r.stdout
