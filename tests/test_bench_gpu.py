"""GPU: bench.py's plain run and --dump-outputs.  A plain run (no --full) prints the line with the headline only — no roofline, CPU
baseline or pose check — and with the same arguments writes the same outputs of its last timed step: float64 arrays, nav records of
every sequence and the KeyLines of a fixed sample of them, bit for bit the same from one run to the next."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(tmp_path, tag, extra):
    env = dict(os.environ, BENCH_EXTRAS_FILE=str(tmp_path / f"{tag}_extras.json"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--nseq", "12", "--pool", "6", "--input", "pool",
                        "--steps", "4", "--warmup", "3"] + extra, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_dumps_the_same_outputs_every_time(tmp_path):
    outs = []
    for tag in ("a", "b"):
        line = _bench(tmp_path, tag, ["--dump-outputs", str(tmp_path / tag)])
        assert line["steps"] == 4 and line["warmup"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
        assert abs(line["value"] - 12 * 1e3 / line["ms_per_step"]) < 1e-3 * line["value"]
        assert line["roofline"] is None and line["cpu_baseline"] is None and line["pose_rmse"] is None
        assert "kernel_us_per_step_top" not in line and "host_surface" not in line
        files = sorted(os.listdir(tmp_path / tag))
        outs.append({f: np.load(tmp_path / tag / f) for f in files})
    a, b = outs
    assert sorted(a) == sorted(b) and "nav_V.npy" in a and "nav_Pos.npy" in a and "keylines_rho.npy" in a
    assert sum(x.nbytes for x in a.values()) <= 64 * 2 ** 20
    for f in a:
        assert a[f].dtype == np.float64, f
        assert np.array_equal(a[f], b[f], equal_nan=True), f
    assert a["nav_V.npy"].shape == (12, 3) and np.all(a["nav_frame.npy"] == a["nav_frame.npy"][0])
    seqs = a["keylines_sequence.npy"]
    assert len(seqs) > 1000 and np.all(np.diff(seqs) >= 0) and len(np.unique(seqs)) == 8
    for s in np.unique(seqs).astype(int):
        assert np.sum(seqs == s) == a["nav_kn.npy"][s]      # the sample's KeyLines are its sequences' whole lists


def test_full_run_keeps_the_per_kernel_figures(tmp_path):
    """--full: the per-kernel times and the roofline of every kernel group that moves bytes.  (At 12 sequences the dominant group
    can be one that moves none, the LM step, so the line's `roofline` may be null here; the record's per-group rooflines are not.)"""
    line = _bench(tmp_path, "full", ["--full", "--cpu-frames", "0", "--no-extras", "--no-live-pmc"])
    assert line["steps"] == 4 and line["ms_per_step"] > 0 and "roofline" in line and len(line["kernel_us_per_step_top"]) == 5
    full = json.load(open(tmp_path / "full_extras.json"))
    assert full["kernel_us_per_step"] and full["traffic_calibration"]
    assert full["roofline_kernels"] and all(r["launch_us"] > 0 and r["frac"] >= 0 for r in full["roofline_kernels"].values())
