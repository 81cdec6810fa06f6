"""bench.py's plain run and --dump-outputs on one GPU (ecc_small): the plain line holds the timed steps' figures and none
of the --full legs, --steps sets the number of timed steps, and two runs with the same arguments write the same outputs
(float32 / float64, within the 64 MB budget). Named *_00_* so the children start before this process has touched the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(out_dir, steps):
    cmd = [sys.executable, BENCH, "--gpus", "1", "--workload", "ecc_small", "--steps", str(steps), "--warmup", "1",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.timeout(900)
def test_bench_plain_run_dumps_the_same_outputs_twice(tmp_path):
    a = _run(tmp_path / "a", 3)
    b = _run(tmp_path / "b", 2)
    for v, steps in ((a, 3), (b, 2)):
        assert v["steps"] == steps and v["warmup"] == 1 and v["ms_per_step"] > 0 and v["higher_is_better"] is True
        assert abs(v["value"] - 8 * steps / (v["ms_per_step"] * steps * 1e-3)) <= 1e-2 * v["value"]
        assert v["unit"] == "frames/s" and v["dtype"] == "f32"
        assert not {"roofline", "kernels", "host_fed", "files", "cpu_baseline"} & set(v)          # --full legs only
        assert v["stages"]["frames_folded_last_step"] == 8 and v["stages"]["frames_dropped_last_step"] == 0
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"stacked.npy", "stacked_rows.npy", "counts.npy", "warps.npy", "frame_iterations.npy"} <= set(names)
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64e6
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64), n
        assert np.array_equal(x, y, equal_nan=True), n                  # seeded inputs, deterministic engine
    img = np.load(tmp_path / "a" / "stacked.npy")
    assert img.shape == (480, 640, 3) and img.dtype == np.float32 and np.isfinite(img).all() and img.max() > 0
    assert np.array_equal(np.load(tmp_path / "a" / "stacked_rows.npy"), np.arange(480))
    assert np.array_equal(np.load(tmp_path / "a" / "counts.npy"), [8, 0])
    w = np.load(tmp_path / "a" / "warps.npy")
    assert w.shape == (8, 3, 3) and np.array_equal(w[0], np.eye(3))
