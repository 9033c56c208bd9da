"""A plain `bench.py --gpus 1` run (no --full) on a small scene: the headline line alone, reporting the --steps it was
given, and --dump-outputs writing what the last timed step computed -- the same arrays, from the same inputs, every
run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--ns", "6000", "--nd", "3000", "--width", "320", "--height", "240", "--prewarm", "2"]


def _run(args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_run_reports_the_headline_and_dumps_outputs(hip_device, tmp_path):
    dirs = [tmp_path / "a", tmp_path / "b"]
    lines = [_run(["--steps", str(k), "--warmup", "1", *SMALL, "--dump-outputs", str(d)]) for k, d in zip((3, 5), dirs)]
    for k, line in zip((3, 5), lines):
        assert line["steps"] == k and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["unit"] == "renders/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        # what moved behind --full stays out of a plain line
        assert not {"roofline", "cpu_baseline", "deblur", "repeat", "train_iteration", "scale_anchor"} & set(line)
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    assert {"render.npy", "depth.npy", "radii.npy", "grad_stat_xyz.npy", "grad_dyn_control_xyz.npy"} <= set(names)
    total = 0
    for n in names:
        a, b = np.load(dirs[0] / n), np.load(dirs[1] / n)
        assert a.dtype in (np.float32, np.float64) and a.shape == b.shape, n
        assert np.isfinite(a).all(), n
        total += a.nbytes
    assert total <= 64 * 2 ** 20
    assert np.load(dirs[0] / "render.npy").shape == (3, 240, 320)
    # the same inputs in both runs (different step counts): the same image, to rounding
    ra, rb = np.load(dirs[0] / "render.npy"), np.load(dirs[1] / "render.npy")
    assert np.abs(ra - rb).max() <= 1e-4 * max(1.0, float(np.abs(ra).max()))
