#!/usr/bin/env python
"""Time the one-down control-point kernel (csrc/control_prune.hip through mobgs_amd.scene_init) on one GPU, beside a
straightforward torch version of the same formulation on the same device: the float64 pseudo-inverse table gathered per
row and applied with one batched product, then the two splines evaluated and projected view by view in fp32.

    python scripts/control_prune_timing.py [--out profiles/control_prune_timing.json] [--rows 100000] [--views 48]

HIP events around each call after warm-up, median of `runs`.  Both are dry runs (nothing is committed), so every
repetition sees the same input; the two results are compared on the way."""
import argparse
import datetime
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mobgs_amd import scene_init  # noqa: E402
from oracle.render_torch import hermite  # noqa: E402


def synthetic_set(n, n_views, seed=0):
    """A seeded dynamic set on the host: counts uniform in 4..12, trajectories from nearly straight to strongly
    oscillating sampled at each row's knot times (x 100, unused slots zero), cameras on an arc around the cloud.
    -> dict(control_xyz [n,12,3], control_num [n,1], w2c [V,4,4], times [V], focal, width, height)."""
    g = torch.Generator().manual_seed(seed)
    num = torch.randint(4, 13, (n,), generator=g)
    centre = torch.tensor([4.0, -1.5, 6.0])
    base = centre + 1.2 * torch.randn(n, 3, generator=g)
    amp = 10.0 ** (-2.8 + 2.8 * torch.rand(n, 1, 1, generator=g))
    freq = 0.4 + 2.6 * torch.rand(n, 1, 3, generator=g)
    phase = 6.2831853 * torch.rand(n, 1, 3, generator=g)
    drift = 0.3 * torch.randn(n, 1, 3, generator=g)
    k = torch.arange(12, dtype=torch.float32)[None, :, None]
    t = k / (num[:, None, None] - 1).float()
    pos = base[:, None, :] + drift * t + amp * torch.sin(6.2831853 * freq * t + phase)
    control = torch.where((k >= num[:, None, None]).expand(-1, -1, 3), torch.zeros(()), pos * 100.0).float()
    mats = []
    for v in range(n_views):
        a = -0.9 + 1.8 * v / (n_views - 1)
        eye = torch.tensor([float(centre[0]) + 7.5 * math.sin(a), float(centre[1]) + 0.8 * math.cos(3.0 * a),
                            float(centre[2]) + 7.5 * math.cos(a)], dtype=torch.float64)
        f = centre.double() - eye
        f = f / f.norm()
        r = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), f)
        r = r / r.norm()
        R = torch.stack([r, torch.linalg.cross(f, r), f])
        M = torch.eye(4, dtype=torch.float64)
        M[:3, :3], M[:3, 3] = R, -R @ eye
        mats.append(M.float())
    times = torch.linspace(0, 1, n_views)
    times[1:-1] = (times[1:-1] + 0.3 / n_views * torch.randn(n_views - 2, generator=g)).clamp(0.01, 0.99)
    return {"control_xyz": control.contiguous(), "control_num": num.reshape(n, 1), "w2c": torch.stack(mats),
            "times": times, "focal": 520.0, "width": 640, "height": 480}


def torch_one_down(control, num, w2c, times, focal, width, height, table64):
    """The same computation with torch operators on the tensors' device -> (new [N,11,3] fp32, error [N] fp32)."""
    N = control.shape[0]
    n = num.reshape(N)
    cand = n > 4
    slot = torch.arange(12, device=control.device)[None, :, None]
    masked = torch.where(slot < n[:, None, None], control, torch.zeros((), device=control.device))
    fit = torch.bmm(table64[(n - 5).clamp_min(0)], masked.double()).float()
    new = torch.where(cand[:, None, None], fit, masked[:, :11])
    m = torch.where(cand, n - 1, n)[:, None]
    full = torch.cat([new, control[:, 11:]], 1)
    cx, cy = width / 2, height / 2
    one = torch.ones(N, 1, device=control.device)

    def pixels(p, M):
        h = torch.cat([p, one], 1) @ M.T
        cam = h[:, :3] / (h[:, 3:] + 0.0000001)
        d = cam[:, 2] + 0.0000001
        return torch.stack([(focal * cam[:, 0] + cx * cam[:, 2]) / d, (focal * cam[:, 1] + cy * cam[:, 2]) / d], 1)

    total = torch.zeros(N, device=control.device)
    V = w2c.shape[0]
    for v in range(1, V - 1):
        total += (pixels(hermite(control, times[v], num) * 1e-2, w2c[v])
                  - pixels(hermite(full, times[v], m) * 1e-2, w2c[v])).norm(dim=1)
    return new, torch.where(cand, total / (V - 2), torch.zeros_like(total))


def time_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "runs": runs}


def measure(rows=100000, views=48, runs=20, warmup=3, alt_runs=5):
    dev = torch.device("cuda")
    s = synthetic_set(rows, views)
    control, num, w2c, times = (s[k].to(dev) for k in ("control_xyz", "control_num", "w2c", "times"))
    focal, W, H = s["focal"], s["width"], s["height"]
    table64 = torch.zeros(8, 11, 12, dtype=torch.float64)
    for n in range(5, 13):
        table64[n - 5, :n - 1, :n] = torch.linalg.pinv(scene_init.one_down_design(n))
    table64 = table64.to(dev)
    scene_init.one_down_tables(dev)

    def kernel():
        return scene_init._one_down_launch(control, num, w2c, times, focal, W / 2, H / 2, 1.0, True, False)

    def alt():
        return torch_one_down(control, num, w2c, times, focal, W, H, table64)

    rec = {"rows": rows, "views": views, "mobgs_control_onedown": time_ms(kernel, runs, warmup),
           "torch_same_formulation": time_ms(alt, alt_runs, 1)}
    rec["ratio_torch_over_kernel"] = rec["torch_same_formulation"]["median_ms"] / rec["mobgs_control_onedown"]["median_ms"]
    err, new, _ = kernel()
    new_t, err_t = alt()
    rec["max_abs_diff_new_vs_torch"] = float((new - new_t).abs().max())
    rec["max_abs_diff_error_px_vs_torch"] = float((err - err_t).abs().max())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--views", type=int, default=48)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    rec = measure(a.rows, a.views)
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(),
                       "records": [rec]}, f, indent=1)


if __name__ == "__main__":
    main()
