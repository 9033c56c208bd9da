#!/usr/bin/env python
"""Time the 3-NN initial-scale kernel (csrc/knn.hip through mobgs_amd.scene_init) on one GPU, beside the one alternative
this platform offers: a chunked torch.cdist + topk(3, largest=False) in the same process.

    python scripts/knn_timing.py [--out profiles/knn_timing.json] [--sizes 100000 300000 1000000] [--alt-size 300000]

Clouds: the benchmark cloud of scripts/heavy_tail.py (synth.splat_inputs), uniform and with 30 % of the points pulled
into 8 % of the screen.  HIP events around each call after warm-up, median of `runs`; results are compared on the way
(the alternative's fp32 cdist is only close, so the comparison is a tolerance, not an identity)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mobgs_amd import scene_init  # noqa: E402
from mobgs_amd.synth import SynthCamera, splat_inputs  # noqa: E402


def cloud(n, clustered, frac=0.3, region=0.08):
    """The two generators of scripts/heavy_tail.py, positions only."""
    cam = SynthCamera()
    m = splat_inputs(n, cam, 0, 9)["means"].clone()
    if clustered:
        g = torch.Generator().manual_seed(5)
        k = int(frac * n)
        z = m[:k, 2]
        m[:k, 0] = (torch.rand(k, generator=g) - 0.5) * region * z * cam.width / cam.focal
        m[:k, 1] = (torch.rand(k, generator=g) - 0.5) * region * z * cam.height / cam.focal
    return m


def cdist_topk(points, chunk=4096):
    """The alternative: rows in chunks, full distance matrix of a chunk, three smallest per row (self masked by index)."""
    n = points.shape[0]
    out = torch.empty(n, dtype=torch.float32, device=points.device)
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        d = torch.cdist(points[a:b], points)
        d[torch.arange(b - a, device=points.device), torch.arange(a, b, device=points.device)] = float("inf")
        out[a:b] = (d.topk(3, dim=1, largest=False).values ** 2).sum(1) / 3.0
    return out


def time_ms(fn, runs, warmup):
    """Median / min / max of `runs` calls, each between two HIP events, after `warmup` calls."""
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


def measure(n, clustered, runs=20, warmup=3, alt_runs=0):
    """-> a record: the whole knn3_mean_dist2 (Morton sort + kernel + scatter), the kernel alone on sorted rows and,
    with alt_runs > 0, the alternative."""
    dev = torch.device("cuda")
    pts = cloud(n, clustered).to(dev)
    srt = pts[scene_init.morton_order(pts)].contiguous()
    rec = {"n": n, "cloud": "clustered" if clustered else "uniform",
           "knn3_mean_dist2": time_ms(lambda: scene_init.knn3_mean_dist2(pts), runs, warmup),
           "kernel_only_sorted_rows": time_ms(lambda: scene_init.knn3_sorted(srt), runs, warmup)}
    if alt_runs:
        rec["cdist_topk"] = time_ms(lambda: cdist_topk(pts), alt_runs, 1)
        rec["ratio_alt_over_knn"] = rec["cdist_topk"]["median_ms"] / rec["knn3_mean_dist2"]["median_ms"]
        a, b = scene_init.knn3_mean_dist2(pts), cdist_topk(pts)
        rec["max_rel_diff_vs_alt"] = float(((a - b).abs() / a.clamp_min(1e-30)).max())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 300000, 1000000])
    ap.add_argument("--alt-size", type=int, default=300000)
    ap.add_argument("--alt-runs", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    recs = []
    for n in a.sizes:
        for clustered in (False, True):
            r = measure(n, clustered, alt_runs=a.alt_runs if n == a.alt_size else 0)
            recs.append(r)
            print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "records": recs}, f, indent=1)


if __name__ == "__main__":
    main()
