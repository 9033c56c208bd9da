#!/usr/bin/env python
"""Time tOF of one test split (24 frames, prediction + ground truth) three ways on one device:

  torch    the same computation composed from torch operations on the device in fp32: the grey conversion, per level
           F.conv2d (the Gaussian blur over reflect padding, the polynomial expansion as five 11x11 kernels over replicate
           padding), F.interpolate (the level image, the x2 flow), F.grid_sample (the warp of the update matrices),
           avg_pool2d over replicate padding (the 15x15 box mean), the solve and the crop -- all pairs of a sequence in one batch
  fused    metrics.temporal_of(pred, gt): csrc/tof.hip for both sequences
  cached   metrics.temporal_of(pred, TofTarget): the ground truth's flows computed once, outside the timed window

    python scripts/bench_tof.py [--rounds 10] [--inner 3] [--warmup 2] [--out FILE.json] [--limit SECONDS]

Sizes: 512x288 and 1352x1014.  Each size is measured in a child process of its own, started under a time limit; after a child
that fails or runs out of time nothing more is started.  Inside a child the routes alternate round by round in ONE process: a
round is `inner` calls of one route between two device synchronisations on the host clock, divided by `inner`.  Reported per
route: median, min and max over the rounds, and the largest distance between the routes' tOF values, one JSON line per size.
Needs a HIP device: no fallback.  (`--check-cpu` instead compares the torch composition with tests/tof_restatement.py in
float64 on the CPU at a small size: the baseline computes the same thing.)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((24, 288, 512), (24, 1014, 1352))     # (frames, H, W)


def tof_levels(H, W):
    """[(width, height, taps, sigma)], coarsest first (include/mobgs_hip.h K25, mobgs_tof_levels)."""
    scale, k = 1.0, 0
    while k < 3:
        scale *= 0.5
        if W * scale < 32 or H * scale < 32:
            break
        k += 1
    out = []
    for kk in range(k, -1, -1):
        s = 0.5 ** kk
        sigma = (1.0 / s - 1.0) * 0.5
        out.append((round(W * s), round(H * s), max(int(round(sigma * 5)) | 1, 3), sigma))   # (round: half to even)
    return out


def crop_window(H, W):
    h, w = (H // 32) * 32, (W // 32) * 32
    while h > H - 16:
        h -= 32
    while w > W - 16:
        w -= 32
    return (H - h) // 2, (W - w) // 2, h, w


def torch_grey(x, clamp, quantize):
    import torch
    if clamp:
        x = x.clamp(0, 1)
    if quantize:
        x = torch.floor(x.clamp(0, 1) * 255.0) / 255.0
    q = torch.trunc(x * 255.0).clamp(0, 255).to(torch.int32)
    return ((4899 * q[:, 0] + 9617 * q[:, 1] + 1868 * q[:, 2] + 8192) >> 14).to(x.dtype)


def poly_kernels(dtype, device):
    """[5,1,11,11]: the rows r_x, r_y, r_xx, r_yy, r_xy of the weighted least-squares solution operator."""
    import torch
    t = torch.arange(-5, 6, dtype=torch.float64)
    g = torch.exp(-t * t / (2 * 1.2 * 1.2))
    g = g / g.sum()
    Y, X = torch.meshgrid(t, t, indexing="ij")
    basis = torch.stack([torch.ones_like(X), X, Y, X * X, Y * Y, X * Y])
    wgt = torch.outer(g, g)
    gram = torch.einsum("ayx,byx,yx->ab", basis, basis, wgt)
    op = torch.linalg.solve(gram, (basis * wgt).reshape(6, -1)).reshape(6, 11, 11)
    return op[1:, None].to(dtype=dtype, device=device)


def torch_flows(grey):
    """[F,H,W] -> [F-1,H,W,2]: every consecutive pair in one batch."""
    import torch
    import torch.nn.functional as F
    Fr, H, W = grey.shape
    dt, dev = grey.dtype, grey.device
    pk = poly_kernels(dt, dev)
    border = torch.tensor([0.14, 0.14, 0.4472, 0.4472, 0.4472], dtype=dt, device=dev)

    def side(n):
        s = torch.ones(n, dtype=dt, device=dev)
        s[:5] *= border
        s[n - 5:] *= border.flip(0)
        return s

    flow = None
    for w, h, taps, sigma in tof_levels(H, W):
        if sigma > 0:
            t = torch.arange(taps, dtype=torch.float64) - taps // 2
            g = torch.exp(-t * t / (2 * sigma * sigma))
            g = (g / g.sum()).to(dtype=dt, device=dev)
        else:
            g = torch.tensor([0.25, 0.5, 0.25], dtype=dt, device=dev)
        r = taps // 2
        img = F.pad(grey[:, None], (r, r, r, r), mode="reflect")
        img = F.conv2d(F.conv2d(img, g.reshape(1, 1, 1, taps)), g.reshape(1, 1, taps, 1))
        img = F.interpolate(img, size=(h, w), mode="bilinear", align_corners=False)
        R = F.conv2d(F.pad(img, (5, 5, 5, 5), mode="replicate"), pk)                       # [F,5,h,w]
        R0, R1 = R[:-1], R[1:]
        if flow is None:
            flow = torch.zeros(Fr - 1, 2, h, w, dtype=dt, device=dev)
        else:
            flow = 2.0 * F.interpolate(flow, size=(h, w), mode="bilinear", align_corners=False)
        ys, xs = torch.meshgrid(torch.arange(h, dtype=dt, device=dev), torch.arange(w, dtype=dt, device=dev), indexing="ij")
        scale = torch.outer(side(h), side(w))

        def update(flow):
            u, v = flow[:, 0], flow[:, 1]
            fx, fy = xs + u, ys + v
            inb = ((fx >= 0) & (fx < w - 1) & (fy >= 0) & (fy < h - 1))[:, None]
            grid = torch.stack([fx * (2.0 / (w - 1)) - 1.0, fy * (2.0 / (h - 1)) - 1.0], -1)
            S = F.grid_sample(R1, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
            a_xx = torch.where(inb, (R0[:, 2:3] + S[:, 2:3]) * 0.5, R0[:, 2:3])
            a_yy = torch.where(inb, (R0[:, 3:4] + S[:, 3:4]) * 0.5, R0[:, 3:4])
            a_xy = torch.where(inb, (R0[:, 4:5] + S[:, 4:5]) * 0.25, R0[:, 4:5] * 0.5)
            b_x = torch.where(inb, (R0[:, 0:1] - S[:, 0:1]) * 0.5, R0[:, 0:1] * 0.5)
            b_y = torch.where(inb, (R0[:, 1:2] - S[:, 1:2]) * 0.5, R0[:, 1:2] * 0.5)
            b_x = b_x + a_xx * u[:, None] + a_xy * v[:, None]
            b_y = b_y + a_xy * u[:, None] + a_yy * v[:, None]
            a_xx, a_yy, a_xy, b_x, b_y = a_xx * scale, a_yy * scale, a_xy * scale, b_x * scale, b_y * scale
            return torch.cat([a_xx * a_xx + a_xy * a_xy, (a_xx + a_yy) * a_xy, a_yy * a_yy + a_xy * a_xy,
                              a_xx * b_x + a_xy * b_y, a_xy * b_x + a_yy * b_y], 1)

        M = update(flow)
        for i in range(3):
            B = F.avg_pool2d(F.pad(M, (7, 7, 7, 7), mode="replicate"), 15, stride=1)
            det = B[:, 0] * B[:, 2] - B[:, 1] * B[:, 1] + 1e-3
            flow = torch.stack([(B[:, 2] * B[:, 3] - B[:, 1] * B[:, 4]) / det, (B[:, 0] * B[:, 4] - B[:, 1] * B[:, 3]) / det], 1)
            if i < 2:
                M = update(flow)
    return flow.permute(0, 2, 3, 1)


def torch_tof(pred, gt, clamp=False, quantize=False):
    fa, fb = torch_flows(torch_grey(gt, clamp, False)), torch_flows(torch_grey(pred, clamp, quantize))
    y, x, h, w = crop_window(*fa.shape[1:3])
    d = (fa - fb)[:, y:y + h, x:x + w]
    return (d * d).sum(-1).sqrt().mean((1, 2)).double()


def sequence(Fr, H, W, seed, device):
    """A smooth colour texture drifting by about a pixel a frame, and a prediction of it with a little noise."""
    import torch
    g = torch.Generator(device=device).manual_seed(seed)
    base = torch.nn.functional.avg_pool2d(torch.rand(1, 3, H + 64, W + 64, generator=g, device=device), 9, stride=1, padding=4)
    base = ((base - base.mean()) * 6.0 + 0.5).clamp(0, 1)
    gt = torch.stack([base[0, :, 16 + (f * 5) // 7:16 + (f * 5) // 7 + H, 16 + f:16 + f + W] for f in range(Fr)])
    pred = gt + 0.02 * torch.randn(Fr, 3, H, W, generator=g, device=device)
    return pred.contiguous(), gt.contiguous()


def check_cpu():
    import numpy as np
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import tof_restatement as TR
    for H, W in ((50, 75), (259, 262)):
        rgb = TR.moving_frames(3, H, W, seed=H)
        assert [tuple(l) for l in tof_levels(H, W)] == TR.levels(H, W) and crop_window(H, W) == TR.crop_window(H, W)
        grey = torch_grey(torch.from_numpy(rgb), False, False).double()
        assert np.array_equal(grey.numpy(), TR.grey(rgb))
        got, want = torch_flows(grey).numpy(), TR.flows(TR.grey(rgb))
        print(f"{W}x{H}: torch composition (float64, CPU) against the restatement: largest flow difference "
              f"{np.abs(got - want).max():.2e} px of {np.abs(want).max():.2f}")


def measure(index, rounds, inner, warmup):
    import torch
    sys.path.insert(0, ROOT)
    from mobgs_amd.metrics import TofTarget, temporal_of
    if not torch.cuda.is_available():
        raise SystemExit("bench_tof.py needs a HIP device")
    dev = torch.device("cuda:0")
    Fr, H, W = SIZES[index]
    pred, gt = sequence(Fr, H, W, index, dev)
    target = TofTarget.from_frames(gt)
    results = {}

    def torch_route():
        with torch.no_grad():
            results["torch"] = torch_tof(pred, gt)

    def fused_route():
        results["fused"] = temporal_of(pred, gt)

    def cached_route():
        results["cached"] = temporal_of(pred, target)

    routes = (("torch", torch_route), ("fused", fused_route), ("cached", cached_route))
    times = {name: [] for name, _ in routes}
    for r in range(warmup + rounds):
        for name, fn in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            if r >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e3 / inner)
    row = {"frames": Fr, "height": H, "width": W, "rounds": rounds, "inner": inner}
    for name, ts in times.items():
        row[name + "_ms_median"], row[name + "_ms_min"], row[name + "_ms_max"] = statistics.median(ts), min(ts), max(ts)
    row["torch_over_fused"] = row["torch_ms_median"] / row["fused_ms_median"]
    row["torch_over_cached"] = row["torch_ms_median"] / row["cached_ms_median"]
    row["largest_relative_distance_torch_fused"] = float(((results["torch"] - results["fused"]).abs()
                                                          / results["fused"].abs()).max())
    row["cached_equals_fused"] = bool(torch.equal(results["cached"], results["fused"]))
    row["mean_tof"] = float(results["fused"].mean())
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds a size may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--check-cpu", action="store_true")
    ap.add_argument("--size", type=int, default=None, help="(internal) measure SIZES[i] in this process")
    a = ap.parse_args()
    if a.check_cpu:
        check_cpu()
        return
    if a.size is not None:
        measure(a.size, a.rounds, a.inner, a.warmup)
        return
    rows = []
    for i in range(len(SIZES)):
        cmd = [sys.executable, os.path.abspath(__file__), "--size", str(i), "--rounds", str(a.rounds), "--inner",
               str(a.inner), "--warmup", str(a.warmup)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"size {SIZES[i]}: no result within {a.limit:.0f} s; nothing more is started")
        if r.returncode != 0:
            raise SystemExit(f"size {SIZES[i]}: exit status {r.returncode}; nothing more is started")
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        rows.append(json.loads(line))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
