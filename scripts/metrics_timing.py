#!/usr/bin/env python
"""Time the scoring of a batch of image pairs two ways on one device:

  torch   the same seven numbers per image composed from torch operations on the device in fp32: the error means, the box
          SSIM (symmetric padding by concatenation, avg_pool2d 7x7, the crop) and the Gaussian partial-convolution SSIM
          (conv2d 1x11 and 11x1 over z x mask and over the mask, the two renormalisations)
  fused   metrics.image_metrics(pred, gt, mask, data_range=2.0, clamp=True): two window launches and the finishing launch
          of csrc/metrics.hip

    python scripts/metrics_timing.py [--rounds 15] [--inner 10] [--warmup 3] [--out FILE.json] [--limit SECONDS]

Sizes: 24 pairs (one test split) at 512x288 and at 1352x1014, with a 60 % random mask.  Each size is measured in a child
process of its own, started under a time limit; after a child that fails or runs out of time nothing more is started.
Inside a child the two routes alternate round by round in ONE process: a round is `inner` calls of one route between two
device synchronisations on the host clock, divided by `inner`.  Reported per route: median, min and max over the rounds,
and the largest distance between the two routes' numbers, one JSON line per size.  Needs a HIP device: no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((24, 288, 512), (24, 1014, 1352))     # (pairs, H, W)


def torch_metrics(pred, gt, mask, data_range):
    import torch
    import torch.nn.functional as F
    B, C, H, W = pred.shape
    a, b = pred.clamp(0, 1), gt.clamp(0, 1)
    d = a - b
    se = d * d
    l1 = d.abs().mean((1, 2, 3))
    mse = se.mean((1, 2, 3))
    psnr = 20 * torch.log10(1.0 / torch.sqrt(mse))
    m = mask[:, None]
    big_m = 3 * mask.sum((1, 2))
    psnr_masked = -10.0 / torch.log(torch.tensor(10.0)) * torch.log((se * m).sum((1, 2, 3)) / big_m.clamp_min(1e-6))
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2

    def sym(x):          # scipy's `reflect`: d c b a | a b c d | d c b a
        x = torch.cat([x[..., :3].flip(-1), x, x[..., -3:].flip(-1)], -1)
        return torch.cat([x[..., :3, :].flip(-2), x, x[..., -3:, :].flip(-2)], -2)

    box = lambda x: F.avg_pool2d(sym(x), 7, stride=1)                         # noqa: E731
    ux, uy = box(a), box(b)
    vx, vy, vxy = (49 / 48) * (box(a * a) - ux * ux), (49 / 48) * (box(b * b) - uy * uy), (49 / 48) * (box(a * b) - ux * uy)
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    ssim_box = s[..., 3:-3, 3:-3].mean((2, 3)).mean(1)
    ssim_box_masked = (s * m).sum((1, 2, 3)) / (big_m + 1e-8)
    taps = torch.exp(-0.5 * ((torch.arange(11, device=pred.device, dtype=torch.float32) - 5) / 1.5) ** 2)
    taps = taps / taps.sum()
    ones = torch.ones_like(taps)

    def pconv(z, mm, k, shape):
        z_ = F.conv2d((z * mm).reshape(B * C, 1, *z.shape[-2:]), k.reshape(1, 1, *shape))
        z_ = z_.reshape(B, C, *z_.shape[-2:])
        m_ = F.conv2d(mm, ones.reshape(1, 1, *shape))
        return torch.where(m_ != 0, z_ * 11 / m_, torch.zeros_like(z_)), (m_ != 0).float()

    def filt(z):
        h, hm = pconv(z, m, taps, (1, 11))
        return pconv(h, hm, taps, (11, 1))[0]

    mu0, mu1 = filt(a), filt(b)
    s00 = (filt(a * a) - mu0 * mu0).clamp_min(0)
    s11 = (filt(b * b) - mu1 * mu1).clamp_min(0)
    s01 = filt(a * b) - mu0 * mu1
    s01 = torch.sign(s01) * torch.minimum(torch.sqrt(s00 * s11), s01.abs())
    g = ((2 * mu0 * mu1 + c1) * (2 * s01 + c2)) / ((mu0 * mu0 + mu1 * mu1 + c1) * (s00 + s11 + c2))
    ssim_gauss = g.mean((1, 2, 3))
    return torch.stack([l1, mse, psnr, psnr_masked, ssim_box, ssim_box_masked, ssim_gauss], 1).double()


def measure(index, rounds, inner, warmup):
    import torch
    sys.path.insert(0, ROOT)
    from mobgs_amd.metrics import image_metrics
    if not torch.cuda.is_available():
        raise SystemExit("metrics_timing.py needs a HIP device")
    dev = torch.device("cuda:0")
    B, H, W = SIZES[index]
    g = torch.Generator(device=dev).manual_seed(index)
    gt = torch.nn.functional.avg_pool2d(torch.rand(B, 3, H + 4, W + 4, generator=g, device=dev), 5, stride=1) * 1.6 - 0.3
    pred = gt + 0.05 * torch.randn(B, 3, H, W, generator=g, device=dev)
    mask = (torch.rand(B, H, W, generator=g, device=dev) < 0.6).float()
    results = {}

    def torch_route():
        with torch.no_grad():
            results["torch"] = torch_metrics(pred, gt, mask, 2.0)

    def fused_route():
        m = image_metrics(pred, gt, mask, data_range=2.0, clamp=True)
        results["fused"] = torch.stack([m.l1, m.mse, m.psnr, m.psnr_masked, m.ssim_box, m.ssim_box_masked, m.ssim_gauss], 1)

    routes = (("torch", torch_route), ("fused", fused_route))
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
    row = {"pairs": B, "height": H, "width": W, "rounds": rounds, "inner": inner}
    for name, ts in times.items():
        row[name + "_ms_median"], row[name + "_ms_min"], row[name + "_ms_max"] = statistics.median(ts), min(ts), max(ts)
    row["ratio_of_medians"] = row["torch_ms_median"] / row["fused_ms_median"]
    err = (results["torch"] - results["fused"]).abs().max(0).values
    in_db = torch.tensor([0, 0, 1, 1, 0, 0, 0], dtype=torch.bool, device=dev)
    diff = torch.where(in_db, err, err / results["fused"].abs().max(0).values)
    row["largest_distance_between_routes"] = dict(zip(("l1_rel", "mse_rel", "psnr_db", "psnr_masked_db", "ssim_box_rel",
                                                       "ssim_box_masked_rel", "ssim_gauss_rel"), diff.tolist()))
    row["fused_first_image"] = results["fused"][0].tolist()
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds a size may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", type=int, default=None, help="(internal) measure SIZES[i] in this process")
    a = ap.parse_args()
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
