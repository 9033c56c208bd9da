#!/usr/bin/env python
"""Time forward + backward of the regularisation block of one training iteration (the reference's train.py:622 and
:651-655) two ways on one device:

  torch   the statements as the reference writes them, on the device: psnr(image, gt).mean(), l1_loss(depth, gt_depth),
          entropy_loss(d_alpha), sparsity_loss(d_alpha), the weighted sum, .backward()
  fused   loss_utils.regularisation_terms(...) and .backward(): two launches forward, one backward (csrc/regterms.hip)

    python scripts/reg_terms_timing.py [--rounds 15] [--inner 20] [--warmup 3] [--out FILE.json] [--limit SECONDS]

Sizes: 2 views x 512x288 (the reference's operating point) and 2 views x 1352x1014.  Each size is measured in a child
process of its own, started under a time limit; after a child that fails or runs out of time nothing more is started.
Inside a child the two routes alternate round by round in ONE process: a round is `inner` calls of one route between two
device synchronisations on the host clock, divided by `inner`.  Reported per route: median and min over the rounds (and
the largest round, for the spread), one JSON line per size.  Needs a HIP device: there is no CPU path and no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((2, 288, 512), (2, 1014, 1352))     # (views, H, W)


def measure(index, rounds, inner, warmup):
    import torch
    sys.path.insert(0, ROOT)
    from mobgs_amd.loss_utils import regularisation_terms
    if not torch.cuda.is_available():
        raise SystemExit("reg_terms_timing.py needs a HIP device")
    dev = torch.device("cuda:0")
    B, H, W = SIZES[index]
    g = torch.Generator().manual_seed(index)
    gt_depth = (0.5 + 4.0 * torch.rand(B, 1, H, W, generator=g)).to(dev)
    depth = (gt_depth.cpu() + 0.3 * torch.randn(B, 1, H, W, generator=g)).to(dev).requires_grad_(True)
    alpha = torch.rand(B, 1, H, W, generator=g)
    alpha[:, :, : H // 2] = 0.0                       # half of the map is empty, as a dynamic alpha map is
    alpha = alpha.to(dev).requires_grad_(True)
    gt_image = torch.rand(B, 3, H, W, generator=g).to(dev)
    image = (gt_image.cpu() + 0.05 * torch.randn(B, 3, H, W, generator=g)).clamp(0, 1).to(dev)
    eps = 1e-6
    results = {}

    def torch_route():
        depth.grad = alpha.grad = None
        mse = ((image - gt_image) ** 2).view(B, -1).mean(1, keepdim=True)
        psnr_ = (20 * torch.log10(1.0 / torch.sqrt(mse.float()))).detach().mean().double()
        reg_loss = 0
        depth_loss = torch.abs(depth - gt_depth).mean()
        reg_loss += 0.2 * depth_loss
        entropy = -torch.sum(alpha * torch.log(alpha + eps) + (1 - alpha) * torch.log(1 - alpha + eps))
        mask_loss = 1e-7 * entropy + 1e-7 * torch.sum(alpha ** 2)
        reg_loss += mask_loss
        reg_loss.backward()
        results["torch"] = (reg_loss.detach(), psnr_)

    def fused_route():
        depth.grad = alpha.grad = None
        t = regularisation_terms(depth, gt_depth, alpha, image=image, gt_image=gt_image)
        psnr_ = t.psnr.mean().double()
        t.reg_loss.backward()
        results["fused"] = (t.reg_loss.detach(), psnr_)

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
    row = {"views": B, "height": H, "width": W, "rounds": rounds, "inner": inner}
    for name, ts in times.items():
        row[name + "_ms_median"], row[name + "_ms_min"], row[name + "_ms_max"] = statistics.median(ts), min(ts), max(ts)
        row[name + "_reg_loss"], row[name + "_psnr"] = float(results[name][0]), float(results[name][1])
    row["ratio_of_medians"] = row["torch_ms_median"] / row["fused_ms_median"]
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a size may take")
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
