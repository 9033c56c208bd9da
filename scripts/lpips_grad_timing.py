#!/usr/bin/env python
"""Time LPIPS as a loss (forward + backward into the prediction) for one and for two image pairs on one device:

  fused_fwd        LpipsAlex(pred, gt): the forward-only call (13 launches), for scale
  fused_loss_fwd   LpipsAlex.loss(pred, gt) with a prediction that requires a gradient: the forward that keeps the taps
  fused_fwd_bwd    LpipsAlex.loss(pred, gt).sum().backward(): + mobgs_lpips_alex_bwd with one side wanted (12 launches)
  torch_fwd_bwd    the same loss composed from torch operations in fp32 on the same device (the scaling layer, F.conv2d +
                   relu, F.max_pool2d, the normalisation, the 1x1 head, the mean) and torch autograd, over the same weights

    python scripts/lpips_grad_timing.py [--rounds 10] [--warmup 3] [--out FILE.json]

Sizes: 512x288 and 1352x1014, 1 and 2 pairs.  The routes alternate round by round in one process; a round is one call of a
route between two device events (the call ends in the event's synchronise); reported per route: median, min and max over the
rounds in ms, one JSON line per size, with the largest distance between the two gradients relative to the gradient's largest
magnitude, and the backward GEMMs' FLOP next to the forward's.  Needs a HIP device: no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1, 288, 512), (2, 288, 512), (1, 1014, 1352), (2, 1014, 1352))     # (pairs, H, W)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def gemm_flop(pairs, H, W):
    """(forward convolutions of both images, backward-data GEMMs of layers 5 .. 2 for one wanted side), FLOP."""
    from mobgs_amd.lpips import CIN, COUT, KS, tap_sizes
    taps = tap_sizes(H, W)
    fwd = sum(2.0 * 2 * pairs * h * w * COUT[l] * CIN[l] * KS[l] ** 2 for l, (h, w) in enumerate(taps))
    bwd = sum(2.0 * pairs * taps[l][0] * taps[l][1] * COUT[l] * CIN[l] * KS[l] ** 2 for l in range(1, 5))
    return fwd, bwd


def measure(index, rounds, warmup):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import lpips_restatement as LR
    from lpips_timing import torch_lpips
    from mobgs_amd.lpips import LpipsAlex
    if not torch.cuda.is_available():
        raise SystemExit("lpips_grad_timing.py needs a HIP device")
    dev = torch.device("cuda:0")
    B, H, W = SIZES[index]
    trunk, heads_sd = LR.seeded_trunk(), LR.reference_heads()
    model = LpipsAlex(trunk, heads_sd, device=dev)
    weights = [trunk[f"features.{i}.weight"].to(dev) for i in LR.TRUNK_INDEX]
    biases = [trunk[f"features.{i}.bias"].to(dev) for i in LR.TRUNK_INDEX]
    heads = [heads_sd[f"lin{l}.model.1.weight"].to(dev) for l in range(5)]
    g = torch.Generator(device=dev).manual_seed(index)
    gt = torch.rand(B, 3, H, W, generator=g, device=dev)
    pred = (gt + 0.1 * torch.randn(B, 3, H, W, generator=g, device=dev)).clamp(0, 1).requires_grad_(True)
    grads = {}

    def fused_fwd():
        model(pred, gt)

    def fused_loss_fwd():
        model.loss(pred, gt)

    def fused_fwd_bwd():
        (grads["fused"],) = torch.autograd.grad(model.loss(pred, gt).sum(), pred)

    def torch_fwd_bwd():
        (grads["torch"],) = torch.autograd.grad(torch_lpips(pred, gt, weights, biases, heads).float().sum(), pred)

    routes = (("fused_fwd", fused_fwd), ("fused_loss_fwd", fused_loss_fwd), ("fused_fwd_bwd", fused_fwd_bwd),
              ("torch_fwd_bwd", torch_fwd_bwd))
    times = {name: [] for name, _ in routes}
    for r in range(warmup + rounds):
        for name, fn in routes:
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            fn()
            end.record()
            end.synchronize()
            if r >= warmup:
                times[name].append(start.elapsed_time(end))
    fwd, bwd = gemm_flop(B, H, W)
    row = {"pairs": B, "height": H, "width": W, "rounds": rounds, "forward_conv_gflop": fwd / 1e9,
           "backward_gemm_gflop_one_side": bwd / 1e9}
    for name, ts in times.items():
        row[name + "_ms_median"], row[name + "_ms_min"], row[name + "_ms_max"] = statistics.median(ts), min(ts), max(ts)
    row["backward_ms"] = row["fused_fwd_bwd_ms_median"] - row["fused_loss_fwd_ms_median"]
    row["backward_over_forward"] = row["backward_ms"] / row["fused_fwd_ms_median"]
    row["torch_over_fused"] = row["torch_fwd_bwd_ms_median"] / row["fused_fwd_bwd_ms_median"]
    row["largest_gradient_distance_over_largest_magnitude"] = float((grads["torch"] - grads["fused"]).abs().max()
                                                                    / grads["fused"].abs().max())
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [measure(i, a.rounds, a.warmup) for i in range(len(SIZES))]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
