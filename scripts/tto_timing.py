#!/usr/bin/env python
"""Time one camera's test-time pose refinement (the reference's eval.py:99-150 with its __main__ settings: 100 steps,
decay_start 30, lr 3e-4, lr_final 1e-6) two ways on one device:

  composed  the loop from torch's own parts: the pose matrix and the -PSNR loss from torch ops, render(w2c=...),
            loss.backward(), torch.optim.Adam, CosineAnnealingLR, the loss read back every step -- what a caller could do
            before mobgs_amd.tto existed (of this package it uses render and the plain-torch quaternion_to_matrix)
  fused     mobgs_amd.tto.refine_pose: the same render, the loss kernels, the backward restricted to the pose, one launch
            for head backward + Adam + head forward; the loss history is read back once, after the loop

    python scripts/tto_timing.py [--reps 10] [--warmup 2] [--out FILE.json]

Both start from the same pose against the same ground truth (rendered at a pose 0.5 degrees and 0.005 units away) and are
run alternately, each refinement between two device synchronisations on the host clock; the medians, the quartiles and
both final losses are printed as one JSON line per size.  `render_only` is 100 forward + backward renders with the
gradient of a fixed cotangent and nothing else: what either loop spends inside render(); `forward_only` is the 100 forward
renders under no_grad.  Their difference is the backward pass, which forms every leaf gradient although only the pose's
is kept: the ceiling of what a pose-only backward compositor could save.  Needs a HIP device: there is no CPU path and no fallback."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mobgs_amd.camera import PinholeCamera  # noqa: E402
from mobgs_amd.gaussian_model import GaussianParams  # noqa: E402
from mobgs_amd.gaussian_renderer import render  # noqa: E402
from mobgs_amd.helper_model import Sandwich  # noqa: E402
from mobgs_amd.synth import SynthCamera, dynamic_extras, gaussian_cloud  # noqa: E402
from mobgs_amd.tto import matrix_to_quaternion, quaternion_to_matrix, refine_pose  # noqa: E402

SIZES = ((512, 288, 30000), (1352, 1014, 300000))
MAIN = dict(steps=100, decay_start=30, lr_p=3e-4, lr_q=3e-4, lr_final=1e-6)        # eval.py:257-264


def build(dev, W, H, n_splats):
    scam = SynthCamera().scaled(W, H)
    torch.manual_seed(0)
    dec = Sandwich(9, 3).to(dev)
    ns = n_splats * 2 // 3
    sp, dp = gaussian_cloud(ns, scam, 0), gaussian_cloud(n_splats - ns, scam, 1)
    stat = GaussianParams(sp, None, dec, dev, requires_grad=False)
    dyn = GaussianParams(dp, dynamic_extras(dp["xyz"], 0), dec, dev, requires_grad=False)
    a = math.radians(0.5) / 2
    start = torch.eye(4)
    start[:3, :3] = quaternion_to_matrix(torch.tensor([math.cos(a), 0.0, math.sin(a), 0.0]))
    start[:3, 3] = torch.tensor([0.003, -0.004, 0.0])
    cam = PinholeCamera(W, H, scam.K, start, time=scam.time, max_time=scam.max_time, device=dev)
    return stat, dyn, cam


E33 = None


def pose_from(quat, trans):
    """[4,4] world-to-camera matrix of a quaternion and a translation, differentiable: torch ops only."""
    top = torch.cat((quaternion_to_matrix(quat), trans.unsqueeze(1)), dim=1)
    return torch.nn.functional.pad(top, (0, 0, 0, 1)) + E33


def composed(cam, gt, stat, dyn, bg, q0, t0, steps, decay_start, lr_p, lr_q, lr_final):
    """The refinement from torch's own parts around this project's render: autograd through the pose matrix and the -PSNR
    loss (a difference, a square, a mean, a square root, a reciprocal, a logarithm and a scale: the operations the
    reference's loss consists of), one torch.optim.Adam with a group per pose part, CosineAnnealingLR from decay_start on,
    and the loss read back every step.  -> the losses."""
    quat = q0.detach().clone().requires_grad_(True)
    trans = t0.detach().clone().requires_grad_(True)
    adam = torch.optim.Adam([dict(params=[quat], lr=lr_q), dict(params=[trans], lr=lr_p)])
    cosine = torch.optim.lr_scheduler.CosineAnnealingLR(adam, T_max=steps - decay_start, eta_min=lr_final)
    history = []
    for s in range(steps):
        adam.zero_grad(set_to_none=True)
        image = render(cam, stat, dyn, None, bg, stage="fine", get_static=False, get_dynamic=False,
                       w2c=pose_from(quat, trans))["render"]
        rms = torch.sqrt(torch.square(image - gt).mean())
        loss = -20.0 * torch.log10(rms.reciprocal())
        loss.backward()
        adam.step()
        if s >= decay_start:
            cosine.step()
        history.append(float(loss.detach()))
    return history


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tto_timing.py needs a HIP device")
    dev = torch.device("cuda:0")
    results = []
    for W, H, n_splats in SIZES:
        stat, dyn, cam = build(dev, W, H, n_splats)
        bg = torch.zeros(9, device=dev)
        with torch.no_grad():
            gt = render(cam, stat, dyn, None, bg, w2c=torch.eye(4, device=dev))["render"].clamp(0, 1).contiguous()
        global E33
        E33 = torch.zeros(4, 4, device=dev)
        E33[3, 3] = 1.0
        w2c0 = cam.world_view_transform.transpose(0, 1)
        q0, t0 = matrix_to_quaternion(w2c0[:3, :3]), w2c0[:3, 3].clone()
        cot = torch.randn(3, H, W, device=dev)
        last = {}

        def run_composed():
            last["composed"] = composed(cam, gt, stat, dyn, bg, q0, t0, **MAIN)[-1]

        def run_fused():
            out = refine_pose(cam, gt, stat, dyn, None, bg, q0=q0, t0=t0, **MAIN)
            last["fused"] = out.loss_history.cpu().tolist()[-1]

        def run_render_only():
            leaf = w2c0.clone().requires_grad_(True)
            for _ in range(MAIN["steps"]):
                leaf.grad = None
                render(cam, stat, dyn, None, bg, stage="fine", get_static=False, get_dynamic=False,
                       w2c=leaf)["render"].backward(cot)

        @torch.no_grad()
        def run_forward_only():
            for _ in range(MAIN["steps"]):
                render(cam, stat, dyn, None, bg, stage="fine", get_static=False, get_dynamic=False, w2c=w2c0)

        runs = (("composed", run_composed), ("fused", run_fused), ("render_only", run_render_only),
                ("forward_only", run_forward_only))
        times = {name: [] for name, _ in runs}
        for rep in range(a.warmup + a.reps):
            for name, fn in runs:
                torch.cuda.synchronize()
                t0_ = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    times[name].append((time.perf_counter() - t0_) * 1e3)
        row = {"width": W, "height": H, "splats": n_splats, "reps": a.reps, **{k: v for k, v in MAIN.items()}}
        for name, ts in times.items():
            q = statistics.quantiles(ts, n=4)
            row[name + "_ms_median"], row[name + "_ms_q1"], row[name + "_ms_q3"] = statistics.median(ts), q[0], q[2]
            row[name + "_ms_min"], row[name + "_ms_max"] = min(ts), max(ts)
        row["composed_final_loss"], row["fused_final_loss"] = last["composed"], last["fused"]
        row["speedup"] = row["composed_ms_median"] / row["fused_ms_median"]
        row["render_share_of_fused"] = row["render_only_ms_median"] / row["fused_ms_median"]
        print(json.dumps(row), flush=True)
        results.append(row)
        del stat, dyn
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
