#!/usr/bin/env python
"""Time the exposure-time estimate of one view (the reference's train.py:474-492) two ways on one device:

  old   two get_flow_static calls, then torch.norm-free magnitudes, torch.quantile, the boolean-mask gather (a host
        synchronisation), torch.median and the store into exposure_time_expo -- what a caller could do before
        blceKernel.estimate_exposure_time existed
  new   blceKernel.estimate_exposure_time: one projection batch, one 4-channel pass, the selection kernels
        (csrc/exposure.hip), the store on the device

    python scripts/exposure_timing.py [--reps 30] [--warmup 5] [--out FILE.json]

Both routes get the same cameras (the latent pair is handed in, so the BLCE forward is in neither figure) and are run
alternately, each repetition between two device synchronisations on the host clock; the medians, the quartiles and the
two results are printed as one JSON line per size.  Needs a HIP device: there is no CPU path and no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mobgs_amd.blce import blceKernel  # noqa: E402
from mobgs_amd.camera import PinholeCamera  # noqa: E402
from mobgs_amd.gaussian_model import GaussianParams  # noqa: E402
from mobgs_amd.gaussian_renderer import get_flow_static  # noqa: E402
from mobgs_amd.helper_model import Sandwich  # noqa: E402
from mobgs_amd.synth import SynthCamera, dynamic_extras, gaussian_cloud  # noqa: E402

SIZES = ((512, 288, 30000), (1352, 1014, 300000))


def build(dev, W, H, n_splats):
    scam = SynthCamera().scaled(W, H)
    torch.manual_seed(0)
    dec = Sandwich(9, 3).to(dev)
    ns = n_splats * 2 // 3
    sp, dp = gaussian_cloud(ns, scam, 0), gaussian_cloud(n_splats - ns, scam, 1)
    stat = GaussianParams(sp, None, dec, dev, requires_grad=False)
    dyn = GaussianParams(dp, dynamic_extras(dp["xyz"], 0), dec, dev, requires_grad=False)

    def cam(f, uid):
        w2c = torch.eye(4)
        w2c[:3, 3] = f * torch.tensor([0.04, -0.02, 0.03])
        c = PinholeCamera(W, H, scam.K, w2c, time=scam.time, max_time=scam.max_time, device=dev)
        c.uid = uid
        return c
    return stat, dyn, {"bwd": cam(-1.0, 0), "view": cam(0.0, 1), "fwd": cam(1.0, 2), "start": cam(-0.35, 1),
                       "end": cam(0.3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exposure_timing.py needs a HIP device")
    dev = torch.device("cuda:0")
    results = []
    for W, H, n_splats in SIZES:
        stat, dyn, c = build(dev, W, H, n_splats)
        bg = torch.zeros(9, device=dev)
        kernel = blceKernel(num_views=3, num_warp=9).to(dev)
        expo = kernel.model.exposure_time_expo
        warped = [c["start"]] + [None] * 7 + [c["end"]]

        @torch.no_grad()
        def old():
            cf = get_flow_static(c["bwd"], c["fwd"], c["view"], stat, dyn, None, bg)[1]
            lf = get_flow_static(c["start"], c["end"], c["view"], stat, dyn, None, bg)[1]
            cm = torch.sqrt(cf[..., 0] * cf[..., 0] + cf[..., 1] * cf[..., 1])
            lm = torch.sqrt(lf[..., 0] * lf[..., 0] + lf[..., 1] * lf[..., 1])
            valid = cm > torch.quantile(cm, 0.01)
            kernel.model.update_exposure_time(1, torch.median(lm[valid] / cm[valid]))

        @torch.no_grad()
        def new():
            kernel.estimate_exposure_time(c["view"], c["bwd"], c["fwd"], stat, dyn, None, bg, warped_cams=warped)

        times = {"old": [], "new": []}
        values = {}
        for rep in range(a.warmup + a.reps):
            for name, fn in (("old", old), ("new", new)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    times[name].append((time.perf_counter() - t0) * 1e3)
                values[name] = float(expo[1])
        row = {"width": W, "height": H, "splats": n_splats, "reps": a.reps}
        for name, ts in times.items():
            q = statistics.quantiles(ts, n=4)
            row[name + "_ms_median"], row[name + "_ms_q1"], row[name + "_ms_q3"] = statistics.median(ts), q[0], q[2]
            row[name + "_value"] = values[name]
        row["speedup"] = row["old_ms_median"] / row["new_ms_median"]
        print(json.dumps(row), flush=True)
        results.append(row)
        del stat, dyn, kernel
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
