#!/usr/bin/env python
"""Time the two resize routes of TrainableGaussians on one 300 k-row static and one 100 k-row dynamic table:

    existing   densify_pruneclone(...)  then  prune_points((get_opacity < t).squeeze())
    planned    pruneclone_planned(...)  then  prune_opacity_below(t)          (mobgs_densify_plan, include/mobgs_hip.h K34)

    python scripts/densify_timing.py [--ns 300000] [--nd 100000] [--reps 10]

Every repetition starts from a fresh clone of the same table (parameters, Adam moments after one step, statistics that make
about 30 % of the rows hot) and the same seed, so both routes do the same work and leave the same tables (checked).  Per
call: host clock from the call to its return (both routes end after their last read-back; the kernels behind it are still
in flight) and device events around it; the median of the repetitions and their range.  Prints one JSON line per set and
operation."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
from mobgs_amd.densify import TrainableGaussians  # noqa: E402
from mobgs_amd.synth import SynthCamera, dynamic_extras, gaussian_cloud  # noqa: E402
from train_synth import Opt  # noqa: E402

EXTENT, THR, OPTHR = 4.0, 2.0e-4, 0.3


def fresh(params, extras, dev, seed):
    pc = TrainableGaussians(params, extras, device=dev)
    pc.training_setup(Opt())
    g = torch.Generator(device=dev).manual_seed(seed)
    for gr in pc.optimizer.param_groups:
        for p in gr["params"]:
            if p.requires_grad and p.numel():
                p.grad = 0.01 * torch.randn(p.shape, generator=g, device=dev)
    pc.optimizer.step()
    n = pc.get_xyz.shape[0]
    denom = torch.randint(0, 4, (n, 1), generator=g, device=dev).float()
    hot = torch.rand(n, 1, generator=g, device=dev) < 0.3
    pc.xyz_gradient_accum.copy_(torch.where(hot, 2.0, 0.5) * THR * denom)
    pc.denom.copy_(denom)
    # half of the rows above the size threshold, so that both clones and splits happen
    s = pc.table_state()["scaling"]
    s += (torch.log(torch.tensor(pc.percent_dense * EXTENT)) - s.max(dim=1, keepdim=True).values
          + torch.where(torch.rand(n, 1, generator=g, device=dev) < 0.5, 0.5, -0.5))
    torch.cuda.synchronize()
    return pc


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    b.record()
    torch.cuda.synchronize()
    return host, a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, default=300000)
    ap.add_argument("--nd", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    dev = "cuda:0"
    scam = SynthCamera().scaled(640, 360)
    sets = {"static": (gaussian_cloud(a.ns, scam, 0), None)}
    dp = gaussian_cloud(a.nd, scam, 1)
    sets["dynamic"] = (dp, dynamic_extras(dp["xyz"], 0))
    routes = {"existing": (lambda pc: pc.densify_pruneclone(THR, 0.005, EXTENT, 20, splitN=2),
                           lambda pc: pc.prune_points((pc.get_opacity < OPTHR).squeeze())),
              "planned": (lambda pc: pc.pruneclone_planned(THR, EXTENT, splitN=2),
                          lambda pc: pc.prune_opacity_below(OPTHR))}
    for name, (params, extras) in sets.items():
        times = {r: {"pruneclone": [], "prune": []} for r in routes}
        tables = {}
        for rep in range(a.reps + 1):          # repetition 0 warms up (allocator, first launches) and is dropped
            for r, (resize, prune) in routes.items():
                pc = fresh(params, extras, dev, 7)
                torch.manual_seed(11)
                t_resize = timed(lambda: resize(pc))
                rows_mid = pc.get_xyz.shape[0]
                t_prune = timed(lambda: prune(pc))
                if rep:
                    times[r]["pruneclone"].append(t_resize)
                    times[r]["prune"].append(t_prune)
                tables[r] = (rows_mid, {k: v.clone() for k, v in pc.table_state().items()})
                del pc
            same = tables["existing"][0] == tables["planned"][0] and all(
                torch.equal(v, tables["planned"][1][k]) for k, v in tables["existing"][1].items())
            assert same, "the two routes left different tables"
        for op in ("pruneclone", "prune"):
            line = {"set": name, "op": op, "rows_in": a.ns if name == "static" else a.nd,
                    "rows_after_pruneclone": tables["planned"][0], "rows_after_prune": int(tables["planned"][1]["xyz"].shape[0])}
            for r in routes:
                host = [t[0] for t in times[r][op]]
                devt = [t[1] for t in times[r][op]]
                line[r] = {"host_ms_median": round(statistics.median(host), 3), "host_ms_range": [round(min(host), 3), round(max(host), 3)],
                           "event_ms_median": round(statistics.median(devt), 3), "event_ms_range": [round(min(devt), 3), round(max(devt), 3)]}
            print(json.dumps(line))


if __name__ == "__main__":
    main()
