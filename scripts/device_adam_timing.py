#!/usr/bin/env python
"""Host-clock timing of examples/train_deblur_synth.py's loop with the Adam step outside and inside the graph.

    python scripts/device_adam_timing.py [--runs 10] [--iters 50] [--ns 20000 --nd 10000 --width 512 --height 288]

Three arms, each on its own DeblurTrainer of the same seed:
  graph            forward + backward replayed as one graph, fused_adam_step on the host at constant rates: train(graph=True)
                   as it was before DeviceAdam existed, the baseline (it does no schedule work at all)
  graph-optimizer  forward + backward + DeviceAdam.step() in one graph with the schedules on, after_replay() on the host
  eager            no graph; update_learning_rate + fused_adam_step + adjust_lr on the host (what graph-optimizer computes)
A run is `iters` iterations between two device synchronisations, timed with the host clock; the arms ALTERNATE run by run,
so that whatever else the host is doing hits all three alike.  Printed per arm: median and spread (max - min, and the
interquartile range) of the per-iteration time over the runs.  Also printed: the host time of one fused_adam_step call (the
Python walk over the parameter groups the graph-optimizer arm no longer does; host clock around the call, no
synchronisation) and of one after_replay(), and the device time of the two new launches (device events around each, eager).
One JSON line at the end.
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import train_deblur_synth as T  # noqa: E402
from mobgs_amd import _lib  # noqa: E402
from mobgs_amd.graphed import GraphedCallable  # noqa: E402


class Arm:
    def __init__(self, name, a, horizon):
        self.name, self.it = name, 0
        self.scheduled = name != "graph"
        self.t = T.DeblurTrainer(a.dev, a.ns, a.nd, a.width, a.height, 2, 0, 0.0, None, horizon, False, self.scheduled)
        self.fb, self.adam, self.horizon = None, None, horizon
        self.walk = []          # host seconds of the fused_adam_step calls (graph arm)
        self.after = []         # host seconds of the after_replay calls (graph-optimizer arm)

    def iteration(self):
        self.it += 1
        t, it = self.t, self.it
        if self.name != "eager" and it == 2:   # (iteration 1 ran eagerly: arenas and hints exist)
            if self.name == "graph-optimizer":
                self.adam = adam = t.device_adam(first_iteration=it, horizon=self.horizon)

                def forward_backward_step():
                    loss = t.forward_backward()
                    adam.step()
                    return loss
                self.fb = GraphedCallable(forward_backward_step, warmup=0)
            else:
                self.fb = GraphedCallable(t.forward_backward, warmup=0)
        if self.scheduled and self.adam is None:
            t.update_learning_rate(it)
        if self.fb is None:
            t.iteration()
        else:
            self.fb()
            if self.adam is not None:
                t0 = time.perf_counter()
                self.adam.after_replay()
                self.after.append(time.perf_counter() - t0)
            else:
                t0 = time.perf_counter()
                t.optimizer_step()
                self.walk.append(time.perf_counter() - t0)
        if self.scheduled and self.adam is None:
            t.blce.adjust_lr()

    def run(self, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            self.iteration()
        torch.cuda.synchronize()
        seconds = (time.perf_counter() - t0) / iters
        if self.fb is not None and not self.fb.check():
            # the moving scene outgrew an arena (its frames saw empty lists): record again, as the example's loop does, and
            # let the caller repeat the run -- a run with cheap frames in it is not a measurement
            if self.adam is not None:
                self.adam.rebuild()
            self.fb.recapture()
            return None
        return seconds


def spread(xs):
    q = statistics.quantiles(xs, n=4)
    return {"median_ms": 1e3 * statistics.median(xs), "min_ms": 1e3 * min(xs), "max_ms": 1e3 * max(xs),
            "range_ms": 1e3 * (max(xs) - min(xs)), "iqr_ms": 1e3 * (q[2] - q[0])}


def new_launch_times(adam, reps=20):
    """Device events around each of the two launches, eager, on the plan of the graph-optimizer arm (steps its parameters
    with the gradients of the last iteration: call it last)."""
    lib, s = _lib.load(), _lib.stream()
    n = len(adam._plan)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for e in ev:
        e[0].record()
        _lib.check(lib.mobgs_adam_dev_factors(n, adam._sched_dev.data_ptr(), adam._counters.data_ptr(),
                                              adam._factors.data_ptr(), s), "mobgs_adam_dev_factors")
        e[1].record()
        _lib.check(lib.mobgs_adam_dev_step(n, adam._tensor_dev.data_ptr(), adam._factors.data_ptr(), adam._longest, s),
                   "mobgs_adam_dev_step")
        e[2].record()
    torch.cuda.synchronize()
    return (1e3 * statistics.median(e[0].elapsed_time(e[1]) for e in ev),
            1e3 * statistics.median(e[1].elapsed_time(e[2]) for e in ev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--ns", type=int, default=20000)
    ap.add_argument("--nd", type=int, default=10000)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=288)
    ap.add_argument("--dev", default="cuda:0")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("device_adam_timing.py needs a HIP device: a host clock without one measures nothing")
    reps = 20
    horizon = a.warmup + 4 * a.runs * a.iters + reps + 2
    arms = [Arm(n, a, horizon) for n in ("graph", "graph-optimizer", "eager")]
    for arm in arms:
        arm.run(a.warmup)
        arm.walk.clear()
        arm.after.clear()
    gc.collect()
    gc.freeze()
    times = {arm.name: [] for arm in arms}
    for r in range(a.runs):
        for arm in arms:
            for attempt in range(4):
                seconds = arm.run(a.iters)
                if seconds is not None:
                    break
                print(f"run {r:2d}  {arm.name}: an arena overflowed, recorded again, run repeated", flush=True)
            else:
                raise RuntimeError(f"{arm.name}: four runs in a row outgrew an arena")
            times[arm.name].append(seconds)
        print(f"run {r:2d}  " + "  ".join(f"{arm.name} {1e3 * times[arm.name][-1]:.3f} ms" for arm in arms), flush=True)
    out = {"what": "device_adam_timing", "width": a.width, "height": a.height, "ns": a.ns, "nd": a.nd, "runs": a.runs,
           "iters": a.iters, "arms": {k: spread(v) for k, v in times.items()}}
    base, new = out["arms"]["graph"], out["arms"]["graph-optimizer"]
    out["graph_optimizer_minus_graph_ms"] = new["median_ms"] - base["median_ms"]
    out["within_baseline_spread"] = bool(new["median_ms"] <= base["median_ms"] + base["range_ms"])
    out["host_fused_adam_step_us"] = 1e6 * statistics.median(arms[0].walk)
    out["host_after_replay_us"] = 1e6 * statistics.median(arms[1].after)
    out["planned_tensors"] = len(arms[1].adam._plan)
    f_us, s_us = new_launch_times(arms[1].adam, reps)
    out["adam_dev_factors_kernel_us"], out["adam_dev_step_kernel_us"] = f_us, s_us
    for k, v in out["arms"].items():
        print(f"{k:16s} median {v['median_ms']:.3f} ms / iteration   range {v['range_ms']:.3f}   iqr {v['iqr_ms']:.3f}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
