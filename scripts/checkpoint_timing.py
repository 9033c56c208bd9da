#!/usr/bin/env python
"""What one training checkpoint costs (mobgs_amd.checkpoint, include/mobgs_hip.h K29), against the only route there was
before it: table_state() of both sets plus the optimiser and module state dicts, cloned to the CPU and passed to torch.save.

    python scripts/checkpoint_timing.py [--sizes small,full] [--repeats 10] [--dir DIR]

Per operating point (512x288 / 30 k splats and 1352x1014 / 300 k splats, the trainer of examples/train_deblur_synth.py after
two iterations, so that every moment exists) the median of `repeats` saves of
  stream_ms   how long the TRAINING stream is occupied by the save: device events right before and after the snapshot launches,
              recorded by the save itself (checkpoint.TIME_SNAPSHOT) on an idle stream -- it enqueues nothing else there; the
              old route's copies each wait for the stream, so for it this is the host time until the last copy has arrived:
              training cannot go on before
  call_ms     host time of the call (new: save_training_state(blocking=False) returns; old: until torch.save returns)
  file_ms     from the call until the file exists (new: handle.wait())
and one JSON line per point.  The claim to check: the stream is held for the snapshot launches, not for the transfer or the
write, i.e. stream_ms is a small fraction of file_ms on the new route.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
from mobgs_amd import checkpoint  # noqa: E402
from mobgs_amd.checkpoint import save_training_state  # noqa: E402
from train_deblur_synth import DeblurTrainer  # noqa: E402

POINTS = {"small": dict(width=512, height=288, ns=20_000, nd=10_000), "full": dict(width=1352, height=1014, ns=200_000, nd=100_000)}


def old_route(t, path):
    """table_state() + state dicts -> CPU -> torch.save; -> (seconds until the last copy has arrived, seconds until saved)."""
    t0 = time.perf_counter()
    cpu = lambda d: {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in d.items()}  # noqa: E731

    def opt_cpu(o):
        sd = o.state_dict()
        return {"param_groups": sd["param_groups"], "state": {i: cpu(s) for i, s in sd["state"].items()}}
    blob = {"stat": cpu(t.stat.table_state()), "dyn": cpu(t.dyn.table_state()), "decoder": cpu(t.stat.rgbdecoder.state_dict()),
            "blce": cpu(t.blce.state_dict()), "opt": [opt_cpu(o) for o in (t.stat.optimizer, t.dyn.optimizer, t.blce.optimizer)]}
    t1 = time.perf_counter()
    torch.save(blob, path)
    return t1 - t0, time.perf_counter() - t0


def new_route(t, path, it):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    handle = save_training_state(path, stat=t.stat, dyn=t.dyn, blce=t.blce, iteration=it)
    t1 = time.perf_counter()
    handle.result()
    t2 = time.perf_counter()
    begin, end = handle.snapshot_events   # (recorded by the save itself, right before and after its launches)
    return begin.elapsed_time(end) * 1e-3, t1 - t0, t2 - t0


def measure(name, repeats, directory, dev="cuda:0"):
    p = POINTS[name]
    checkpoint.TIME_SNAPSHOT = True
    t = DeblurTrainer(dev, p["ns"], p["nd"], p["width"], p["height"], 2, 0, 0.0, None, 100, False, True)
    for it in (1, 2):
        t.update_learning_rate(it)
        t.iteration()
    t.stat.table_state(), t.dyn.table_state()   # (moments adopted into the tables once, outside the timed region)
    torch.cuda.synchronize()
    new_path, old_path = os.path.join(directory, f"{name}.mobgs"), os.path.join(directory, f"{name}.pt")
    new_route(t, new_path, 2)                   # (first save: staging buffers and descriptors are built)
    old_route(t, old_path)
    new = [new_route(t, new_path, 2) for _ in range(repeats)]
    old = [old_route(t, old_path) for _ in range(repeats)]
    med = lambda rows, i: round(1e3 * statistics.median(r[i] for r in rows), 3)  # noqa: E731
    out = {"point": name, **p, "repeats": repeats, "bytes_new": os.path.getsize(new_path), "bytes_old": os.path.getsize(old_path),
           "new": {"stream_ms": med(new, 0), "call_ms": med(new, 1), "file_ms": med(new, 2)},
           "old": {"stream_ms": med(old, 0), "call_ms": med(old, 1), "file_ms": med(old, 1)}}
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="small,full")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.sizes.split(","):
            measure(name, a.repeats, a.dir or tmp)
