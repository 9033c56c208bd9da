#!/usr/bin/env python
"""Time LPIPS (AlexNet, v0.1) of a batch of image pairs two ways on one device:

  torch   the same computation composed from torch operations on the device in fp32: the scaling layer, F.conv2d + relu,
          F.max_pool2d, the normalisation, the squared difference, the 1x1 head as F.conv2d, the spatial mean
  fused   mobgs_amd.lpips.LpipsAlex(pred, gt): csrc/lpips.hip, 13 launches per chunk of the batch

    python scripts/lpips_timing.py [--rounds 10] [--inner 1] [--warmup 2] [--out FILE.json] [--limit SECONDS]
    python scripts/lpips_timing.py --size 1 --only fused --rounds 2        # one route in this process, for a kernel trace
    python scripts/lpips_timing.py --trace kernel_trace.csv --size 1 --chunk 12   # per-launch times of such a trace
    python scripts/lpips_timing.py --arm spatial [...]                    # the spatial map and the masked averages

Sizes: 24 pairs (one test split) at 512x288 and at 1352x1014; the trunk is the seeded one of tests/lpips_restatement.py
(the speed does not depend on the weights), the heads are the reference's.  Each size is measured in a child process of
its own, started under a time limit; after a child that fails or runs out of time nothing more is started.  Inside a child
the two routes alternate round by round in ONE process: a round is `inner` calls of one route between two device
synchronisations on the host clock, divided by `inner`.  Reported per route: median, min and max over the rounds, the
largest relative distance between the two routes' totals, and the convolutions' FLOP (2 M N K per layer, K unpadded), one
JSON line per size.  --trace reads a kernel trace (CSV with Kernel_Name, Start_Timestamp, End_Timestamp in ns) of a
--only fused run and prints, per kernel of the LAST call, its time and for the five convolutions the achieved fraction of
the 157.3 TF fp32-MFMA peak.

--arm spatial times LpipsAlex.spatial(pred, gt, mask) -- `spatial` with want_map=False, `spatial_map` with want_map=True --
against `torch_spatial`, the same computation composed from torch operations (the torch trunk above, per layer the 1x1
head, F.interpolate(size=, bilinear) and the sum of the five maps, dycheck's masked mean, and per layer the nearest-resized
mask with the reference's masked average), and against `fused`, the plain call, for the increment.  The routes alternate
round by round in one process; --only picks one of them (spatial_map for a kernel trace, which --trace reads as above).

Needs a HIP device for everything but --trace: no fallback."""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((24, 288, 512), (24, 1014, 1352))     # (pairs, H, W)
PEAK_F32_MFMA = 157.3e12
sys.path.insert(0, ROOT)


def conv_flop(pairs, H, W):
    """Per layer: 2 x (output pixels of the 2 x pairs images) x Cout x Cin k k."""
    from mobgs_amd.lpips import CIN, COUT, KS, tap_sizes
    return [2.0 * 2 * pairs * h * w * COUT[l] * CIN[l] * KS[l] ** 2 for l, (h, w) in enumerate(tap_sizes(H, W))]


def torch_lpips(pred, gt, weights, biases, heads):
    import torch
    import torch.nn.functional as F
    shift = torch.tensor([-.030, -.088, -.188], device=pred.device).reshape(1, 3, 1, 1)
    scale = torch.tensor([.458, .448, .450], device=pred.device).reshape(1, 3, 1, 1)
    h = ((2 * torch.cat([gt, pred]) - 1) - shift) / scale
    B = pred.shape[0]
    total = 0
    for l in range(5):
        if l in (1, 2):
            h = F.max_pool2d(h, 3, 2)
        h = torch.relu(F.conv2d(h, weights[l], biases[l], stride=4 if l == 0 else 1, padding=(2, 2, 1, 1, 1)[l]))
        n = h / (torch.sqrt(torch.sum(h * h, dim=1, keepdim=True)) + 1e-10)
        d = (n[:B] - n[B:]) ** 2
        total = total + F.conv2d(d, heads[l]).mean((2, 3)).reshape(-1)
    return total.double()


def torch_spatial(pred, gt, mask, weights, biases, heads):
    """-> (map [B,1,H,W], dycheck's masked mean [B], the reference's masked average per pair [B]), fp32."""
    import torch
    import torch.nn.functional as F
    shift = torch.tensor([-.030, -.088, -.188], device=pred.device).reshape(1, 3, 1, 1)
    scale = torch.tensor([.458, .448, .450], device=pred.device).reshape(1, 3, 1, 1)
    h = ((2 * torch.cat([gt, pred]) - 1) - shift) / scale
    B, _, H, W = pred.shape
    val, total = None, 0
    for l in range(5):
        if l in (1, 2):
            h = F.max_pool2d(h, 3, 2)
        h = torch.relu(F.conv2d(h, weights[l], biases[l], stride=4 if l == 0 else 1, padding=(2, 2, 1, 1, 1)[l]))
        n = h / (torch.sqrt(torch.sum(h * h, dim=1, keepdim=True)) + 1e-10)
        d = F.conv2d((n[:B] - n[B:]) ** 2, heads[l])
        up = F.interpolate(d, size=(H, W), mode="bilinear", align_corners=False)
        val = up if val is None else val + up
        ml = F.interpolate(mask[:, None], size=d.shape[2:])
        total = total + (d * ml).sum((1, 2, 3)) / (ml.sum((1, 2, 3)) + 1e-8)
    masked = (val[:, 0] * mask).sum((1, 2)) / mask.sum((1, 2)).clamp(min=1e-6)
    return val, masked, total


def measure_spatial(index, rounds, inner, warmup, only):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import lpips_restatement as LR
    from mobgs_amd.lpips import LpipsAlex
    if not torch.cuda.is_available():
        raise SystemExit("lpips_timing.py needs a HIP device")
    dev = torch.device("cuda:0")
    B, H, W = SIZES[index]
    trunk, heads_sd = LR.seeded_trunk(), LR.reference_heads()
    model = LpipsAlex(trunk, heads_sd, device=dev)
    weights = [trunk[f"features.{i}.weight"].to(dev) for i in LR.TRUNK_INDEX]
    biases = [trunk[f"features.{i}.bias"].to(dev) for i in LR.TRUNK_INDEX]
    heads = [heads_sd[f"lin{l}.model.1.weight"].to(dev) for l in range(5)]
    g = torch.Generator(device=dev).manual_seed(index)
    gt = torch.rand(B, 3, H, W, generator=g, device=dev)
    pred = (gt + 0.1 * torch.randn(B, 3, H, W, generator=g, device=dev)).clamp(0, 1)
    mask = (torch.rand(B, H, W, generator=g, device=dev) < 0.6).float()
    results = {}

    def torch_route():
        with torch.no_grad():
            results["torch_spatial"] = torch_spatial(pred, gt, mask, weights, biases, heads)

    def spatial_route():
        results["spatial"] = model.spatial(pred, gt, mask, want_map=False)

    def map_route():
        results["spatial_map"] = model.spatial(pred, gt, mask, want_map=True)

    def fused_route():
        results["fused"] = model(pred, gt).total

    routes = [r for r in (("torch_spatial", torch_route), ("spatial", spatial_route), ("spatial_map", map_route),
                          ("fused", fused_route)) if only in (None, r[0])]
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
    row = {"arm": "spatial", "pairs": B, "height": H, "width": W, "rounds": rounds, "inner": inner,
           "pairs_per_chunk": model._chunk(B, H, W, spatial=True)}
    for name, ts in times.items():
        row[name + "_ms_median"], row[name + "_ms_min"], row[name + "_ms_max"] = statistics.median(ts), min(ts), max(ts)
    if only is None:
        for name in ("spatial", "spatial_map"):
            row[f"torch_over_{name}"] = row["torch_spatial_ms_median"] / row[name + "_ms_median"]
            row[f"{name}_minus_plain_ms"] = row[name + "_ms_median"] - row["fused_ms_median"]
        val, masked, total = results["torch_spatial"]
        ours = results["spatial_map"]
        row["largest_relative_distance_masked_mean"] = float(((masked.double() - ours.masked_mean).abs()
                                                              / ours.masked_mean.abs()).max())
        row["largest_relative_distance_masked_total"] = float(((total.double() - ours.masked_total).abs()
                                                               / ours.masked_total.abs()).max())
        row["largest_map_distance_over_map_max"] = float((val - ours.map).abs().max() / ours.map.max())
    print(json.dumps(row), flush=True)


def measure(index, rounds, inner, warmup, only):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import lpips_restatement as LR
    from mobgs_amd.lpips import LpipsAlex
    if not torch.cuda.is_available():
        raise SystemExit("lpips_timing.py needs a HIP device")
    dev = torch.device("cuda:0")
    B, H, W = SIZES[index]
    trunk, heads_sd = LR.seeded_trunk(), LR.reference_heads()
    model = LpipsAlex(trunk, heads_sd, device=dev)
    weights = [trunk[f"features.{i}.weight"].to(dev) for i in LR.TRUNK_INDEX]
    biases = [trunk[f"features.{i}.bias"].to(dev) for i in LR.TRUNK_INDEX]
    heads = [heads_sd[f"lin{l}.model.1.weight"].to(dev) for l in range(5)]
    g = torch.Generator(device=dev).manual_seed(index)
    gt = torch.rand(B, 3, H, W, generator=g, device=dev)
    pred = (gt + 0.1 * torch.randn(B, 3, H, W, generator=g, device=dev)).clamp(0, 1)
    results = {}

    def torch_route():
        with torch.no_grad():
            results["torch"] = torch_lpips(pred, gt, weights, biases, heads)

    def fused_route():
        results["fused"] = model(pred, gt).total

    routes = [r for r in (("torch", torch_route), ("fused", fused_route)) if only in (None, r[0])]
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
    flop = conv_flop(B, H, W)
    row = {"pairs": B, "height": H, "width": W, "rounds": rounds, "inner": inner, "conv_gflop": [f / 1e9 for f in flop],
           "pairs_per_chunk": model._chunk(B, H, W)}
    for name, ts in times.items():
        row[name + "_ms_median"], row[name + "_ms_min"], row[name + "_ms_max"] = statistics.median(ts), min(ts), max(ts)
    if len(routes) == 2:
        row["ratio_of_medians"] = row["torch_ms_median"] / row["fused_ms_median"]
        rel = ((results["torch"] - results["fused"]).abs() / results["fused"].abs()).max()
        row["largest_relative_distance_between_routes"] = float(rel)
    if "fused" in times:
        row["fused_conv_tflops_end_to_end"] = sum(flop) / (row["fused_ms_median"] * 1e-3) / 1e12
        row["fused_first_pairs"] = results["fused"][:3].tolist()
    print(json.dumps(row), flush=True)


def read_trace(path, index, pairs_in_chunk):
    """Per kernel of the last chunk in a kernel trace of a --only fused run (the launches between the last two finishing
    launches): name, microseconds, and for the five convolutions the fraction of the fp32-MFMA peak.  pairs_in_chunk: the
    "pairs_per_chunk" that run printed."""
    B, H, W = SIZES[index]
    with open(path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "lpips_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    finishes = [i for i, r in enumerate(rows) if "finish_kernel" in r["Kernel_Name"]]      # (the plain or the spatial one)
    if not finishes:
        raise SystemExit(f"{path}: no finishing launch")
    last = rows[(finishes[-2] + 1 if len(finishes) > 1 else 0):finishes[-1] + 1]
    flop = conv_flop(pairs_in_chunk, H, W)
    out, layer = [], 0
    for r in last:
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        item = {"kernel": r["Kernel_Name"].split("(")[0], "us": us}
        if "lpips_conv" in item["kernel"]:
            item["layer"], item["gflop"] = layer + 1, flop[layer] / 1e9
            item["fraction_of_fp32_mfma_peak"] = flop[layer] / (us * 1e-6) / PEAK_F32_MFMA
            layer += 1
        out.append(item)
    print(json.dumps({"pairs_in_chunk": pairs_in_chunk, "height": H, "width": W, "launches": out,
                      "chunk_us": sum(i["us"] for i in out)}, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--inner", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds a size may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", type=int, default=None, help="measure SIZES[i] in this process")
    ap.add_argument("--only", choices=("torch", "fused", "torch_spatial", "spatial", "spatial_map"), default=None,
                    help="with --size: one route only")
    ap.add_argument("--arm", choices=("plain", "spatial"), default="plain", help="what to time (see above)")
    ap.add_argument("--trace", default=None, help="a kernel-trace CSV of a `--size i --only fused` run: print its breakdown")
    ap.add_argument("--chunk", type=int, default=None, help="with --trace: pairs per chunk of that run (default: all)")
    a = ap.parse_args()
    if a.trace:
        read_trace(a.trace, a.size or 0, a.chunk or SIZES[a.size or 0][0])
        return
    if a.size is not None:
        (measure_spatial if a.arm == "spatial" else measure)(a.size, a.rounds, a.inner, a.warmup, a.only)
        return
    rows = []
    for i in range(len(SIZES)):
        cmd = [sys.executable, os.path.abspath(__file__), "--size", str(i), "--rounds", str(a.rounds), "--inner",
               str(a.inner), "--warmup", str(a.warmup), "--arm", a.arm]
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
