#!/usr/bin/env python
"""Time the three scene-seeding launches (csrc/scene_seed.hip through mobgs_amd.scene_init) on one GPU, beside the torch
composition the package offered before them, on the same device: the V x V loop over deformation.inverse_warp_rt1_rt2
with the masked error, the mean and the threshold; points_from_DRTK per view; cdist-style square().sum().argmin() over the
tracks in ten chunks; grid_sample(mode="nearest") of the point maps.

    python scripts/scene_seed_timing.py [--out profiles/scene_seed_timing.json] [--views 24] [--width 512] [--height 288]

Each figure is the median over `runs` windows of HIP events; a window holds `reps` back-to-back calls and is divided by
`reps` (the classify launch alone takes tens of microseconds, less than an event pair resolves).  The comparison that
counts -- `public_api` against `torch_total` -- alternates the two inside one loop, window by window, so both see the
same machine.  What each side pays for:
  three_launches   the raw C-ABI launches on prepared buffers: no table build, no allocation, no depth check
  public_api       scene_init.seed_maps + track_trajectories as a caller uses them: the float64 pair / unproject tables
                   built on the host and copied, the depth check's read-back, the output allocations, the launches
  torch_total      the torch composition, including its own torch.inverse(K) per call
No input is written, so every repetition sees the same data.  The two results are compared on the way and the script
fails if the track indices differ or the thresholded masks disagree on more than 0.1 % of the pixels (a reprojection
within rounding of a view's border may fall either way).  The workload is synthetic (smooth seeded images, a slanted
plane's depth, cameras on an arc): the kernels' time does not depend on the values, only on how many reprojections land
inside."""
import argparse
import datetime
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mobgs_amd import deformation, scene_init  # noqa: E402


def synthetic_views(V, H, W, M, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    focal = 0.9 * W
    K = torch.tensor([[focal, 0, W / 2 + 0.3], [0, focal, H / 2 - 0.2], [0, 0, 1.0]], dtype=torch.float64)
    n, c = torch.tensor([0.2, -0.1, 1.0], dtype=torch.float64), 0.3
    vv, uu = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    rays = torch.stack([uu, vv, torch.ones_like(uu)], -1).reshape(-1, 3) @ torch.linalg.inv(K).T
    w2c, depths, images = [], [], []
    for i in range(V):
        a = (i - (V - 1) / 2) * 0.02
        eye = torch.tensor([4.2 * math.sin(a), 0.1 * math.cos(2 * a), -4.2 * math.cos(a)], dtype=torch.float64)
        f = -eye / eye.norm()
        r = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), f)
        r = r / r.norm()
        R = torch.stack([r, torch.linalg.cross(f, r), f])
        wr = rays @ R
        d = (c - n @ eye) / (wr @ n)
        X = eye + d[:, None] * wr
        images.append(torch.stack([0.5 + 0.3 * torch.sin(1.7 * X[:, 0] + 0.1 * i), 0.5 + 0.3 * torch.sin(1.3 * X[:, 1]),
                                   0.5 + 0.3 * torch.cos(0.9 * X[:, 0] - 1.6 * X[:, 1])]).reshape(3, H, W))
        depths.append(d.reshape(H, W))
        w2c.append(torch.cat([R, (-R @ eye)[:, None]], 1))
    tracklet = torch.stack([torch.rand(V, M, generator=g) * (W + 8) - 4, torch.rand(V, M, generator=g) * (H + 8) - 4], -1)
    coords = torch.stack([torch.randint(0, W, (N,), generator=g), torch.randint(0, H, (N,), generator=g)], 1).float()
    motion = (torch.rand(V, H, W, generator=g) < 0.1).to(torch.uint8)
    return (torch.stack(images).float(), torch.stack(depths).float(), torch.stack(w2c), K[None].expand(V, 3, 3).contiguous(),
            motion, tracklet.float(), coords)


def torch_maps(images, depths, w2c, K):
    """The composition of train.py:71-113 with the package's torch helpers -> (accum_error, inconsistent, points)."""
    V, _, H, W = images.shape
    Kf, Kinv = K[:1].float(), torch.inverse(K[:1].float())
    accum, inc, pts = [], [], []
    for i in range(V):
        depth = depths[i][None, None]
        acc = 0
        for j in range(V):
            warped = deformation.inverse_warp_rt1_rt2(images[j][None], depth, w2c[i][None], w2c[j][None], Kf, Kinv)
            seen = (torch.sum(warped, dim=1, keepdim=True) > 0).type_as(warped)
            acc = acc + torch.mean(seen * torch.abs(warped - images[i][None]), dim=1, keepdim=True)
        accum.append(acc[0, 0])
        inc.append(acc[0, 0] > torch.mean(acc))
        pts.append(deformation.points_from_DRTK(depth, w2c[i][None], Kf)[0].T.reshape(H, W, 3))
    return torch.stack(accum), torch.stack(inc), torch.stack(pts)


def torch_tracks(coords, tracklet, points):
    V, H, W, _ = points.shape
    maps = points.permute(0, 3, 1, 2)
    chunk = max(1, coords.shape[0] // 10)
    index, traj = [], []
    for a in range(0, coords.shape[0], chunk):
        idx = torch.square(coords[a:a + chunk, None] - tracklet[0][None]).sum(-1).argmin(-1)
        own = tracklet[:, idx, :].clone()[:, None]
        own[..., 0] /= W
        own[..., 1] /= H
        got = F.grid_sample(maps, own * 2 - 1.0, mode="nearest", align_corners=False)
        index.append(idx)
        traj.append(got[:, :, 0, :].permute(2, 0, 1))
    return torch.cat(index), torch.cat(traj)


def _window_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def _stats(ts, reps):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "runs": len(ts), "reps": reps}


def time_ms(fn, runs, warmup, reps=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return _stats([_window_ms(fn, reps) for _ in range(runs)], reps)


def time_alternating(fn_a, fn_b, runs, warmup):
    """(stats of a, stats of b): one window of each in turn."""
    for _ in range(warmup):
        fn_a(), fn_b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(runs):
        ta.append(_window_ms(fn_a, 1))
        tb.append(_window_ms(fn_b, 1))
    return _stats(ta, 1), _stats(tb, 1)


def measure(V=24, H=288, W=512, M=4000, N=10000, runs=20, warmup=3, alt_runs=5):
    dev = torch.device("cuda")
    images, depths, w2c64, K64, motion, tracklet, coords = synthetic_views(V, H, W, M, N)
    images, depths, motion, tracklet, coords = (t.to(dev) for t in (images, depths, motion, tracklet, coords))
    w2c, K = w2c64.float().to(dev), K64.float().to(dev)
    pairs, unproj = scene_init.pair_table(w2c64, K64).to(dev), scene_init.unproject_table(w2c64, K64).to(dev)
    lib = scene_init._lib.load()
    ptr, stream, check = scene_init.ptr, scene_init.stream, scene_init.check
    nbytes = int(lib.mobgs_seed_scratch_bytes(V, H, W))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    accum = torch.empty(V, H, W, device=dev)
    inc, cls = torch.empty(V, H, W, dtype=torch.uint8, device=dev), torch.empty(V, H, W, dtype=torch.uint8, device=dev)
    points, mean = torch.empty(V, H, W, 3, device=dev), torch.empty(V, device=dev)
    index, traj = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, V, 3, device=dev)

    def consistency():
        check(lib.mobgs_seed_consistency(V, H, W, ptr(images), ptr(depths), ptr(pairs), ptr(accum), ptr(scratch), nbytes,
                                         stream()), "mobgs_seed_consistency")

    def classify():
        check(lib.mobgs_seed_classify(V, H, W, ptr(accum), ptr(scratch), nbytes, ptr(depths), ptr(motion), ptr(unproj),
                                      ptr(inc), ptr(cls), ptr(points), ptr(mean), stream()), "mobgs_seed_classify")

    def trajectories():
        check(lib.mobgs_seed_trajectories(N, V, M, V, H, W, ptr(coords), ptr(tracklet), ptr(points), ptr(index),
                                          ptr(traj), stream()), "mobgs_seed_trajectories")

    def kernels():
        consistency(), classify(), trajectories()

    held = {}

    def alt_maps():
        held["maps"] = torch_maps(images, depths, w2c, K)

    def alt_tracks():
        held["tracks"] = torch_tracks(coords, tracklet, points)

    def alt_total():
        alt_maps(), alt_tracks()

    def public_api():
        m = scene_init.seed_maps(images, depths, w2c64, K64, motion)
        held["api"] = (m, scene_init.track_trajectories(coords, tracklet, m.points))

    rec = {"views": V, "height": H, "width": W, "tracks": M, "points": N,
           "mobgs_seed_consistency": time_ms(consistency, runs, warmup, reps=5),
           "mobgs_seed_classify": time_ms(classify, runs, warmup, reps=50),
           "mobgs_seed_trajectories": time_ms(trajectories, runs, warmup, reps=20),
           "three_launches": time_ms(kernels, runs, warmup, reps=5),
           "torch_maps": time_ms(alt_maps, alt_runs, 1), "torch_tracks": time_ms(alt_tracks, alt_runs, 1)}
    rec["public_api"], rec["torch_total"] = time_alternating(public_api, alt_total, alt_runs, 1)
    rec["ratio_torch_over_public_api"] = rec["torch_total"]["median_ms"] / rec["public_api"]["median_ms"]
    rec["ratio_torch_over_three_launches"] = rec["torch_total"]["median_ms"] / rec["three_launches"]["median_ms"]
    acc_t, inc_t, pts_t = held["maps"]
    idx_t, traj_t = held["tracks"]
    rec["max_abs_diff_accum_vs_torch"] = float((accum - acc_t).abs().max())
    rec["mask_disagreements_vs_torch"] = int((inc.bool() != inc_t).sum())
    rec["max_abs_diff_points_vs_torch"] = float((points - pts_t).abs().max())
    rec["track_index_disagreements_vs_torch"] = int((index.long() != idx_t).sum())
    rec["trajectory_rows_differing_vs_torch"] = int((traj != traj_t).any(-1).any(-1).sum())
    api_maps, (api_index, api_traj) = held["api"]
    assert torch.equal(api_maps.accum_error, accum) and torch.equal(api_index, index) and torch.equal(api_traj, traj)
    assert rec["track_index_disagreements_vs_torch"] == 0, rec
    assert rec["mask_disagreements_vs_torch"] <= 1e-3 * inc.numel(), rec
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=288)
    ap.add_argument("--tracks", type=int, default=4000)
    ap.add_argument("--points", type=int, default=10000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    rec = measure(a.views, a.height, a.width, a.tracks, a.points)
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(),
                       "records": [rec]}, f, indent=1)


if __name__ == "__main__":
    main()
