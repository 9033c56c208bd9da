"""Generate tests/golden/seed.npz by RUNNING THE REFERENCE'S OWN scene.deformation.inverse_warp_rt1_rt2 and
points_from_DRTK on CPU, in the container that holds the reference.

    python tests/golden/make_golden_seed.py

The reference's scene_initialization (train.py:58-199) itself cannot be called here: `train` does not import under
ref_harness (it pulls Scene, the dataset readers and the cameras module).  So this script runs the loop of that function
over the reference's two geometry functions -- every view warped into every view, the masked error, the threshold at the
view's mean, the unprojection, the selection with a seeded `random`, the chunked argmin over the tracks and the
nearest grid_sample -- with the same torch calls in fp32, and stores what comes out.

The fixture holds data only: the inputs (images, depths, poses, masks, tracks), the reference's fp32 accum_error,
means, masks, picks, point clouds and trajectories, the same quantities from the float64 restatement
tests/seed_restatement.py, and the gaps between the two (`ref_gaps`), the reference's own noise floor; the GPU tests
allow 3 x it."""
from __future__ import annotations

import math
import os
import random
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_harness as RH  # noqa: E402
from helpers import save_npz  # noqa: E402
import seed_restatement as SR  # noqa: E402

V, H, W, FOCAL = 6, 48, 80, 70.0
CX, CY = W / 2 + 0.3, H / 2 - 0.2
M, STAT_NPTS, DYN_NPTS, SEED = 1500, 2000, 300, 733
YAW_STEP, RADIUS = 0.06, 4.2
PLANE_N, PLANE_C = np.array([0.22, -0.12, 1.0]), 0.3          # the plane n . X = c, slanted against every camera
DISC_R, DISC_START, DISC_STEP = 0.42, np.array([-0.95, 0.12]), np.array([0.36, -0.05])
DISC_COLOUR = np.array([0.95, 0.12, 0.10])


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    f = (target - eye) / np.linalg.norm(target - eye)
    r = np.cross(up, f)
    r /= np.linalg.norm(r)
    u = np.cross(f, r)
    R = np.stack([r, u, f])
    return R, -R @ eye


def plane_z(x, y):
    return (PLANE_C - PLANE_N[0] * x - PLANE_N[1] * y) / PLANE_N[2]


def texture(x, y):
    """Strictly positive and smooth, in [0.2, 0.8]."""
    return np.stack([0.5 + 0.3 * np.sin(1.7 * x + 0.4) * np.cos(1.1 * y),
                     0.5 + 0.3 * np.sin(1.3 * y - 0.7 + 0.5 * x),
                     0.5 + 0.3 * np.cos(0.9 * x - 1.6 * y + 0.2)], 0)


def disc_centre(i):
    return DISC_START + i * DISC_STEP


def project(Rw, tw, X):
    cam = X @ Rw.T + tw
    return np.stack([FOCAL * cam[:, 0] / cam[:, 2] + CX, FOCAL * cam[:, 1] / cam[:, 2] + CY], 1)


def scene():
    Kinv = np.linalg.inv(np.array([[FOCAL, 0, CX], [0, FOCAL, CY], [0, 0, 1.0]]))
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = np.stack([uu, vv, np.ones_like(uu)], -1).reshape(-1, 3) @ Kinv.T
    images, depths, masks, Rs, Ts = [], [], [], [], []
    for i in range(V):
        a = (i - (V - 1) / 2) * YAW_STEP
        eye = np.array([RADIUS * math.sin(a), 0.15 * math.cos(2.0 * a) - 0.1, -RADIUS * math.cos(a)])
        Rw, tw = look_at(eye, (0.05, 0.0, plane_z(0.05, 0.0)))
        wr = rays @ Rw                                               # world ray of every pixel (R^T applied)
        d = (PLANE_C - PLANE_N @ eye) / (wr @ PLANE_N)               # z-depth: the camera ray has z = 1
        X = eye + d[:, None] * wr
        c = disc_centre(i)
        on_disc = (X[:, 0] - c[0]) ** 2 + (X[:, 1] - c[1]) ** 2 < DISC_R ** 2
        col = texture(X[:, 0], X[:, 1])
        col[:, on_disc] = DISC_COLOUR[:, None]
        images.append(col.reshape(3, H, W))
        depths.append(d.reshape(H, W))
        masks.append(on_disc.reshape(H, W))
        Rs.append(Rw)
        Ts.append(tw)
    f = lambda a: np.stack(a).astype(np.float32)  # noqa: E731
    return f(images), f(depths), np.stack(masks).astype(np.uint8), f(Rs), f(Ts)


def make_tracks(Rs, Ts, rng):
    """[V,M,2] float32 pixel tracks of points on the plane: a third starts inside the disc of view 0 and moves with it,
    the rest is still; a band near the right edge and a quarter of the disc tracks leave the image in later frames."""
    xy = np.stack([rng.uniform(-2.6, 2.6, M), rng.uniform(-1.6, 1.6, M)], 1)
    n_disc = M // 3
    ang, rad = rng.uniform(0, 2 * math.pi, n_disc), DISC_R * np.sqrt(rng.uniform(0, 1, n_disc))
    xy[:n_disc] = disc_centre(0) + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    order = rng.permutation(M)
    xy, moving = xy[order], (np.arange(M) < n_disc)[order]
    drifting = (~moving) & (xy[:, 0] > 1.6)
    leaving = moving & (np.arange(M) % 4 == 0)                       # disc tracks that run off the top of the image
    tracks = np.empty((V, M, 2))
    for t in range(V):
        p = xy + np.where(moving[:, None], t * DISC_STEP, 0.0) + np.where(drifting[:, None], t * np.array([0.3, 0.0]), 0.0) \
            + np.where(leaving[:, None], t * np.array([0.0, -0.45]), 0.0)
        X = np.concatenate([p, plane_z(p[:, 0], p[:, 1])[:, None]], 1)
        tracks[t] = project(Rs[t].astype(np.float64), Ts[t].astype(np.float64), X)
    return tracks.astype(np.float32), moving


def keep_off_half_way(tracks):
    """No coordinate within 2e-3 of an integer: nearbyint(u - 0.5) is then the same pixel in every precision."""
    near = np.abs(tracks - np.rint(tracks)) < 2e-3
    return np.where(near, tracks + np.float32(5e-3), tracks).astype(np.float32)


def reference_run(ref, images, depths, masks, Rs, Ts, tracklet):
    """The loop of train.py:68-189 over the reference's inverse_warp_rt1_rt2 / points_from_DRTK, fp32 on CPU."""
    T_ = torch.from_numpy
    K = torch.tensor([[[FOCAL, 0, CX], [0, FOCAL, CY], [0, 0, 1.0]]], dtype=torch.float32)
    w2c = [torch.cat((T_(Rs[i])[None], T_(Ts[i])[None, :, None]), -1) for i in range(V)]
    accums, means, incs, points = [], [], [], []
    for i in range(V):
        image, depth = T_(images[i])[None], T_(depths[i])[None, None]
        acc = 0
        for j in range(V):
            warped, _ = ref.inverse_warp_rt1_rt2(T_(images[j])[None], depth, w2c[i], w2c[j], K, torch.inverse(K),
                                                 ret_grid=True)
            seen = (torch.sum(warped, dim=1, keepdim=True) > 0).type_as(warped)
            acc = acc + torch.mean(seen * torch.abs(warped - image), dim=1, keepdim=True)
        mean = torch.mean(acc)
        accums.append(acc[0, 0].numpy())
        means.append(float(mean))
        incs.append((acc > mean)[0, 0].numpy())
        points.append(ref.points_from_DRTK(depth, w2c[i], K)[0].T.reshape(H, W, 3).numpy())
    accum, inc, pts = np.stack(accums), np.stack(incs), np.stack(points)
    motion = masks.astype(bool)
    stat_at = np.flatnonzero((~inc & ~motion).reshape(-1))
    dyn_at = np.flatnonzero((inc[0] & motion[0]).reshape(-1))
    random.seed(SEED)
    if len(dyn_at) < DYN_NPTS:
        dyn_idx = random.choices(range(len(dyn_at)), k=DYN_NPTS)
    else:
        dyn_idx = random.sample(range(len(dyn_at)), DYN_NPTS)
    stat_idx = random.sample(range(len(stat_at)), STAT_NPTS)
    return {"accum": accum, "mean": np.array(means, np.float32), "inc": inc.astype(np.uint8), "points": pts,
            "stat_idx": np.array(stat_idx, np.int64), "dyn_idx": np.array(dyn_idx, np.int64), "n_dyn": len(dyn_at)}


def reference_tracks(coords, tracklet, points):
    """train.py:171-189: the argmin over the tracks in ten chunks and the nearest grid_sample, fp32."""
    tr = torch.from_numpy(tracklet)
    maps = torch.from_numpy(points).permute(0, 3, 1, 2)
    chunk = coords.shape[0] // 10
    index, traj = [], []
    for a in range(0, coords.shape[0], chunk):
        c = torch.from_numpy(coords[a:a + chunk])
        idx = torch.square(c[:, None] - tr[0][None]).sum(-1).argmin(-1)
        own = tr[:, idx, :].clone()[:, None]                          # [T,1,n,2]
        own[..., 0] /= W
        own[..., 1] /= H
        got = F.grid_sample(maps, own * 2 - 1.0, mode="nearest", align_corners=False)   # [T,3,1,n]
        index.append(idx)
        traj.append(got[:, :, 0, :].permute(2, 0, 1))
    return torch.cat(index).numpy(), torch.cat(traj).numpy()


def main():
    ref = RH.ref_import("scene.deformation")
    rng = np.random.default_rng(SEED)
    images, depths, masks, Rs, Ts = scene()
    times = (np.arange(V) / (V - 1.0)).astype(np.float32)
    tracklet, moving = make_tracks(Rs, Ts, rng)
    w2c = np.concatenate([Rs, Ts[:, :, None]], -1)
    K = np.tile(np.array([[FOCAL, 0, CX], [0, FOCAL, CY], [0, 0, 1.0]]), (V, 1, 1))
    with RH.CudaToCpu():
        r = reference_run(ref, images, depths, masks, Rs, Ts, tracklet)
    assert r["n_dyn"] < DYN_NPTS, r["n_dyn"]                         # the with-replacement branch
    ref_cls = np.full(masks.shape, 2, np.uint8)
    ref_cls[(r["inc"] == 0) & (masks == 0)] = 0
    ref_cls[(r["inc"] == 1) & (masks == 1)] = 1
    rc = SR.clouds(images, r["points"], ref_cls, times, r["stat_idx"], r["dyn_idx"])

    # ---- planted ties: two picked pixels, each with two tracks at exactly the same distance, all others further away
    picked = np.unique(rc["dyn_coords"], axis=0)
    pa, pb = picked[len(picked) // 3], picked[2 * len(picked) // 3]
    assert np.abs(pa - pb).max() >= 3
    for p in (pa, pb):
        crowd = ((tracklet[0] - p) ** 2).sum(-1) < 1.0
        tracklet[0, crowd, 0] += 1.5                                  # nobody else within 1 px of a planted pixel
    planted = {"tie_a": (10, 700, np.array([0.25, 0.0], np.float32)), "tie_b": (900, 40, np.array([0.0, 0.25], np.float32))}
    for (m0, m1, off), p in zip(planted.values(), (pa, pb)):
        step = tracklet[:, m0] - tracklet[0, m0]
        tracklet[:, m0] = p + off + step
        tracklet[:, m1] = p - off + step
    tracklet = keep_off_half_way(tracklet)
    ref_index, ref_traj = reference_tracks(rc["dyn_coords"], tracklet, r["points"])

    # ---- float64 restatement ------------------------------------------------------------------------------------------
    accum64, mean64, near = SR.consistency(images, depths, w2c, K)
    inc64, cls64 = SR.classify(accum64, mean64, masks)
    pts64 = SR.world_points(depths, w2c, K)
    index64, pixel64 = SR.track_lookup(rc["dyn_coords"], tracklet, H, W)
    traj64 = SR.gather_trajectory(pts64, pixel64)
    c64 = SR.clouds(images, pts64, cls64, times, r["stat_idx"], r["dyn_idx"])

    # ---- what the fixture must cover, and the reference's own noise floor ----------------------------------------
    gap_accum = float(np.abs(r["accum"] - accum64)[~near].max())
    gap_mean = float(np.abs(r["mean"] - mean64).max())
    gap_points = float(np.abs(r["points"] - pts64).max())
    skipped = float(near.mean())
    margin = 3 * gap_accum + 3 * gap_mean
    close_to_thr = np.abs(accum64 - mean64[:, None, None]) <= margin
    flips = int(((r["inc"] != inc64) & ~close_to_thr & ~near).sum())
    assert skipped <= 0.01, skipped
    assert flips == 0 and float(close_to_thr.mean()) <= 1e-3, (flips, float(close_to_thr.mean()))
    assert np.array_equal(ref_cls, cls64), int((ref_cls != cls64).sum())   # the picks index the same candidate lists
    assert np.array_equal(ref_index, index64)
    for (m0, m1, _), p in zip(planted.values(), (pa, pb)):
        dd = np.sort(((tracklet[0] - p) ** 2).sum(-1))
        rows = (rc["dyn_coords"] == p).all(1)
        assert dd[0] == dd[1] < dd[2] and rows.any() and (index64[rows] == min(m0, m1)).all(), (m0, m1)
    left = (pixel64 < 0)
    assert left.any() and not left[:, 0].any() and (pixel64 >= 0).all(1).any()
    assert np.array_equal(ref_traj, SR.gather_trajectory(r["points"], pixel64))     # a pure gather: bit-equal
    assert float(np.abs(ref_traj - traj64).max()) <= gap_points
    inconsistent_share = float(inc64.mean())
    assert 0.04 <= inconsistent_share <= 0.30, inconsistent_share
    assert images.min() > 0.05 and depths.min() > 1.0

    out = {"images": images, "depths": depths, "masks": masks, "R": np.ascontiguousarray(Rs.transpose(0, 2, 1)), "T": Ts,
           "intrinsics": np.array([FOCAL, CX, CY], np.float64), "times": times, "tracklet": tracklet,
           "npts": np.array([STAT_NPTS, DYN_NPTS], np.int64),
           "stat_idx": r["stat_idx"], "dyn_idx": r["dyn_idx"], "planted": np.array([[10, 700], [40, 900]], np.int64),
           "ref_accum": r["accum"], "ref_mean": r["mean"], "ref_inconsistent": r["inc"], "ref_cls": ref_cls,
           "ref_track_index": ref_index.astype(np.int64), "ref_traj": ref_traj,
           "f64_accum": accum64, "f64_mean": mean64, "f64_traj": traj64,
           "ref_gaps": np.array([gap_accum, gap_mean, gap_points], np.float64)}
    out.update({"ref_" + k: v for k, v in rc.items()})
    out.update({"f64_" + k: v for k, v in c64.items() if k.endswith("points")})
    path = os.path.join(HERE, "seed.npz")
    files = save_npz(path, out)
    sizes = [os.path.getsize(f) for f in files]
    print(f"wrote {', '.join(files)}  ({sum(sizes) / 1024:.0f} KiB, {len(out)} arrays)")
    assert max(sizes) <= 1024 * 1024
    print(f"views {V}, {H} x {W}, tracks {M}; inconsistent {inconsistent_share:.1%}; static candidates "
          f"{int((cls64 == 0).sum())}, dynamic candidates in view 0: {r['n_dyn']}; tracks outside in some frame: "
          f"{int(left.any(1).sum())} of {len(index64)} picked")
    print(f"reference fp32 vs float64: accum_error max |diff| = {gap_accum:.3e} (values up to {accum64.max():.2f}), mean "
          f"{gap_mean:.3e}, points {gap_points:.3e} (coordinates up to {np.abs(pts64).max():.2f}); pixels near a border "
          f"(skipped) {skipped:.2%}; mask flips outside the margin {flips}; pixels within the margin of their threshold "
          f"{float(close_to_thr.mean()):.3%}")


if __name__ == "__main__":
    main()
