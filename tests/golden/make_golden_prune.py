"""Generate tests/golden/prune.npz by RUNNING THE REFERENCE'S OWN GaussianModel.inverse_cubic_hermite_for_prune,
compute_prune_error and onedown_control_pts (scene/gaussian_model.py:274-371) on CPU, in the container that holds the
reference.

    python tests/golden/make_golden_prune.py

The fixture holds data only: the inputs (control points, counts, cameras), what the reference's fp32 code made of them
(the refitted control points, the pixel errors, the keep / prune decisions, the counts after its commit) and the same
quantities from the float64 restatement tests/prune_restatement.py.  The gap between the two is the reference's own
noise floor; it is printed, stored, and the tests allow 3 x it.
"""
from __future__ import annotations

import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_harness as RH  # noqa: E402
from helpers import save_npz  # noqa: E402
import prune_restatement as PR  # noqa: E402

N, V, SEED = 1000, 24, 131
W, H, FOCAL = 640, 480, 520.0
THRESHOLD = 1.0


def look_at(eye, target, up=(0.0, 1.0, 0.0)) -> torch.Tensor:
    """World-to-camera matrix (column vectors, +z forward) of a camera at `eye` looking at `target`."""
    eye, target, up = (torch.tensor(v, dtype=torch.float64) for v in (eye, target, up))
    f = (target - eye) / (target - eye).norm()
    r = torch.linalg.cross(up, f)
    r = r / r.norm()
    u = torch.linalg.cross(f, r)
    R = torch.stack([r, u, f])
    M = torch.eye(4, dtype=torch.float64)
    M[:3, :3] = R
    M[:3, 3] = -R @ eye
    return M.float()


def scene():
    """Seeded: counts over all of 4..12 (the first nine rows pin one of each), trajectories from nearly straight to
    strongly oscillating, sampled at each row's own knot times and stored x 100 like control_xyz; unused slots hold
    zeros, or arbitrary finite numbers in every eighth row (the fit has to mask them).  24 cameras on an arc around a
    scene centre that is NOT the world origin, every one several units away from the origin."""
    g = torch.Generator().manual_seed(SEED)
    num = torch.randint(4, 13, (N,), generator=g)
    num[:9] = torch.arange(4, 13)
    centre = torch.tensor([4.0, -1.5, 6.0])
    base = centre + 1.2 * torch.randn(N, 3, generator=g)
    amp = 10.0 ** (-2.8 + 2.8 * torch.rand(N, 1, 1, generator=g))            # 1.6e-3 .. 1 world units
    freq = 0.4 + 2.6 * torch.rand(N, 1, 3, generator=g)
    phase = 6.2831853 * torch.rand(N, 1, 3, generator=g)
    drift = 0.3 * torch.randn(N, 1, 3, generator=g)
    k = torch.arange(12, dtype=torch.float32)[None, :, None]
    t = k / (num[:, None, None] - 1).float()
    pos = base[:, None, :] + drift * t + amp * torch.sin(6.2831853 * freq * t + phase)
    control = (pos * 100.0).float()
    unused = (k >= num[:, None, None]).expand(-1, -1, 3)
    junk = 300.0 * torch.randn(N, 12, 3, generator=g)
    junk[torch.arange(N) % 8 != 0] = 0.0
    control = torch.where(unused, junk, control)
    cams, times = [], []
    for v in range(V):
        a = -0.9 + 1.8 * v / (V - 1)
        eye = (float(centre[0]) + 7.5 * math.sin(a), float(centre[1]) + 0.8 * math.cos(3.0 * a),
               float(centre[2]) + 7.5 * math.cos(a))
        cams.append(look_at(eye, tuple(float(x) for x in centre)))
        times.append(v / (V - 1.0))
    tt = torch.tensor(times, dtype=torch.float32)
    tt[1:-1] = (tt[1:-1] + 0.015 * torch.randn(V - 2, generator=g)).clamp(0.01, 0.99)
    return control, num.reshape(N, 1), torch.stack(cams), tt


def viewpoints(w2c, times):
    md = types.SimpleNamespace(focal_length=FOCAL)
    return [types.SimpleNamespace(metadata=md, image_width=W, image_height=H, time=float(times[v]),
                                  world_view_transform=w2c[v].transpose(0, 1).contiguous()) for v in range(len(times))]


def main():
    gm = RH.ref_import("scene.gaussian_model")
    control, num, w2c, times = scene()
    vps = viewpoints(w2c, times)
    assert min(float(c[:3, 3].norm()) for c in torch.linalg.inv(w2c)) > 3.0   # every camera away from the origin
    out = {"control_xyz": control.numpy(), "control_num": num.numpy(), "w2c": w2c.numpy(), "times": times.numpy(),
           "intrinsics": np.array([FOCAL, W, H, THRESHOLD], dtype=np.float64)}
    with RH.CudaToCpu():
        pc = gm.GaussianModel(0, RH.Args())
        pc.control_xyz = control.clone()
        pc.current_control_num = num.clone()
        # the reference's own steps (:275-286), each through its own function
        step = torch.arange(0, pc.control_num, 1).float()[None].repeat(N, 1)
        t_step = (step * (1 / (num.squeeze(-1) - 1.0))[..., None])[..., None]
        new_num = num - 1
        new_num[new_num < 4] = 4
        value = pc.inverse_cubic_hermite_for_prune(pc.control_xyz, t_step, N_pts=new_num)
        new_pts = pc.control_xyz.clone()
        new_pts[:, :pc.control_num - 1] = value
        err = pc.compute_prune_error(new_pts, new_num, vps)
        pc.onedown_control_pts(vps)   # ... and the method itself, for the committed state
    out.update({"ref_new": value.numpy(), "ref_err": err.numpy(), "ref_prune": (err <= THRESHOLD).numpy(),
                "ref_num_after": pc.current_control_num.numpy()})
    assert torch.equal(pc.current_control_num, torch.where((err <= THRESHOLD)[:, None], new_num, num))

    new64, num64 = PR.one_down_f64(control, num)
    err64 = PR.prune_error_f64(control, num, new64, num64, w2c, times, FOCAL, W / 2, H / 2)
    out.update({"f64_new": new64.numpy(), "f64_err": err64.numpy()})

    # ---- what the fixture must cover -------------------------------------------------------------------------------
    n = num.reshape(-1)
    cand = n >= 5
    assert sorted(set(n.tolist())) == list(range(4, 13))
    within = float((err64[cand] <= THRESHOLD).double().mean())
    assert 0.30 <= within <= 0.70, within
    assert int((err64 > 5.0).sum()) >= 10
    assert bool(torch.isfinite(value).all()) and bool(torch.isfinite(err).all())
    # count 4: the reference's fit moves these rows (the upstream defect); the restatement leaves them alone
    four = n == 4
    moved = (value[four, :4].double() - control[four, :4].double()).abs().max()
    assert float(moved) > 1.0 and float(err[four].max()) > 0.1, (float(moved), float(err[four].max()))
    assert bool((err64[four] == 0).all()) and torch.equal(new64[four, :4], control[four, :4].double())

    # ---- the reference's own noise floor: fp32 against float64, rows with count >= 5 ---------------------------
    scale = float(control.abs().max())
    gap_new = float((value.double() - new64)[cand].abs().max())
    own = new64[cand].abs().reshape(int(cand.sum()), -1).max(1).values
    gap_rel = float(((value.double() - new64)[cand].abs().reshape(int(cand.sum()), -1).max(1).values / own).max())
    gap_err = float((err.double() - err64)[cand].abs().max())
    margin = 3 * gap_err
    near = (err64 - THRESHOLD).abs() <= margin
    flips = int((((err <= THRESHOLD) != (err64 <= THRESHOLD)) & cand & ~near).sum())
    skipped = float((near & cand).double().sum() / cand.double().sum())
    assert flips == 0 and skipped <= 0.02, (flips, skipped)
    out["ref_gaps"] = np.array([gap_new, gap_rel, gap_err], dtype=np.float64)
    path = os.path.join(HERE, "prune.npz")
    files = save_npz(path, out)
    size = sum(os.path.getsize(f) for f in files)
    print(f"wrote {', '.join(files)}  ({size / 1024:.0f} KiB, {len(out)} arrays)")
    assert len(files) == 1 and size <= os.path.getsize(os.path.join(HERE, "init.npz"))
    print(f"rows {N} ({int(cand.sum())} with count >= 5), views {V}; within {THRESHOLD} px: {within:.1%}; errors above 5 px: "
          f"{int((err64 > 5.0).sum())}; largest {float(err64.max()):.2f} px")
    print(f"reference fp32 vs float64, count >= 5: control points max |diff| = {gap_new:.3e} (scale {scale:.1f}), "
          f"{gap_rel:.3e} of the row's own largest coordinate; pixel error max |diff| = {gap_err:.3e} px; decisions "
          f"flipped outside the 3x margin: {flips}; rows inside it: {skipped:.2%}")
    print(f"count 4 (reference only): fitted points move by up to {float(moved):.1f}, error up to "
          f"{float(err[four].max()):.3f} px")


if __name__ == "__main__":
    main()
