"""Generate tests/golden/init.npz by RUNNING THE REFERENCE'S OWN create_from_pcd / create_from_pcd_dynamic
(scene/gaussian_model.py:406-582) and inverse_cubic_hermite (:18-88) on CPU, in the container that holds the reference.

    python tests/golden/make_golden_init.py

simple_knn (a CUDA extension) does not exist here: the module's `distCUDA2` is set to the float64 brute force below,
the DEFINITION of what it computes (mean of the three smallest squared distances to other points, self excluded by
index).  The fixture holds the inputs, every tensor the two methods leave in the model, and the control points of the
same trajectories fitted in float64 (the reference's function run under a float64 default dtype): data only.
"""
from __future__ import annotations

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

N, T, SEED = 500, 24, 77
FIELDS = ["_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest", "_features_t", "_omega",
          "_zeta", "_motion", "_trbf_center", "_trbf_scale", "control_xyz", "current_control_num", "max_radii2D",
          "_deformation_table"]


def brute_force_dist2(points: torch.Tensor) -> torch.Tensor:
    """float64: mean of the three smallest |p_i - p_j|^2 over j != i."""
    p = points.double()
    d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    d.fill_diagonal_(float("inf"))
    return d.topk(3, dim=1, largest=False).values.sum(1) / 3.0


def cloud():
    """A seeded cloud with three clusters of different density, 25 exact duplicates (one point four times: its three
    nearest neighbours are all at distance 0) and one far outlier; colours, time centres and noisy tracked trajectories."""
    g = torch.Generator().manual_seed(SEED)
    pts = torch.cat([torch.randn(N // 2, 3, generator=g) * 1.5,
                     torch.randn(N // 4, 3, generator=g) * 0.05 + torch.tensor([2.0, -1.0, 0.5]),
                     torch.rand(N - N // 2 - N // 4, 3, generator=g) * 6.0 - 3.0])
    src = torch.randperm(N, generator=g)[:22]
    dst = torch.randperm(N, generator=g)[:22]
    pts[dst] = pts[src].clone()
    pts[[5, 6, 7]] = pts[4].clone()
    pts[N - 1] = torch.tensor([400.0, -250.0, 90.0])
    colors = torch.rand(N, 3, generator=g)
    times = torch.rand(N, 1, generator=g)
    t = torch.linspace(0, 1, T)[None, :, None]
    amp = 0.3 * torch.randn(N, 1, 3, generator=g)
    phase = 6.28 * torch.rand(N, 1, 3, generator=g)
    traj = pts[:, None, :] + amp * torch.sin(5.0 * t + phase) + 0.4 * amp * torch.sin(23.0 * t * t + 2.0 * phase) \
        + 0.01 * torch.randn(N, T, 3, generator=g)
    return pts, colors, times, traj.float()


def state(pc):
    return {k: getattr(pc, k).detach().cpu().numpy() for k in FIELDS}


def main():
    gm = RH.ref_import("scene.gaussian_model")
    gm.distCUDA2 = lambda p: brute_force_dist2(p).float()
    pts, colors, times, traj = cloud()
    pcd = types.SimpleNamespace(points=pts.numpy(), colors=colors.numpy(), times=times.numpy())
    out = {"points": pts.numpy(), "colors": colors.numpy(), "times": times.numpy(), "traj": traj.numpy(),
           "dist2_f64": brute_force_dist2(pts).numpy(), "spatial_lr_scale": np.array(5.0)}
    with RH.CudaToCpu():
        torch.manual_seed(SEED)
        spc = gm.GaussianModel(0, RH.Args())
        dpc = gm.GaussianModel(0, RH.Args())
        spc.create_from_pcd(pcd, 5.0, 0)
        dpc.create_from_pcd_dynamic(pcd, 5.0, 0, traj)
        out.update({"static." + k: v for k, v in state(spc).items() if k != "control_xyz"})  # (:527: random numbers)
        out.update({"dynamic." + k: v for k, v in state(dpc).items()})
        assert spc.spatial_lr_scale == 5.0 and dpc.spatial_lr_scale == 5.0
        # the same fit in float64: the reference's function, float64 inputs, float64 default dtype for its zeros()
        time_step = 1 / (T - 1.0)
        t_step = torch.arange(0, 1 + time_step, time_step).float()[:T]
        out["t_step"] = t_step.numpy()
        torch.set_default_dtype(torch.float64)
        try:
            c64 = gm.inverse_cubic_hermite(traj.double() * 1e2, t_step.double()[None, :, None].expand(N, -1, -1), N_pts=12)
        finally:
            torch.set_default_dtype(torch.float32)
        assert c64.dtype == torch.float64
        out["control_f64"] = c64.numpy()
    path = os.path.join(HERE, "init.npz")
    files = save_npz(path, out)
    print(f"wrote {', '.join(files)}  ({sum(os.path.getsize(f) for f in files) / 1024:.0f} KiB, {len(out)} arrays)")
    gap = float(np.abs(out["dynamic.control_xyz"].astype(np.float64) - out["control_f64"]).max())
    print(f"reference fp32 vs float64 control points: max |diff| = {gap:.3e} (scale {np.abs(out['control_f64']).max():.1f})")


if __name__ == "__main__":
    main()
