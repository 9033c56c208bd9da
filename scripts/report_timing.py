"""Time the report sheets of ONE training view with blur kernels: image + decomp + 9 flow colours + 9 latent frames.

    python scripts/report_timing.py [--sizes 512x288:30000,1352x1014:300000] [--reps 10]

The renders are excluded: the view's render and the nine latent renders (get_flow=True) are done once, and the clock
starts from their outputs.  Two ways to the same bytes on the host:

    device    mobgs_amd.scene_utils.compose_sheet x 4 (+ the ten-image mean) and ONE device-to-host copy per sheet
    host      the reference's statements (utils/scene_utils.py:94-104, :130-212) composed from torch ops and numpy on the
              same render outputs, with a .cpu().numpy() where the reference has one, and the flows through the numpy
              path of mobgs_amd.flow_vis (the package's own text).  This script's own copy of that composition.

Host clock around work that ends in a synchronise (the host path ends in numpy arrays, the device path in .cpu()), median
of --reps after two warm-up rounds.  Needs a HIP device; prints one JSON line per size.  Recorded in
docs/MEASUREMENT_LOG.md; no test asserts a time.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mobgs_amd import flow_vis  # noqa: E402
from mobgs_amd.blce import blceKernel  # noqa: E402
from mobgs_amd.camera import PinholeCamera  # noqa: E402
from mobgs_amd.gaussian_model import GaussianParams  # noqa: E402
from mobgs_amd.gaussian_renderer import render  # noqa: E402
from mobgs_amd.helper_model import Sandwich  # noqa: E402
from mobgs_amd.scene_utils import camera_intrinsics, compose_sheet  # noqa: E402
from mobgs_amd.synth import SynthCamera, dynamic_extras, gaussian_cloud  # noqa: E402


def outputs(W, H, n, dev):
    """The render outputs of one blurry training view: (view, its result dict, the nine latent result dicts)."""
    scam = SynthCamera().scaled(W, H)
    torch.manual_seed(0)
    dec = Sandwich(9, 3).to(dev)
    ns = 2 * n // 3
    sp, dp = gaussian_cloud(ns, scam, 0), gaussian_cloud(n - ns, scam, 1)
    stat = GaussianParams(sp, None, dec, dev, requires_grad=False)
    dyn = GaussianParams(dp, dynamic_extras(dp["xyz"], 0), dec, dev, requires_grad=False)
    bg = torch.zeros(9, device=dev)
    g = torch.Generator().manual_seed(5)
    v = PinholeCamera(W, H, scam.K, torch.eye(4), time=5.0 / 23.0, max_time=23, device=dev)
    v.uid = 0
    v.original_image = v.image = torch.rand(3, H, W, generator=g).to(dev)
    nrm = torch.randn(3, H, W, generator=g)
    v.normal = (nrm / nrm.norm(dim=0, keepdim=True)).to(dev)
    v.depth = (1.0 + 3.0 * torch.rand(1, H, W, generator=g)).to(dev)
    v.metadata = types.SimpleNamespace(focal_length=float(scam.K[0, 0]), principal_point_x=float(scam.K[0, 2]),
                                       principal_point_y=float(scam.K[1, 2]), skew=0.0, use_center=True)
    blce = blceKernel(num_views=1, num_warp=9, iteration=1).to(dev)
    with torch.no_grad():
        pkg = render(v, stat, dyn, None, bg, get_static=True, get_dynamic=True)
        cams, expo = blce.get_warped_cams(v, v, v)
        lat = [render(c, stat, dyn, None, bg, get_static=True, get_dynamic=True, delta_exposure=expo[k], get_flow=True)
               for k, c in enumerate(cams)]
        for p in [pkg] + lat:       # materialise what the sheets read, outside the clock
            for k in ("render", "d_alpha", "depth"):
                p[k]
        for p in lat:
            p["ori_flow"]
    torch.cuda.synchronize()
    return v, pkg, lat


def device_path(v, pkg, lat):
    H, W = pkg["render"].shape[-2:]
    frames = [p["render"] for p in lat]
    blurry = torch.mean(torch.stack(frames + [pkg["render"]]), dim=0)
    flows = compose_sheet([("FLOW", p["ori_flow"].squeeze(0)) for p in lat], H, W, vertical=True)
    latents = compose_sheet([("RGB", f) for f in frames], H, W, vertical=True)
    image = compose_sheet([("RGB", v.original_image), ("RGB", blurry), ("RGB", pkg["render"]), ("GREY", pkg["d_alpha"])],
                          H, W)
    decomp = compose_sheet([("SIGNED3", v.normal), ("NORMALS_FD", pkg["depth"]), ("GREY_DIV_MAX", v.depth),
                            ("GREY_DIV_MAX", pkg["depth"])], H, W, camera=camera_intrinsics(v.metadata))
    return [t.cpu().numpy() for t in (image, decomp, flows, latents)]


def host_path(v, pkg, lat):
    """The reference's composition (this script's own copy of its statements)."""
    def u8(a):
        return (np.clip(a, 0, 1) * 255).astype("uint8")

    flows, latents, frames = [], [], []
    for p in lat:
        flows.append(flow_vis.flow_to_color(p["ori_flow"].squeeze(0).detach().cpu().numpy(), convert_to_bgr=False))
        latents.append(u8(p["render"].permute(1, 2, 0).cpu().numpy()))
        frames.append(p["render"])
    frames.append(pkg["render"])
    blurry_np = torch.mean(torch.stack(frames), dim=0).permute(1, 2, 0).cpu().numpy()
    m = v.metadata
    z = pkg["depth"] + 1e-6
    H, W = z.shape[-2:]
    xx, yy = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    pixels = np.stack([xx, yy], axis=-1) + 0.5
    y = (pixels[..., 1] - m.principal_point_y) / m.focal_length
    x = (pixels[..., 0] - m.principal_point_x - y * m.skew) / m.focal_length
    viewdirs = torch.from_numpy(np.stack([x, y, np.ones_like(x)], axis=-1).astype(np.float32)).to(z.device)
    coords = (viewdirs[None] * z[..., None]).permute(0, 3, 1, 2)
    du = coords[..., :, 1:] - coords[..., :, :-1]
    du = torch.cat([du, du[..., :, -1:]], dim=-1)
    dv = coords[..., 1:, :] - coords[..., :-1, :]
    dv = torch.cat([dv, dv[..., -1:, :]], dim=-2)
    n = torch.stack([dv[:, 1] * du[:, 2] - du[:, 1] * dv[:, 2], dv[:, 2] * du[:, 0] - du[:, 2] * dv[:, 0],
                     dv[:, 0] * du[:, 1] - du[:, 0] * dv[:, 1]], dim=-3)
    pred_normal_np = (torch.nn.functional.normalize(n, dim=-3)[0].permute(1, 2, 0).cpu().numpy() + 1) / 2
    gt_np = v.original_image.permute(1, 2, 0).cpu().numpy()
    image_np = pkg["render"].permute(1, 2, 0).cpu().numpy()
    d_alpha_np = np.repeat(pkg["d_alpha"].reshape(1, H, W).permute(1, 2, 0).cpu().numpy(), 3, axis=2)
    depth_np = pkg["depth"].permute(1, 2, 0).cpu().numpy()
    depth_np = np.repeat(depth_np / depth_np.max(), 3, axis=2)
    gt_normal_np = ((v.normal + 1) / 2).permute(1, 2, 0).cpu().numpy()
    gt_depth_np = v.depth.permute(1, 2, 0).cpu().numpy()
    gt_depth_np = np.repeat(gt_depth_np / gt_depth_np.max(), 3, axis=2)
    decomp = u8(np.concatenate((gt_normal_np, pred_normal_np, gt_depth_np, depth_np), axis=1))
    image = u8(np.concatenate((gt_np, blurry_np, image_np, d_alpha_np), axis=1))
    return [image, decomp, np.stack(flows), np.stack(latents)]


def clock(fn, reps):
    for _ in range(2):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512x288:30000,1352x1014:300000")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("report_timing.py needs a HIP device: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    for spec in args.sizes.split(","):
        size, n = spec.split(":")
        W, H = (int(s) for s in size.split("x"))
        v, pkg, lat = outputs(W, H, int(n), dev)
        a, b = device_path(v, pkg, lat), host_path(v, pkg, lat)
        off = [int((x.astype(np.int16) - y.astype(np.int16)).__abs__().max()) for x, y in zip(a, b)]
        differ = [float((x != y).mean()) for x, y in zip(a, b)]
        d = clock(lambda: device_path(v, pkg, lat), args.reps)
        h = clock(lambda: host_path(v, pkg, lat), args.reps)
        print(json.dumps({"size": size, "splats": int(n), "reps": args.reps, "clock": "host, median (min, max), seconds",
                          "device_path_s": [round(t, 6) for t in d], "host_path_s": [round(t, 6) for t in h],
                          "speedup": round(h[0] / d[0], 2), "max_level_difference_per_sheet": off,
                          "fraction_of_bytes_that_differ_per_sheet": differ}), flush=True)


if __name__ == "__main__":
    main()
