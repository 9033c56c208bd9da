"""Generate tests/golden/report_sheets.npz by running the reference's OWN render_training_image (utils/scene_utils.py) on
the CPU, through ref_harness.py, on the 80 x 48 scene of make_golden.py (900 static + 500 dynamic splats).

    python tests/golden/make_golden_report.py

Three cases: a test view, a training view without blur kernels, a training view with blur kernels.  PIL.Image.fromarray
is wrapped while the reference runs, so the uint8 arrays are captured BEFORE JPEG coding and before the labels are drawn.
Next to them the fixture stores what the sheets were made from: the tensors of the reference's result dict, the
intrinsics, the target depth and normals, the mask.  Data only, no reference source.

flow_vis is not installed here: the generator stubs it with tests/report_restatement.py, and the names of the arrays
that came out of the stub are listed under "unpinned".  Every other panel is the reference's own output.  To keep the
file small, of the nine flows only 0, 4 and 8 are stored.
"""
from __future__ import annotations

import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402
import ref_harness as RH  # noqa: E402
import report_restatement as RR  # noqa: E402

from mobgs_amd.camera import PinholeCamera  # noqa: E402
from mobgs_amd.synth import SynthCamera  # noqa: E402

W, H, NS, ND, SEED = 80, 48, 900, 500, 1
FLOWS_KEPT = (0, 4, 8)


def metadata(K, skew=0.0):
    """What scene_utils.py:131-136 reads from a dycheck camera, as float32 like dycheck holds them."""
    f32 = np.float32
    xx, yy = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32))
    pixels = np.stack([xx, yy], axis=-1) + f32(0.5)
    return types.SimpleNamespace(get_pixels=lambda: pixels, principal_point_x=f32(K[0, 2]), principal_point_y=f32(K[1, 2]),
                                 focal_length=f32(K[0, 0]), skew=f32(skew), use_center=True)


def make_views(scam, n=2):
    g = torch.Generator().manual_seed(SEED + 500)
    views = []
    for i in range(n):
        w2c = MG.small_w2c()
        w2c[:3, 3] += torch.tensor([0.02 * i, -0.01 * i, 0.0])
        cam = PinholeCamera(W, H, scam.K, w2c, time=scam.time, max_time=scam.max_time)
        cam.uid, cam.image_name = i, f"view{i}"
        cam.original_image = torch.rand(3, H, W, generator=g)
        nrm = torch.randn(3, H, W, generator=g)
        cam.normal = nrm / nrm.norm(dim=0, keepdim=True)
        cam.depth = 1.0 + 3.0 * torch.rand(1, H, W, generator=g)
        cam.mask = (torch.rand(1, H, W, generator=g) > 0.5).float()
        cam.metadata = metadata(scam.K, skew=0.0625)
        cam._w2c_full = w2c
        views.append(cam)
    return views


class WarpStub:
    """blcekernel.get_warped_cams with the reference's own BLCE model and get_cam's pose algebra (scene/blce.py:150-163),
    as make_golden.gen_blurry_view builds the latent cameras (the reference's Camera class cannot be imported here)."""

    def __init__(self, scam, num_views=2):
        bl = RH.ref_import("scene.blce")
        self.bl, self.scam = bl, scam
        with RH.CudaToCpu():
            torch.manual_seed(SEED)
            self.model = m = bl.BLCE(num_views=num_views, view_dim=32, num_warp=9, method="euler", adjoint=False)
            g = torch.Generator().manual_seed(SEED)
            with torch.no_grad():
                for i in range(num_views):
                    for dec, sc in ((m.rot_decoder[i], 0.3), (m.trans_decoder[i], 0.02), (m.theta_decoder[i], 0.03)):
                        dec.weight.copy_(sc * torch.randn(dec.weight.shape, generator=g))
                        dec.bias.copy_(0.1 * sc * torch.randn(dec.bias.shape, generator=g))
                    m.wv_derivative[i].time_embedder.data = 0.5 * torch.randn(9, 8, generator=g)
                m.view_embedder.data = torch.randn(num_views, 32, generator=g)
                m.exposure_time_expo.data = torch.tensor([0.4, 0.3])[:num_views]

    def get_warped_cams(self, view, fwd, bwd):
        with RH.CudaToCpu(), torch.no_grad():
            blur = self.bl.compute_frequency_blur_feature(view.original_image)
            warped_c2w, expo = self.model(torch.inverse(view._w2c_full), blur, view.uid)
            warped_w2c = torch.inverse(warped_c2w)
            cams = []
            for k in range(9):
                R, T = warped_c2w[k, :3, :3], warped_w2c[k, :3, 3]
                w2c_k = torch.cat([torch.cat([R.transpose(0, 1), T[:, None]], dim=1), torch.tensor([[0.0, 0, 0, 1]])], dim=0)
                cams.append(PinholeCamera(W, H, self.scam.K, w2c_k, time=view.time, max_time=view.max_time))
        return cams, expo


def run_case(su, gr, views, spc, dpc, bg, is_train, blce):
    """-> (the arrays PIL.Image.fromarray received for view 0, in call order; the render dicts of view 0, in call order)"""
    captured, renders = [], []
    real_fromarray = su.Image.fromarray
    real_truetype = su.ImageFont.truetype

    def fromarray(a, *args, **kw):
        captured.append(np.array(a, copy=True))
        return real_fromarray(a, *args, **kw)

    def render(cam, *args, **kw):
        with RH.CudaToCpu():
            out = gr.render(cam, *args, **kw)
        renders.append((cam, kw, out))
        return out

    default_font = su.ImageFont.load_default()
    su.Image.fromarray = fromarray
    su.ImageFont.truetype = lambda *a, **k: default_font   # (./utils/TIMES.TTF is a path relative to the reference)
    try:
        with tempfile.TemporaryDirectory() as tmp, RH.CudaToCpu():
            su.render_training_image(types.SimpleNamespace(model_path=tmp), spc, dpc, views, render, None,
                                     bg, "fine", 100, 30.0, "dycheck", is_train=is_train, blcekernel=blce)
    finally:
        su.Image.fromarray = real_fromarray
        su.ImageFont.truetype = real_truetype
    per_view = len(captured) // len(views)
    n_renders = len(renders) // len(views)
    return captured[:per_view], renders[:n_renders]


def main():
    RH.install()
    unpinned = []

    def stub_flow_to_color(flow, clip_flow=None, convert_to_bgr=False):
        return RR.flow_to_color(flow, clip_flow, convert_to_bgr)

    sys.modules["flow_vis"] = types.ModuleType("flow_vis")
    sys.modules["flow_vis"].flow_to_color = stub_flow_to_color
    gr = RH.ref_import("gaussian_renderer")
    su = RH.ref_import("utils.scene_utils")
    scam = SynthCamera().scaled(W, H)
    stat, dyn = MG.scene_params(NS, ND, scam, SEED)
    spc, dpc = MG.ref_models(stat, dyn, SEED)
    bg = torch.tensor([0.1, 0.2, 0.3, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    views = make_views(scam)
    v0 = views[0]
    md = v0.metadata
    arrays = {"cam": np.array([md.focal_length, md.principal_point_x, md.principal_point_y, md.skew, 0.5], dtype=np.float64),
              "gt": MG.np_(v0.original_image), "gt_normal": MG.np_(v0.normal), "gt_depth": MG.np_(v0.depth),
              "mask": MG.np_(v0.mask)}
    for case, is_train, blce in (("test", False, None), ("train", True, None), ("train_blur", True, WarpStub(scam))):
        captured, renders = run_case(su, gr, views, spc, dpc, bg, is_train, blce)
        main_pkg = renders[0][2]
        for k in ("render", "d_render", "s_render", "d_alpha", "depth"):
            arrays[f"{case}_{k}"] = MG.np_(main_pkg[k])
        if blce is not None:
            # per latent camera: flow image, latent image (scene_utils.py:94-100); then the two sheets
            assert len(captured) == 20 and len(renders) == 11, (len(captured), len(renders))
            latents = [renders[1 + k][2] for k in range(9)]
            for k in range(9):
                arrays[f"{case}_latent_{k}"] = MG.np_(latents[k]["render"])
                arrays[f"{case}_latent_img_{k}"] = captured[2 * k + 1]
                if k in FLOWS_KEPT:
                    arrays[f"{case}_flow_{k}"] = MG.np_(latents[k]["ori_flow"].squeeze(0))
                    arrays[f"{case}_flow_img_{k}"] = captured[2 * k]
                    unpinned.append(f"{case}_flow_img_{k}")
            arrays[f"{case}_exposure"] = MG.np_(torch.stack([r[1]["delta_exposure"] for r in renders[1:10]]))
            arrays[f"{case}_blurry"] = MG.np_(torch.mean(torch.stack([p["render"] for p in latents] + [main_pkg["render"]]),
                                                         dim=0))
            captured = captured[18:]
        assert len(captured) == 2, len(captured)
        arrays[f"{case}_image"], arrays[f"{case}_decomp"] = captured
    arrays["unpinned"] = np.array(unpinned)
    MG.save("report_sheets", **arrays)


if __name__ == "__main__":
    main()
