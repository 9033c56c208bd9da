"""`render_training_image` of the reference's utils/scene_utils.py (:15-260), with the sheets composed on the GPU.

    render_training_image(scene, stat_gaussians, dyn_gaussians, viewpoints, render, pipe, background, stage, iteration,
                          time_now, dataset_type, is_train=..., blcekernel=...)          # train.py:776-790

The reference builds every sheet from about twenty `.cpu().numpy()` round trips of float32 [H,W,3] arrays, normalises,
repeats, concatenates and clips them on the host and sends the flows through `flow_vis` in numpy.  Here a sheet is laid out
as uint8 by two kernel launches (include/mobgs_hip.h K26, csrc/report.hip) and ONE device-to-host copy carries the final
bytes:

    report_stats     min / max of fp32 maps on the device, bit-equal to torch.amin / torch.amax
    compose_sheet    a list of panels -> one uint8 sheet
    report_sheets    the sheets of one view as uint8 device tensors (no file, no PIL)
    render_training_image   the reference's loop, directories, file names and labels around report_sheets

Kept from the reference: `blurry` is the mean of TEN images, the nine latent frames and the view's own render
(:102-104).  Dropped, because it reaches no output: the stage="coarse" render (:107) whose `coarse_image` and `st_depth`
are never put on a sheet.  Not here: the latent frames through render_many (it has no get_flow), the warm stage (the
reference's own branch reads names that no longer exist there), the point-cloud scatter plot (never called).
"""
from __future__ import annotations

import ctypes
import os
from typing import List, NamedTuple, Optional

import torch

from . import _lib
from ._lib import check, f32c, ptr, stream

PANEL_KINDS = ("RGB", "GREY", "GREY_DIV_MAX", "ERROR", "SIGNED3", "NORMALS_FD", "FLOW")
_KIND = {n: _lib._DEFINES["MOBGS_REPORT_" + n] for n in PANEL_KINDS}
_STAT = {n: _lib._DEFINES["MOBGS_REPORT_STAT_" + n] for n in ("MINMAX", "SQERR", "FLOW_RAD")}
MAX_PANELS, MAX_STATS = _lib._DEFINES["MOBGS_REPORT_MAX_PANELS"], _lib._DEFINES["MOBGS_REPORT_MAX_STATS"]
# what a panel kind needs from mobgs_report_stats
_STAT_OF = {"GREY_DIV_MAX": "MINMAX", "ERROR": "SQERR", "FLOW": "FLOW_RAD"}
_CHANNELS = {"RGB": 3, "GREY": 1, "GREY_DIV_MAX": 1, "ERROR": 3, "SIGNED3": 3, "NORMALS_FD": 1, "FLOW": 2}


def _clip(clip) -> float:
    if clip is None:
        return -1.0
    if not float(clip) >= 0.0:
        raise ValueError(f"report: clip_flow = {clip} must not be negative")
    return float(clip)


def _source(what, name, t, numel, dev):
    _lib.device_tensor(what, name, t)
    if t.numel() != numel:
        raise ValueError(f"{what}: {name} has {t.numel()} elements, {numel} expected")
    if dev is not None and t.device != dev:
        raise ValueError(f"{what}: {name} is on {t.device}, the other sources on {dev}")
    return f32c(t.detach())


def _run_stats(lib, specs, dev):
    """specs: (kind name, a, b | None, clip) with a, b already float32 + contiguous -> the float buffer of
    mobgs_report_stats (its first 2 S entries are the results)."""
    n = len(specs)
    if not 1 <= n <= MAX_STATS:
        raise ValueError(f"report: {n} statistics; 1 .. {MAX_STATS} fit one launch")
    recs = (_lib.MobgsReportStat * n)()
    for r, (kind, a, b, clip) in zip(recs, specs):
        r.kind, r.n = _STAT[kind], a.numel() // (2 if kind == "FLOW_RAD" else 1)
        r.a, r.b, r.clip = a.data_ptr(), (b.data_ptr() if b is not None else None), clip
    buf = torch.empty(int(lib.mobgs_report_stats_floats(n)), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.mobgs_report_stats(n, ctypes.cast(recs, ctypes.c_void_p), ptr(buf), stream()), "mobgs_report_stats")
    return buf


def report_stats(maps) -> torch.Tensor:
    """maps: a list of ("MINMAX", a) | ("SQERR", a, b) | ("FLOW_RAD", flow [...,2][, clip_flow]) -> [S, 2] float32 on the
    device: (min, max) of a, of (a - b)^2 formed in fp32 as written, of sqrt(u u + v v).  Bit-equal to torch.amin /
    torch.amax of the same fp32 expression; one launch for all maps, no read-back.  Inputs are finite."""
    lib = _lib.load()
    specs, dev = [], None
    for m in maps:
        kind, a = m[0], m[1]
        if kind not in _STAT:
            raise ValueError(f"report_stats: unknown kind {kind!r}")
        _lib.device_tensor("report_stats", "map", a)
        if a.numel() == 0 or (kind == "FLOW_RAD" and a.shape[-1] != 2):
            raise ValueError("report_stats: a map must not be empty, and a flow must be [...,2]")
        dev = a.device if dev is None else dev
        a = _source("report_stats", "map", a, a.numel(), dev)
        b = _source("report_stats", "second map", m[2], a.numel(), dev) if kind == "SQERR" else None
        specs.append((kind, a, b, _clip(m[2] if kind == "FLOW_RAD" and len(m) > 2 else None)))
    return _run_stats(lib, specs, dev)[:2 * len(specs)].view(len(specs), 2)


def camera_intrinsics(metadata):
    """(focal, cx, cy, skew, pixel offset) as the sheet's normals read them from a dycheck camera (scene_utils.py:131-136):
    the single `focal_length` for both axes; pixel centres at +0.5 under `use_center` (default True)."""
    m = metadata
    return (float(m.focal_length), float(m.principal_point_x), float(m.principal_point_y),
            float(getattr(m, "skew", 0.0)), 0.5 if getattr(m, "use_center", True) else 0.0)


def compose_sheet(panels, H: int, W: int, *, camera=None, vertical: bool = False, out=None) -> torch.Tensor:
    """panels: a list of (kind, a[, b[, clip_flow]]) with kind one of PANEL_KINDS and a, b tensors on a HIP device:

        RGB [3,H,W] | GREY [1,H,W] | GREY_DIV_MAX [1,H,W]: a / max(a), 0 where the maximum is 0 (the reference divides by
        zero there) | ERROR a, b [3,H,W]: (e - min e) / max(max e - min e, 1e-8), e = (a - b)^2 | SIGNED3 [3,H,W]: (a + 1)
        / 2 | NORMALS_FD depth [1,H,W] (needs `camera`, H, W >= 2) | FLOW [H,W,2][, clip_flow]: flow_vis.flow_to_color

    -> uint8 [H, P W, 3] (side by side, as PIL.Image.fromarray takes it), or [P, H, W, 3] with `vertical` (every panel its
    own contiguous image).  Every panel ends in the reference's (np.clip(x, 0, 1) * 255).astype('uint8').  `camera`: what
    camera_intrinsics returns, or the metadata object itself.  `out`: a contiguous uint8 tensor of that shape to write into
    (every byte of it is written).  Two launches, nothing read back."""
    lib = _lib.load()
    H, W, P = int(H), int(W), len(panels)
    if H < 1 or W < 1 or not 1 <= P <= MAX_PANELS:
        raise ValueError(f"compose_sheet: H = {H}, W = {W}, {P} panels (1 .. {MAX_PANELS})")
    if camera is not None and not isinstance(camera, tuple):
        camera = camera_intrinsics(camera)
    recs = (_lib.MobgsReportPanel * P)()
    specs, keep, dev = [], [], None
    for r, p in zip(recs, panels):
        kind, a = p[0], p[1]
        if kind not in _KIND:
            raise ValueError(f"compose_sheet: unknown panel kind {kind!r}")
        if kind == "NORMALS_FD":
            if H < 2 or W < 2:
                raise ValueError(f"compose_sheet: a NORMALS_FD panel needs H >= 2 and W >= 2 (H = {H}, W = {W})")
            if camera is None:
                raise ValueError("compose_sheet: a NORMALS_FD panel needs the camera intrinsics")
        _lib.device_tensor("compose_sheet", f"{kind} source", a)
        dev = a.device if dev is None else dev
        a = _source("compose_sheet", f"{kind} source", a, _CHANNELS[kind] * H * W, dev)
        b = _source("compose_sheet", "ERROR target", p[2], 3 * H * W, dev) if kind == "ERROR" else None
        clip = _clip(p[3] if kind == "FLOW" and len(p) > 3 else None)
        keep += [a, b]     # (a converted copy lives until the launches are enqueued)
        r.kind, r.slot, r.a, r.b, r.clip = _KIND[kind], 0, a.data_ptr(), (b.data_ptr() if b is not None else None), clip
        if kind in _STAT_OF:
            r.slot = len(specs)
            specs.append((_STAT_OF[kind], a, b, clip))
    stats = _run_stats(lib, specs, dev) if specs else None
    shape = (P, H, W, 3) if vertical else (H, P * W, 3)
    if out is None:
        sheet = torch.empty(shape, dtype=torch.uint8, device=dev)
    else:
        if not (torch.is_tensor(out) and out.dtype == torch.uint8 and tuple(out.shape) == shape and out.device == dev
                and out.is_contiguous()):
            raise ValueError(f"compose_sheet: out must be a contiguous uint8 tensor {shape} on {dev}")
        sheet = out
    cam = camera if camera is not None else (0.0, 0.0, 0.0, 0.0, 0.0)
    with torch.cuda.device(dev):
        check(lib.mobgs_report_compose(H, W, P, ctypes.cast(recs, ctypes.c_void_p), ptr(stats), len(specs), *cam,
                                       1 if vertical else 0, ptr(sheet), stream()), "mobgs_report_compose")
    return sheet


class ReportSheets(NamedTuple):
    """uint8 device tensors.  image: test view [gt | render | error | d_alpha | d_render | s_render] (H x 6W), training
    view [gt | render | d_alpha | d_render | s_render] (H x 5W), training view with blur kernels [gt | blurry | render |
    d_alpha] (H x 4W).  decomp: training view [target normal | predicted normal | target depth | depth], otherwise
    [predicted normal | depth].  flows, latents: [9, H, W, 3] with blur kernels, else None."""
    image: torch.Tensor
    decomp: torch.Tensor
    flows: Optional[torch.Tensor]
    latents: Optional[torch.Tensor]
    blurry: Optional[torch.Tensor]   # the float ten-image mean behind the `blurry` panel (None without blur kernels)


@torch.no_grad()
def report_sheets(viewpoint, fwd_viewpoint, bwd_viewpoint, stat_gaussians, dyn_gaussians, render_func, pipe, background,
                  *, stage="fine", cam_type=None, is_train=False, blcekernel=None) -> ReportSheets:
    """The sheets of one view (scene_utils.py:34-232 without its files): the view's render with its static and dynamic
    layers, and for a training view with blur kernels one render per latent camera as the reference issues them --
    render_func(cam_k, ..., stage="fine", get_static=True, get_dynamic=True, delta_exposure=exposure_time[k],
    get_flow=True) -- whose flows go onto the colour wheel.  Touches no file and needs no PIL."""
    if stage == "warm":
        raise NotImplementedError("report_sheets: the warm stage is not ported (the reference's own branch reads names "
                                  "that no longer exist there)")
    pkg = render_func(viewpoint, stat_gaussians, dyn_gaussians, pipe, background, stage=stage, cam_type=cam_type,
                      get_static=True, get_dynamic=True, over_t=viewpoint.time)
    image = pkg["render"]
    H, W = int(image.shape[-2]), int(image.shape[-1])
    if H < 2 or W < 2:
        raise ValueError(f"report_sheets: the sheet's normals need H >= 2 and W >= 2 (H = {H}, W = {W})")
    flows = latents = blurry = None
    if is_train and blcekernel is not None:
        warped_cams, exposure_time = blcekernel.get_warped_cams(viewpoint, fwd_viewpoint, bwd_viewpoint)
        flow_maps, frames = [], []
        for k, cam in enumerate(warped_cams):
            lp = render_func(cam, stat_gaussians, dyn_gaussians, pipe, background, stage="fine", cam_type=cam_type,
                             get_static=True, get_dynamic=True, delta_exposure=exposure_time[k], get_flow=True)
            flow_maps.append(lp["ori_flow"].squeeze(0))
            frames.append(lp["render"])
        blurry = torch.mean(torch.stack(frames + [image]), dim=0)    # ten images (:102-104)
        flows = compose_sheet([("FLOW", f) for f in flow_maps], H, W, vertical=True)
        latents = compose_sheet([("RGB", f) for f in frames], H, W, vertical=True)
    dev = image.device   # (the view's own images may still be on the host: the reference calls .cuda() on them)
    gt = (viewpoint["image"] if cam_type == "PanopticSports" else viewpoint.original_image).to(dev)
    d_alpha = ("GREY", pkg["d_alpha"])
    depth = ("GREY_DIV_MAX", pkg["depth"])
    normal = ("NORMALS_FD", pkg["depth"])
    if is_train:
        decomp = [("SIGNED3", viewpoint.normal.to(dev)), normal, ("GREY_DIV_MAX", viewpoint.depth.to(dev)), depth]
        if blcekernel is not None:
            sheet = [("RGB", gt), ("RGB", blurry), ("RGB", image), d_alpha]
        else:
            sheet = [("RGB", gt), ("RGB", image), d_alpha, ("RGB", pkg["d_render"]), ("RGB", pkg["s_render"])]
    else:
        decomp = [normal, depth]
        sheet = [("RGB", gt), ("RGB", image), ("ERROR", image, gt), d_alpha, ("RGB", pkg["d_render"]),
                 ("RGB", pkg["s_render"])]
    return ReportSheets(compose_sheet(sheet, H, W), compose_sheet(decomp, H, W, camera=viewpoint.metadata), flows,
                        latents, blurry)


def _font(path, size=40):
    from PIL import ImageFont
    if path is not None and os.path.exists(path):
        return ImageFont.truetype(path, size=size)
    try:
        return ImageFont.load_default(size=size)
    except TypeError:   # (Pillow before 10.1: the built-in bitmap font has one size)
        return ImageFont.load_default()


def render_training_image(scene, stat_gaussians, dyn_gaussians, viewpoints, render_func, pipe, background, stage, iteration,
                          time_now, dataset_type, is_train=False, over_t=None, blcekernel=None, font=None) -> List[str]:
    """The reference's call (train.py:776-790): for every view of `viewpoints`, with its neighbours as the reference picks
    them (:249-259: the view itself at either end), write under scene.model_path

        {stage}_render/train|val/images/<image_name>.jpg            the image sheet, labelled "stage:..,iter:.." and "time:.."
        ...                            /<image_name>_decomp.jpg     normals and depth
        ...                            /<image_name>_flow_XX.jpg, _latent_XX.jpg    with blur kernels, XX = 00 .. 08

    and create {stage}_render/pointclouds as the reference does.  The labels are drawn by PIL on the one host copy of the
    sheet; `font`: a TrueType file (the reference reads ./utils/TIMES.TTF, which is not shipped here), PIL's built-in font
    when absent.  -> the paths of the image sheets."""
    if stage == "warm":
        raise NotImplementedError("render_training_image: the warm stage is not ported (the reference's own branch reads "
                                  "names that no longer exist there)")
    from PIL import Image, ImageDraw
    base = os.path.join(scene.model_path, f"{stage}_render")
    image_path = os.path.join(base, "train/images" if is_train else "val/images")
    os.makedirs(os.path.join(base, "pointclouds"), exist_ok=True)
    os.makedirs(image_path, exist_ok=True)
    label1 = f"stage:{stage},iter:{iteration}"
    minutes = time_now / 60
    label2 = "time:%.2f" % minutes + ("min" if minutes < 1 else "mins")
    face = _font(font)
    written, last = [], len(viewpoints) - 1
    for idx, view in enumerate(viewpoints):
        path = os.path.join(image_path, f"{view.image_name}.jpg")
        sheets = report_sheets(view, viewpoints[min(idx + 1, last)], viewpoints[max(idx - 1, 0)], stat_gaussians,
                               dyn_gaussians, render_func, pipe, background, stage=stage, cam_type=dataset_type,
                               is_train=is_train, blcekernel=blcekernel)
        img = Image.fromarray(sheets.image.cpu().numpy())
        draw = ImageDraw.Draw(img)
        draw.text((10, 10), label1, fill=(255, 0, 0), font=face)
        draw.text((img.width - 100 - len(label2) * 10, 10), label2, fill=(255, 0, 0), font=face)
        img.save(path)
        Image.fromarray(sheets.decomp.cpu().numpy()).save(path.replace(".jpg", "_decomp.jpg"))
        for name, stack in (("flow", sheets.flows), ("latent", sheets.latents)):
            if stack is not None:
                for k, frame in enumerate(stack.cpu().numpy()):
                    Image.fromarray(frame).save(path.replace(".jpg", f"_{name}_{str(k).zfill(2)}.jpg"))
        written.append(path)
    return written
