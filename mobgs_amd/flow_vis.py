"""The public names of the `flow_vis` package (0.1), for the import swap of INTEGRATION.md:

    import mobgs_amd.flow_vis as flow_vis
    flow_color = flow_vis.flow_to_color(render_pkg["ori_flow"].squeeze(0), convert_to_bgr=False)   # scene_utils.py:94

A tensor on a HIP device runs the two report kernels (include/mobgs_hip.h K26) and comes back as a uint8 tensor on that
device: no `.cpu().numpy()` of the float flow.  A numpy array (or a host tensor) runs the numpy text below and comes back
as uint8 numpy, as the package returns it.

UNPINNED: `flow_vis` is not installed where this was written and is no part of the reference's tree, so the wheel and the
colour rule are restated from memory of the package (README, "The flow colour wheel is UNPINNED";
scripts/dump_flowvis_vectors.py writes the vectors that pin them on a machine that has the package).
"""
from __future__ import annotations

import numpy as np

__all__ = ["make_colorwheel", "flow_uv_to_colors", "flow_to_color"]


def make_colorwheel():
    """The Middlebury wheel (Baker et al., ICCV 2007): [55, 3] float64 with values 0 .. 255.  Segments RY 15, YG 6, GC 4,
    CB 11, BM 13, MR 6; inside a segment of length L one channel rises as floor(255 i / L) or falls as 255 - floor(255 i /
    L) while another stays at 255."""
    RY, YG, GC, CB, BM, MR = 15, 6, 4, 11, 13, 6
    ncols = RY + YG + GC + CB + BM + MR
    colorwheel = np.zeros((ncols, 3))
    col = 0
    colorwheel[0:RY, 0] = 255
    colorwheel[0:RY, 1] = np.floor(255 * np.arange(0, RY) / RY)
    col += RY
    colorwheel[col:col + YG, 0] = 255 - np.floor(255 * np.arange(0, YG) / YG)
    colorwheel[col:col + YG, 1] = 255
    col += YG
    colorwheel[col:col + GC, 1] = 255
    colorwheel[col:col + GC, 2] = np.floor(255 * np.arange(0, GC) / GC)
    col += GC
    colorwheel[col:col + CB, 1] = 255 - np.floor(255 * np.arange(CB) / CB)
    colorwheel[col:col + CB, 2] = 255
    col += CB
    colorwheel[col:col + BM, 2] = 255
    colorwheel[col:col + BM, 0] = np.floor(255 * np.arange(0, BM) / BM)
    col += BM
    colorwheel[col:col + MR, 2] = 255 - np.floor(255 * np.arange(MR) / MR)
    colorwheel[col:col + MR, 0] = 255
    return colorwheel


def flow_uv_to_colors(u, v, convert_to_bgr=False):
    """u, v: [H, W] arrays, already normalised so that the radius is at most 1 -> [H, W, 3] uint8.  The `col * 0.75` arm
    (radius above 1) is here and in tests/report_restatement.py only: flow_to_color divides by rad_max + 1e-5 first, so
    the kernel, which is reached through flow_to_color alone, cannot meet it."""
    u, v = np.asarray(u), np.asarray(v)
    flow_image = np.zeros((u.shape[0], u.shape[1], 3), np.uint8)
    colorwheel = make_colorwheel()
    ncols = colorwheel.shape[0]
    rad = np.sqrt(np.square(u) + np.square(v))
    a = np.arctan2(-v, -u) / np.pi
    fk = (a + 1) / 2 * (ncols - 1)
    k0 = np.floor(fk).astype(np.int32)
    k1 = k0 + 1
    k1[k1 == ncols] = 0
    f = fk - k0
    for i in range(colorwheel.shape[1]):
        tmp = colorwheel[:, i]
        col0 = tmp[k0] / 255.0
        col1 = tmp[k1] / 255.0
        col = (1 - f) * col0 + f * col1
        idx = rad <= 1
        col[idx] = 1 - rad[idx] * (1 - col[idx])
        col[~idx] = col[~idx] * 0.75
        ch_idx = 2 - i if convert_to_bgr else i
        flow_image[:, :, ch_idx] = np.floor(255 * col)
    return flow_image


def _flow_to_color_numpy(flow_uv, clip_flow, convert_to_bgr):
    if clip_flow is not None:
        flow_uv = np.clip(flow_uv, 0, clip_flow)
    u = flow_uv[:, :, 0]
    v = flow_uv[:, :, 1]
    rad = np.sqrt(np.square(u) + np.square(v))
    rad_max = np.max(rad)
    epsilon = 1e-5
    u = u / (rad_max + epsilon)
    v = v / (rad_max + epsilon)
    return flow_uv_to_colors(u, v, convert_to_bgr)


def flow_to_color(flow_uv, clip_flow=None, convert_to_bgr=False):
    """flow_uv: [H, W, 2] -> [H, W, 3] uint8, the flow on the colour wheel: hue from the direction (a flow to the right is
    red), saturation from the radius over the image's largest radius (a zero flow is white).  `clip_flow`: clip both
    components to [0, clip_flow] first.  numpy in, numpy out; a tensor on a HIP device in, a uint8 tensor on that device
    out (two kernel launches, nothing copied to the host)."""
    try:
        import torch
    except ImportError:  # the numpy path needs no torch
        torch = None
    if torch is not None and torch.is_tensor(flow_uv):
        if flow_uv.dim() != 3 or flow_uv.shape[2] != 2:
            raise ValueError("flow_to_color: input flow must have shape [H,W,2]")
        if flow_uv.is_cuda:
            from .scene_utils import compose_sheet
            H, W = int(flow_uv.shape[0]), int(flow_uv.shape[1])
            img = compose_sheet([("FLOW", flow_uv.detach(), None, clip_flow)], H, W)
            return img.flip(-1) if convert_to_bgr else img
        flow_uv = flow_uv.detach().numpy()
    flow_uv = np.asarray(flow_uv)
    if flow_uv.ndim != 3 or flow_uv.shape[2] != 2:
        raise ValueError("flow_to_color: input flow must have shape [H,W,2]")
    return _flow_to_color_numpy(flow_uv, clip_flow, convert_to_bgr)
