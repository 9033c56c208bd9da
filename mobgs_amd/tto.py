"""Test-time pose refinement on the HIP path (csrc/pose.hip, include/mobgs_hip.h K23): what the reference's eval.py does
to every test camera before it writes the image that metrics.py scores.

    q = matrix_to_quaternion(w2c[:3, :3]);  R = quaternion_to_matrix(q)         # pytorch3d's names and conventions
    w2c = pose_matrix(q, t)                                                     # autograd over the head kernels
    loss = neg_psnr_loss(pred, gt)                                              # -PSNR, differentiable in pred
    solved = refine_pose(cam, gt, stat_pc, dyn_pc, pipe, bg, steps=25, decay_start=15, lr_p=3e-3, lr_q=3e-3, lr_final=1e-4)
    result = render_test_tto(H, W, scene, test_cams, save_dir, gt_images, renderArgs=[pipe, bg])

mirrors /root/reference/eval.py:43-166 (render_test_tto) and :245-255 (the frozen Gaussians): per camera, Adam on a
quaternion and a translation of w2c through render(..., w2c=curr_w2c) with the loss -PSNR, one camera after another, step for
step, eager.  Per step the loop here is: the lean render, two launches for the loss, one for its gradient, the render's
backward restricted to the pose, and ONE launch for head backward + Adam + head forward (mobgs_pose_step).  The loss of
every step is written into a device tensor; nothing is read back inside the loop.

THE QUATERNION CONVENTION is restated from memory of pytorch3d, which is not installed here: real part first,
quaternion_to_matrix does not normalise (two_s = 2 / (q . q)).  scripts/dump_pose_vectors.py records what the package itself
gives, for a machine that has it (README, "UNPINNED").

Not here: use_sgd and loss_type != "psnr" (never enabled by the reference: NotImplementedError), batching cameras, graph
capture.  LPIPS of the written images: render_test_tto(..., lpips=model) with a mobgs_amd.lpips.LpipsAlex.  Tensors must live
on a HIP device.
"""
from __future__ import annotations

import math
import os
from typing import List, NamedTuple, Optional

import torch

from . import _lib
from ._lib import check, device_tensor, f32c, ptr, stream

BETAS, EPS = (0.9, 0.999), 1e-8          # torch.optim.Adam's defaults: eval.py:105-110 passes none


# ---- pytorch3d.transforms ---------------------------------------------------------------------------------------------

def quaternion_to_matrix(quaternions: torch.Tensor) -> torch.Tensor:
    """[..., 4] quaternions, real part first -> [..., 3, 3] rotation matrices.  NOT normalised: two_s = 2 / (q . q), so any
    non-zero q gives a rotation.  Plain torch (any device, differentiable); the kernel form is pose_matrix."""
    r, i, j, k = torch.unbind(quaternions, -1)
    two_s = 2.0 / (quaternions * quaternions).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(quaternions.shape[:-1] + (3, 3))


def matrix_to_quaternion(matrix: torch.Tensor) -> torch.Tensor:
    """[..., 3, 3] rotation matrices -> [..., 4] unit quaternions, real part first, in the matrix's dtype and on its device.
    Host-side and float64 inside (it runs once per camera): of the four ways to read q off the matrix, the one whose
    leading component is largest is taken, so nothing is divided by a small number at a trace close to -1.  The sign is
    the one that branch gives (q and -q are the same rotation, and Adam's update is odd in the gradient: both trace the
    same matrices)."""
    if matrix.shape[-2:] != (3, 3):
        raise ValueError(f"matrix_to_quaternion: expected [..., 3, 3], got {tuple(matrix.shape)}")
    m = matrix.detach().to("cpu", torch.float64).reshape(-1, 3, 3)
    m00, m11, m22 = m[:, 0, 0], m[:, 1, 1], m[:, 2, 2]
    # 4 q_c^2 for c = r, i, j, k
    four_sq = torch.stack((1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22), -1)
    # row c: 4 q_c q, read off the matrix
    cand = torch.stack((
        torch.stack((four_sq[:, 0], m[:, 2, 1] - m[:, 1, 2], m[:, 0, 2] - m[:, 2, 0], m[:, 1, 0] - m[:, 0, 1]), -1),
        torch.stack((m[:, 2, 1] - m[:, 1, 2], four_sq[:, 1], m[:, 1, 0] + m[:, 0, 1], m[:, 0, 2] + m[:, 2, 0]), -1),
        torch.stack((m[:, 0, 2] - m[:, 2, 0], m[:, 1, 0] + m[:, 0, 1], four_sq[:, 2], m[:, 2, 1] + m[:, 1, 2]), -1),
        torch.stack((m[:, 1, 0] - m[:, 0, 1], m[:, 0, 2] + m[:, 2, 0], m[:, 2, 1] + m[:, 1, 2], four_sq[:, 3]), -1)), 1)
    best = four_sq.argmax(-1)
    q = cand[torch.arange(m.shape[0]), best]
    q = q / q.norm(dim=-1, keepdim=True)
    return q.reshape(matrix.shape[:-2] + (4,)).to(matrix.dtype).to(matrix.device)


# ---- the head and the loss as autograd functions ---------------------------------------------------------------------

def _head_fwd(lib, q, t, w2c):
    check(lib.mobgs_pose_head_fwd(ptr(q), ptr(t), ptr(w2c), stream()), "mobgs_pose_head_fwd")


class _PoseMatrix(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, t):
        lib = _lib.load()
        qc, tc = f32c(q.detach()), f32c(t.detach())
        w2c = torch.empty(4, 4, dtype=torch.float32, device=q.device)
        with torch.cuda.device(q.device):
            _head_fwd(lib, qc, tc, w2c)
        ctx.save_for_backward(qc)
        return w2c

    @staticmethod
    def backward(ctx, v_w2c):
        (q,) = ctx.saved_tensors
        v = f32c(v_w2c)
        v_q, v_t = torch.empty(4, dtype=torch.float32, device=q.device), torch.empty(3, dtype=torch.float32, device=q.device)
        with torch.cuda.device(q.device):
            check(_lib.load().mobgs_pose_head_bwd(ptr(q), ptr(v), ptr(v_q), ptr(v_t), stream()), "mobgs_pose_head_bwd")
        return v_q, v_t


def pose_matrix(q: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """q [4] (real part first, not normalised), t [3] -> w2c [4,4] = [[quaternion_to_matrix(q), t], [0 0 0 1]]: eval.py:122-123
    in one launch, with the exact Jacobian in one more.  For callers who write their own loop."""
    device_tensor("pose_matrix", "q", q), device_tensor("pose_matrix", "t", t)
    if q.shape != (4,) or t.shape != (3,):
        raise ValueError(f"pose_matrix: q must be [4] and t [3], got {tuple(q.shape)} and {tuple(t.shape)}")
    return _PoseMatrix.apply(q, t)


def _loss_pair(what, pred, gt):
    device_tensor(what, "pred", pred), device_tensor(what, "gt", gt)
    if pred.shape != gt.shape or pred.numel() == 0:
        raise ValueError(f"{what}: pred and gt must have one non-empty shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")


class _NegPsnr(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt):
        lib = _lib.load()
        p, g = f32c(pred.detach()), f32c(gt.detach())
        n, dev = p.numel(), p.device
        partial = torch.empty(int(lib.mobgs_neg_psnr_scratch_doubles(n)), dtype=torch.float64, device=dev)
        mse = torch.empty(1, dtype=torch.float64, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(lib.mobgs_neg_psnr_fwd(n, ptr(p), ptr(g), ptr(partial), ptr(mse), ptr(loss), stream()),
                  "mobgs_neg_psnr_fwd")
        ctx.save_for_backward(p, g, mse)
        return loss

    @staticmethod
    def backward(ctx, v_loss):
        p, g, mse = ctx.saved_tensors
        v_pred = torch.empty_like(p)
        with torch.cuda.device(p.device):
            check(_lib.load().mobgs_neg_psnr_bwd(p.numel(), ptr(p), ptr(g), ptr(mse), ptr(f32c(v_loss)), ptr(v_pred),
                                                 stream()), "mobgs_neg_psnr_bwd")
        return v_pred, None


def neg_psnr_loss(pred: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """-20 log10(1 / sqrt(mean((pred - gt)^2))) as a 0-dim fp32 device tensor (eval.py:137-139), differentiable in pred only.
    Equal images give -inf and a gradient of NaN, as the reference's own statements do.  Bit-identical from run to run and
    from address to address."""
    _loss_pair("neg_psnr_loss", pred, gt)
    return _NegPsnr.apply(pred, gt)


# ---- the schedule ----------------------------------------------------------------------------------------------------

def tto_learning_rates(steps: int, decay_start: int, lr: float, lr_final: float) -> List[float]:
    """The learning rate each of the `steps` optimiser steps runs with under eval.py:111-115, :147-148:
    CosineAnnealingLR(T_max=steps - decay_start, eta_min=lr_final), stepped after step s only when s >= decay_start.  Closed
    form (torch steps the scheduler recursively: the two agree to a few ulps).  decay_start >= steps: the scheduler is never
    stepped and the rate is constant."""
    t_max = steps - decay_start
    rates = []
    for s in range(steps):
        k = max(0, s - decay_start)           # scheduler steps taken before optimiser step s
        rates.append(lr if k == 0 else lr_final + (lr - lr_final) * (1.0 + math.cos(math.pi * k / t_max)) / 2.0)
    return rates


def adam_step_scalars(step: int, lr: float):
    """(step_size, bias2_sqrt) of Adam's `step`-th update (1-based), formed as optim.fused_adam_step forms them."""
    return lr / (1.0 - BETAS[0] ** float(step)), math.sqrt(1.0 - BETAS[1] ** float(step))


# ---- one camera ------------------------------------------------------------------------------------------------------

class RefinedPose(NamedTuple):
    w2c: torch.Tensor            # [4,4] the solved world-to-camera matrix (row format, as render's w2c=)
    q: torch.Tensor              # [4] real part first, not normalised
    t: torch.Tensor              # [3]
    loss_history: torch.Tensor   # [steps] -PSNR before each update, on the device


def refine_pose(cam, gt, stat_pc, dyn_pc, pipe, bg, *, steps, decay_start, lr_p, lr_q, lr_final,
                q0: Optional[torch.Tensor] = None, t0: Optional[torch.Tensor] = None, stage="fine",
                **render_kw) -> RefinedPose:
    """The inner loop of eval.py:99-150 for one camera: starts at the camera's own world_view_transform (or at q0 / t0),
    runs `steps` Adam steps on (q, t) with the rates tto_learning_rates gives for lr_p (t) and lr_q (q), and returns the
    solved pose with the loss of every step, all on the device.  gt: [3,H,W].  lr_final: eta_min of both groups.

    The Gaussians and the decoder are frozen, as eval.py:245-255 freezes them: the backward pass is restricted to the pose,
    so no model tensor gains a .grad and no requires_grad flag is touched.  Nothing here waits for the device beyond what
    render() itself does."""
    from .gaussian_renderer import render
    what = "refine_pose"
    gt = f32c(device_tensor(what, "gt", gt).detach())
    H, W = int(cam.image_height), int(cam.image_width)
    if gt.shape != (3, H, W):
        raise ValueError(f"{what}: gt must be [3,{H},{W}] like the camera's image, got {tuple(gt.shape)}")
    if steps < 0:
        raise ValueError(f"{what}: steps = {steps}")
    lib = _lib.load()
    dev = gt.device
    for name, x, shape in (("q0", q0, (4,)), ("t0", t0, (3,))):
        if x is not None and (not torch.is_tensor(x) or x.shape != shape):
            # (the kernels read and write exactly 4 and 3 values through raw pointers)
            raise ValueError(f"{what}: {name} must be a tensor of shape {list(shape)}, got "
                             f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
    w2c0 = cam.world_view_transform.transpose(0, 1).detach().to(dev, torch.float32)
    t = (w2c0[:3, 3] if t0 is None else t0.detach().to(dev, torch.float32)).clone().contiguous()
    q = (matrix_to_quaternion(w2c0[:3, :3]) if q0 is None else q0.detach().to(dev, torch.float32)).clone().contiguous()
    moments = torch.zeros(2, 7, dtype=torch.float32, device=dev)            # exp_avg, exp_avg_sq: q's four, then t's three
    w2c = torch.empty(4, 4, dtype=torch.float32, device=dev)
    n = gt.numel()
    partial = torch.empty(int(lib.mobgs_neg_psnr_scratch_doubles(n)), dtype=torch.float64, device=dev)
    mse = torch.empty(1, dtype=torch.float64, device=dev)
    history = torch.empty(steps, dtype=torch.float32, device=dev)
    v_pred = torch.empty(3, H, W, dtype=torch.float32, device=dev)
    rates_p = tto_learning_rates(steps, decay_start, lr_p, lr_final)
    rates_q = tto_learning_rates(steps, decay_start, lr_q, lr_final)
    with torch.cuda.device(dev):
        _head_fwd(lib, q, t, w2c)
        w2c.requires_grad_(True)
        for s in range(steps):
            with torch.enable_grad():
                pred = render(cam, stat_pc, dyn_pc, pipe, bg, stage=stage, get_static=False, get_dynamic=False, w2c=w2c,
                              **render_kw)["render"]
            p = f32c(pred.detach())
            check(lib.mobgs_neg_psnr_fwd(n, ptr(p), ptr(gt), ptr(partial), ptr(mse), ptr(history[s:s + 1]), stream()),
                  "mobgs_neg_psnr_fwd")
            check(lib.mobgs_neg_psnr_bwd(n, ptr(p), ptr(gt), ptr(mse), None, ptr(v_pred), stream()), "mobgs_neg_psnr_bwd")
            pred.backward(v_pred, inputs=[w2c])                  # the pose only: the model's leaves are not accumulated into
            size_p, bias2_sqrt = adam_step_scalars(s + 1, rates_p[s])
            size_q, _ = adam_step_scalars(s + 1, rates_q[s])
            check(lib.mobgs_pose_step(ptr(q), ptr(t), ptr(w2c.grad), ptr(moments[0]), ptr(moments[1]), size_q, size_p,
                                      bias2_sqrt, BETAS[0], BETAS[1], EPS, ptr(w2c.detach()), stream()), "mobgs_pose_step")
            # (the kernel wrote the leaf through a raw pointer: what keys on Tensor._version must see it, as after
            # optim.fused_adam_step)
            torch.autograd.graph.increment_version(w2c)
    return RefinedPose(w2c.detach(), q, t, history)


# ---- eval.py's render_test_tto -----------------------------------------------------------------------------------------

def render_test_tto(H, W, scene, test_cams, save_dir, gt_images, tto_steps=25, decay_start=15, lr_p=0.003, lr_q=0.003,
                    lr_final=0.0001, use_sgd=False, loss_type="psnr", initialize_from_previous_camera=True,
                    initialize_from_previous_step_factor=10, initialize_from_previous_lr_factor=0.1, fg_mask_th=0.1,
                    local_viewdirs=None, batch_shape=None, renderArgs=None, ssim_data_range=2.0, lpips=None,
                    tof=None):
    """eval.py:43-166 with the reference's keyword names and defaults, ground-truth TENSORS (gt_images [K,3,H,W] in [0, 1],
    or K tensors [3,H,W]) in place of a directory of PNGs, and a result in place of None.  scene: anything with
    .stat_gaussians and .dyn_gaussians (and optionally .dataset_type); renderArgs = [pipe, background].

    Kept as written, quirks included: initialize_from_previous_camera never copies a pose -- it only gives camera 0
    step_factor = initialize_from_previous_step_factor with lr_factor 1 and every other camera step_factor 1 with
    lr_factor = initialize_from_previous_lr_factor (without it, EVERY camera gets the latter pair); every camera starts at
    its own world_view_transform; the final render asks for get_dynamic=True; fg_mask_th, local_viewdirs and batch_shape are
    accepted and unused.

    save_dir (None: nothing is written): <save_dir>/test_refined/img_<image_name>.png.png -- the doubled extension is the
    reference's -- through PIL, clamped and truncated to 8 bits as eval.py:160-162 does, and <save_dir>/solved_poses.npy.

    -> {"poses": [K,4,4], "images": [K,3,H,W] as rendered (not clamped), "loss_histories": K device tensors (camera k's
    has tto_steps * step_factor[k] entries), "step_factors", "lr_factors": what each camera ran with, "metrics":
    metrics.image_metrics(images, gt, data_range=ssim_data_range, clamp=True, quantize=True) -- the scores of the written
    PNGs, without reading them back}.  lpips: None, or a mobgs_amd.lpips.LpipsAlex: the result then also holds "lpips", its
    LpipsResult on the same pairs with clamp=True, quantize=True (metrics.py:127-131 on the written PNGs).  tof: None, True,
    or a metrics.TofTarget built from these ground truths with clamp=True: the cameras are then taken as consecutive frames
    and the result also holds "tof_per_pair" ([K-1] float64, device: metrics.temporal_of with clamp=True, quantize=True,
    metrics.py:108-120 on the written PNGs) and "tof", its mean as a Python float."""
    from .gaussian_renderer import render
    from .metrics import TofTarget, image_metrics, temporal_of
    what = "render_test_tto"
    if use_sgd:
        raise NotImplementedError(f"{what}: use_sgd=True (the reference never enables it)")
    if loss_type != "psnr":
        raise NotImplementedError(f"{what}: loss_type={loss_type!r} (the reference only runs 'psnr'; 'abs' raises there too)")
    cams = list(test_cams)
    if not cams:
        raise ValueError(f"{what}: no cameras")
    gts = list(gt_images) if not torch.is_tensor(gt_images) else list(gt_images.unbind(0))
    if len(gts) != len(cams):
        raise ValueError(f"{what}: {len(cams)} cameras but {len(gts)} ground-truth images")
    if renderArgs is None or len(renderArgs) != 2:
        raise ValueError(f"{what}: renderArgs must be [pipe, background], as eval.py passes it; got {renderArgs!r}")
    pipe, bg = renderArgs
    stat_pc, dyn_pc = scene.stat_gaussians, scene.dyn_gaussians
    device = stat_pc.get_xyz.device
    cam_type = getattr(scene, "dataset_type", None)
    poses, images, histories, step_factors, lr_factors = [], [], [], [], []
    for k, (cam, gt) in enumerate(zip(cams, gts)):
        boosted = bool(initialize_from_previous_camera) and k == 0          # the long first pass at the full rate
        step_factor = initialize_from_previous_step_factor if boosted else 1
        lr_factor = 1.0 if boosted else initialize_from_previous_lr_factor
        gt = device_tensor(what, "gt_images", gt).to(device).float()
        if gt.shape != (3, H, W):
            raise ValueError(f"{what}: ground truth {k} must be [3,{H},{W}], got {tuple(gt.shape)}")
        solved = refine_pose(cam, gt, stat_pc, dyn_pc, pipe, bg, steps=tto_steps * step_factor, decay_start=decay_start,
                             lr_p=lr_p * lr_factor, lr_q=lr_q * lr_factor, lr_final=lr_final * lr_factor, cam_type=cam_type)
        with torch.no_grad():
            final = render(cam, stat_pc, dyn_pc, pipe, bg, stage="fine", get_static=False, get_dynamic=True,
                           cam_type=cam_type, w2c=solved.w2c)["render"]
        poses.append(solved.w2c)
        images.append(final)
        histories.append(solved.loss_history)
        step_factors.append(step_factor)
        lr_factors.append(lr_factor)
    poses, images = torch.stack(poses), torch.stack(images)
    gt_stack = torch.stack([g.to(device).float() for g in gts])
    metrics = image_metrics(images, gt_stack, data_range=ssim_data_range, clamp=True, quantize=True)
    if save_dir is not None:
        import numpy as np
        from PIL import Image
        folder = os.path.join(save_dir, "test_refined")
        os.makedirs(folder, exist_ok=True)
        # 8 bits by truncation, on the device: the bytes metrics.image_metrics(quantize=True) scored
        bytes_hwc = (images.clamp(0.0, 1.0) * 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous().cpu().numpy()
        for k, cam in enumerate(cams):
            name = getattr(cam, "image_name", f"{k:05d}")
            Image.fromarray(bytes_hwc[k]).save(os.path.join(folder, f"img_{name}.png.png"))
        np.save(os.path.join(save_dir, "solved_poses.npy"), poses.cpu().numpy())
    result = {"poses": poses, "images": images, "loss_histories": histories, "step_factors": step_factors,
              "lr_factors": lr_factors, "metrics": metrics}
    if lpips is not None:
        result["lpips"] = lpips(images, gt_stack, clamp=True, quantize=True)
    if tof is not None and tof is not False:
        result["tof_per_pair"] = temporal_of(images, tof if isinstance(tof, TofTarget) else gt_stack, clamp=True,
                                             quantize=True)
        result["tof"] = float(result["tof_per_pair"].mean())
    return result
