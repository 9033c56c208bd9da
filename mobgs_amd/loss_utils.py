"""Photometric loss functions with the reference's signatures, on fused gfx950 kernels (csrc/loss.hip).

    from mobgs_amd.loss_utils import l1_loss, ssim, psnr          # drop-in for utils/loss_utils.py, utils/image_utils.py
    loss = photometric_loss(image, gt, lambda_dssim=0.2)          # L1 + lambda * (1 - SSIM) in ONE forward kernel

mirrors /root/reference/utils/loss_utils.py:233-239 (l1_loss), :351-381 (ssim, 11x11 Gaussian window sigma 1.5, zero
padding), /root/reference/utils/image_utils.py:17-38 (psnr) and the combination of /root/reference/train.py:621-628.
Gradients flow to the first argument (the rendered image); the second (ground truth) is treated as a constant, as
in every reference call.  The masked L1 exists in the reference only inside the flow-consistency loss
(train.py:651-671): `flow_warp_loss` below is that whole block -- coordinate normalisation, both grid_sample warps and
both masked L1 terms -- as one forward and one backward kernel (csrc/flowloss.hip), differentiable in all six inputs.
`exposure_ratio` is the statistic of train.py:482-491 on two flow maps (csrc/exposure.hip): no sort, no read-back.
`entropy_loss` and `sparsity_loss` (utils/loss_utils.py:264-295) and `regularisation_terms` -- the depth, entropy and
sparsity terms of train.py:651-655 with the PSNR of :622 next to them -- are one forward launch pair and one backward
launch of csrc/regterms.hip.  `lpips_loss` (utils/loss_utils.py:228-230) is the perceptual term: LpipsAlex.loss, forward and
backward on csrc/lpips.hip.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _lib
from ._lib import check, f32c, ptr, stream


class _SsimL1(torch.autograd.Function):
    """(img1, img2) [C,H,W] -> per-channel sums of the SSIM map and of |img1 - img2|."""

    @staticmethod
    def forward(ctx, img1, img2):
        lib = _lib.load()
        img1, img2 = f32c(img1), f32c(img2)
        C, H, W = img1.shape
        dev = img1.device
        nb = lib.mobgs_ssim_l1_blocks(C, H, W)
        partial = torch.empty(nb, 2, dtype=torch.float32, device=dev)
        need_grad = ctx.needs_input_grad[0]
        dmaps = torch.empty(3, C, H, W, dtype=torch.float32, device=dev) if need_grad else None
        check(lib.mobgs_ssim_l1_fwd(C, H, W, ptr(img1), ptr(img2), ptr(partial), ptr(dmaps), stream()),
              "mobgs_ssim_l1_fwd")
        sums = partial.reshape(C, -1, 2).sum(dim=1)  # [C,2], fixed order -> deterministic
        ctx.save_for_backward(img1, img2, dmaps)
        return sums[:, 0], sums[:, 1]

    @staticmethod
    def backward(ctx, v_ssim_sum, v_l1_sum):
        lib = _lib.load()
        img1, img2, dmaps = ctx.saved_tensors
        C, H, W = img1.shape
        zero = torch.zeros(C, dtype=torch.float32, device=img1.device)
        scales = torch.stack([f32c(v_ssim_sum) if v_ssim_sum is not None else zero,
                              f32c(v_l1_sum) if v_l1_sum is not None else zero], dim=1).contiguous()
        v_img1 = torch.empty_like(img1)
        check(lib.mobgs_ssim_l1_bwd(C, H, W, ptr(img1), ptr(img2), ptr(dmaps), ptr(scales), ptr(v_img1), stream()),
              "mobgs_ssim_l1_bwd")
        return v_img1, None


def _sums(img1, img2):
    if img1.shape != img2.shape:
        raise ValueError("image shapes differ")
    if img2.requires_grad:
        raise NotImplementedError("mobgs_amd.loss_utils: only the first image receives a gradient")
    H, W = img1.shape[-2:]
    s, l1 = _SsimL1.apply(img1.reshape(-1, H, W), img2.reshape(-1, H, W))
    return s, l1, H * W


def l1_loss(network_output, gt, mask=None):
    if mask is not None:
        channel = gt.shape[1]
        mask = mask.expand(-1, channel, -1, -1)
        return torch.abs((network_output - gt) * mask).sum() / (mask.sum() + 1e-8)
    # the reference's l1_loss is a plain abs().mean() that differentiates both arguments and takes any shape
    # (utils/loss_utils.py:233-239); the fused SSIM+L1 kernel is for image pairs whose second member is a constant.
    # An L1 alone (e.g. the depth term, train.py:651) does not need the 11x11 window pass either: torch.
    return torch.abs(network_output - gt).mean()


def ssim(img1, img2, window_size=11, size_average=True):
    if window_size != 11:
        raise NotImplementedError("the fused SSIM kernel is built for window_size = 11 (the reference's default)")
    s, _, hw = _sums(img1, img2)
    if size_average:
        return s.sum() / (s.numel() * hw)
    if img1.dim() != 4:
        raise ValueError("size_average=False needs [B,C,H,W] input")
    B, C = img1.shape[:2]
    return s.reshape(B, C).sum(1) / (C * hw)


def photometric_loss(image, gt, lambda_dssim=0.2):
    """L1 + lambda_dssim * (1 - SSIM) (train.py:621-628) from one forward and one backward kernel."""
    s, l1, hw = _sums(image, gt)
    n = s.numel() * hw
    ll1 = l1.sum() / n
    if lambda_dssim == 0:
        return ll1
    return ll1 + lambda_dssim * (1.0 - s.sum() / n)


class _FlowWarpLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ori, latent, e2m, m2e, la, da, combine_taps):
        lib = _lib.load()
        ori, latent, e2m, m2e, la, da = (f32c(t) for t in (ori, latent, e2m, m2e, la, da))
        B, K, _, H, W = latent.shape
        dev = ori.device
        partial = torch.empty(lib.mobgs_flow_warp_loss_blocks(B, H, W), 4, dtype=torch.float32, device=dev)
        out = torch.empty(5, dtype=torch.float32, device=dev)  # sums[4], loss
        check(lib.mobgs_flow_warp_loss_fwd(B, K, H, W, ptr(ori), ptr(latent), ptr(e2m), ptr(m2e), ptr(la), ptr(da),
                                           ptr(partial), ptr(out), ptr(out[4:]), stream()), "mobgs_flow_warp_loss_fwd")
        ctx.save_for_backward(ori, latent, e2m, m2e, la, da, out)
        ctx.combine_taps = int(combine_taps)
        return out[4]

    @staticmethod
    def backward(ctx, v):
        lib = _lib.load()
        ori, latent, e2m, m2e, la, da, out = ctx.saved_tensors
        B, K, _, H, W = latent.shape
        need = ctx.needs_input_grad
        v = f32c(v).reshape(1)
        g_ori = torch.zeros_like(ori) if need[0] else None          # scatter targets: accumulated with atomics
        g_latent = torch.zeros_like(latent) if need[1] else None
        g_e2m = torch.empty_like(e2m) if need[2] else None
        g_m2e = torch.empty_like(m2e) if need[3] else None
        g_la = torch.empty_like(la) if need[4] else None
        g_da = torch.empty_like(da) if need[5] else None
        scratch = None
        if need[0] or need[1]:
            scratch = torch.empty(lib.mobgs_flow_warp_loss_bwd_scratch_floats(B, K, H, W), dtype=torch.float32,
                                  device=ori.device)
        check(lib.mobgs_flow_warp_loss_bwd(B, K, H, W, ptr(ori), ptr(latent), ptr(e2m), ptr(m2e), ptr(la), ptr(da),
                                           ptr(out), ptr(v), ptr(g_ori), ptr(g_latent), ptr(g_e2m), ptr(g_m2e),
                                           ptr(g_la), ptr(g_da), ptr(scratch), ctx.combine_taps, stream()),
              "mobgs_flow_warp_loss_bwd")
        return g_ori, g_latent, g_e2m, g_m2e, g_la, g_da, None


def flow_warp_loss(ori_image_tensor, latent_img_final_tensor, exp2mid_coord_final_tensor, mid2exp_coord_final_tensor,
                   latent_alpha_final_tensor, d_alpha_tensor, lambda_flow_loss=1.0, combine_taps=True):
    """The flow-consistency term of /root/reference/train.py:651-671 from the tensors of :608-617:

        flow_loss = lambda_flow_loss * (l1(grid_sample(ori, norm(exp2mid)), latent, mask=latent_alpha)
                                        + l1(grid_sample(latent, norm(mid2exp)), ori, mask=d_alpha))

    ori [B,3,H,W]; latent [B,K,3,H,W]; exp2mid / mid2exp [B,K,H,W,2] pixel coordinates exactly as get_flow() returns
    them (the reference normalises them in place before sampling; this function does not modify its arguments);
    latent_alpha [B,K,1,H,W] (or [B,K,H,W]); d_alpha [B,1,H,W] (or [B,H,W]).  Differentiable in all six tensors.
    lambda_flow_loss == 0 (the shipped seesaw / children configs): a zero that is part of no graph -- the reference
    evaluates and back-propagates the whole block to multiply it by zero."""
    B, K = latent_img_final_tensor.shape[:2]
    H, W = ori_image_tensor.shape[-2:]
    if latent_img_final_tensor.shape != (B, K, 3, H, W) or ori_image_tensor.shape != (B, 3, H, W):
        raise ValueError("flow_warp_loss: ori [B,3,H,W] and latent [B,K,3,H,W] expected")
    for name, t in (("exp2mid", exp2mid_coord_final_tensor), ("mid2exp", mid2exp_coord_final_tensor)):
        if t.shape != (B, K, H, W, 2):
            raise ValueError(f"flow_warp_loss: {name} coordinates must be [B,K,H,W,2], got {tuple(t.shape)}")
    if latent_alpha_final_tensor.numel() != B * K * H * W or d_alpha_tensor.numel() != B * H * W:
        raise ValueError("flow_warp_loss: latent_alpha [B,K,1,H,W] and d_alpha [B,1,H,W] expected")
    if isinstance(lambda_flow_loss, (int, float)) and lambda_flow_loss == 0:
        return ori_image_tensor.new_zeros(())
    loss = _FlowWarpLoss.apply(ori_image_tensor, latent_img_final_tensor, exp2mid_coord_final_tensor,
                               mid2exp_coord_final_tensor, latent_alpha_final_tensor.reshape(B, K, H, W),
                               d_alpha_tensor.reshape(B, H, W), combine_taps)
    return lambda_flow_loss * loss


def lpips_loss(img1, img2, lpips_model):
    """/root/reference/utils/loss_utils.py:228-230: the mean over the batch of the perceptual distance, inputs in [-1, 1]
    as the reference's model takes them.  lpips_model: a mobgs_amd.lpips.LpipsAlex; the gradient reaches whichever image
    requires one (csrc/lpips.hip, forward and backward)."""
    return lpips_model.loss(img1, img2, normalize=False).mean()


@torch.no_grad()
def psnr(img1, img2, mask=None):
    """/root/reference/utils/image_utils.py:17-38 (mask=None branch): per-image 20 log10(1 / sqrt(mse))."""
    if mask is not None:
        raise NotImplementedError("masked psnr is not on the training path")
    mse = ((img1 - img2) ** 2).reshape(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse.float()))


@torch.no_grad()
def exposure_ratio(cam_flow, latent_flow, q=0.01, scale=1.0, out=None):
    """/root/reference/train.py:482-491 on two flow maps of equal size [...,2] (include/mobgs_hip.h K20):

        scale * median((|latent_flow| / |cam_flow|)[|cam_flow| > quantile(|cam_flow|, q)])

    bit-equal to torch.quantile / torch.median on the magnitudes sqrt(x x + y y), computed by radix select on the device:
    no sort, no boolean indexing, no host synchronisation.  -> (value, stats): stats is the int32 tensor {n_valid,
    n_nonfinite, updated, 0}.  With `out` (one fp32 element on the device, e.g. a view into a parameter) the value is
    stored there and `out` is returned as value.  Where the reference would store NaN -- no pixel above the threshold, or
    an inf / NaN magnitude in either map -- nothing is stored and updated = 0: `out` keeps its value (without `out`, value
    is NaN)."""
    lib = _lib.load()
    for name, t in (("cam_flow", cam_flow), ("latent_flow", latent_flow)):
        if not torch.is_tensor(t) or t.dim() < 1 or t.shape[-1] != 2 or t.numel() == 0:
            raise ValueError(f"exposure_ratio: {name} must be a non-empty [...,2] tensor")
        _lib.device_tensor("exposure_ratio", name, t)
    if cam_flow.numel() != latent_flow.numel() or cam_flow.device != latent_flow.device:
        raise ValueError("exposure_ratio: the two flow maps must have the same number of pixels and share a device")
    if not 0.0 <= float(q) <= 1.0:
        raise ValueError(f"exposure_ratio: quantile {q} outside [0, 1]")
    cam, lat = f32c(cam_flow.detach()), f32c(latent_flow.detach())
    dev = cam.device
    if out is None:
        value = torch.full((), float("nan"), dtype=torch.float32, device=dev)
    else:
        if not (torch.is_tensor(out) and out.is_cuda and out.device == dev and out.dtype == torch.float32
                and out.numel() == 1):
            raise ValueError("exposure_ratio: out must be one float32 element on the flow maps' device")
        value = out
    n = cam.numel() // 2
    stats = torch.empty(4, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(lib.mobgs_exposure_scratch_bytes(n)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.mobgs_exposure_estimate(n, ptr(cam), ptr(lat), float(q), float(scale), ptr(value), ptr(stats),
                                          ptr(scratch), stream()), "mobgs_exposure_estimate")
    if out is not None:   # written through a raw pointer: move Tensor._version as an in-place torch op would have
        torch.autograd.graph.increment_version(out)
    return value, stats


# include/mobgs_hip.h MOBGS_REG_ENTROPY / MOBGS_REG_SPARSITY
REG_ENTROPY, REG_SPARSITY = _lib._DEFINES["MOBGS_REG_ENTROPY"], _lib._DEFINES["MOBGS_REG_SPARSITY"]


def _numel_or_zero(t):
    return 0 if t is None else t.numel()


class _RegTerms(torch.autograd.Function):
    """(depth | None, gt_depth | None, alpha | None, image | None, gt_image | None, terms, w_d, w_e, w_s) -> (reg_loss,
    rest): reg_loss differentiable in depth and alpha, rest = {depth_loss, mask_loss, entropy, sparsity, psnr[B]} without
    a graph (include/mobgs_hip.h K21).  Backward recomputes from the inputs."""

    @staticmethod
    def forward(ctx, depth, gt_depth, alpha, image, gt_image, terms, w_d, w_e, w_s):
        lib = _lib.load()
        depth, gt_depth, alpha, image, gt_image = (None if t is None else f32c(t)
                                                   for t in (depth, gt_depth, alpha, image, gt_image))
        B, H, W = (image.shape[0], image.shape[2], image.shape[3]) if image is not None else (0, 0, 0)
        n_d, n_a = _numel_or_zero(depth), _numel_or_zero(alpha)
        dev = (depth if depth is not None else alpha).device
        nb = lib.mobgs_reg_terms_blocks(max(n_d, n_a, 3 * H * W))
        partial = torch.empty(nb, 3 + B, dtype=torch.float64, device=dev)
        out = torch.empty(5 + B, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(lib.mobgs_reg_terms_fwd(n_d, ptr(depth), ptr(gt_depth), n_a, ptr(alpha), terms, w_d, w_e, w_s, B, H, W,
                                          ptr(image), ptr(gt_image), ptr(partial), ptr(out), stream()),
                  "mobgs_reg_terms_fwd")
        ctx.save_for_backward(depth, gt_depth, alpha)
        ctx.scalars = (terms, w_d, w_e, w_s)
        rest = out[1:]
        ctx.mark_non_differentiable(rest)
        return out[0], rest

    @staticmethod
    def backward(ctx, v_reg, _v_rest):
        lib = _lib.load()
        depth, gt_depth, alpha = ctx.saved_tensors
        terms, w_d, w_e, w_s = ctx.scalars
        v = f32c(v_reg).reshape(1)
        v_depth = torch.empty_like(depth) if depth is not None and ctx.needs_input_grad[0] else None
        v_alpha = torch.empty_like(alpha) if alpha is not None and ctx.needs_input_grad[2] else None
        with torch.cuda.device(v.device):
            check(lib.mobgs_reg_terms_bwd(_numel_or_zero(depth), ptr(depth), ptr(gt_depth), _numel_or_zero(alpha),
                                          ptr(alpha), terms, w_d, w_e, w_s, ptr(v), ptr(v_depth), ptr(v_alpha),
                                          stream()), "mobgs_reg_terms_bwd")
        return v_depth, None, v_alpha, None, None, None, None, None, None


def _reg_map(what, name, t):
    if not torch.is_tensor(t) or t.numel() == 0:
        raise ValueError(f"{what}: {name} must be a non-empty tensor")
    return _lib.device_tensor(what, name, t)


def entropy_loss(alpha):
    """utils/loss_utils.py:264-276: -sum(alpha log(alpha + 1e-6) + (1 - alpha) log(1 - alpha + 1e-6)) over a map of any
    shape, differentiable in alpha; NaN for a value outside [-1e-6, 1 + 1e-6], as the reference (nothing is clamped)."""
    _reg_map("entropy_loss", "alpha", alpha)
    return _RegTerms.apply(None, None, alpha, None, None, REG_ENTROPY, 0.0, 1.0, 0.0)[0]


def sparsity_loss(alpha):
    """utils/loss_utils.py:285-295: sum(alpha ** 2) over a map of any shape, differentiable in alpha."""
    _reg_map("sparsity_loss", "alpha", alpha)
    return _RegTerms.apply(None, None, alpha, None, None, REG_SPARSITY, 0.0, 0.0, 1.0)[0]


class RegularisationTerms(NamedTuple):
    reg_loss: torch.Tensor               # differentiable in depth and d_alpha
    depth_loss: torch.Tensor             # the three below: device tensors without a graph
    mask_loss: torch.Tensor
    psnr: Optional[torch.Tensor]         # [B,1], or None without images


def regularisation_terms(depth, gt_depth, d_alpha, *, depth_weight=0.2, entropy_weight=1e-7, sparsity_weight=1e-7,
                         image=None, gt_image=None):
    """/root/reference/train.py:651-655, and :622 when the images are given, as ONE autograd node:

        depth_loss = l1_loss(depth, gt_depth);  reg_loss = 0 + depth_weight * depth_loss
        mask_loss  = entropy_weight * entropy_loss(d_alpha) + sparsity_weight * sparsity_loss(d_alpha)
        reg_loss  += mask_loss
        psnr       = psnr(image, gt_image)                     # [B,1]: per image, as utils/image_utils.py:30-31

    depth and gt_depth share a shape; d_alpha has any shape; image and gt_image are [B,3,H,W].  One forward launch pair,
    one backward launch; no synchronisation, no read-back, no allocation whose size depends on the data (it can be
    recorded into a graph).  Gradients flow to depth and d_alpha; gt_depth is a constant, the images are only measured."""
    what = "regularisation_terms"
    for name, t in (("depth", depth), ("gt_depth", gt_depth), ("d_alpha", d_alpha)):
        _reg_map(what, name, t)
    if depth.shape != gt_depth.shape:
        raise ValueError(f"{what}: depth {tuple(depth.shape)} and gt_depth {tuple(gt_depth.shape)} differ in shape")
    if gt_depth.requires_grad:
        raise NotImplementedError("mobgs_amd.loss_utils: only depth and d_alpha receive a gradient, gt_depth does not")
    if (image is None) != (gt_image is None):
        raise ValueError(f"{what}: image and gt_image go together")
    if image is not None:
        for name, t in (("image", image), ("gt_image", gt_image)):
            _reg_map(what, name, t)
        if image.dim() != 4 or image.shape[1] != 3 or image.shape != gt_image.shape:
            raise ValueError(f"{what}: image and gt_image must both be [B,3,H,W]")
        image, gt_image = image.detach(), gt_image.detach()
    reg, rest = _RegTerms.apply(depth, gt_depth, d_alpha, image, gt_image, REG_ENTROPY | REG_SPARSITY,
                                float(depth_weight), float(entropy_weight), float(sparsity_weight))
    return RegularisationTerms(reg, rest[0], rest[1], rest[4:].reshape(-1, 1) if image is not None else None)
