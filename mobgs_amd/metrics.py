"""Evaluation metrics on the HIP path (csrc/metrics.hip, include/mobgs_hip.h K22): what the reference scores a trained
model with, for a whole batch of image pairs in one call, without scikit-image, OpenCV or jax.

    m = image_metrics(pred, gt, mask, data_range=2.0)      # [B,3,H,W] pairs -> a record of [B] float64 device tensors
    report = evaluate_views(cams, stat_pc, dyn_pc, pipe, bg, gt_images)   # training_report's loop, one scoring call

mirrors /root/reference/metrics.py:54-79 and :123-125 (calculate_ssim, calculate_psnr, skimage's peak_signal_noise_ratio
and structural_similarity), dycheck_metrics.py:67-200 (compute_psnr, compute_ssim), train.py:879-938 (training_report) and
train.py:757-760 (the aligned test pose).  Forward only, under no_grad; tensors must live on a HIP device.

THE DATA RANGE.  metrics.py calls structural_similarity without a data_range on float images.  On the scikit-image
versions that still accept multichannel=True (<= 0.18) this means R = 2 (the range of the dtype, -1 .. 1), not 1: C1 and C2
are four times what the images' own range would give.  This is a reading of that package's source; nobody could run it
here.  So `data_range` is a required keyword of everything below that evaluates the box SSIM, and evaluate_views defaults
to 2.0 (README, "UNPINNED").

LPIPS is mobgs_amd.lpips (csrc/lpips.hip, K24); evaluate_views(..., lpips=model) adds it.  Not here: tOF (OpenCV's
Farneback flow), gradients.  The test-time pose optimisation of eval.py is mobgs_amd.tto, which scores its images through
image_metrics(clamp=True, quantize=True).
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._lib import check, f32c, ptr, stream

ARMS = {"box": _lib._DEFINES["MOBGS_METRICS_BOX"], "gauss": _lib._DEFINES["MOBGS_METRICS_GAUSS"]}
CLAMP, QUANTIZE = _lib._DEFINES["MOBGS_METRICS_CLAMP"], _lib._DEFINES["MOBGS_METRICS_QUANTIZE"]
COLUMNS = _lib._DEFINES["MOBGS_METRICS_COLUMNS"]
MIN_EDGE = {"box": 7, "gauss": 11}


class ImageMetrics(NamedTuple):
    """[B] float64 device tensors (include/mobgs_hip.h K22 has the formulas); None for an SSIM window not asked for."""
    l1: torch.Tensor
    mse: torch.Tensor
    psnr: torch.Tensor                       # 20 log10(1 / sqrt(mse)): training_report's
    psnr_masked: torch.Tensor                # dycheck's: -10 / ln 10 * ln(sum se m / max(sum m, 1e-6))
    ssim_box: Optional[torch.Tensor]         # skimage structural_similarity(multichannel=True)
    ssim_box_masked: Optional[torch.Tensor]  # metrics.py calculate_ssim
    ssim_gauss: Optional[torch.Tensor]       # dycheck compute_ssim (partial convolution)
    se_masked: torch.Tensor                  # sum (pred - gt)^2 mask, and the sum of the mask broadcast to [3,H,W]
    mask_sum: torch.Tensor


def _device_image(what, name, t):
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: {name} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{what}: tensors must live on a HIP device (device='cuda'); there is no CPU path")
    return t


@torch.no_grad()
def image_metrics(pred, gt, mask=None, *, data_range, clamp=False, quantize=False, arms=("box", "gauss")) -> ImageMetrics:
    """Scores B image pairs in one call: pred, gt [B,3,H,W] (or [3,H,W]), mask [B,H,W] / [B,1,H,W] of {0, 1} or None.

    clamp: both images are clamped to [0, 1] first (train.py:903-907).  quantize: the prediction is then replaced by its
    8-bit version, floor(clip(pred, 0, 1) * 255) / 255 in fp32 (eval.py:162): the metrics equal what metrics.py computes
    from the written PNG, without writing one.  data_range: R of the SSIM constants C1 = (0.01 R)^2, C2 = (0.03 R)^2 (see the
    module docstring; dycheck's max_val).  arms: the SSIM windows to evaluate; "box" needs H, W >= 7, "gauss" >= 11
    (ValueError otherwise).  Two or three launches on the current stream, no synchronisation, no allocation that depends on
    the data: the call can be recorded into a graph.  Bit-identical from run to run, and per image whatever the batch."""
    what = "image_metrics"
    pred, gt = _device_image(what, "pred", pred), _device_image(what, "gt", gt)
    if pred.dim() == 3:
        pred, gt = pred[None], gt[None] if gt.dim() == 3 else gt
    if pred.dim() != 4 or pred.shape[1] != 3 or pred.shape != gt.shape:
        raise ValueError(f"{what}: pred and gt must both be [B,3,H,W], got {tuple(pred.shape)} and {tuple(gt.shape)}")
    B, _, H, W = pred.shape
    if B < 1:
        raise ValueError(f"{what}: an empty batch")
    arms = (arms,) if isinstance(arms, str) else tuple(arms)
    if not arms or any(a not in ARMS for a in arms):
        raise ValueError(f"{what}: arms must name at least one of {tuple(ARMS)}, got {arms}")
    for a in arms:
        if H < MIN_EDGE[a] or W < MIN_EDGE[a]:
            raise ValueError(f"{what}: the {a} SSIM window needs H, W >= {MIN_EDGE[a]}, got {H} x {W}")
    if not (float(data_range) > 0.0 and math.isfinite(float(data_range))):
        raise ValueError(f"{what}: data_range must be positive and finite, got {data_range}")
    if mask is not None:
        _device_image(what, "mask", mask)
        if mask.numel() != B * H * W or mask.shape[-2:] != (H, W):
            raise ValueError(f"{what}: mask must be [B,H,W] or [B,1,H,W], got {tuple(mask.shape)}")
        mask = f32c(mask.detach().reshape(B, H, W))
    pred, gt = f32c(pred.detach()), f32c(gt.detach())
    lib = _lib.load()
    dev = pred.device
    partial = torch.empty(int(lib.mobgs_image_metrics_scratch_doubles(B, H, W)), dtype=torch.float64, device=dev)
    out = torch.empty(B, COLUMNS, dtype=torch.float64, device=dev)
    bits = sum({ARMS[a] for a in arms})
    flags = (CLAMP if clamp else 0) | (QUANTIZE if quantize else 0)
    with torch.cuda.device(dev):
        check(lib.mobgs_image_metrics(B, H, W, ptr(pred), ptr(gt), ptr(mask), bits, flags, float(data_range), ptr(partial),
                                      ptr(out), stream()), "mobgs_image_metrics")
    col = out.unbind(1)
    box, gauss = "box" in arms, "gauss" in arms
    return ImageMetrics(col[0], col[1], col[2], col[3], col[4] if box else None, col[5] if box else None,
                        col[6] if gauss else None, col[7], col[8])


# ---- the reference's names: one HWC image pair in, one number out -------------------------------------------------------

def _chw(what, name, img):
    """[H,W,3] array or tensor -> [1,3,H,W] device tensor (an array is uploaded; a host TENSOR is refused like everywhere)."""
    if not torch.is_tensor(img):
        img = torch.as_tensor(img).to("cuda")
    _device_image(what, name, img)
    if img.dim() != 3 or img.shape[-1] != 3:
        raise ValueError(f"{what}: {name} must be [H,W,3], got {tuple(img.shape)}")
    return img.permute(2, 0, 1)[None]


def _hw_mask(what, mask, like):
    """None, [H,W], [H,W,1] or [H,W,3] (its first channel) -> None or [1,H,W] on the images' device."""
    if mask is None:
        return None
    if not torch.is_tensor(mask):
        mask = torch.as_tensor(mask).to(like.device)
    _device_image(what, "mask", mask)
    if mask.dim() == 3:
        mask = mask[..., 0]
    if mask.shape != like.shape[-2:]:
        raise ValueError(f"{what}: mask must be [H,W], [H,W,1] or [H,W,3], got {tuple(mask.shape)}")
    return mask[None]


def compute_psnr(img0, img1, mask=None) -> float:
    """dycheck_metrics.py:67-92: -10 / ln 10 * ln(masked mean of the squared error); +inf where that mean is 0 (equal
    images, an empty mask)."""
    a = _chw("compute_psnr", "img0", img0)
    m = image_metrics(a, _chw("compute_psnr", "img1", img1), _hw_mask("compute_psnr", mask, a), data_range=1.0,
                      arms=("box",))
    return float(m.psnr_masked)


def compute_ssim(img0, img1, mask=None, max_val=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03) -> float:
    """dycheck_metrics.py:95-200; exactly 1.0 for an empty mask."""
    if (filter_size, filter_sigma, k1, k2) != (11, 1.5, 0.01, 0.03):
        raise NotImplementedError("compute_ssim: the kernel is built for filter_size 11, sigma 1.5, k1 0.01, k2 0.03")
    a = _chw("compute_ssim", "img0", img0)
    m = image_metrics(a, _chw("compute_ssim", "img1", img1), _hw_mask("compute_ssim", mask, a), data_range=max_val,
                      arms=("gauss",))
    return float(m.ssim_gauss)


def calculate_psnr(img1, img2, mask) -> float:
    """metrics.py:66-79: 10 log10(1 / mse) with mse = sum(se mask) / (sum(mask) + 1e-8), the mask broadcast over the
    channels; 0 (not +inf) when mse == 0, as the reference returns."""
    a = _chw("calculate_psnr", "img1", img1)
    m = image_metrics(a, _chw("calculate_psnr", "img2", img2), _hw_mask("calculate_psnr", mask, a), data_range=1.0,
                      arms=("box",))
    mse = float(m.se_masked) / (float(m.mask_sum) + 1e-8)
    return 0 if mse == 0 else 10 * math.log10(1.0 / mse)


def calculate_ssim(img1, img2, mask, *, data_range) -> float:
    """metrics.py:54-64: sum(ssim_map mask) / (sum(mask) + 1e-8) over the uncropped box-window map, the mask broadcast over
    the channels."""
    a = _chw("calculate_ssim", "img1", img1)
    m = image_metrics(a, _chw("calculate_ssim", "img2", img2), _hw_mask("calculate_ssim", mask, a), data_range=data_range,
                      arms=("box",))
    return float(m.ssim_box_masked)


def peak_signal_noise_ratio(image_true, image_test, *, data_range) -> float:
    """skimage.metrics.peak_signal_noise_ratio as metrics.py:123 calls it: 10 log10(data_range^2 / mse).  (Without a
    data_range scikit-image takes 1 for float images that are not negative, 2 otherwise.)"""
    a = _chw("peak_signal_noise_ratio", "image_true", image_true)
    m = image_metrics(a, _chw("peak_signal_noise_ratio", "image_test", image_test), data_range=1.0, arms=("box",))
    mse = float(m.mse)
    return math.inf if mse == 0 else 10 * math.log10(float(data_range) ** 2 / mse)


def structural_similarity(im1, im2, *, data_range, multichannel=True, full=False) -> float:
    """skimage.metrics.structural_similarity(im1, im2, multichannel=True) as metrics.py:124 calls it (7x7 uniform window,
    sample covariance, the mean over the map cropped by 3).  data_range: see the module docstring."""
    if not multichannel or full:
        raise NotImplementedError("structural_similarity: only multichannel=True, full=False (the map is not stored)")
    a = _chw("structural_similarity", "im1", im1)
    m = image_metrics(a, _chw("structural_similarity", "im2", im2), data_range=data_range, arms=("box",))
    return float(m.ssim_box)


# ---- training_report ---------------------------------------------------------------------------------------------------

def aligned_test_pose(input_train, input_test, output_train):
    """train.py:757-760: the test camera's pose carried along with the optimised training pose,
    input_test @ inverse(input_train) @ output_train (world_view_transform matrices, [4,4] or batched), on their device."""
    return input_test @ torch.linalg.inv(input_train) @ output_train


@torch.no_grad()
def evaluate_views(cams, stat_pc, dyn_pc, pipe, bg, gt_images, *, stage="fine", ssim_data_range=2.0, lpips=None,
                   **render_kw):
    """The test loop of training_report (train.py:895-925) with the SSIMs next to it: renders every camera through
    gaussian_renderer.render, stacks the images and scores them against gt_images ([K,3,H,W], or K tensors [3,H,W]) in ONE
    image_metrics call with clamp=True, then reads the result back ONCE.

    ssim_data_range = 2.0: what metrics.py's structural_similarity call means on scikit-image <= 0.18 for float images
    (see the module docstring; this is a reading of that package's source, nobody could run it here).

    -> {"per_view": ImageMetrics (device, [K]), "l1", "psnr", "ssim_box", "ssim_gauss": the means over the views as Python
    floats (l1 and psnr are what training_report prints), "images": [K,3,H,W] as rendered (not clamped)}.

    lpips: None, or a mobgs_amd.lpips.LpipsAlex: the result then also holds "lpips_per_view" ([K] float64, device: the
    model on the clamped images, in the same pass) and "lpips", its mean as a Python float."""
    from .gaussian_renderer import render
    cams = list(cams)
    if not cams:
        raise ValueError("evaluate_views: no cameras")
    images = torch.stack([render(cam, stat_pc, dyn_pc, pipe, bg, stage=stage, **render_kw)["render"] for cam in cams])
    gt = gt_images if torch.is_tensor(gt_images) else torch.stack(list(gt_images))
    per_view = image_metrics(images, gt.to(images.device), data_range=ssim_data_range, clamp=True)
    means = torch.stack([per_view.l1, per_view.psnr, per_view.ssim_box, per_view.ssim_gauss]).mean(1).tolist()
    report = {"per_view": per_view, "l1": means[0], "psnr": means[1], "ssim_box": means[2], "ssim_gauss": means[3],
              "images": images}
    if lpips is not None:
        report["lpips_per_view"] = lpips(images, gt.to(images.device), clamp=True).total
        report["lpips"] = float(report["lpips_per_view"].mean())
    return report
