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

LPIPS is mobgs_amd.lpips (csrc/lpips.hip, K24); evaluate_views(..., lpips=model) adds it, compute_lpips is dycheck's masked
one, and evaluate_views(..., masks=) reports dycheck's masked triple mPSNR / mSSIM / mLPIPS.  tOF, the temporal optical-flow
metric of metrics.py:14-47 and :108-120 (OpenCV's Farneback flow between consecutive frames, prediction against ground truth),
is temporal_of / TofTarget below (csrc/tof.hip, K25); evaluate_views(..., tof=True) adds it.  Not here: gradients.  The
test-time pose optimisation of eval.py is mobgs_amd.tto, which scores its images through image_metrics(clamp=True,
quantize=True).

    flows = farneback_flow(grey_frames(frames))             # [F,3,H,W] -> [F,H,W] 8-bit grey -> [F-1,H,W,2]
    tof = temporal_of(pred, gt)                              # [F-1] float64, device; .mean() is the reference's mean_tof
    target = TofTarget.from_frames(gt); temporal_of(pred, target)   # the ground truth's flows computed once
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._lib import check, device_tensor, f32c, ptr, stream

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


def _flags(clamp, quantize) -> int:
    return (CLAMP if clamp else 0) | (QUANTIZE if quantize else 0)


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
    pred, gt = device_tensor(what, "pred", pred), device_tensor(what, "gt", gt)
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
        device_tensor(what, "mask", mask)
        if mask.numel() != B * H * W or mask.shape[-2:] != (H, W):
            raise ValueError(f"{what}: mask must be [B,H,W] or [B,1,H,W], got {tuple(mask.shape)}")
        mask = f32c(mask.detach().reshape(B, H, W))
    pred, gt = f32c(pred.detach()), f32c(gt.detach())
    lib = _lib.load()
    dev = pred.device
    partial = torch.empty(int(lib.mobgs_image_metrics_scratch_doubles(B, H, W)), dtype=torch.float64, device=dev)
    out = torch.empty(B, COLUMNS, dtype=torch.float64, device=dev)
    bits = sum({ARMS[a] for a in arms})
    with torch.cuda.device(dev):
        check(lib.mobgs_image_metrics(B, H, W, ptr(pred), ptr(gt), ptr(mask), bits, _flags(clamp, quantize), float(data_range), ptr(partial),
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
    device_tensor(what, name, img)
    if img.dim() != 3 or img.shape[-1] != 3:
        raise ValueError(f"{what}: {name} must be [H,W,3], got {tuple(img.shape)}")
    return img.permute(2, 0, 1)[None]


def _hw_mask(what, mask, like):
    """None, [H,W], [H,W,1] or [H,W,3] (its first channel) -> None or [1,H,W] on the images' device."""
    if mask is None:
        return None
    if not torch.is_tensor(mask):
        mask = torch.as_tensor(mask).to(like.device)
    device_tensor(what, "mask", mask)
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


@torch.no_grad()
def compute_lpips(lpips_model, img0, img1, mask=None, device=None) -> float:
    """dycheck_metrics.py:203-244 (mLPIPS): both images [H,W,3] in [0, 1] are multiplied by the mask ([H,W,1] or [H,W];
    None = ones), mapped to [-1, 1], and the masked mean of the model's spatial map is returned, sum(map m) / max(sum(m),
    1e-6); 0 for an empty mask.  lpips_model: a mobgs_amd.lpips.LpipsAlex.  device: where arrays are uploaded to (default:
    the model's device); tensors must already live on a HIP device."""
    what = "compute_lpips"
    dev = device if device is not None else getattr(lpips_model, "device", "cuda")

    def up(x):
        return x if torch.is_tensor(x) else torch.as_tensor(x).to(dev)

    a, b = _chw(what, "img0", up(img0)), _chw(what, "img1", up(img1))
    if a.shape != b.shape:
        raise ValueError(f"{what}: img0 and img1 must have one shape, got {tuple(a.shape[-2:])} and {tuple(b.shape[-2:])}")
    m = _hw_mask(what, None if mask is None else up(mask), a)
    if m is None:
        m = torch.ones(1, a.shape[2], a.shape[3], device=a.device)
    m = m.to(torch.float32)
    r = lpips_model.spatial(a.float() * m[:, None], b.float() * m[:, None], m, want_map=False)
    return float(r.masked_mean)


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


# ---- tOF: Farneback flow between consecutive frames, prediction against ground truth (K25) ---------------------------------

TOF_MIN_EDGE = 48                    # below it crop_8x8's window is empty
TOF_SCRATCH_BUDGET = 1 << 30         # bytes of scratch per mobgs_tof_flow call; longer sequences run in overlapping pieces


def _tof_frames(what, name, t, channels):
    device_tensor(what, name, t)
    want = "[F,3,H,W]" if channels else "[F,H,W]"
    if t.dim() != (4 if channels else 3) or (channels and t.shape[1] != 3):
        raise ValueError(f"{what}: {name} must be {want}, got {tuple(t.shape)}")
    if t.shape[-2] < TOF_MIN_EDGE or t.shape[-1] < TOF_MIN_EDGE:
        raise ValueError(f"{what}: {name} needs H, W >= {TOF_MIN_EDGE} (crop_8x8's window is empty below), got "
                         f"{t.shape[-2]} x {t.shape[-1]}")
    return f32c(t.detach())


def crop_window(H, W):
    """metrics.py:32-47 -> (y, x, h, w) of crop_8x8's window (the library's own arithmetic: mobgs_tof_crop)."""
    import ctypes
    yxhw = (ctypes.c_int32 * 4)()
    check(_lib.load().mobgs_tof_crop(int(H), int(W), ctypes.cast(yxhw, ctypes.c_void_p)), "mobgs_tof_crop")
    return tuple(yxhw)


def crop_8x8(img):
    """metrics.py:32-47 on a [H,W] or [H,W,C] tensor (or array): -> (the window, a view; y; x)."""
    if img.shape[0] < TOF_MIN_EDGE or img.shape[1] < TOF_MIN_EDGE:
        raise ValueError(f"crop_8x8: needs H, W >= {TOF_MIN_EDGE}, got {img.shape[0]} x {img.shape[1]}")
    y, x, h, w = crop_window(img.shape[0], img.shape[1])
    return img[y:y + h, x:x + w], y, x


@torch.no_grad()
def grey_frames(frames, *, clamp=False, quantize=False):
    """[F,3,H,W] float images -> [F,H,W] fp32 holding the 8-bit grey values the reference hands to OpenCV
    (metrics.py:109-110: (img * 255.0).astype(np.uint8) in fp32, then cv2.COLOR_RGB2GRAY in 14-bit fixed point).  clamp:
    clip to [0, 1] first; quantize: then floor(clip(x) * 255) / 255 in fp32, the written PNG read back.  One launch."""
    what = "grey_frames"
    frames = _tof_frames(what, "frames", frames, True)
    F_, _, H, W = frames.shape
    grey = torch.empty(F_, H, W, dtype=torch.float32, device=frames.device)
    with torch.cuda.device(frames.device):
        check(_lib.load().mobgs_tof_grey(F_, H, W, ptr(frames), _flags(clamp, quantize), ptr(grey), stream()), "mobgs_tof_grey")
    return grey


@torch.no_grad()
def farneback_flow(frames_grey):
    """[F,H,W] grey frames (8-bit values in a float tensor) -> [F-1,H,W,2] fp32: cv2.calcOpticalFlowFarneback(prev, next, None,
    0.5, 3, 15, 3, 5, 1.2, 0) of every consecutive pair, channel 0 along x.  Six launches per pyramid level (at most 24) per
    piece of the sequence; a sequence whose scratch would pass TOF_SCRATCH_BUDGET runs in pieces that overlap by one frame,
    which changes no bit of any pair's flow.  No synchronisation; bit-identical from run to run and whatever F is."""
    what = "farneback_flow"
    grey = _tof_frames(what, "frames_grey", frames_grey, False)
    F_, H, W = grey.shape
    if F_ < 2:
        raise ValueError(f"{what}: needs at least two frames, got {F_}")
    lib = _lib.load()
    dev = grey.device
    flow = torch.empty(F_ - 1, H, W, 2, dtype=torch.float32, device=dev)
    piece = F_
    while piece > 2 and int(lib.mobgs_tof_scratch_bytes(piece, H, W)) > TOF_SCRATCH_BUDGET:
        piece -= 1
    nbytes = int(lib.mobgs_tof_scratch_bytes(piece, H, W))
    if nbytes == 0:
        raise ValueError(f"{what}: the library refuses F = {piece}, H = {H}, W = {W}")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        for first in range(0, F_ - 1, piece - 1):
            n = min(piece, F_ - first)
            check(lib.mobgs_tof_flow(n, H, W, ptr(grey[first:first + n]), ptr(scratch), ptr(flow[first:first + n - 1]),
                                     stream()), "mobgs_tof_flow")
    return flow


@torch.no_grad()
def flow_distance(flow_a, flow_b, mask=None):
    """Two flow stacks [P,H,W,2] (mask [P,H,W] of weights, or None) -> [P] float64 on the device: per pair the mean of
    |flow_a - flow_b|_2 over crop_8x8's window, or sum(. mask) / sum(mask) (metrics.py:18-29).  Two launches."""
    what = "flow_distance"
    device_tensor(what, "flow_a", flow_a), device_tensor(what, "flow_b", flow_b)
    if flow_a.dim() != 4 or flow_a.shape[-1] != 2 or flow_a.shape != flow_b.shape:
        raise ValueError(f"{what}: flows must both be [P,H,W,2], got {tuple(flow_a.shape)} and {tuple(flow_b.shape)}")
    P, H, W, _ = flow_a.shape
    if P < 1 or H < TOF_MIN_EDGE or W < TOF_MIN_EDGE:
        raise ValueError(f"{what}: needs P >= 1 and H, W >= {TOF_MIN_EDGE}, got {tuple(flow_a.shape)}")
    if mask is not None:
        device_tensor(what, "mask", mask)
        if mask.numel() != P * H * W or mask.shape[-2:] != (H, W):
            raise ValueError(f"{what}: mask must be [P,H,W] or [P,1,H,W], got {tuple(mask.shape)}")
        mask = f32c(mask.detach().reshape(P, H, W))
    flow_a, flow_b = f32c(flow_a.detach()), f32c(flow_b.detach())
    lib = _lib.load()
    dev = flow_a.device
    partial = torch.empty(int(lib.mobgs_tof_score_scratch_doubles(P, H, W)), dtype=torch.float64, device=dev)
    out = torch.empty(P, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib.mobgs_tof_score(P, H, W, ptr(flow_a), ptr(flow_b), ptr(mask), ptr(partial), ptr(out), stream()),
              "mobgs_tof_score")
    return out


class TofTarget:
    """The ground truth's side of tOF: its F - 1 flows, computed once.  They do not change between evaluations, and
    training_report runs at every testing iteration: temporal_of(pred, target) then computes the prediction's flows only.
    (The flows are kept whole; crop_8x8's window is an index range of the scoring kernel.)"""

    def __init__(self, flows):
        self.flows = flows

    @classmethod
    def from_frames(cls, gt, *, clamp=False):
        """gt [F,3,H,W] in [0, 1] (clamp: clipped to it first, as evaluate_views scores its images)."""
        return cls(farneback_flow(grey_frames(gt, clamp=clamp)))

    @property
    def frames(self):
        return self.flows.shape[0] + 1


@torch.no_grad()
def temporal_of(pred, gt, mask=None, *, clamp=False, quantize=False):
    """tOF of a sequence: pred [F,3,H,W], gt [F,3,H,W] or a TofTarget of F frames, mask [F-1,H,W] or None (pair p = frames
    p, p + 1) -> [F-1] float64 on the device; its mean is the reference's mean_tof (metrics.py:141-142: the -1.0 of frame 0
    is filtered out there).  clamp: both sequences are clipped to [0, 1] first; quantize: the prediction is then replaced by
    its 8-bit version, as image_metrics does: the tOF of the written PNGs without writing them.  No synchronisation."""
    what = "temporal_of"
    flows = farneback_flow(grey_frames(pred, clamp=clamp, quantize=quantize))
    if isinstance(gt, TofTarget):
        if gt.flows.shape != flows.shape:
            raise ValueError(f"{what}: the target holds flows {tuple(gt.flows.shape)}, the prediction gives "
                             f"{tuple(flows.shape)}")
        target = gt.flows
    else:
        device_tensor(what, "gt", gt)
        if gt.shape != pred.shape:
            raise ValueError(f"{what}: pred and gt must have one shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")
        target = farneback_flow(grey_frames(gt.to(flows.device), clamp=clamp))
    return flow_distance(target, flows, mask)


def _grey_hw(what, name, img):
    if not torch.is_tensor(img):
        img = torch.as_tensor(img).to("cuda")
    device_tensor(what, name, img)
    if img.dim() != 2:
        raise ValueError(f"{what}: {name} must be a [H,W] grey image, got {tuple(img.shape)}")
    return img.float()


def get_tOF(pre_gt_grey, gt_grey, pre_output_grey, output_grey, mask=None) -> float:
    """metrics.py:14-29 under its own name: four [H,W] 8-bit grey images (device tensors of any dtype, or arrays, which are
    uploaded), mask [H,W] / [H,W,1] or None -> the tOF of the pair as a Python float."""
    what = "get_tOF"
    a = torch.stack([_grey_hw(what, "pre_gt_grey", pre_gt_grey), _grey_hw(what, "gt_grey", gt_grey)])
    b = torch.stack([_grey_hw(what, "pre_output_grey", pre_output_grey), _grey_hw(what, "output_grey", output_grey)])
    if mask is not None:
        if not torch.is_tensor(mask):
            mask = torch.as_tensor(mask).to(a.device)
        mask = mask.squeeze()[None]
    return float(flow_distance(farneback_flow(a), farneback_flow(b), mask))


# ---- training_report ---------------------------------------------------------------------------------------------------

def aligned_test_pose(input_train, input_test, output_train):
    """train.py:757-760: the test camera's pose carried along with the optimised training pose,
    input_test @ inverse(input_train) @ output_train (world_view_transform matrices, [4,4] or batched), on their device."""
    return input_test @ torch.linalg.inv(input_train) @ output_train


@torch.no_grad()
def evaluate_views(cams, stat_pc, dyn_pc, pipe, bg, gt_images, *, stage="fine", ssim_data_range=2.0, lpips=None,
                   tof=None, masks=None, **render_kw):
    """The test loop of training_report (train.py:895-925) with the SSIMs next to it: renders every camera through
    gaussian_renderer.render, stacks the images and scores them against gt_images ([K,3,H,W], or K tensors [3,H,W]) in ONE
    image_metrics call with clamp=True, then reads the result back ONCE.

    ssim_data_range = 2.0: what metrics.py's structural_similarity call means on scikit-image <= 0.18 for float images
    (see the module docstring; this is a reading of that package's source, nobody could run it here).

    -> {"per_view": ImageMetrics (device, [K]), "l1", "psnr", "ssim_box", "ssim_gauss": the means over the views as Python
    floats (l1 and psnr are what training_report prints), "images": [K,3,H,W] as rendered (not clamped)}.

    lpips: None, or a mobgs_amd.lpips.LpipsAlex: the result then also holds "lpips_per_view" ([K] float64, device: the
    model on the clamped images, in the same pass) and "lpips", its mean as a Python float.

    tof: None, True, or a TofTarget built from these ground truths with clamp=True: the cameras are then taken as
    consecutive frames, and the result also holds "tof_per_pair" ([K-1] float64, device: temporal_of on the clamped images)
    and "tof", its mean as a Python float -- the mean_tof metrics.py:141-142 prints.  Needs K >= 2 and H, W >= 48.

    masks: None, or [K,H,W] / [K,1,H,W] co-visibility masks in [0, 1]: the result then also holds dycheck's masked triple on
    the clamped images: "mpsnr" and "mssim" (the means of a second image_metrics call with the mask and data_range 1:
    psnr_masked and the masked ssim_gauss; "per_view_masked" is its record) and, with lpips, "mlpips_per_view" ([K] float64,
    device: compute_lpips's convention, both images times the mask, then the masked mean of the spatial map) and "mlpips".
    Every other entry is what it is without masks."""
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
    if masks is not None:
        gt_dev = gt.to(images.device)
        masked = image_metrics(images, gt_dev, masks, data_range=1.0, clamp=True, arms=("gauss",))
        report["per_view_masked"] = masked
        report["mpsnr"], report["mssim"] = torch.stack([masked.psnr_masked, masked.ssim_gauss]).mean(1).tolist()
        if lpips is not None:
            m = masks.detach().reshape(len(cams), 1, *images.shape[-2:]).to(images.device, torch.float32)
            report["mlpips_per_view"] = lpips.spatial(images.clamp(0, 1) * m, gt_dev.clamp(0, 1) * m, m[:, 0],
                                                      want_map=False).masked_mean
            report["mlpips"] = float(report["mlpips_per_view"].mean())
    if tof is not None and tof is not False:
        report["tof_per_pair"] = temporal_of(images, tof if isinstance(tof, TofTarget) else gt.to(images.device), clamp=True)
        report["tof"] = float(report["tof_per_pair"].mean())
    return report
