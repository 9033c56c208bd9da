"""The regularisation block of the training loss (include/mobgs_hip.h K21) restated in torch on the CPU, for the tests
to compare against: the statements of /root/reference/train.py:651-655 and :622 in our own words, parameterised by dtype.

    block(depth, gt_depth, alpha, image, gt_image, dtype)   values and autograd gradients of the whole block
    alone(alpha, dtype)                                     entropy_loss and sparsity_loss on their own, with gradients

dtype=torch.float32 runs the same torch operations in the same order as the reference's functions, so on the CPU it
reproduces their values and gradients bit for bit (tests/test_regterms_cpu.py holds it to that against the fixture that
tests/golden/make_golden_regterms.py records from the reference itself).  dtype=torch.float64 is the truth the GPU tests
measure against: inputs widened exactly, weights and epsilon as Python floats.

Also here: the fixture's cases (make_case), the tolerance rule of the GPU tests (allowed, gaps) and the random maps of
the grid-stride test (random_maps)."""
from __future__ import annotations

import math

import torch

EPS = 1e-6
W_DEPTH, W_ENTROPY, W_SPARSITY = 0.2, 1e-7, 1e-7       # train.py:652, :654
CASES = ((1, 5, 3), (2, 37, 53), (2, 96, 160))         # (B, H, W)
SCALARS = ("reg_loss", "depth_loss", "mask_loss", "entropy", "sparsity")
FLOOR = 8 * 2.0 ** -24                                 # an fp32 result's own rounding chain, relative
FLOOR_DB = 10.0 / math.log(10.0) * FLOOR               # ... of a mean squared error, seen through 10 log10


def l1(a, b):
    return torch.abs(a - b).mean()


def entropy(alpha):
    return -torch.sum(alpha * torch.log(alpha + EPS) + (1 - alpha) * torch.log(1 - alpha + EPS))


def sparsity(alpha):
    return torch.sum(alpha ** 2)


def psnr(image, gt_image):
    mse = ((image - gt_image) ** 2).view(image.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def _leaf(t, dtype):
    return t.detach().to(dtype).clone().requires_grad_(True)


def block(depth, gt_depth, alpha, image=None, gt_image=None, dtype=torch.float32, w_depth=W_DEPTH, w_entropy=W_ENTROPY,
          w_sparsity=W_SPARSITY, cotangent=1.0):
    """-> {reg_loss, depth_loss, mask_loss, entropy, sparsity, psnr ([B,1] or absent), g_depth, g_alpha}: the block as
    train.py writes it, and the gradients of cotangent * reg_loss."""
    d, a = _leaf(depth, dtype), _leaf(alpha, dtype)
    reg_loss = 0
    depth_loss = l1(d, gt_depth.to(dtype))
    reg_loss += w_depth * depth_loss
    e, s = entropy(a), sparsity(a)
    mask_loss = w_entropy * e + w_sparsity * s
    reg_loss += mask_loss
    (reg_loss * cotangent if cotangent != 1.0 else reg_loss).backward()
    out = {"reg_loss": reg_loss, "depth_loss": depth_loss, "mask_loss": mask_loss, "entropy": e, "sparsity": s}
    out = {k: v.detach() for k, v in out.items()}
    out["g_depth"], out["g_alpha"] = d.grad, a.grad
    if image is not None:
        with torch.no_grad():
            out["psnr"] = psnr(image.to(dtype), gt_image.to(dtype))
    return out


def alone(alpha, dtype=torch.float32):
    """-> {entropy, sparsity, g_entropy, g_sparsity}: each function called and differentiated by itself."""
    out = {}
    for name, fn in (("entropy", entropy), ("sparsity", sparsity)):
        a = _leaf(alpha, dtype)
        v = fn(a)
        v.backward()
        out[name], out["g_" + name] = v.detach(), a.grad
    return out


def make_case(B, H, W, seed=0):
    """Inputs of one fixture case -> {depth, gt_depth [B,1,H,W], alpha [B,1,H,W], image, gt_image [B,3,H,W]}, fp32.
    alpha: whole rows of exact 0 (empty pixels), exact 1, one element at 1 + 2^-23 (what a + (1 - a) bg can round to),
    values below epsilon, 1e-30.  depth: pixels equal to gt_depth and differences of both signs.  Depths, images and
    ground truth take values that fp16 / uint8 hold exactly, so that the fixture can store them in those types."""
    g = torch.Generator().manual_seed(1000 * seed + 31 * H + W)
    gt_depth = (0.5 + 4.0 * torch.rand(B, 1, H, W, generator=g)).half().float()
    diff = (0.3 * torch.randn(B, 1, H, W, generator=g)).half().float()
    diff[torch.rand(B, 1, H, W, generator=g) < 0.25] = 0.0                  # pixels where the two maps agree
    depth = (gt_depth + diff).half().float()
    alpha = torch.rand(B, 1, H, W, generator=g)
    alpha[:, :, ::3, :] = 0.0                                               # every third row is empty
    flat = alpha.view(-1)
    live = torch.nonzero(flat).view(-1)                                     # (the empty rows stay empty)
    idx = live[torch.randperm(live.numel(), generator=g)]
    k = max(1, live.numel() // 16)
    flat[idx[:k]] = 1.0
    flat[idx[k:2 * k]] = 1e-6 * torch.rand(k, generator=g)                  # below epsilon
    flat[idx[2 * k]] = 1.0 + 2.0 ** -23
    flat[idx[2 * k + 1]] = 1e-30
    flat[idx[2 * k + 2]] = 0.5
    gt_image = (torch.randint(0, 256, (B, 3, H, W), generator=g).float() / 255.0)
    image = (gt_image + 0.05 * torch.randn(B, 3, H, W, generator=g)).clamp(0, 1).half().float()
    return {"depth": depth, "gt_depth": gt_depth, "alpha": alpha, "image": image, "gt_image": gt_image}


def fixture_case(fx, i):
    """Case i of tests/golden/regterms.npz -> (inputs as make_case returns them, the case's other entries by name)."""
    p = f"c{i}_"
    T = torch.from_numpy
    c = {k: T(fx[p + "in_" + k]).float() for k in ("depth", "gt_depth", "alpha", "image")}
    c["gt_image"] = T(fx[p + "in_gt_image"]).float() / 255.0
    return c, {k[len(p):]: v for k, v in fx.items() if k.startswith(p) and not k.startswith(p + "in_")}


def random_maps(n, seed=0):
    """Flat maps of n elements for the grid-stride test: depth, gt_depth, alpha in (0, 1) with a fifth exact zeros."""
    g = torch.Generator().manual_seed(seed)
    gt_depth = 0.5 + 4.0 * torch.rand(n, generator=g)
    depth = gt_depth + 0.3 * torch.randn(n, generator=g)
    alpha = torch.rand(n, generator=g)
    alpha[torch.rand(n, generator=g) < 0.2] = 0.0
    return depth, gt_depth, alpha


def rel_gap(a, b):
    """Relative distance of a scalar a from the truth b."""
    a, b = float(a), float(b)
    return abs(a - b) / abs(b) if b != 0.0 else abs(a - b)


def map_gap(a, b):
    """Largest element-wise distance of a gradient map from the truth b, relative to the truth's largest magnitude."""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max()) / float(b.abs().max())


def db_gap(a, b):
    return float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs().max())


def allowed(ref_gap, floor=FLOOR):
    """three times the distance of the reference's own fp32 result from float64 on the same inputs,
    but not less than an fp32 result's own rounding chain (one ulp for each logarithm, half an ulp for each of the two
    products and for the final rounding): 8 x 2^-24 relative."""
    return max(3.0 * float(ref_gap), floor)
