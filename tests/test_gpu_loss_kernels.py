"""The fused SSIM + L1 kernels (csrc/loss.hip through mobgs_amd.loss_utils) and the normals kernels (csrc/normals.hip through
mobgs_amd.main_utils.get_normals) against the float64 oracles on the cases of tests/loss_cases.py.

Cases (tests/test_loss_cases_cpu.py shows from the oracles alone that each reaches its edge).  SSIM + L1: images of 1 x 1,
5 x 6 (the window hangs over the image everywhere), exactly one 16 x 16 tile, a second tile of one live row / column, ragged
15 x 33, and 48 x 48 x 6 planes whose centre tile reads no padding; noisy, flat (E[x^2] - mu^2 cancels against C2), black,
img == gt on a block around a tile corner, and unclamped values; a [3,H,W] input and a non-contiguous view; photometric_loss
with lambda 0.2 / 1 / 0 (the arm of the backward without LDS staging), ssim() as a mean and per image with the cotangents
(0.7, -1.3) and (1, 0) -- both arms in one launch --, the separate l1_loss + 0.2 (1 - ssim) form and the forward without a
graph.  Normals: maps without interior, one interior pixel, one interior row across four workgroups, 256 and 272 pixels,
two cameras (the second: no skew, corner pixels, principal point outside), and depth maps that are exactly 0 in two holes,
where both kernels take the clamped branch of F.normalize (n / 1e-12, gradient x 1e12).

Compared (tests/loss_cases.py): values as scalars -- relative error at most 3 x the fp32 oracle's own gap, floor 8 x 2^-24 --,
maps per stratum with deform_cases.close_to_f64 at k = 3 (a rule that needs no run of the code under
test) and exact zeros where float64 has them; the SSIM tensors get the window allowance max |ref64_separable - ref64| on
top (1e-11 .. 6e-8, at most 0.03 x the fp32 gap of the same gradient), the SSIM gradients the term allowance (the 2^-23
floor taken of the gradient's terms in absolute value: they cancel, 15 and 165 to 1 on one-pixel planes); a RATIO line shows
the k of the plain rule unless it says `with extra`.  The fixed-order sums and the gather backward are
bit-reproducible: one case of each family runs twice.

Worst k needed on an MI355X per family and stratum (docs/MEASUREMENT_LOG.md, "Loss, normals and BLCE kernels against
float64"):

    family / stratum                      worst k needed (case, tensor)                                     k
    SSIM + L1 values                      1.21  (flat_17x16, ssim per image)                                 3
    SSIM + L1 gradient, whole map         1.58  (noisy_1x1, ssim mean)                                       3
    SSIM + L1 gradient, per plane         2.53  (noisy_1x1, per_image_b plane 1); two one-pixel planes       3
                                          need 12.6 and 3.02 alone and 0 with the term allowance
    normals forward / unit                0.99  (smooth_3x300_cam2)                                          3
    normals forward / hole                0.92  (holes_20x24_cam2)                                           3
    normals forward / border              0     (exact zeros)                                                3
    normals depth gradient / unit         1.05  (smooth_20x24)                                               3
    normals depth gradient / hole         1.73  (holes_20x24)                                                3
    normals depth gradient / border       0.96  (smooth_3x300)                                               3
    normals depth gradient / corner       0     (exact zeros)                                                3

Before the two fixes of this change the same run failed: the window taps were normalised by a sum one ulp below the
reference's (noisy_15x33, photometric_loss(lambda = 1): relative error 4.98e-7 against max(3 x 8.9e-8, 4.77e-7)), and the
back-projected differences were contracted into FMAs (6 to 40 normal components of ~1e-8 where float64 has exact zeros, in
every map with a flat patch or a hole)."""
import pytest
import torch

import loss_cases as C

pytestmark = pytest.mark.gpu


def _call(LU, call, img, gt):
    """-> (value, cotangent or None) of one call variant through mobgs_amd.loss_utils."""
    if call.startswith("photo_"):
        return LU.photometric_loss(img, gt, float(call[6:])), None
    if call == "separate":
        return LU.l1_loss(img, gt) + 0.2 * (1.0 - LU.ssim(img, gt)), None
    if call == "ssim_mean":
        return LU.ssim(img, gt), None
    v = LU.ssim(img, gt, size_average=False)
    return v, torch.tensor(C.PER_IMAGE_COTS[call][:v.numel()], device=v.device)


def _run(LU, case, call, dev):
    img = case.img.to(dev).requires_grad_(True)
    assert case.layout != "permuted" or (not img.is_contiguous() and img.stride() == case.img.stride())
    gt = case.gt.to(dev)
    value, cot = _call(LU, call, img, gt)
    value.backward(cot)
    with torch.no_grad():
        again, _ = _call(LU, call, img, gt)
    assert not again.requires_grad and torch.equal(again, value.detach()), f"{case.name} {call}: forward without a graph differs"
    return value.detach(), img.grad


@pytest.mark.parametrize("name", C.SSIM_CASES)
def test_ssim_l1_matches_float64(hip_device, name):
    from mobgs_amd import loss_utils as LU
    case = C.ssim_case(name)
    for call in C.calls_of(case) + ("separate",):
        value, grad = _run(LU, case, call, hip_device)
        ref_call = "photo_0.2" if call == "separate" else call  # the same oracle statement
        C.compare_ssim(case, ref_call, value, grad, f"ssim {name} {call}", refs=C.ssim_reference(name, ref_call))
        if case.content == "equal_block" and call == "photo_0":
            r1, c1 = min(C.BLOCK[1], case.H), min(C.BLOCK[1], case.W)
            assert not grad[..., C.BLOCK[0]:r1, C.BLOCK[0]:c1].any(), "sign(0) = 0: no gradient where img == gt"
        if call == "per_image_b" and case.B == 2:
            assert not grad[1].any() and (case.content == "black" or grad[0].any())


def test_ssim_l1_is_bit_reproducible(hip_device):
    from mobgs_amd import loss_utils as LU
    case = C.ssim_case("noisy_48x48")
    for call in ("photo_0.2", "per_image_a"):
        a, b = _run(LU, case, call, hip_device), _run(LU, case, call, hip_device)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), call


def _normals(case, dev, two_dim=False):
    from mobgs_amd.main_utils import get_normals
    depth = (case.depth[0] if two_dim else case.depth).to(dev).requires_grad_(True)
    z = depth + 1e-6  # the caller's statement (train.py:590)
    assert torch.equal(z.detach().cpu().reshape(case.z.shape), case.z)
    n = get_normals(z, case.cam)
    n.backward(case.cot.to(dev))
    return n.detach(), depth.grad


@pytest.mark.parametrize("name", C.NORMALS_CASES)
def test_normals_match_float64(hip_device, name):
    case = C.normals_case(name)
    n, grad = _normals(case, hip_device)
    assert tuple(grad.shape) == (1, case.H, case.W)
    C.compare_normals(name, n, grad, f"normals {name}")
    H, W = case.H, case.W
    assert not n[0, :, 0, :].any() and not n[0, :, H - 1, :].any() and not n[0, :, :, 0].any() and not n[0, :, :, W - 1].any()
    assert all(float(grad[0, i, j]) == 0.0 for i in (0, H - 1) for j in (0, W - 1))
    if not case.interior:
        assert not n.any() and not grad.any()
    n2, grad2 = _normals(case, hip_device, two_dim=True)  # [H,W] input: the same values, the gradient in its shape
    assert tuple(n2.shape) == (1, 3, H, W) and tuple(grad2.shape) == (H, W)
    assert torch.equal(n2, n) and torch.equal(grad2, grad[0])


def test_normals_are_bit_reproducible(hip_device):
    case = C.normals_case("holes_20x24")
    a, b = _normals(case, hip_device), _normals(case, hip_device)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
