"""The two autograd functions of mobgs_amd.deformation, each by itself, against the float64 oracle at tile tails,
borders and pile-ups: `_HexPlane` (csrc/deform.hip, csrc/hexplane_bwd.hip) and `_MlpUpdate` (csrc/deform_bwd.hip).

Cases, references and the comparator are tests/deform_cases.py (tests/test_deform_cases_cpu.py shows from the oracle alone
that each case reaches its edge).  Every row is kept away from ReLU / clamp / grid-line kinks by the float64 oracle, so
fp32 and float64 take the same branch everywhere: every output and every gradient is compared in full, no flip allowance.
Per tensor:  max |got - ref64| <= k max |ref32 - ref64| + 2^-23 max |ref64|,  ref32 = the oracle's statements in fp32 on
the CPU, and got == 0 wherever ref64 == 0 exactly (clipped coordinates, clamped channels, untouched plane cells).

k per tensor family = twice the worst k any tensor of the family needed on an MI355X (all 24 cases, 504 tensors),
rounded up, at most 8 (docs/MEASUREMENT_LOG.md, "Deformation kernels against float64"):

    family                 worst k needed (case, tensor)           k
    outputs                1.79  (HexPlane N = 1, feat)            4
    per-row gradients      2.28  (HexPlane N = 33, v_times)        5
    MLP weight gradients   1.88  (MLP N = 1, rot_b2)               4
    plane gradients        5.07  (HexPlane N = 1, plane 17)        8   (twice the worst is 11: the cap holds)

Every MLP tensor from N = 63 on needed at most 1.25, every plane gradient from N = 31 on at most 2.51.  The plane
gradients of N = 1, 2, 3 needed 5.07, 3.59, 4.73, all on planes of the finest level: a bilinear fraction is ix - floor(ix)
with ix up to 31, so it carries ulp(ix) = 2e-6 of absolute error in any fp32 evaluation, and with one to three points both
the kernel's error and the fp32 reference's are single draws of it rather than maxima over many (over 198 single points
the reference's own fp32 error on plane 17 ranges from 0.07e-6 to 4.1e-6 of the plane's maximum, median 1.1e-6; this
case drew 0.70e-6, the kernel 3.7e-6).
"""
import pytest
import torch

import deform_cases as C

pytestmark = pytest.mark.gpu

K = {"outputs": 4, "rows": 5, "weights": 4, "planes": 8}


def _leaf(t, dev):
    return t.to(dev).requires_grad_(True)


@pytest.mark.parametrize("name", C.HEX_CASES)
def test_hexplane_matches_float64(hip_device, name):
    from mobgs_amd.deformation import _HexPlane
    case = C.hex_case(name)
    ref64, ref32 = C.hex_reference(name)
    pts, times = _leaf(case.pts, hip_device), _leaf(case.times, hip_device)
    planes = [_leaf(p, hip_device) for p in case.planes]
    assert all(p.is_contiguous(memory_format=torch.channels_last) for p in planes)
    feat = _HexPlane.apply(pts, times, case.aabb.to(hip_device), *planes)
    assert feat.shape == (case.N, 96)
    feat.backward(case.cot.to(hip_device))
    torch.cuda.synchronize()
    tag = f"HexPlane {name}"
    C.close_to_f64(feat, ref64["feat"], ref32["feat"], K["outputs"], f"{tag} [outputs] feat")
    for key, t in (("v_pts", pts), ("v_times", times)):
        C.close_to_f64(t.grad, ref64[key], ref32[key], K["rows"], f"{tag} [rows] {key}")
    for i, p in enumerate(planes):
        assert p.grad is not None and p.grad.shape == p.shape
        C.close_to_f64(p.grad, ref64[f"plane{i}"], ref32[f"plane{i}"], K["planes"], f"{tag} [planes] plane{i}")
    if name == "border":  # what the comparator's exact-zero rule covered, spelled out
        q = C.normalised(case.pts, case.times, case.aabb)
        assert not pts.grad.cpu()[q[:, :3].abs() >= 1].any()
        assert not times.grad.cpu()[q[:, 3:].abs() >= 1].any()


@pytest.mark.parametrize("name", C.MLP_CASES)
def test_mlp_update_matches_float64(hip_device, name):
    from mobgs_amd.deformation import _W_KEYS, _MlpUpdate
    assert tuple(_W_KEYS) == C.W_KEYS
    case = C.mlp_case(name)
    ref64, ref32 = C.mlp_reference(name)
    rows = [_leaf(t, hip_device) for t in (case.feat, case.pts, case.scales, case.rots)]
    W = {k: _leaf(case.W[k], hip_device) for k in C.W_KEYS}
    outs = _MlpUpdate.apply(*rows, *[W[k] for k in C.W_KEYS])
    assert [tuple(o.shape) for o in outs] == [(case.N, 3), (case.N, 3), (case.N, 4)]
    torch.autograd.backward(outs, [c.to(hip_device) for c in case.cots])
    torch.cuda.synchronize()
    tag = f"MLP {name}"
    for key, o in zip(("out_pts", "out_scales", "out_rots"), outs):
        C.close_to_f64(o, ref64[key], ref32[key], K["outputs"], f"{tag} [outputs] {key}")
    for key, t in zip(("g_feat", "g_pts", "g_scales", "g_rots"), rows):
        assert t.grad is not None
        C.close_to_f64(t.grad, ref64[key], ref32[key], K["rows"], f"{tag} [rows] {key}")
    for k in C.W_KEYS:
        assert W[k].grad is not None and W[k].grad.shape == W[k].shape
        C.close_to_f64(W[k].grad, ref64[k], ref32[k], K["weights"], f"{tag} [weights] {k}")
    assert torch.equal(rows[2].grad.cpu(), case.cots[1])  # the scales input passes its cotangent on untouched
    if name == "clamp":  # channels 0 and 1 clamp in every row: nothing reaches their weights
        assert not W["scl_w2"].grad[:2].any() and not W["scl_b2"].grad[:2].any()
        assert W["scl_w2"].grad[2].any()
        out = outs[1].detach().cpu() - case.scales
        assert (out[:, 0] - C.LOG100).abs().max() < 1e-6 and (out[:, 1] + C.LOG100).abs().max() < 1e-6
    if case.N == 0:
        assert all(not W[k].grad.any() for k in C.W_KEYS)
