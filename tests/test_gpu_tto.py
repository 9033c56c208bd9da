"""The test-time pose refinement on the MI355X (csrc/pose.hip through mobgs_amd.tto) against the float64 restatement
(tests/tto_restatement.py) under the rule of DESIGN.md 3a -- 3 x the distance of the reference's own fp32 statements from
float64 on the same cases, not less than an fp32 rounding chain (8 x 2^-24; in dB for a loss) --, the bit-identity
conditions of include/mobgs_hip.h K23, the frozen model, and the loop against eval.py's own, composed from torch ops around
this project's render.

Every test prints its figures before it asserts (run with -s); docs/MEASUREMENT_LOG.md, "K23", is where they are kept."""
import math
import os
import types

import numpy as np
import pytest
import torch

import tto_restatement as TR
from helpers import bits, same_bits

pytestmark = pytest.mark.gpu
F64 = torch.float64


# ---- the head ----------------------------------------------------------------------------------------------------------

def head_cases():
    g = torch.Generator().manual_seed(20)
    unit = torch.randn(6, 4, generator=g, dtype=F64)
    unit = unit / unit.norm(dim=-1, keepdim=True)
    small_t = torch.randn(3, generator=g, dtype=F64)
    cases = [("identity", torch.tensor([1.0, 0, 0, 0], dtype=F64), torch.zeros(3, dtype=F64))]
    cases += [(f"unit{n}", unit[n], small_t * (n + 1)) for n in range(3)]
    cases += [(f"norm{s:g}", unit[3] * s, small_t) for s in (1e-3, 0.5, 2.0)]
    neg = unit[4] * torch.sign(unit[4][0]) * -1.0
    cases += [("negative_real", neg, small_t), ("large_t", unit[5], torch.tensor([1234.5, -9876.25, 4321.125], dtype=F64))]
    # (the fp32 inputs are the case; float64 sees them widened exactly)
    return [(name, q.float(), t.float()) for name, q, t in cases]


def test_head_forward_and_backward(hip_device):
    from mobgs_amd.tto import pose_matrix
    dev = hip_device
    g = torch.Generator().manual_seed(21)
    rows = []
    for name, q, t in head_cases():
        cot = torch.randn(4, 4, generator=g)
        qd, td = q.to(dev).requires_grad_(True), t.to(dev).requires_grad_(True)
        w = pose_matrix(qd, td)
        w.backward(cot.to(dev))
        # float64 truth and the fp32 torch composition of the same expression, on the host
        out = {}
        for dtype in (F64, torch.float32):
            qa, ta = q.to(dtype).requires_grad_(True), t.to(dtype).requires_grad_(True)
            wa = TR.head(qa, ta)
            va_q, va_t = torch.autograd.grad(wa, (qa, ta), cot.to(dtype))
            out[dtype] = (wa.detach(), va_q, va_t)
        w64, vq64, vt64 = out[F64]
        vq_written, _ = TR.head_vjp(q.double(), cot.double())
        assert TR.max_gap(vq_written, vq64) <= 1e-12                       # the restated Jacobian is autograd's
        assert w.shape == (4, 4) and w.dtype == torch.float32 and bits(w[3]).tolist() == bits(torch.tensor([0.0, 0, 0, 1])).tolist()
        assert same_bits(w[:3, 3].cpu(), t) and same_bits(td.grad.cpu(), cot[:3, 3])       # copies
        # R does not depend on |q|: the truth has no component along q, so the kernel's is a part of its error
        radial = abs(float((qd.grad.double().cpu() * q.double()).sum())) / float(q.double().norm())
        # the rotation block on its own: the translation is a copy (asserted above), and next to a large one the block's
        # error would vanish in the scale of the whole matrix
        rows.append((name, TR.max_gap(w[:3, :3], w64[:3, :3]), TR.max_gap(out[torch.float32][0][:3, :3], w64[:3, :3]),
                     TR.max_gap(qd.grad, vq64), TR.max_gap(out[torch.float32][1], vq64), radial / float(vq64.abs().max())))
        if name == "identity":
            assert same_bits(w.cpu(), torch.eye(4))
    ref_fwd, ref_bwd = max(r[2] for r in rows), max(r[4] for r in rows)
    tol_fwd, tol_bwd = TR.allowed(ref_fwd), TR.allowed(ref_bwd)
    for name, fwd, rf, bwd, rb, radial in rows:
        print(f"[tto] head {name}: rotation gap {fwd:.2e} (fp32 torch {rf:.2e}, allowed {tol_fwd:.2e}), v_q gap {bwd:.2e} "
              f"(fp32 torch {rb:.2e}, allowed {tol_bwd:.2e}), component of v_q along q {radial:.2e} of its largest entry")
    for name, fwd, rf, bwd, rb, radial in rows:
        assert fwd <= tol_fwd and bwd <= tol_bwd, name
        assert radial <= 2 * tol_bwd, name                     # |(v_q - truth) . q / |q|| <= the 2-norm of a 4-vector of errors


# ---- the loss ----------------------------------------------------------------------------------------------------------

SHAPES = ((1, 1), (7, 5), (16, 16), (17, 33), (64, 80), (288, 512))


def image_pair(H, W):
    g = torch.Generator().manual_seed(1000 * H + W)
    gt = torch.rand(3, H, W, generator=g)
    return (gt + 0.05 * torch.randn(3, H, W, generator=g)), gt


def loss_and_grad(pred, gt, v=None):
    from mobgs_amd.tto import neg_psnr_loss
    p = pred.detach().requires_grad_(True)
    loss = neg_psnr_loss(p, gt)
    loss.backward(v)
    return loss.detach(), p.grad


@pytest.mark.parametrize("H, W", SHAPES)
def test_loss_forward_and_backward(hip_device, H, W):
    dev = hip_device
    pred, gt = image_pair(H, W)
    v = 0.7
    truth = TR.neg_psnr(pred.double(), gt.double())
    truth_grad = TR.neg_psnr_grad(pred.double(), gt.double(), v)
    # the reference's own fp32 chain with autograd's gradient
    pa = pred.clone().requires_grad_(True)
    ref = TR.neg_psnr(pa, gt)
    ref.backward(torch.tensor(v))
    ref_gap, ref_grad_gap = abs(float(ref) - float(truth)), TR.max_gap(pa.grad, truth_grad)
    loss, grad = loss_and_grad(pred.to(dev), gt.to(dev), torch.tensor(v, device=dev))
    assert loss.shape == () and loss.dtype == torch.float32 and grad.shape == (3, H, W) and grad.is_cuda
    gap, grad_gap = abs(float(loss) - float(truth)), TR.max_gap(grad, truth_grad)
    tol, grad_tol = TR.allowed(ref_gap, TR.FLOOR_DB), TR.allowed(ref_grad_gap)
    print(f"[tto] loss {H}x{W}: {float(loss)!r} dB, float64 {float(truth)!r}, error {gap:.2e} dB (fp32 chain {ref_gap:.2e}, "
          f"allowed {tol:.2e}); gradient gap {grad_gap:.2e} (fp32 autograd {ref_grad_gap:.2e}, allowed {grad_tol:.2e})")
    assert gap <= tol and grad_gap <= grad_tol
    # without an upstream gradient (refine_pose's call: v_loss = NULL) the factor is 1
    from mobgs_amd import _lib
    from mobgs_amd._lib import check, ptr, stream
    lib = _lib.load()
    p, g = pred.to(dev), gt.to(dev)
    n = p.numel()
    partial = torch.empty(int(lib.mobgs_neg_psnr_scratch_doubles(n)), dtype=F64, device=dev)
    mse, out = torch.empty(1, dtype=F64, device=dev), torch.empty(1, device=dev)
    v_pred = torch.full_like(p, math.nan)
    check(lib.mobgs_neg_psnr_fwd(n, ptr(p), ptr(g), ptr(partial), ptr(mse), ptr(out), stream()), "fwd")
    check(lib.mobgs_neg_psnr_bwd(n, ptr(p), ptr(g), ptr(mse), None, ptr(v_pred), stream()), "bwd")
    assert same_bits(out[0], loss) and TR.max_gap(v_pred, truth_grad / v) <= grad_tol
    assert abs(float(mse) - float(((pred.double() - gt.double()) ** 2).mean())) <= 4 * 2.0 ** -24 * float(mse)


def test_loss_bit_identity_slices_and_equal_images(hip_device):
    from mobgs_amd.tto import neg_psnr_loss
    dev = hip_device
    H, W = 37, 53                                              # 3 H W = 5883 = 4 * 1470 + 3: a tail, several workgroups
    pred, gt = (t.to(dev) for t in image_pair(H, W))
    a, ga = loss_and_grad(pred, gt)
    b, gb = loss_and_grad(pred, gt)
    assert same_bits(a, b) and same_bits(ga, gb)               # run to run
    # the same data at other addresses: 4-byte aligned but not 16-byte aligned (one, two and three elements off), a
    # slice of a stack, and the two arrays at different offsets
    n = pred.numel()
    for off_p, off_g in ((1, 1), (2, 3), (3, 0), (0, 1)):
        bp, bg_ = torch.zeros(n + 8, device=dev), torch.zeros(n + 8, device=dev)
        sp, sg = bp[off_p:off_p + n].view(3, H, W), bg_[off_g:off_g + n].view(3, H, W)
        sp.copy_(pred), sg.copy_(gt)
        assert sp.data_ptr() % 16 == 4 * off_p and sg.data_ptr() % 16 == 4 * off_g and sp.is_contiguous()
        c, gc = loss_and_grad(sp, sg)
        assert same_bits(a, c) and same_bits(ga, gc), (off_p, off_g)
    stack = torch.rand(3, 3, H, W, device=dev)                 # images[k] of a stack: 3 H W is odd, so k = 1 is misaligned
    stack[1] = pred
    assert stack[1].data_ptr() % 16 != 0
    c, gc = loss_and_grad(stack[1], gt)
    assert same_bits(a, c) and same_bits(ga, gc)
    # layouts are converted, not reinterpreted
    c, _ = loss_and_grad(pred.permute(1, 2, 0).contiguous().permute(2, 0, 1), gt.double())
    assert same_bits(a, c)
    # equal images: -inf and NaN, as the reference's statements give
    loss, grad = loss_and_grad(gt, gt.clone())
    assert float(loss) == -math.inf and bool(torch.isnan(grad).all())
    with pytest.raises(ValueError):
        neg_psnr_loss(pred, gt[:, :-1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        neg_psnr_loss(pred, gt.cpu())


# ---- the step ----------------------------------------------------------------------------------------------------------

def test_pose_step_equals_its_three_parts(hip_device):
    """mobgs_pose_step == mobgs_pose_head_bwd, mobgs_adam_step on the same state, mobgs_pose_head_fwd: bit for bit, over
    three consecutive steps with changing rates."""
    from mobgs_amd import _lib
    from mobgs_amd._lib import check, ptr, stream
    from mobgs_amd.optim import _AdamTensor
    from mobgs_amd.tto import BETAS, EPS, adam_step_scalars
    dev = hip_device
    lib = _lib.load()
    g = torch.Generator().manual_seed(30)
    q0 = torch.randn(4, generator=g)
    t0 = torch.randn(3, generator=g)
    fused = dict(q=q0.to(dev), t=t0.to(dev), mom=torch.zeros(2, 7, device=dev), w2c=torch.full((4, 4), math.nan, device=dev))
    parts = dict(q=q0.to(dev), t=t0.to(dev), mom=torch.zeros(2, 7, device=dev), w2c=torch.full((4, 4), math.nan, device=dev))
    rates = ((3e-3, 3e-3), (2.1e-3, 2.9e-3), (1e-4, 3.3e-4))                 # (lr_p, lr_q) of the step
    q64, t64 = q0.double(), t0.double()
    m64 = [torch.zeros(4, dtype=F64), torch.zeros(4, dtype=F64), torch.zeros(3, dtype=F64), torch.zeros(3, dtype=F64)]
    for step, (lr_p, lr_q) in enumerate(rates, 1):
        cot = torch.randn(4, 4, generator=g) * 10.0 ** (step - 2)
        vq64, vt64 = TR.head_vjp(q64, cot.double())
        q64, m64[0], m64[1] = TR.adam_update(q64, vq64, m64[0], m64[1], step, lr_q)
        t64, m64[2], m64[3] = TR.adam_update(t64, vt64, m64[2], m64[3], step, lr_p)
        size_p, b2 = adam_step_scalars(step, lr_p)
        size_q, _ = adam_step_scalars(step, lr_q)
        v = cot.to(dev)
        s = fused
        check(lib.mobgs_pose_step(ptr(s["q"]), ptr(s["t"]), ptr(v), ptr(s["mom"][0]), ptr(s["mom"][1]), size_q, size_p, b2,
                                  BETAS[0], BETAS[1], EPS, ptr(s["w2c"]), stream()), "mobgs_pose_step")
        assert bits(v).abs().max() == 0                                      # v_w2c is +0 everywhere afterwards
        s = parts
        v, v_q, v_t = cot.to(dev), torch.empty(4, device=dev), torch.empty(3, device=dev)
        check(lib.mobgs_pose_head_bwd(ptr(s["q"]), ptr(v), ptr(v_q), ptr(v_t), stream()), "mobgs_pose_head_bwd")
        m, vv = s["mom"][0], s["mom"][1]
        descs = (_AdamTensor * 2)(
            _AdamTensor(s["q"].data_ptr(), v_q.data_ptr(), m[:4].data_ptr(), vv[:4].data_ptr(), 4, size_q, b2),
            _AdamTensor(s["t"].data_ptr(), v_t.data_ptr(), m[4:].data_ptr(), vv[4:].data_ptr(), 3, size_p, b2))
        check(lib.mobgs_adam_step(2, descs, BETAS[0], BETAS[1], EPS, stream()), "mobgs_adam_step")
        check(lib.mobgs_pose_head_fwd(ptr(s["q"]), ptr(s["t"]), ptr(s["w2c"]), stream()), "mobgs_pose_head_fwd")
        assert same_bits(v, cot.to(dev))                                     # the separate calls only read it
        for k in ("q", "t", "mom", "w2c"):
            assert same_bits(fused[k], parts[k]), (step, k)
        assert not same_bits(fused["q"].cpu(), q0) and bool(torch.isfinite(fused["w2c"]).all())
    # and the values are Adam's: three steps of the float64 restatement on the same cotangents.  A step adds a term of the
    # size of its rate (<= 3e-3 of a value of order 1) and rounds the value once: half an ulp per step, far inside FLOOR
    assert TR.max_gap(fused["q"], q64) <= TR.FLOOR and TR.max_gap(fused["t"], t64) <= TR.FLOOR
    assert TR.max_gap(fused["w2c"], TR.head(q64, t64)) <= TR.FLOOR


# ---- the scene of test_evaluate_views ------------------------------------------------------------------------------------

W_, H_ = 80, 64


def small_rotation(deg, axis):
    a = math.radians(deg) / 2
    q = torch.zeros(4, dtype=F64)
    q[0], q[1 + axis] = math.cos(a), math.sin(a)
    return TR.rotation(q)


def make_models(dev, requires_grad):
    from mobgs_amd.gaussian_model import GaussianParams
    from mobgs_amd.helper_model import Sandwich
    from mobgs_amd.synth import SynthCamera, dynamic_extras, gaussian_cloud
    scam = SynthCamera().scaled(W_, H_)
    torch.manual_seed(0)
    dec = Sandwich(9, 3).to(dev)
    stat_p, dyn_p = gaussian_cloud(1500, scam, 0), gaussian_cloud(700, scam, 1)
    stat = GaussianParams(stat_p, None, dec, dev, requires_grad=requires_grad)
    dyn = GaussianParams(dyn_p, dynamic_extras(dyn_p["xyz"], 0), dec, dev, requires_grad=requires_grad)
    for p in dec.parameters():
        p.requires_grad_(requires_grad)
    return scam, stat, dyn


def model_tensors(stat, dyn):
    out = {}
    for tag, pc in (("stat", stat), ("dyn", dyn)):
        for k, t in vars(pc).items():
            if torch.is_tensor(t):
                out[f"{tag}.{k}"] = t
    for k, p in dyn.rgbdecoder.named_parameters():
        out["decoder." + k] = p
    return out


@pytest.fixture(scope="module")
def scene(hip_device):
    """Three cameras whose ground truth is rendered at a KNOWN pose; each camera itself starts 0.5 degrees and 0.005 units
    away from it (what refinement has to recover)."""
    from mobgs_amd import _lib
    from mobgs_amd.camera import PinholeCamera
    from mobgs_amd.gaussian_renderer import render
    dev = hip_device
    _lib.load(build_if_missing=False)
    scam, stat, dyn = make_models(dev, False)
    bg = torch.zeros(9, device=dev)
    cams, truths, gts = [], [], []
    for k in range(3):
        true = torch.eye(4, dtype=F64)
        true[0, 3] = 0.05 * (k - 1)
        off = torch.eye(4, dtype=F64)
        off[:3, :3] = small_rotation(0.5, k % 3)
        off[:3, 3] = torch.tensor([0.003, -0.004, 0.0], dtype=F64).roll(k)            # 0.005 units
        start = (off @ true).float()
        cam = PinholeCamera(W_, H_, scam.K, start, (3 + 8 * k) / 23.0, scam.max_time, device=dev)
        cam.image_name = f"view_{k:03d}"
        with torch.no_grad():
            gt = render(cam, stat, dyn, None, bg, w2c=true.float().to(dev))["render"].clamp(0, 1)
        cams.append(cam), truths.append(true), gts.append(gt)
    assert float(torch.stack(gts).std()) > 0.01
    return types.SimpleNamespace(dev=dev, scam=scam, stat=stat, dyn=dyn, bg=bg, cams=cams, truths=truths, gts=torch.stack(gts),
                                 stat_gaussians=stat, dyn_gaussians=dyn)


def start_of(cam):
    from mobgs_amd.tto import matrix_to_quaternion
    w2c = cam.world_view_transform.transpose(0, 1)
    return matrix_to_quaternion(w2c[:3, :3]).contiguous(), w2c[:3, 3].clone().contiguous()


def pose_error(q, t, true):
    return float((TR.head(q.double().cpu(), t.double().cpu()) - true).abs().max())


def test_frozen_models(scene, hip_device):
    from mobgs_amd.gaussian_renderer import render
    from mobgs_amd.tto import refine_pose
    dev = hip_device
    g = torch.Generator().manual_seed(40)
    v = torch.randn(3, H_, W_, generator=g).to(dev)
    cam = scene.cams[0]
    grads = []
    for requires_grad in (False, True):
        _, stat, dyn = make_models(dev, requires_grad)
        leaf = cam.world_view_transform.transpose(0, 1).clone().requires_grad_(True)
        (render(cam, stat, dyn, None, scene.bg, w2c=leaf)["render"] * v).sum().backward()
        grads.append(leaf.grad.clone())
    assert float(grads[0].abs().max()) > 0 and same_bits(grads[0], grads[1])
    # (stat, dyn: the models that require gradients, with the .grad the backward above left on them)
    tensors = model_tensors(stat, dyn)
    assert sum(t.requires_grad for t in tensors.values()) > 10
    for t in tensors.values():
        t.grad = None
    marker = next(t for t in tensors.values() if t.requires_grad)
    marker.grad = torch.ones_like(marker)                                       # a .grad that was there before stays as it is
    flags = {k: t.requires_grad for k, t in tensors.items()}
    out = refine_pose(cam, scene.gts[0], stat, dyn, None, scene.bg, steps=3, decay_start=1, lr_p=3e-3, lr_q=3e-3, lr_final=1e-4)
    assert out.loss_history.shape == (3,) and bool(torch.isfinite(out.loss_history).all())
    after = model_tensors(stat, dyn)
    assert after.keys() == tensors.keys()
    for k, t in after.items():
        assert t is tensors[k] and t.requires_grad == flags[k], k
        assert (t.grad is None) or t is marker, k
    assert bool((marker.grad == 1).all())
    assert not out.w2c.requires_grad and out.w2c.shape == (4, 4) and out.q.shape == (4,) and out.t.shape == (3,)


def composed(scene, k, q0, t0, settings, read_back=True):
    from mobgs_amd.gaussian_renderer import render
    f = TR.render_loss(render, scene.cams[k], scene.stat, scene.dyn, None, scene.bg, scene.gts[k])
    return TR.composed_loop(f, q0, t0, read_back=read_back, **settings)


def fused(scene, k, settings, **kw):
    from mobgs_amd.tto import refine_pose
    s = dict(settings)
    return refine_pose(scene.cams[k], scene.gts[k], scene.stat, scene.dyn, None, scene.bg, steps=s.pop("tto_steps"), **s, **kw)


def final_gap(a, b):
    """Largest difference of the final (q, t) of two runs that started from (nearly) the same values."""
    return max(float((a[0].double() - b[0].double()).abs().max()), float((a[1].double() - b[1].double()).abs().max()))


def test_loop_parity_with_the_composed_loop(scene):
    """refine_pose against eval.py's loop composed from torch ops, with the reference's defaults (25 steps).  The yardstick
    for the final pose is the composed loop's own sensitivity to ONE rounding: the largest final gap between it and itself
    restarted with one of the seven start values moved by one fp32 ulp.  The fused loop rounds differently in a few places
    per step (the head's sum of squares, the loss in float64, Adam's fused multiply-adds), so it may end at most 3 x that
    far away: the margin of DESIGN 3a."""
    from mobgs_amd.gaussian_renderer import render
    from mobgs_amd.tto import pose_matrix
    k = 1
    q0, t0 = start_of(scene.cams[k])
    base = composed(scene, k, q0, t0, TR.DEFAULTS)
    sens = 0.0
    for c in range(7):
        q1, t1 = q0.clone(), t0.clone()
        x = q1 if c < 4 else t1
        x[c % 4 if c < 4 else c - 4] = torch.nextafter(x[c % 4 if c < 4 else c - 4], torch.tensor(math.inf, device=x.device))
        sens = max(sens, final_gap(composed(scene, k, q1, t1, TR.DEFAULTS), base))
    ours = fused(scene, k, TR.DEFAULTS, q0=q0, t0=t0)
    gap = final_gap((ours.q, ours.t), base)
    hist = ours.loss_history.cpu().tolist()
    # step 0: both loops render the same start; the loss tolerance of test_loss_forward_and_backward, with the distance of
    # the composed loop's own fp32 loss from float64 on that image as the reference's error
    with torch.no_grad():
        w0 = pose_matrix(q0, t0)
        pred0 = render(scene.cams[k], scene.stat, scene.dyn, None, scene.bg, w2c=w0)["render"]
        same_start = same_bits(w0, TR.head(q0, t0))
    truth0 = float(TR.neg_psnr(pred0.double().cpu(), scene.gts[k].double().cpu()))
    tol0 = TR.allowed(abs(base[2][0] - truth0), TR.FLOOR_DB)
    print(f"[tto] loop parity, camera {k}, 25 steps: loss {hist[0]:.6f} -> {hist[-1]:.6f} dB (composed {base[2][0]:.6f} -> "
          f"{base[2][-1]:.6f}); step 0: fused {hist[0]!r}, composed {base[2][0]!r}, float64 {truth0!r}, allowed {tol0:.2e} dB, "
          f"head kernel and torch head bit-equal at the start: {same_start}; final (q, t) gap fused - composed {gap:.3e}, "
          f"composed loop's sensitivity to one ulp {sens:.3e} (allowed 3 x = {3 * sens:.3e})")
    assert len(hist) == 25 and all(math.isfinite(x) for x in hist)
    assert abs(hist[0] - truth0) <= tol0 and abs(hist[0] - base[2][0]) <= tol0
    assert gap <= 3 * sens


def test_recovery(scene):
    """Ground truth rendered at a known pose, the start 0.5 degrees and 0.005 units away, 100 steps with eval.py's __main__
    settings: the loss and the pose error must both come down -- for the reference's own loop too (if that one does not
    meet it on a scene, the scene is wrong, not the condition)."""
    k = 0
    q0, t0 = start_of(scene.cams[k])
    true = scene.truths[k]
    e0 = pose_error(q0, t0, true)
    assert 0.004 < e0 < 0.02
    q_c, t_c, l_c = composed(scene, k, q0, t0, TR.MAIN)
    ours = fused(scene, k, TR.MAIN)
    l_f = ours.loss_history.cpu().tolist()
    with torch.no_grad():
        from mobgs_amd.tto import neg_psnr_loss
        from mobgs_amd.gaussian_renderer import render
        end_f = float(neg_psnr_loss(render(scene.cams[k], scene.stat, scene.dyn, None, scene.bg, w2c=ours.w2c)["render"],
                                    scene.gts[k]))
    e_c, e_f = pose_error(q_c, t_c, true), pose_error(ours.q, ours.t, true)
    print(f"[tto] recovery, camera {k}, 100 steps: start error {e0:.3e}; fused: loss {l_f[0]:.3f} -> {l_f[-1]:.3f} dB (after "
          f"the last update {end_f:.3f}), gained {l_f[0] - l_f[-1]:.2f} dB, pose error {e_f:.3e}; composed: loss {l_c[0]:.3f} -> "
          f"{l_c[-1]:.3f} dB, gained {l_c[0] - l_c[-1]:.2f} dB, pose error {e_c:.3e}")
    assert l_c[-1] < l_c[0] and e_c < e0
    assert l_f[-1] < l_f[0] and e_f < e0 and end_f < l_f[0]
    assert same_bits(ours.w2c[3].cpu(), torch.tensor([0.0, 0, 0, 1]))


def test_render_test_tto(scene, tmp_path):
    from mobgs_amd.gaussian_renderer import render
    from mobgs_amd.metrics import image_metrics
    from mobgs_amd.tto import render_test_tto
    save = str(tmp_path / "out")
    res = render_test_tto(H_, W_, scene, scene.cams, save, scene.gts, tto_steps=4, decay_start=2, renderArgs=[None, scene.bg])
    assert res["poses"].shape == (3, 4, 4) and res["images"].shape == (3, 3, H_, W_) and res["poses"].is_cuda
    # camera 0 runs step_factor = 10 times the steps at the full rate, the others the plain count at a tenth of it
    assert [h.shape[0] for h in res["loss_histories"]] == [40, 4, 4]
    assert res["step_factors"] == [10, 1, 1] and res["lr_factors"] == [1.0, 0.1, 0.1]
    for k, cam in enumerate(scene.cams):
        with torch.no_grad():
            want = render(cam, scene.stat, scene.dyn, None, scene.bg, stage="fine", get_static=False, get_dynamic=True,
                          w2c=res["poses"][k])["render"]
        assert same_bits(res["images"][k], want), k
        assert not same_bits(res["poses"][k], cam.world_view_transform.transpose(0, 1))
        assert bool(torch.isfinite(res["loss_histories"][k]).all())
    m = image_metrics(res["images"], scene.gts, data_range=2.0, clamp=True, quantize=True)
    for name, col in res["metrics"]._asdict().items():
        assert same_bits(col, getattr(m, name)), name
    # the files, with the reference's names
    names = sorted(os.listdir(os.path.join(save, "test_refined")))
    assert names == [f"img_view_{k:03d}.png.png" for k in range(3)] and sorted(os.listdir(save)) == ["solved_poses.npy", "test_refined"]
    assert np.array_equal(np.load(os.path.join(save, "solved_poses.npy")), res["poses"].cpu().numpy())
    from PIL import Image
    for k in range(3):
        png = np.asarray(Image.open(os.path.join(save, "test_refined", names[k])))
        want = (np.clip(res["images"][k].clamp(0, 1).permute(1, 2, 0).cpu().numpy(), 0, 1) * 255).astype("uint8")
        assert png.shape == (H_, W_, 3) and np.array_equal(png, want)
    # Adam's first update moves a value by its rate (times g / (|g| + eps)): one step shows the rate each camera ran with.
    # Without initialize_from_previous_camera EVERY camera gets step_factor 1 and the reduced rate.
    for flag, factors in ((True, [1.0, 0.1, 0.1]), (False, [0.1, 0.1, 0.1])):
        one = render_test_tto(H_, W_, scene, scene.cams, None, list(scene.gts), tto_steps=1, renderArgs=[None, scene.bg],
                              initialize_from_previous_camera=flag, initialize_from_previous_step_factor=1)
        assert one["lr_factors"] == factors and [h.shape[0] for h in one["loss_histories"]] == [1, 1, 1]
        for k, cam in enumerate(scene.cams):
            moved = float((one["poses"][k][:3, 3] - cam.world_view_transform.transpose(0, 1)[:3, 3]).abs().max())
            assert abs(moved / (0.003 * factors[k]) - 1) <= 1e-3, (flag, k, moved)
    assert not os.path.exists(str(tmp_path / "None"))
