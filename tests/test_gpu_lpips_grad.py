"""LPIPS as a loss on the MI355X (mobgs_lpips_alex_bwd through LpipsAlex.loss and loss_utils.lpips_loss): the gradient with
respect to the images and, through tap_grads, to the five pre-activations, against torch autograd in float64 on the vetted,
kink-safe cases of lpips_grad_cases, under the rule of DESIGN.md 3a (per quantity 3 x the reference's own fp32 distance from
float64, measured into tests/golden/lpips_grad.npz, not below 8 x 2^-24; an error is the largest absolute error over a
pair's array relative to the array's largest float64 magnitude).  Then the loss value's bits, batch weights and cotangents,
the exact zeros, bit identity (run to run, batch, permutation, chunking, tap_grads, wanted sides), the untouched forward, the
refusals, a captured graph and the chain through render()."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import lpips_grad_cases as G
import lpips_restatement as LR
from helpers import load, same_bits

pytestmark = pytest.mark.gpu

BOTH_SIDES = (G.CASES.index((31, 48, 2, "noisy")), G.CASES.index((64, 97, 2, "clamp")))


@pytest.fixture(scope="module")
def fx():
    return load("lpips_grad")


@pytest.fixture(scope="module")
def ref_gaps(fx):
    return G.reference_gaps(fx)


@pytest.fixture(scope="module")
def nets():
    return LR.seeded_trunk(), LR.reference_heads()


@pytest.fixture(scope="module")
def model(hip_device, nets):
    from mobgs_amd.lpips import LpipsAlex
    return LpipsAlex(*nets, device=hip_device)


@functools.lru_cache(maxsize=None)
def case(i):
    return G.make_case(i)


@functools.lru_cache(maxsize=None)
def truth(i):
    """The float64 gradients of case i with v = 1, computed once and shared."""
    return G.gradients(case(i), LR.seeded_trunk(), LR.reference_heads(), conv=G.truth_conv(G.CASES[i][3]))


def on_device(c, dev):
    return torch.from_numpy(c["pred"]).to(dev), torch.from_numpy(c["gt"]).to(dev)


def public(model, c, dev, want=("pred",), v=None):
    """Through LpipsAlex.loss and autograd -> (loss [B], {side: gradient})."""
    pred, gt = on_device(c, dev)
    leaves = dict(pred=pred, gt=gt)
    for k in want:
        leaves[k].requires_grad_(True)
    loss = model.loss(pred, gt, clamp=c["clamp"])
    loss.backward(torch.ones_like(loss) if v is None else torch.as_tensor(v, dtype=torch.float32, device=dev))
    return loss.detach(), {k: leaves[k].grad for k in want}


def direct(model, c, dev, want=("pred",), v=None, tap_grads=True, chunk=None):
    """Through the model's two calls -> ({side: gradient}, tap gradients [n B, h, w, C] or None)."""
    from mobgs_amd.lpips import CLAMP, UNIT_RANGE
    pred, gt = on_device(c, dev)
    flags = UNIT_RANGE | (CLAMP if c["clamp"] else 0)
    _, taps, n = model._loss_forward(gt, pred, flags)
    B = pred.shape[0]
    v = torch.ones(B, device=dev) if v is None else torch.as_tensor(v, dtype=torch.float32, device=dev)
    g_gt, g_pred, tg = model._loss_backward(gt, pred, flags, taps, v, "gt" in want, "pred" in want, chunk=chunk or n,
                                            want_tap_grads=tap_grads)
    return dict(gt=g_gt, pred=g_pred), tg


def check(what, got, want, tol):
    gaps = G.pair_gap(got.cpu(), want)
    for b, err in enumerate(gaps):
        print(f"[lpips-grad] {what} pair {b}: largest error / largest magnitude {err:.2e} (allowed {tol:.2e}), largest "
              f"magnitude {float(want[b].abs().max()):.3e}")
    assert np.isfinite(gaps).all() and (gaps <= tol).all(), (what, gaps.tolist(), tol)


@pytest.mark.parametrize("i", range(len(G.CASES)))
def test_parity_with_float64_autograd(fx, ref_gaps, model, i, hip_device):
    c, t = case(i), truth(i)
    name = G.case_name(i)
    assert np.array_equal(G.probe(c), fx["probe"][i])
    loss, g = public(model, c, hip_device)
    pred, gt = on_device(c, hip_device)
    assert loss.dtype == torch.float32 and loss.shape == (pred.shape[0],)
    assert same_bits(loss, model(pred, gt, clamp=c["clamp"]).total.float())
    gd, tg = direct(model, c, hip_device)
    assert same_bits(gd["pred"], g["pred"]) and gd["gt"] is None
    check(f"{name} g_pred", g["pred"], t["image"][1], G.tolerance("image", ref_gaps))
    for l in range(5):
        q = f"tap{l + 1}"
        assert tg[l].shape[0] == pred.shape[0]
        check(f"{name} {q} of pred", tg[l].permute(0, 3, 1, 2), t[q][1], G.tolerance(q, ref_gaps))
    if i in BOTH_SIDES:
        _, g_gt = public(model, c, hip_device, want=("gt",))
        check(f"{name} g_gt", g_gt["gt"], t["image"][0], G.tolerance("image", ref_gaps))
        _, both = public(model, c, hip_device, want=("pred", "gt"))
        assert same_bits(both["pred"], g["pred"]) and same_bits(both["gt"], g_gt["gt"])
        gb, tb = direct(model, c, hip_device, want=("pred", "gt"))
        assert same_bits(gb["pred"], g["pred"]) and same_bits(gb["gt"], g_gt["gt"])
        for l in range(5):                                   # image 2 b + k: side k of pair b, ground truth first
            q = f"tap{l + 1}"
            assert same_bits(tb[l][1::2], tg[l])
            check(f"{name} {q} of gt", tb[l][0::2].permute(0, 3, 1, 2), t[q][0], G.tolerance(q, ref_gaps))


def test_batch_weights_and_cotangents(ref_gaps, nets, model, hip_device):
    from mobgs_amd.loss_utils import lpips_loss
    i = G.CASES.index((31, 48, 2, "noisy"))
    c = case(i)
    pred, gt = on_device(c, hip_device)
    x, y = (2 * pred - 1).requires_grad_(True), 2 * gt - 1
    per_pair = model.loss(x, y, normalize=False)
    (g_sum,) = torch.autograd.grad(per_pair.sum(), x)
    mean = lpips_loss(x, y, model)
    assert mean.dim() == 0 and same_bits(mean.detach(), per_pair.detach().mean())
    mean.backward()
    assert same_bits(x.grad, g_sum * 0.5)                    # B = 2: the scaling by 1 / B is exact
    assert float(g_sum.abs().max()) > 0
    # a cotangent per pair: powers of two scale the bits, other values hold against float64
    _, g1 = public(model, c, hip_device)
    _, g = public(model, c, hip_device, v=[0.5, 2.0])
    assert same_bits(g["pred"], g1["pred"] * torch.tensor([0.5, 2.0], device=hip_device).reshape(2, 1, 1, 1))
    v = [0.3, 1.7]
    _, g = public(model, c, hip_device, v=v)
    want = G.gradients(c, *nets, v_total=v)
    check("v = (0.3, 1.7) g_pred", g["pred"], want["image"][1], G.tolerance("image", ref_gaps))
    # inputs in [-1, 1]: half the unit-range gradient, exactly
    assert same_bits(g_sum * 2.0, g1["pred"])


def test_exact_zeros(ref_gaps, model, hip_device):
    i = G.CASES.index(G.EXTRA_SIZE + ("identical",))
    g, tg = direct(model, case(i), hip_device, want=("pred", "gt"))
    for a in [g["pred"], g["gt"]] + tg:
        a = a.cpu().numpy()
        assert (a == 0).all() and not np.signbit(a).any()
    # the last image row and column lie in no window of the first convolution
    i = G.CASES.index((38, 34, 1, "noisy"))
    _, g = public(model, case(i), hip_device)
    a = g["pred"].cpu().numpy()
    for edge, want in ((a[:, :, -1, :], truth(i)["image"][1][:, :, -1, :]), (a[:, :, :, -1], truth(i)["image"][1][:, :, :, -1])):
        assert (edge == 0).all() and not np.signbit(edge).any() and float(want.abs().max()) == 0
    assert (a[:, :, :-1, :-1] != 0).mean() > 0.99
    # the clamp: nothing passes outside [0, 1]; the bounds themselves pass
    i = G.CASES.index(G.EXTRA_SIZE + ("clamp",))
    c, t = case(i), truth(i)["image"][1]
    _, g = public(model, c, hip_device)
    a = g["pred"].cpu()
    outside = torch.from_numpy((c["pred"] < 0) | (c["pred"] > 1))
    bound = torch.from_numpy((c["pred"] == 0) | (c["pred"] == 1))
    assert int(outside.sum()) > 1000 and int(bound.sum()) > 100
    assert (a[outside] == 0).all() and not np.signbit(a[outside].numpy()).any() and (t[outside] == 0).all()
    assert (t[bound] != 0).float().mean() > 0.9
    tol = G.tolerance("image", ref_gaps) * float(t.abs().max())
    assert float((a[bound].double() - t[bound]).abs().max()) <= tol
    assert (a[bound] != 0).float().mean() > 0.9


def test_bit_identity(model, hip_device):
    from mobgs_amd import _lib
    from mobgs_amd.lpips import tap_sizes
    i = G.CASES.index((64, 97, 2, "noisy"))
    c = case(i)
    (g, tg), (g2, tg2) = direct(model, c, hip_device), direct(model, c, hip_device)
    assert same_bits(g["pred"], g2["pred"]) and all(same_bits(a, b) for a, b in zip(tg, tg2))
    assert float(g["pred"].abs().max()) > 0
    without, none = direct(model, c, hip_device, tap_grads=False)
    assert none is None and same_bits(without["pred"], g["pred"])
    for k in range(2):                                       # a pair alone
        one = dict(c, pred=c["pred"][k:k + 1], gt=c["gt"][k:k + 1])
        g1, t1 = direct(model, one, hip_device)
        assert same_bits(g1["pred"], g["pred"][k:k + 1]), k
        assert all(same_bits(a, b[k:k + 1]) for a, b in zip(t1, tg)), k
    perm = dict(c, pred=c["pred"][[1, 0]], gt=c["gt"][[1, 0]])
    assert same_bits(direct(model, perm, hip_device)[0]["pred"], g["pred"][[1, 0]])
    both, tb = direct(model, c, hip_device, want=("pred", "gt"))
    assert same_bits(both["pred"], g["pred"]) and all(same_bits(a[1::2], b) for a, b in zip(tb, tg))
    only_gt, _ = direct(model, c, hip_device, want=("gt",))
    assert same_bits(only_gt["gt"], both["gt"]) and only_gt["pred"] is None
    # a scratch budget that holds one pair only: two chunks, forward and backward
    h = _lib.load()
    budget = model.max_scratch_bytes
    taps_per_pair = 2 * 4 * sum(hh * ww * ch for (hh, ww), ch in zip(tap_sizes(64, 97), LR.COUT))
    try:
        model.max_scratch_bytes = max(int(h.mobgs_lpips_scratch_bytes(1, 64, 97)),
                                      int(h.mobgs_lpips_bwd_scratch_bytes(1, 64, 97))) + taps_per_pair
        assert model._loss_chunk(2, 64, 97) == 1
        loss, gp = public(model, c, hip_device)
        assert same_bits(gp["pred"], g["pred"])
        gc, tc = direct(model, c, hip_device)
        assert same_bits(gc["pred"], g["pred"]) and all(same_bits(a, b) for a, b in zip(tc, tg))
    finally:
        model.max_scratch_bytes = budget
    pred, gt = on_device(c, hip_device)
    assert same_bits(loss, model(pred, gt).total.float())


def test_forward_is_unchanged_by_a_backward(model, hip_device):
    c = case(G.CASES.index((130, 67, 2, "noisy")))
    pred, gt = on_device(c, hip_device)

    def snapshot():
        r = model(pred, gt)
        return [r.total.clone(), r.per_layer.clone()] + [m.clone() for m in model.features(pred)]
    before = snapshot()
    _, g = public(model, c, hip_device, want=("pred", "gt"))
    assert float(g["pred"].abs().max()) > 0 and float(g["gt"].abs().max()) > 0
    assert all(same_bits(a, b) for a, b in zip(before, snapshot()))


def test_refusals(model, hip_device):
    from mobgs_amd import _lib
    from mobgs_amd.lpips import COUT, QUANTIZE, UNIT_RANGE, tap_sizes
    dev = hip_device
    b = torch.rand(1, 3, 40, 40, device=dev)
    with pytest.raises(TypeError):
        model.loss(b, b.clone(), quantize=True)
    a = torch.rand(1, 3, 30, 64, device=dev)
    with pytest.raises(ValueError, match=">= 31"):
        model.loss(a, a.clone())
    for bad in ((b, b[:, :2]), (b, torch.rand(1, 3, 40, 41, device=dev)), (b[:0], b[:0]), (b[0, 0], b[0, 0])):
        with pytest.raises(ValueError):
            model.loss(*bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.loss(b, b.cpu())
    # the C call: QUANTIZE with a wanted g_img1, and no wanted side at all
    h = _lib.load()
    taps = [torch.zeros(2, hh, ww, ch, device=dev) for (hh, ww), ch in zip(tap_sizes(40, 40), COUT)]
    tap_ptrs = (ctypes.c_void_p * 5)(*[t.data_ptr() for t in taps])
    nbytes = int(h.mobgs_lpips_bwd_scratch_bytes(1, 40, 40))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    v, g = torch.ones(1, device=dev), torch.full_like(b, 7.0)

    def call(flags, g0, g1):
        return h.mobgs_lpips_alex_bwd(1, 40, 40, _lib.ptr(b), _lib.ptr(b), ctypes.byref(model._record),
                                      ctypes.byref(model._bwd_record), flags, tap_ptrs, _lib.ptr(v), _lib.ptr(scratch), nbytes,
                                      _lib.ptr(g0), _lib.ptr(g1), None, _lib.stream())
    invalid = _lib._DEFINES["MOBGS_E_INVALID"]
    assert call(UNIT_RANGE | QUANTIZE, None, g) == invalid
    assert b"mobgs_lpips_alex_bwd" in h.mobgs_last_error() and b"QUANTIZE" in h.mobgs_last_error()
    assert call(UNIT_RANGE, None, None) == invalid and b"both NULL" in h.mobgs_last_error()
    torch.cuda.synchronize()
    assert float(g.min()) == 7.0 == float(g.max())           # refused before any launch
    assert call(UNIT_RANGE | QUANTIZE, g, None) == 0         # the truncation of img1 does not stand in img0's way


def test_graph_capture(model, hip_device):
    from mobgs_amd.graphed import GraphedCallable
    dev = hip_device
    cases = [case(G.CASES.index((64, 97, 2, s))) for s in ("noisy", "clamp")]
    pred, gt = (t.clone() for t in on_device(cases[0], dev))
    pred.requires_grad_(True)
    grad = torch.zeros_like(pred)

    def step():
        loss = model.loss(pred, gt, clamp=True)
        (g,) = torch.autograd.grad(loss.sum(), pred)
        grad.copy_(g)
        return loss

    graphed = GraphedCallable(step, warmup=1)
    seen = []
    for c in (cases[0], cases[1], cases[0]):
        p, g = on_device(c, dev)
        with torch.no_grad():
            pred.copy_(p)
            gt.copy_(g)
        loss = graphed()
        eager_loss, eager = public(model, dict(c, clamp=True), dev)
        assert same_bits(loss.detach(), eager_loss) and same_bits(grad, eager["pred"])
        seen.append(grad.clone())
    assert same_bits(seen[0], seen[2]) and not same_bits(seen[0], seen[1])


def test_through_render(model, hip_device):
    """lpips_loss on a rendered image: the Gaussian leaves get the gradients that render's backward makes of g_pred."""
    from mobgs_amd import _lib
    from mobgs_amd.camera import PinholeCamera
    from mobgs_amd.gaussian_model import GaussianParams
    from mobgs_amd.gaussian_renderer import render
    from mobgs_amd.helper_model import Sandwich
    from mobgs_amd.loss_utils import lpips_loss
    from mobgs_amd.synth import SynthCamera, dynamic_extras, gaussian_cloud
    from helpers import leaf_map
    dev = hip_device
    _lib.load(build_if_missing=False)
    W, H = 80, 64                                            # the scene of test_gpu_lpips.py's `synthetic`, with gradients
    scam = SynthCamera().scaled(W, H)
    torch.manual_seed(0)
    dec = Sandwich(9, 3).to(dev)
    stat_p, dyn_p = gaussian_cloud(1500, scam, 0), gaussian_cloud(700, scam, 1)
    stat = GaussianParams(stat_p, None, dec, dev, requires_grad=True)
    dyn = GaussianParams(dyn_p, dynamic_extras(dyn_p["xyz"], 0), dec, dev, requires_grad=True)
    cam = PinholeCamera(W, H, scam.K, torch.eye(4), 3 / 23.0, scam.max_time, device=dev)
    bg = torch.zeros(9, device=dev)
    with torch.no_grad():
        image = render(cam, stat, dyn, None, bg)["render"]
    gen = torch.Generator().manual_seed(11)
    gt = (image.cpu() + 0.2 * torch.randn(1, 3, H, W, generator=gen)).clamp(0, 1).to(dev)
    leaves = {k: p for k, p in leaf_map(stat, dyn).items() if p.requires_grad}

    def grads():
        out = {k: p.grad.clone() for k, p in leaves.items() if p.grad is not None}
        for p in leaves.values():
            p.grad = None
        return out
    lpips_loss(render(cam, stat, dyn, None, bg)["render"][None], gt, model).backward()
    chained = grads()
    assert {"s__xyz", "d_control_xyz", "s__features_dc"} <= set(chained)
    for k, g in chained.items():
        assert bool(torch.isfinite(g).all()), k
    assert all(float(chained[k].abs().max()) > 0 for k in ("s__xyz", "d_control_xyz", "s__features_dc"))
    out = render(cam, stat, dyn, None, bg)["render"]
    x = out.detach()[None].clone().requires_grad_(True)
    lpips_loss(x, gt, model).backward()
    out.backward(x.grad[0])
    fed = grads()
    assert set(fed) == set(chained)
    for k in chained:
        assert torch.equal(fed[k], chained[k]), k
