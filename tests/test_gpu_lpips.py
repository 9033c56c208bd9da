"""LPIPS on the MI355X (csrc/lpips.hip through mobgs_amd.lpips) with the seeded trunk of lpips_restatement and the
reference's heads, against float64 on every case of tests/golden/lpips.npz, under the rule of DESIGN.md 3a: per quantity
3 x the reference's own fp32 distance from float64 -- the larger of torch's fp32 convolution and conv_sequential, largest
over the fixture --, not less than 8 x 2^-24 relative.  Taps are compared per layer, as the largest error over the map
relative to the map's largest value.  Then run-to-run, batch and chunk identity, exact zeros, the reference's forward(), the
quantisation, the features() layout, a captured graph, and the hook-ups of evaluate_views and render_test_tto."""
import types

import numpy as np
import pytest
import torch

import lpips_restatement as LR
from helpers import load, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return load("lpips")


@pytest.fixture(scope="module")
def ref_gaps(fx):
    return LR.reference_gaps(fx)


@pytest.fixture(scope="module")
def nets():
    return LR.seeded_trunk(), LR.reference_heads()


@pytest.fixture(scope="module")
def model(hip_device, nets):
    from mobgs_amd.lpips import LpipsAlex
    return LpipsAlex(*nets, device=hip_device)


def on_device(c, dev):
    return torch.from_numpy(c["pred"]).to(dev), torch.from_numpy(c["gt"]).to(dev)


def score(model, c, dev, **over):
    pred, gt = on_device(c, dev)
    kw = dict(clamp=c["clamp"], quantize=c["quantize"])
    kw.update(over)
    return table(model(pred, gt, **kw))


def table(r):
    """LpipsResult -> [B, 6] float64 on the host: the total, then the five layer values."""
    B = r.total.shape[0]
    assert r.total.dtype == r.per_layer.dtype == torch.float64 and r.total.is_cuda and r.per_layer.is_cuda
    assert r.total.shape == (B,) and r.per_layer.shape == (B, 5)
    return torch.cat([r.total[:, None], r.per_layer], 1).cpu().numpy()


@pytest.mark.parametrize("i", range(len(LR.CASES)))
def test_fixture_parity(fx, ref_gaps, nets, model, i, hip_device):
    c = LR.make_case(i)
    assert np.array_equal(LR.probe(c), fx["probe"][i])
    got = score(model, c, hip_device)
    truth = fx["f64"][int(fx["first"][i]):int(fx["first"][i + 1])]
    assert got.shape == truth.shape
    for j, name in enumerate(LR.QUANTITIES):
        tol = LR.tolerance(name, ref_gaps)
        for b in range(got.shape[0]):
            err = LR.rel_gap(got[b, j], truth[b, j])
            print(f"[lpips] {LR.case_name(i)} pair {b} {name}: {got[b, j]!r}, float64 {truth[b, j]!r}, relative error "
                  f"{err:.2e} (allowed {tol:.2e})")
            assert err <= tol, (LR.case_name(i), b, name)
    what = LR.CASES[i][3]
    if what == "identical":
        assert (got == 0.0).all() and not np.signbit(got).any()
    if what in ("noisy", "flat"):
        # the five ReLU maps of both images against the float64 trunk
        with torch.no_grad():
            want = [LR.trunk_taps(2 * torch.from_numpy(c[k]).double() - 1, nets[0], torch.float64) for k in ("gt", "pred")]
        maps = [model.features(torch.from_numpy(c[k]).to(hip_device)) for k in ("gt", "pred")]
        for l, name in enumerate(LR.TAPS):
            tol = LR.tolerance(name, ref_gaps)
            for s in (0, 1):
                assert maps[s][l].shape == want[s][l].shape and float(want[s][l].max()) > 0
                err = LR.map_gap(maps[s][l].cpu(), want[s][l])
                print(f"[lpips] {LR.case_name(i)} image {s} {name} {tuple(want[s][l].shape)}: largest error / largest value "
                      f"{err:.2e} (allowed {tol:.2e})")
                assert err <= tol, (LR.case_name(i), s, name)


def test_run_to_run_batch_and_chunk_identity(model, hip_device):
    from mobgs_amd import _lib
    c = LR.make_case(LR.CASES.index((64, 97, 3, "noisy")))
    a, b = score(model, c, hip_device), score(model, c, hip_device)
    assert same_bits(a, b) and (a > 0).all()
    for k in range(3):
        one = dict(c, pred=c["pred"][k:k + 1], gt=c["gt"][k:k + 1])
        assert same_bits(score(model, one, hip_device), a[k:k + 1]), k
    order = [2, 0, 1]
    perm = dict(c, pred=c["pred"][order], gt=c["gt"][order])
    assert same_bits(score(model, perm, hip_device), a[order])
    # a scratch budget that holds one pair only: three chunks
    h = _lib.load()
    budget = model.max_scratch_bytes
    try:
        model.max_scratch_bytes = int(h.mobgs_lpips_scratch_bytes(1, 64, 97))
        assert model._chunk(3, 64, 97) == 1
        assert same_bits(score(model, c, hip_device), a)
        model.max_scratch_bytes = int(h.mobgs_lpips_scratch_bytes(2, 64, 97))
        assert model._chunk(3, 64, 97) == 2                              # chunks of 2 and 1
        assert same_bits(score(model, c, hip_device), a)
    finally:
        model.max_scratch_bytes = budget
    assert type(model).max_scratch_bytes == budget


def test_forward_is_the_unit_range_call(model, hip_device):
    c = LR.make_case(LR.CASES.index((31, 48, 2, "noisy")))
    pred, gt = on_device(c, hip_device)
    a = model(pred, gt)
    v = model.forward(2 * pred - 1, 2 * gt - 1)
    assert v.shape == (2, 1, 1, 1) and v.dtype == torch.float32 and v.is_cuda
    assert same_bits(v.reshape(-1).cpu().numpy(), a.total.float().cpu().numpy())
    assert same_bits(model.forward(pred, gt, normalize=True).cpu().numpy(), v.cpu().numpy())
    # the reference's argument order (metrics.py:130 passes the ground truth first): the distance is symmetric, bit for bit
    assert same_bits(model.forward(2 * gt - 1, 2 * pred - 1).cpu().numpy(), v.cpu().numpy())
    # one [3,H,W] pair
    assert same_bits(table(model(pred[1], gt[1])), table(a)[1:2])


def test_quantize_and_clamp_equal_the_host_prepared_tensors(model, hip_device):
    for what in ("quantize", "clamp"):
        c = LR.make_case(LR.CASES.index((64, 97, 3, what)))
        pred, gt = on_device(c, hip_device)
        q = LR.quantize8(torch.from_numpy(c["pred"])).to(hip_device)
        for clamp in (False, True):
            g = gt.clamp(0, 1) if clamp else gt
            want = table(model(q, g))
            assert same_bits(table(model(pred, gt, clamp=clamp, quantize=True)), want), (what, clamp)
            assert not same_bits(table(model(pred, gt, clamp=clamp)), want)
        assert same_bits(table(model(pred, gt, clamp=True)), table(model(pred.clamp(0, 1), gt.clamp(0, 1))))


def test_features_layout(model, hip_device):
    from mobgs_amd.lpips import COUT, tap_sizes
    c = LR.make_case(LR.CASES.index((130, 67, 2, "noisy")))
    pred, _ = on_device(c, hip_device)
    maps = model.features(pred)
    assert [tuple(m.shape) for m in maps] == [(2, ch, h, w) for (h, w), ch in zip(tap_sizes(130, 67), COUT)]
    assert all(m.dtype == torch.float32 and m.is_cuda and float(m.min()) >= 0.0 for m in maps)
    for k in range(2):
        alone = model.features(pred[k])
        for l in range(5):
            assert same_bits(alone[l].cpu().numpy(), maps[l][k:k + 1].cpu().numpy()), (k, l)


def test_refusals(model, hip_device):
    a = torch.rand(1, 3, 30, 64, device=hip_device)
    with pytest.raises(ValueError, match=">= 31"):
        model(a, a.clone())
    with pytest.raises(ValueError, match=">= 31"):
        model.forward(a.permute(0, 1, 3, 2), a.permute(0, 1, 3, 2))
    b = torch.rand(1, 3, 40, 40, device=hip_device)
    for bad in ((b, b[:, :2]), (b, torch.rand(1, 3, 40, 41, device=hip_device)), (b[:0], b[:0]), (b[0, 0], b[0, 0])):
        with pytest.raises(ValueError):
            model(*bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        model(b, b.cpu())
    with pytest.raises(NotImplementedError):
        model.forward(b, b, mask=torch.ones(1, 1, 40, 40, device=hip_device))
    # other storage is converted, not reinterpreted
    want = table(model(b, b.flip(3)))
    cl = b.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not cl.is_contiguous() and same_bits(table(model(cl.double(), b.flip(3))), want)


def test_graph_capture(model, hip_device):
    from mobgs_amd.graphed import GraphedCallable
    dev = hip_device
    cases = [LR.make_case(LR.CASES.index((64, 97, 3, s))) for s in ("noisy", "quantize")]
    static = dict(zip(("pred", "gt"), (t.clone() for t in on_device(cases[0], dev))))

    def step():
        r = model(static["pred"], static["gt"], quantize=True)
        return r.total, r.per_layer

    graphed = GraphedCallable(step, warmup=1)
    seen = []
    for c in (cases[0], cases[1], cases[0]):
        for k, v in zip(("pred", "gt"), on_device(c, dev)):
            static[k].copy_(v)
        total, per_layer = graphed()
        replay = torch.cat([total[:, None], per_layer], 1).detach().cpu().clone().numpy()
        assert same_bits(replay, score(model, c, dev, quantize=True))
        seen.append(replay)
    assert same_bits(seen[0], seen[2]) and not same_bits(seen[0], seen[1])


@pytest.fixture(scope="module")
def synthetic(hip_device):
    from mobgs_amd import _lib
    from mobgs_amd.camera import PinholeCamera
    from mobgs_amd.gaussian_model import GaussianParams
    from mobgs_amd.gaussian_renderer import render
    from mobgs_amd.helper_model import Sandwich
    from mobgs_amd.synth import SynthCamera, dynamic_extras, gaussian_cloud
    dev = hip_device
    _lib.load(build_if_missing=False)
    W, H = 80, 64
    scam = SynthCamera().scaled(W, H)
    torch.manual_seed(0)
    dec = Sandwich(9, 3).to(dev)
    stat_p, dyn_p = gaussian_cloud(1500, scam, 0), gaussian_cloud(700, scam, 1)
    stat = GaussianParams(stat_p, None, dec, dev, requires_grad=False)
    dyn = GaussianParams(dyn_p, dynamic_extras(dyn_p["xyz"], 0), dec, dev, requires_grad=False)
    for p in dec.parameters():
        p.requires_grad_(False)
    cams = []
    for k in range(2):
        w2c = torch.eye(4)
        w2c[0, 3] = 0.05 * (k - 1)
        cams.append(PinholeCamera(W, H, scam.K, w2c, (3 + 8 * k) / 23.0, scam.max_time, device=dev))
    bg = torch.zeros(9, device=dev)
    with torch.no_grad():
        images = torch.stack([render(cam, stat, dyn, None, bg)["render"] for cam in cams])
    g = torch.Generator().manual_seed(11)
    gt = (images.cpu() + 0.2 * torch.randn(2, 3, H, W, generator=g)).clamp(-0.1, 1.1).to(dev)
    return types.SimpleNamespace(W=W, H=H, stat=stat, dyn=dyn, cams=cams, bg=bg, images=images, gt=gt, stat_gaussians=stat,
                                 dyn_gaussians=dyn)


def test_evaluate_views_hook(model, synthetic):
    from mobgs_amd.metrics import evaluate_views
    s = synthetic
    plain = evaluate_views(s.cams, s.stat, s.dyn, None, s.bg, s.gt)
    assert set(plain) == {"per_view", "l1", "psnr", "ssim_box", "ssim_gauss", "images"}
    rep = evaluate_views(s.cams, s.stat, s.dyn, None, s.bg, s.gt, lpips=model)
    assert set(rep) == set(plain) | {"lpips", "lpips_per_view"}
    assert rep["psnr"] == plain["psnr"] and rep["ssim_box"] == plain["ssim_box"]
    want = model(s.images, s.gt, clamp=True).total
    assert same_bits(rep["lpips_per_view"].cpu().numpy(), want.cpu().numpy()) and rep["lpips_per_view"].shape == (2,)
    assert isinstance(rep["lpips"], float) and abs(rep["lpips"] - float(want.mean())) <= 1e-15 and rep["lpips"] > 0


def test_render_test_tto_hook(model, synthetic):
    from mobgs_amd.tto import render_test_tto
    s = synthetic
    gts = s.gt.clamp(0, 1)
    kw = dict(tto_steps=1, renderArgs=[None, s.bg], initialize_from_previous_step_factor=1)
    plain = render_test_tto(s.H, s.W, s, s.cams, None, gts, **kw)
    assert set(plain) == {"poses", "images", "loss_histories", "step_factors", "lr_factors", "metrics"}
    res = render_test_tto(s.H, s.W, s, s.cams, None, gts, lpips=model, **kw)
    assert set(res) == set(plain) | {"lpips"}
    assert torch.equal(res["images"], plain["images"])
    want = model(res["images"], gts, clamp=True, quantize=True)
    assert same_bits(table(res["lpips"]), table(want)) and (table(want) > 0).all()
