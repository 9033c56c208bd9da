"""The spatial and masked forms of LPIPS on the MI355X (mobgs_lpips_alex_spatial through mobgs_amd.lpips and
mobgs_amd.metrics) with the seeded trunk and the reference's heads, against float64 on every case and mask of
tests/golden/lpips_spatial.npz under the rule of DESIGN.md 3a: per quantity 3 x the reference's own fp32 distance from
float64 -- the larger of torch's fp32 convolution and conv_sequential, largest over the fixture --, not less than 8 x 2^-24
relative.  The map is compared element-wise, as the largest error relative to the map's largest value, against a float64 map
recomputed here.  Then the single-pixel masks, the plain call's layer values, bit identity, exact zeros, the reference's
calls, compute_lpips, a captured graph and evaluate_views(masks=).

Observed on the MI355X against allowed (docs/MEASUREMENT_LOG.md has the table): the map 1.7e-6 of 5.0e-6, masked mean 2.1e-6
of 8.7e-6, masked layers up to 8.4e-6 of 1.7e-5, compute_lpips 2.2e-6 of 5.2e-6; every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import lpips_restatement as LR
import lpips_spatial_restatement as LS
from helpers import load, same_bits
from test_gpu_lpips import synthetic  # noqa: F401  (the synthetic scene is built afresh by this module)

pytestmark = pytest.mark.gpu
ROW = ("mean", "masked_mean", "masked_total", "masked_per_layer", "numerators", "denominators", "map_mask_sum", "mask_sum",
       "map_sum")


@pytest.fixture(scope="module")
def fx():
    return load("lpips_spatial")


@pytest.fixture(scope="module")
def ref_gaps(fx):
    return LS.reference_gaps(fx)


@pytest.fixture(scope="module")
def nets():
    return LR.seeded_trunk(), LR.reference_heads()


@pytest.fixture(scope="module")
def model(hip_device, nets):
    from mobgs_amd.lpips import LpipsAlex
    return LpipsAlex(*nets, device=hip_device)


def dev_pair(c, dev):
    return torch.from_numpy(c["pred"]).to(dev), torch.from_numpy(c["gt"]).to(dev)


def table(r):
    """LpipsSpatial -> [B, 8] float64 on the host in LS.VALUES' order."""
    B = r.mean.shape[0]
    for name in ROW:
        t = getattr(r, name)
        assert t.dtype == torch.float64 and t.is_cuda and t.shape[0] == B, name
    assert r.masked_per_layer.shape == r.numerators.shape == r.denominators.shape == (B, 5)
    return torch.cat([r.mean[:, None], r.masked_mean[:, None], r.masked_total[:, None], r.masked_per_layer], 1).cpu().numpy()


def everything(r):
    """All float64 columns of a result, [B, 21], on the host."""
    return torch.cat([getattr(r, n).reshape(r.mean.shape[0], -1) for n in ROW], 1).cpu().numpy()


@pytest.fixture(scope="module")
def noisy3(model, hip_device):
    """The 64 x 97, B = 3 case with its soft mask, scored once: (case, mask, result)."""
    i = LS.CASES.index((64, 97, 3, "noisy"))
    c, m = LS.make_case(i), torch.from_numpy(LS.make_mask(i, "soft")).to(hip_device)
    return c, m, model.spatial(*dev_pair(c, hip_device), m)


@pytest.mark.parametrize("i", range(len(LS.CASES)))
def test_fixture_parity(fx, ref_gaps, nets, model, i, hip_device):
    H, W, B, what = LS.CASES[i]
    c = LS.make_case(i)
    masks = [LS.make_mask(i, n) for n in LS.MASKS]
    assert np.array_equal(LS.probe(c, masks), fx["probe"][i])
    truth = LS.rows(fx, i)
    with torch.no_grad():
        ds = LS.dist_maps(c["gt"], c["pred"], *nets, torch.float64)
        want_map = LS.spatial_map(ds, H, W)
    pred, gt = dev_pair(c, hip_device)
    tol_map = LS.tolerance("map", ref_gaps)
    first_map = None
    for k, name in enumerate(LS.MASKS):
        r = model.spatial(pred, gt, torch.from_numpy(masks[k]).to(hip_device))
        assert r.map.shape == (B, 1, H, W) and r.map.dtype == torch.float32 and r.map.is_cuda
        got_map = r.map.cpu()
        if first_map is None:
            first_map = got_map
            err = LS.map_gap(got_map, want_map)
            print(f"[lpips-spatial] {LS.case_name(i)} map: largest error / largest value {err:.2e} (allowed {tol_map:.2e})")
            assert err <= tol_map, LS.case_name(i)
            if what == "identical":
                assert (got_map == 0).all() and not np.signbit(got_map.numpy()).any()
            else:
                assert float(want_map.max()) > 0
        else:
            assert same_bits(got_map.numpy(), first_map.numpy()), name          # the mask does not touch the map
        got = table(r)
        assert np.isfinite(everything(r)).all(), name
        for j, q in enumerate(LS.VALUES):
            tol = LS.tolerance(q, ref_gaps)
            for b in range(B):
                if truth[k, b, j] == 0.0:
                    # an empty mask, a mask that is empty at this tap (a Bernoulli mask at a 1 x 1 tap, a single pixel
                    # the nearest-neighbour resize does not sample), equal images: exactly 0
                    assert got[b, j] == 0.0 and not np.signbit(got[b, j]), (LS.case_name(i), name, b, q)
                    continue
                err = LS.rel_gap(got[b, j], truth[k, b, j])
                print(f"[lpips-spatial] {LS.case_name(i)} {name} pair {b} {q}: {got[b, j]!r}, float64 {truth[k, b, j]!r}, "
                      f"relative error {err:.2e} (allowed {tol:.2e})")
                assert err <= tol, (LS.case_name(i), name, b, q)


@pytest.mark.parametrize("size", ((31, 31, 1), (49, 61, 1), (130, 67, 2)))
def test_single_pixel_mask_reads_the_map(model, hip_device, size):
    i = LS.CASES.index(size + ("noisy",))
    H, W, B, _ = LS.CASES[i]
    pred, gt = dev_pair(LS.make_case(i), hip_device)
    for name, (y, x) in (("first", (0, 0)), ("last", (H - 1, W - 1))):
        r = model.spatial(pred, gt, torch.from_numpy(LS.make_mask(i, name)).to(hip_device))
        want = r.map[:, 0, y, x].double().cpu().numpy()
        assert (want > 0).all() and same_bits(r.masked_mean.cpu().numpy(), want), name
        assert same_bits(r.map_mask_sum.cpu().numpy(), want) and (r.mask_sum.cpu().numpy() == 1.0).all()


def test_ones_mask_against_the_plain_call(model, hip_device):
    """The fp32 terms are the plain call's; only the float64 order may differ: (P - 1) 2^-53 at most."""
    from mobgs_amd.lpips import tap_sizes
    for size in ((31, 48, 2), (130, 67, 2), (49, 61, 1)):
        i = LS.CASES.index(size + ("noisy",))
        H, W, B, _ = LS.CASES[i]
        pred, gt = dev_pair(LS.make_case(i), hip_device)
        plain = model(pred, gt).per_layer.cpu().numpy()
        none = model.spatial(pred, gt, None)
        ones = model.spatial(pred, gt, torch.ones(B, H, W, device=hip_device))
        assert same_bits(everything(none), everything(ones))                   # no mask is the mask of ones
        pixels = np.array([h * w for h, w in tap_sizes(H, W)], np.float64)
        assert np.array_equal(ones.denominators.cpu().numpy(), np.broadcast_to(pixels, (B, 5)))
        got = ones.numerators.cpu().numpy() / pixels
        err = np.abs(got - plain) / plain
        print(f"[lpips-spatial] {LS.case_name(i)} numerator / P against the plain call: {err.max():.2e} (allowed 1e-12)")
        assert (err <= 1e-12).all()
        assert same_bits(ones.mean.cpu().numpy(), ones.masked_mean.cpu().numpy())


def test_bit_identity(model, noisy3, hip_device):
    from mobgs_amd import _lib
    c, m, r = noisy3
    pred, gt = dev_pair(c, hip_device)
    a, a_map = everything(r), r.map.cpu().numpy()
    assert (a[:, :3] > 0).all()
    again = model.spatial(pred, gt, m)
    assert same_bits(everything(again), a) and same_bits(again.map.cpu().numpy(), a_map)
    for k in range(3):
        one = model.spatial(pred[k:k + 1], gt[k:k + 1], m[k:k + 1])
        assert same_bits(everything(one), a[k:k + 1]) and same_bits(one.map.cpu().numpy(), a_map[k:k + 1]), k
    order = [2, 0, 1]
    perm = model.spatial(pred[order], gt[order], m[order])
    assert same_bits(everything(perm), a[order]) and same_bits(perm.map.cpu().numpy(), a_map[order])
    off = model.spatial(pred, gt, m, want_map=False)
    assert off.map is None and same_bits(everything(off), a)
    h = _lib.load()
    budget = model.max_scratch_bytes
    try:
        model.max_scratch_bytes = int(h.mobgs_lpips_spatial_scratch_bytes(1, 64, 97))
        assert model._chunk(3, 64, 97, spatial=True) == 1                      # one pair per chunk
        chunked = model.spatial(pred, gt, m)
        assert same_bits(everything(chunked), a) and same_bits(chunked.map.cpu().numpy(), a_map)
    finally:
        model.max_scratch_bytes = budget
    assert type(model).max_scratch_bytes == budget


def test_exact_values(model, noisy3, hip_device):
    c, m, _ = noisy3
    pred, gt = dev_pair(c, hip_device)
    same = model.spatial(gt, gt.clone(), m)
    assert (same.map == 0).all() and not np.signbit(same.map.cpu().numpy()).any()
    t = table(same)
    assert (t == 0.0).all() and not np.signbit(t).any()
    assert (same.numerators == 0).all() and (same.denominators > 0).all() and (same.mask_sum > 0).all()
    empty = model.spatial(pred, gt, torch.zeros_like(m))
    e = everything(empty)
    assert np.isfinite(e).all()
    assert (empty.masked_mean == 0).all() and (empty.masked_total == 0).all() and (empty.masked_per_layer == 0).all()
    assert (empty.denominators == 0).all() and (empty.mask_sum == 0).all() and (empty.mean > 0).all()


def test_the_reference_calls(model, noisy3, hip_device):
    c, m, r = noisy3
    pred, gt = dev_pair(c, hip_device)
    fmap = model.forward_spatial(2 * pred - 1, 2 * gt - 1)
    assert fmap.shape == (3, 1, 64, 97) and fmap.dtype == torch.float32
    assert same_bits(fmap.cpu().numpy(), r.map.cpu().numpy())
    assert same_bits(model.forward_spatial(pred, gt, normalize=True).cpu().numpy(), fmap.cpu().numpy())
    # the mask= call divides sums over the whole batch
    two = model.spatial(pred[:2], gt[:2], m[:2], want_map=False)
    want = (two.numerators.sum(0) / (two.denominators.sum(0) + 1e-8)).sum().float()
    for mask in (m[:2], m[:2, None], m[:2, None].expand(2, 3, 64, 97)):
        got = model.forward_masked(pred[:2], gt[:2], mask, normalize=True)
        assert got.shape == () and got.dtype == torch.float32 and got.is_cuda
        assert same_bits(got.cpu().numpy(), want.cpu().numpy())
    assert same_bits(model.forward_masked(2 * pred[:2] - 1, 2 * gt[:2] - 1, m[:2]).cpu().numpy(), want.cpu().numpy())
    assert float(want) > 0
    with pytest.raises(NotImplementedError):
        model.forward(pred, gt, spatial=True)
    with pytest.raises(ValueError, match="mask"):
        model.spatial(pred, gt, m[:2])
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.spatial(pred, gt, m.cpu())


def test_compute_lpips(fx, ref_gaps, model, hip_device):
    from mobgs_amd.metrics import compute_lpips
    tol = LS.tolerance("compute_lpips", ref_gaps)
    for n, i in enumerate(LS.CL_CASES):
        c = LS.make_case(i)
        img0, img1 = (np.ascontiguousarray(c[k][0].transpose(1, 2, 0)) for k in ("gt", "pred"))
        for k, name in enumerate(LS.CL_MASKS):
            m = LS.make_mask(i, name)[0]
            got = compute_lpips(model, img0, img1, m[..., None], device=hip_device)
            truth = float(fx["cl_f64"][n, k])
            err = LS.rel_gap(got, truth)
            print(f"[lpips-spatial] {LS.case_name(i)} compute_lpips {name}: {got!r}, float64 {truth!r}, relative error "
                  f"{err:.2e} (allowed {tol:.2e})")
            assert isinstance(got, float) and truth > 0 and err <= tol, (LS.case_name(i), name)
            if name == "ones":
                assert compute_lpips(model, img0, img1, device=hip_device) == got
                assert compute_lpips(model, torch.from_numpy(img0).to(hip_device), torch.from_numpy(img1).to(hip_device),
                                     torch.from_numpy(m).to(hip_device)) == got
    assert compute_lpips(model, img0, img1, np.zeros_like(m), device=hip_device) == 0.0


def test_graph_capture(model, hip_device):
    from mobgs_amd.graphed import GraphedCallable
    dev = hip_device
    i = LS.CASES.index((64, 97, 3, "noisy"))
    c = LS.make_case(i)
    inputs = [dev_pair(c, dev) + (torch.from_numpy(LS.make_mask(i, n)).to(dev),) for n in ("soft", "rect")]
    static = [t.clone() for t in inputs[0]]

    def step():
        r = model.spatial(static[0], static[1], static[2])
        return (r.map,) + tuple(getattr(r, n) for n in ROW)

    graphed = GraphedCallable(step, warmup=1)
    seen = []
    for k in (0, 1, 0):
        for s, v in zip(static, inputs[k]):
            s.copy_(v)
        out = graphed()
        fmap = out[0].detach().cpu().clone().numpy()
        cols = torch.cat([t.reshape(3, -1) for t in out[1:]], 1).detach().cpu().clone().numpy()
        direct = model.spatial(*inputs[k])
        assert same_bits(fmap, direct.map.cpu().numpy()) and same_bits(cols, everything(direct))
        seen.append(cols)
    assert same_bits(seen[0], seen[2]) and not same_bits(seen[0], seen[1])


def test_evaluate_views_masks(model, synthetic, hip_device):  # noqa: F811
    from mobgs_amd.metrics import evaluate_views, image_metrics
    s = synthetic
    g = torch.Generator().manual_seed(5)
    masks = (torch.rand(2, s.H, s.W, generator=g) < 0.6).float().to(hip_device)
    plain = evaluate_views(s.cams, s.stat, s.dyn, None, s.bg, s.gt, lpips=model)
    rep = evaluate_views(s.cams, s.stat, s.dyn, None, s.bg, s.gt, lpips=model, masks=masks)
    assert set(rep) == set(plain) | {"mpsnr", "mssim", "mlpips", "mlpips_per_view", "per_view_masked"}
    for k in ("l1", "psnr", "ssim_box", "ssim_gauss", "lpips"):
        assert rep[k] == plain[k], k
    assert torch.equal(rep["images"], plain["images"]) and torch.equal(rep["lpips_per_view"], plain["lpips_per_view"])
    for a, b in zip(rep["per_view"], plain["per_view"]):
        assert torch.equal(a, b)
    without = evaluate_views(s.cams, s.stat, s.dyn, None, s.bg, s.gt, masks=masks)
    assert set(without) == (set(rep) - {"lpips", "lpips_per_view", "mlpips", "mlpips_per_view"})
    assert without["mpsnr"] == rep["mpsnr"] and without["mssim"] == rep["mssim"]
    direct = image_metrics(s.images, s.gt, masks, data_range=1.0, clamp=True, arms=("gauss",))
    assert rep["mpsnr"] == float(direct.psnr_masked.mean()) and rep["mssim"] == float(direct.ssim_gauss.mean())
    m = masks[:, None]
    want = model.spatial(s.images.clamp(0, 1) * m, s.gt.clamp(0, 1) * m, masks, want_map=False).masked_mean
    assert rep["mlpips_per_view"].shape == (2,) and same_bits(rep["mlpips_per_view"].cpu().numpy(), want.cpu().numpy())
    assert isinstance(rep["mlpips"], float) and abs(rep["mlpips"] - float(want.mean())) <= 1e-15 and rep["mlpips"] > 0
    assert np.isfinite(rep["mpsnr"]) and 0 < rep["mssim"] < 1
