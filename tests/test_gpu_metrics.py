"""The evaluation metrics on the MI355X (csrc/metrics.hip through mobgs_amd.metrics) against float64 on every case of
tests/golden/metrics.npz, under the rule of DESIGN.md 3a: 3 x the fp32 restatement's own distance from float64 -- per
metric the LARGEST over the fixture, metrics_restatement.reference_gaps says why --, not less than 8 x 2^-24 (FLOOR_DB for
a PSNR in dB); run-to-run and batch identity, other layouts, the quantisation, the wrappers, the refusals, a captured
graph, and evaluate_views on the synthetic scene."""
import math
import os

import numpy as np
import pytest
import torch

import metrics_restatement as MR
from helpers import GOLDEN, load, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return load("metrics")


@pytest.fixture(scope="module")
def ref_gaps(fx):
    return MR.reference_gaps(fx)


def on_device(c, dev):
    mask = None if c["mask"] is None else torch.from_numpy(c["mask"]).to(dev)
    return torch.from_numpy(c["pred"]).to(dev), torch.from_numpy(c["gt"]).to(dev), mask


def score(c, dev, **over):
    from mobgs_amd.metrics import image_metrics
    pred, gt, mask = on_device(c, dev)
    kw = dict(data_range=c["data_range"], clamp=c["clamp"], quantize=c["quantize"], arms=c["arms"])
    kw.update(over)
    return image_metrics(pred, gt, mask, **kw)


def table(m):
    """ImageMetrics -> [B, 7] float64 on the host, NaN for an arm that was not evaluated."""
    B = m.l1.shape[0]
    cols = [getattr(m, k) for k in MR.METRICS]
    assert all(t is None or (t.dtype == torch.float64 and t.shape == (B,) and t.is_cuda) for t in cols)
    return torch.stack([torch.full((B,), math.nan, dtype=torch.float64) if t is None else t.cpu() for t in cols], 1).numpy()


@pytest.mark.parametrize("i", range(len(MR.CASES)))
def test_fixture_parity(fx, ref_gaps, i, hip_device):
    c = MR.make_case(i)
    assert np.array_equal(MR.probe(c), fx["probe"][i])
    got = table(score(c, hip_device))
    truth = fx["f64"][int(fx["first"][i]):int(fx["first"][i + 1])]
    assert got.shape == truth.shape
    for j, name in enumerate(MR.METRICS):
        tol = MR.tolerance(name, ref_gaps)
        for b in range(got.shape[0]):
            err = MR.gap(name, got[b, j], truth[b, j])
            print(f"[metrics] {MR.case_name(i)} image {b} {name}: {got[b, j]!r}, float64 {truth[b, j]!r}, "
                  f"{'dB error' if name in MR.DB else 'relative error'} {err:.2e} (allowed {tol:.2e})")
            assert err <= tol, (MR.case_name(i), b, name)
    H, W, B, what = MR.CASES[i]
    if what in ("identical", "flat"):
        assert got[0, 4] == 1.0 and got[0, 6] == 1.0 and got[0, 2] == math.inf and got[0, 3] == math.inf
    if what == "empty":
        assert (got[:, 3] == math.inf).all() and (got[:, 5] == 0).all()
        assert (got[:, 6] == 1.0).all() or min(H, W) < 11


def test_run_to_run_and_batch_identity(hip_device):
    c = MR.make_case(MR.CASES.index((97, 131, 3, "random60")))
    a, b = table(score(c, hip_device)), table(score(c, hip_device))
    assert same_bits(a, b)
    for k in range(3):
        one = dict(c, pred=c["pred"][k:k + 1], gt=c["gt"][k:k + 1], mask=c["mask"][k:k + 1])
        assert same_bits(table(score(one, hip_device)), a[k:k + 1]), k
    # the arms on their own give their own columns, bit for bit, and leave the other's absent
    box, gauss = score(c, hip_device, arms=("box",)), score(c, hip_device, arms=("gauss",))
    assert box.ssim_gauss is None and gauss.ssim_box is None and gauss.ssim_box_masked is None
    tb, tg = table(box), table(gauss)
    assert same_bits(tb[:, :6], a[:, :6]) and same_bits(tg[:, :4], a[:, :4]) and same_bits(tg[:, 6], a[:, 6])


def test_other_layouts(hip_device):
    from mobgs_amd.metrics import image_metrics
    dev = hip_device
    c = MR.make_case(MR.CASES.index((37, 53, 3, "hole")))           # nothing is a multiple of 4
    plain = table(score(c, dev))
    pred, gt, mask = on_device(c, dev)
    # channels-last storage, a slice of a wider batch / a wider image, a [B,1,H,W] mask
    cl = pred.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    wide = torch.rand(5, 3, 37, 60, device=dev)
    wide[1:4, :, :, 4:57] = gt
    sliced = wide[1:4, :, :, 4:57]
    wide_mask = torch.zeros(3, 2, 37, 53, device=dev)
    wide_mask[:, 1] = mask
    assert not cl.is_contiguous() and not sliced.is_contiguous() and not wide_mask[:, 1:2].is_contiguous()
    got = image_metrics(cl, sliced, wide_mask[:, 1:2], data_range=c["data_range"])
    assert same_bits(table(got), plain)
    # a boolean mask and a float64 image are converted, not reinterpreted
    got = image_metrics(pred.double(), gt, mask.bool(), data_range=c["data_range"])
    assert same_bits(table(got), plain)
    # one [3,H,W] pair
    got = image_metrics(pred[1], gt[1], mask[1:2], data_range=c["data_range"])
    assert same_bits(table(got), plain[1:2])


def test_quantize_equals_the_host_quantised_tensor(hip_device):
    from mobgs_amd.metrics import image_metrics
    for what in ("quantize", "clamp"):
        c = MR.make_case(MR.CASES.index((37, 53, 1, what)))
        pred, gt, mask = on_device(c, hip_device)
        for clamp in (False, True):
            q = torch.from_numpy(MR.quantize8(c["pred"])).to(hip_device)
            g = gt.clamp(0, 1) if clamp else gt
            want = image_metrics(q, g, mask, data_range=1.0)
            got = image_metrics(pred, gt, mask, data_range=1.0, clamp=clamp, quantize=True)
            assert same_bits(table(got), table(want)), (what, clamp)
            assert not same_bits(table(image_metrics(pred, gt, mask, data_range=1.0, clamp=clamp)), table(want))
        # clamp alone equals scoring the clamped tensors
        got = image_metrics(pred, gt, mask, data_range=1.0, clamp=True)
        assert same_bits(table(got), table(image_metrics(pred.clamp(0, 1), gt.clamp(0, 1), mask, data_range=1.0)))


def test_wrappers_agree_with_image_metrics(hip_device):
    from mobgs_amd import metrics as M
    dev = hip_device
    c = MR.make_case(MR.CASES.index((37, 53, 1, "random60")))
    pred, gt, mask = on_device(c, dev)
    m = M.image_metrics(pred, gt, mask, data_range=2.0)
    m1 = M.image_metrics(pred, gt, mask, data_range=1.0)
    p, g, k = pred[0].permute(1, 2, 0), gt[0].permute(1, 2, 0), mask[0]
    assert M.compute_psnr(p, g, k[..., None]) == float(m.psnr_masked)
    assert M.compute_psnr(p, g) == float(M.image_metrics(pred, gt, data_range=1.0).psnr_masked)
    assert M.compute_ssim(p, g, k[..., None]) == float(m1.ssim_gauss)
    assert M.compute_ssim(p, g, k[..., None], max_val=2.0) == float(m.ssim_gauss)
    assert M.calculate_ssim(p, g, k, data_range=2.0) == float(m.ssim_box_masked)
    assert M.calculate_ssim(p, g, k[..., None].expand(-1, -1, 3), data_range=2.0) == float(m.ssim_box_masked)
    assert M.structural_similarity(p, g, data_range=2.0) == float(m.ssim_box)
    assert M.structural_similarity(p, g, data_range=1.0) == float(m1.ssim_box)
    assert M.peak_signal_noise_ratio(g, p, data_range=1.0) == 10 * math.log10(1.0 / float(m.mse))
    assert abs(M.peak_signal_noise_ratio(g, p, data_range=1.0) - float(m.psnr)) <= 1e-12 * float(m.psnr)
    assert M.peak_signal_noise_ratio(g, p, data_range=2.0) == 10 * math.log10(4.0 / float(m.mse))
    mse = float(m.se_masked) / (float(m.mask_sum) + 1e-8)
    assert M.calculate_psnr(p, g, k) == 10 * math.log10(1.0 / mse) and float(m.mask_sum) == 3 * float(k.sum())
    # numpy arrays are uploaded; the reference's edge cases
    assert M.structural_similarity(p.cpu().numpy(), g.cpu().numpy(), data_range=2.0) == float(m.ssim_box)
    assert M.calculate_psnr(g, g, k) == 0 and M.compute_psnr(g, g, k) == math.inf
    assert M.peak_signal_noise_ratio(g, g, data_range=1.0) == math.inf
    empty = torch.zeros_like(k)
    assert M.compute_ssim(p, g, empty) == 1.0 and M.compute_psnr(p, g, empty) == math.inf
    assert M.calculate_ssim(p, g, empty, data_range=2.0) == 0.0 and M.calculate_psnr(p, g, empty) == 0


def test_refusals(hip_device):
    from mobgs_amd.metrics import image_metrics
    dev = hip_device
    for n in (6, 10):
        a = torch.rand(1, 3, n, n, device=dev)
        with pytest.raises(ValueError, match="needs H, W >="):
            image_metrics(a, a.clone(), data_range=2.0)
    a = torch.rand(1, 3, 10, 40, device=dev)
    assert image_metrics(a, a.clone(), data_range=2.0, arms=("box",)).ssim_gauss is None
    with pytest.raises(ValueError, match="gauss"):
        image_metrics(a, a.clone(), data_range=2.0, arms=("gauss",))
    b = torch.rand(1, 3, 16, 16, device=dev)
    for bad, kw in (((b, b[:, :2]), {}), ((b, torch.rand(1, 3, 16, 17, device=dev)), {}), ((b, b), {"arms": ()}),
                    ((b, b), {"arms": ("tent",)}), ((b, b, torch.ones(1, 16, 15, device=dev)), {}),
                    ((b[:0], b[:0]), {})):
        with pytest.raises(ValueError):
            image_metrics(*bad, **{"data_range": 2.0, **kw})
    for r in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="data_range"):
            image_metrics(b, b, data_range=r)
    with pytest.raises(RuntimeError, match="no CPU path"):
        image_metrics(b, b.cpu(), data_range=2.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        image_metrics(b, b, torch.ones(1, 16, 16), data_range=2.0)


def test_graph_capture(hip_device):
    from mobgs_amd.graphed import GraphedCallable
    from mobgs_amd.metrics import image_metrics
    dev = hip_device
    cases = [MR.make_case(MR.CASES.index((37, 53, 3, s))) for s in ("random60", "stripes")]
    static = dict(zip(("pred", "gt", "mask"), (t.clone() for t in on_device(cases[0], dev))))

    def step():
        m = image_metrics(static["pred"], static["gt"], static["mask"], data_range=2.0)
        return tuple(getattr(m, k) for k in MR.METRICS)

    graphed = GraphedCallable(step, warmup=1)
    seen = []
    for c in (cases[0], cases[1], cases[0]):
        for k, v in zip(("pred", "gt", "mask"), on_device(c, dev)):
            static[k].copy_(v)
        replay = torch.stack([t.detach().cpu().clone() for t in graphed()], 1).numpy()
        assert same_bits(replay, table(score(c, dev)))
        seen.append(replay)
    assert same_bits(seen[0], seen[2]) and not same_bits(seen[0], seen[1])


def test_evaluate_views(hip_device):
    from mobgs_amd import _lib
    from mobgs_amd.camera import PinholeCamera
    from mobgs_amd.gaussian_model import GaussianParams
    from mobgs_amd.gaussian_renderer import render
    from mobgs_amd.helper_model import Sandwich
    from mobgs_amd.loss_utils import psnr
    from mobgs_amd.metrics import evaluate_views, image_metrics
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
    cams = []
    for k in range(3):
        w2c = torch.eye(4)
        w2c[0, 3] = 0.05 * (k - 1)
        cams.append(PinholeCamera(W, H, scam.K, w2c, (3 + 8 * k) / 23.0, scam.max_time, device=dev))
    bg = torch.zeros(9, device=dev)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        images = torch.stack([render(cam, stat, dyn, None, bg)["render"] for cam in cams])
    assert images.shape == (3, 3, H, W) and float(images.std()) > 0.01
    gt = (images.cpu() + 0.2 * torch.randn(3, 3, H, W, generator=g)).clamp(-0.1, 1.1).to(dev)
    rep = evaluate_views(cams, stat, dyn, None, bg, gt)
    assert same_bits(rep["images"].double().cpu().numpy(), images.double().cpu().numpy())
    per_view = [image_metrics(images[k:k + 1], gt[k:k + 1], data_range=2.0, clamp=True) for k in range(3)]
    want = np.concatenate([table(m) for m in per_view])
    assert same_bits(table(rep["per_view"]), want)
    for j, name in ((0, "l1"), (2, "psnr"), (4, "ssim_box"), (6, "ssim_gauss")):
        mean = float(want[:, j].mean())                              # (the device adds the three in its own order)
        assert abs(rep[name] - mean) <= 4 * 2.0 ** -52 * abs(mean), name
    # a list of [3,H,W] ground truths on the host, and another data range
    rep1 = evaluate_views(cams, stat, dyn, None, bg, list(gt.cpu()), ssim_data_range=1.0)
    assert rep1["psnr"] == rep["psnr"] and rep1["l1"] == rep["l1"] and rep1["ssim_box"] < rep["ssim_box"]
    ours = rep["per_view"].psnr.cpu()
    theirs = psnr(images.clamp(0, 1), gt.clamp(0, 1)).reshape(-1).double().cpu()
    print(f"[metrics] evaluate_views psnr {ours.tolist()} dB, loss_utils.psnr {theirs.tolist()} dB, largest difference "
          f"{float((ours - theirs).abs().max()):.2e} dB (allowed {MR.FLOOR_DB:.2e})")
    assert float((ours - theirs).abs().max()) <= MR.FLOOR_DB


def test_scikit_image_vectors(hip_device):
    """Present only after scripts/dump_metric_vectors.py ran where scikit-image is installed; skipped otherwise."""
    path = os.path.join(GOLDEN, "metrics_external", "skimage.npz")
    if not os.path.exists(path):
        pytest.skip("no tests/golden/metrics_external/skimage.npz (scripts/dump_metric_vectors.py): UNPINNED")
    ex = dict(np.load(path))
    for n, i in enumerate(ex["case"].tolist()):
        c = MR.make_case(i)
        assert np.array_equal(MR.probe(c), ex["probe"][n])
        for r, key in ((1.0, "ssim_r1"), (2.0, "ssim_r2"), (2.0, "ssim_default")):
            got = float(score(c, hip_device, data_range=r, arms=("box",)).ssim_box)
            assert MR.gap("ssim_box", got, ex[key][n]) <= MR.FLOOR, (MR.case_name(i), key)
