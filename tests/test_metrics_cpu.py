"""The evaluation metrics without a GPU: the fixture (tests/golden/metrics.npz, scripts/make_golden_metrics.py) replayed
through the restatement, the edge cases by value, the restatement's window indexing against a direct double loop, the
aligned test pose, the C ABI's size query and refusals, and the public names with their refusal of host tensors."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

import metrics_restatement as MR
from helpers import GOLDEN, load

# +, -, *, /, abs, max, min, sqrt and the windows: the same bits on every CPU.  The PSNRs pass through a logarithm and the
# Gaussian taps through exp, whose last bit depends on the math library.
BITWISE = ("l1", "mse", "ssim_box", "ssim_box_masked")


@pytest.fixture(scope="module")
def fx():
    return load("metrics")


def rows(fx, i):
    return slice(int(fx["first"][i]), int(fx["first"][i + 1]))


def test_fixture_lists_every_case(fx):
    assert len(MR.CASES) == len(MR.SIZES) * 2 * len(MR.STRATA) + len(MR.EXTRAS) == 88
    assert fx["names"].tolist() == [MR.case_name(i) for i in range(len(MR.CASES))]
    assert fx["f64"].dtype == np.float64 and fx["f32"].dtype == np.float32 and fx["f64"].shape == fx["f32"].shape
    assert fx["f64"].shape == (int(fx["first"][-1]), len(MR.METRICS)) and fx["probe"].shape == (88, 4)
    for i, (H, W, B, what) in enumerate(MR.CASES):
        assert fx["first"][i + 1] - fx["first"][i] == B
        # the Gaussian arm is absent exactly where the size does not allow it
        assert np.isnan(fx["f64"][rows(fx, i), 6]).all() == (min(H, W) < 11), MR.case_name(i)
        assert not np.isnan(fx["f64"][rows(fx, i), :6]).any()


@pytest.mark.parametrize("i", range(len(MR.CASES)))
def test_restatement_replays_the_fixture(fx, i):
    c = MR.make_case(i)
    assert np.array_equal(MR.probe(c), fx["probe"][i]), "the seeded inputs differ from the generator's"
    f32, f64 = MR.evaluate(c, np.float32), MR.evaluate(c, np.float64)
    assert f32.dtype == np.float32 and f64.dtype == np.float64
    want32, want64 = fx["f32"][rows(fx, i)], fx["f64"][rows(fx, i)]
    for j, name in enumerate(MR.METRICS):
        floor = MR.FLOOR_DB if name in MR.DB else MR.FLOOR
        for b in range(f32.shape[0]):
            if name in BITWISE:
                assert f32[b, j].tobytes() == want32[b, j].tobytes(), (name, b)
            else:
                assert MR.gap(name, f32[b, j], want32[b, j]) <= floor, (name, b)
            assert MR.gap(name, f64[b, j], want64[b, j]) <= 1e-12, (name, b)


def value(fx, what, name, size=MR.EXTRA_SIZE, B=1):
    i = MR.CASES.index((size[0], size[1], B, what))
    return fx["f64"][rows(fx, i), MR.METRICS.index(name)]


def test_edge_cases_by_value(fx):
    inf = math.inf
    for kind in ("f64", "f32"):
        v = lambda what, name, **kw: value({**fx, "f64": fx[kind]}, what, name, **kw)   # noqa: E731
        # identical images: no error, both PSNRs infinite, every SSIM exactly 1
        for what in ("identical", "flat"):
            assert v(what, "l1") == 0 and v(what, "mse") == 0 and v(what, "psnr") == inf and v(what, "psnr_masked") == inf
            assert v(what, "ssim_box") == 1 and v(what, "ssim_gauss") == 1
            n = np.dtype(kind.replace("f", "float")).type(3 * 37 * 53)       # calculate_ssim divides by sum(mask) + 1e-8
            assert v(what, "ssim_box_masked") == n / (n + n.dtype.type(1e-8))
        for H, W in MR.SIZES:
            for B in (1, 3):
                # an empty mask: dycheck's PSNR is +inf, its SSIM exactly 1, calculate_ssim 0; the unmasked ones do not care
                assert (v("empty", "psnr_masked", size=(H, W), B=B) == inf).all()
                assert (v("empty", "ssim_box_masked", size=(H, W), B=B) == 0).all()
                if min(H, W) >= 11:
                    assert (v("empty", "ssim_gauss", size=(H, W), B=B) == 1).all()
                for name in ("l1", "mse", "psnr", "ssim_box"):
                    assert np.array_equal(v("empty", name, size=(H, W), B=B) > 0, np.ones(B, bool))
                # all ones is no mask
                a, b = MR.CASES.index((H, W, B, "absent")), MR.CASES.index((H, W, B, "ones"))
                assert MR.make_case(a)["mask"] is None and MR.make_case(b)["mask"].min() == 1
    # the two are the same statement on different draws: compare on one draw
    c = MR.make_case(MR.CASES.index((37, 53, 3, "ones")))
    with_ones = MR.image_metrics(c["pred"], c["gt"], c["mask"], data_range=2.0)
    without = MR.image_metrics(c["pred"], c["gt"], None, data_range=2.0)
    for name in MR.METRICS:
        assert np.array_equal(with_ones[name], without[name]), name
    # psnr and psnr_masked agree without a mask (two ways to write one number); data_range moves the SSIMs only
    assert np.allclose(without["psnr"], without["psnr_masked"], rtol=0, atol=1e-9)
    r1 = MR.image_metrics(c["pred"], c["gt"], None, data_range=1.0)
    assert np.array_equal(r1["mse"], without["mse"]) and (r1["ssim_box"] < without["ssim_box"]).all()
    assert (r1["ssim_gauss"] < without["ssim_gauss"]).all()


def test_clamp_and_quantize_cases():
    c = MR.make_case(MR.CASES.index((37, 53, 1, "clamp")))
    assert c["clamp"] and c["pred"].min() < 0 and c["pred"].max() > 1 and c["gt"].min() < 0 and c["gt"].max() > 1
    got = MR.image_metrics(c["pred"], c["gt"], c["mask"], data_range=1.0, clamp=True)
    by_hand = MR.image_metrics(np.clip(c["pred"], 0, 1), np.clip(c["gt"], 0, 1), c["mask"], data_range=1.0)
    raw = MR.image_metrics(c["pred"], c["gt"], c["mask"], data_range=1.0)
    for name in MR.METRICS:
        assert np.array_equal(got[name], by_hand[name]), name
    assert raw["mse"] > got["mse"]
    c = MR.make_case(MR.CASES.index((37, 53, 1, "quantize")))
    assert c["quantize"] and c["pred"].min() < 0 and c["pred"].max() > 1
    q = MR.quantize8(c["pred"])
    as_png = (np.clip(c["pred"], 0, 1) * 255).astype("uint8")                # what eval.py:162 writes
    assert q.dtype == np.float32 and np.array_equal(q, np.float32(as_png) / 255) and len(np.unique(as_png)) > 200
    assert np.array_equal(np.round(q * 255), as_png) and np.array_equal(MR.quantize8(q), q)
    got = MR.image_metrics(c["pred"], c["gt"], None, data_range=1.0, quantize=True)
    by_hand = MR.image_metrics(q, c["gt"], None, data_range=1.0)
    for name in MR.METRICS:
        assert np.array_equal(got[name], by_hand[name]), name


@pytest.mark.parametrize("stratum", ["ones", "random60", "hole", "stripes", "single"])
def test_bruteforce_windows_agree_with_the_scipy_route(stratum):
    """Both arms on (12, 27): proves the `reflect` and `valid` indexing of the restatement itself."""
    i = MR.CASES.index((12, 27, 1, stratum))
    c = MR.make_case(i)
    a, b, m = c["pred"][0, 1].astype(np.float64), c["gt"][0, 1].astype(np.float64), c["mask"][0].astype(np.float64)
    box, box_bf = MR.ssim_box_map(a, b, 2.0, np.float64), MR.ssim_box_map_bruteforce(a, b, 2.0)
    assert box.shape == box_bf.shape == (12, 27) and np.abs(box - box_bf).max() <= 1e-11
    gauss, gauss_bf = MR.ssim_gauss_map(a, b, m, 1.0, np.float64), MR.ssim_gauss_map_bruteforce(a, b, m, 1.0)
    assert gauss.shape == gauss_bf.shape == (2, 17) and np.abs(gauss - gauss_bf).max() <= 1e-11
    if stratum == "stripes":        # columns 0 .. 11 are masked out: the windows that start in columns 0 and 1 see no pixel
        assert (gauss[:, :2] == 1).all() and not (gauss[:, 2:] == 1).any()


def test_tolerance_rule(fx):
    gaps = MR.reference_gaps(fx)
    assert set(gaps) == set(MR.METRICS) and all(math.isfinite(g) for g in gaps.values())
    for name in MR.METRICS:
        floor = MR.FLOOR_DB if name in MR.DB else MR.FLOOR
        assert MR.tolerance(name, gaps) == max(3 * gaps[name], floor)
    # the fp32 windows' error on E[x^2] - mu^2 is what sets the SSIM tolerances; the error sums sit at the floor
    assert gaps["ssim_gauss"] > MR.FLOOR and gaps["ssim_box"] > MR.FLOOR and gaps["l1"] < MR.FLOOR and gaps["mse"] < MR.FLOOR
    assert MR.gap("psnr", math.inf, math.inf) == 0 and MR.gap("ssim_gauss", math.nan, math.nan) == 0
    assert MR.gap("psnr", 30.0, math.inf) == math.inf and MR.gap("l1", 1.0, math.nan) == math.inf


def test_aligned_test_pose():
    from mobgs_amd.metrics import aligned_test_pose
    g = torch.Generator().manual_seed(3)

    def pose():
        q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
        m = torch.eye(4, dtype=torch.float64)
        m[:3, :3] = q
        m[3, :3] = torch.randn(3, generator=g, dtype=torch.float64)          # world_view_transform: translation in the last row
        return m

    a, b, c = pose(), pose(), pose()
    want = b @ torch.inverse(a) @ c
    assert torch.allclose(aligned_test_pose(a, b, c), want, rtol=0, atol=1e-14)
    got = aligned_test_pose(a.float(), b.float(), c.float())
    assert got.dtype == torch.float32 and float((got.double() - want).abs().max()) <= 1e-5
    assert torch.allclose(aligned_test_pose(a, b, a), b, rtol=0, atol=1e-14)      # an unchanged training pose moves nothing
    batched = aligned_test_pose(torch.stack([a, c]), torch.stack([b, b]), torch.stack([c, a]))
    assert torch.allclose(batched[0], want, rtol=0, atol=1e-14) and batched.shape == (2, 4, 4)


def test_abi_entries_size_query_and_refusals():
    from mobgs_amd import _lib, build
    assert "metrics.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["metrics.hip"]
    h = _lib.load()
    assert _lib.ABI_VERSION == 16 == h.mobgs_abi_version()
    for name in ("mobgs_image_metrics_scratch_doubles", "mobgs_image_metrics"):
        assert name in _lib._SIGS and hasattr(h, name)
    D = _lib._DEFINES
    assert (D["MOBGS_METRICS_BOX"], D["MOBGS_METRICS_GAUSS"], D["MOBGS_METRICS_CLAMP"], D["MOBGS_METRICS_QUANTIZE"],
            D["MOBGS_METRICS_COLUMNS"]) == (1, 2, 1, 2, 9)
    assert _lib._SIGS["mobgs_image_metrics"][1][8] is ctypes.c_double
    # the size query: a host computation, linear in B, monotone in H and W, 0 outside the range
    q = h.mobgs_image_metrics_scratch_doubles
    assert q(1, 7, 7) == 9 and q(3, 7, 7) == 27 and q(1, 16, 64) == 9 and q(1, 17, 65) == 36
    assert q(24, 288, 512) == 24 * q(1, 288, 512) and q(1, 1014, 1352) >= q(1, 288, 512) > 0
    assert [q(0, 8, 8), q(1, 0, 8), q(1, 8, -1), q(1 << 15, 8, 8), q(1, (1 << 15) + 1, 8)] == [0] * 5
    none = ctypes.c_void_p(None)
    buf = (ctypes.c_double * 64)()                     # host memory: every call below is refused before any launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 2)

    def call(B=1, H=16, W=16, pred=p, gt=p, mask=none, arms=3, flags=0, data_range=1.0, partial=p, out=p):
        return h.mobgs_image_metrics(B, H, W, pred, gt, mask, arms, flags, data_range, partial, out, none)

    refused = [dict(H=6, W=6), dict(H=6, W=20, arms=1), dict(H=20, W=6, arms=1), dict(H=10, W=10), dict(H=10, W=20, arms=2),
               dict(H=20, W=10, arms=2), dict(B=0), dict(B=-1), dict(H=0), dict(W=1 << 16), dict(arms=0), dict(arms=4),
               dict(flags=4), dict(data_range=0.0), dict(data_range=-1.0), dict(data_range=math.nan),
               dict(data_range=math.inf), dict(pred=none), dict(gt=none), dict(partial=none), dict(out=none),
               dict(pred=odd), dict(mask=odd), dict(partial=ctypes.c_void_p(p.value + 4))]
    for kw in refused:
        assert call(**kw) == D["MOBGS_E_INVALID"] == -1, kw
        assert b"mobgs_image_metrics:" in h.mobgs_last_error(), kw
    assert b"box" in (call(H=6, W=6), h.mobgs_last_error())[1] and b"Gaussian" in (call(H=10, W=10), h.mobgs_last_error())[1]


def test_public_names_and_refusal_of_host_tensors():
    from mobgs_amd import metrics as M
    a = torch.rand(2, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.image_metrics(a, a.clone(), data_range=2.0)
    with pytest.raises(TypeError):
        M.image_metrics(a, a.clone())                   # data_range is required
    hwc = torch.rand(16, 16, 3)
    for fn, args, kw in ((M.compute_psnr, (hwc, hwc), {}), (M.compute_ssim, (hwc, hwc), {}),
                         (M.calculate_psnr, (hwc, hwc, torch.ones(16, 16)), {}),
                         (M.calculate_ssim, (hwc, hwc, torch.ones(16, 16)), {"data_range": 2.0}),
                         (M.peak_signal_noise_ratio, (hwc, hwc), {"data_range": 1.0}),
                         (M.structural_similarity, (hwc, hwc), {"data_range": 2.0})):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(*args, **kw)
    for fn in (M.image_metrics, M.calculate_ssim, M.peak_signal_noise_ratio, M.structural_similarity):
        par = inspect.signature(fn).parameters["data_range"]                 # a required keyword: no silent R = 1
        assert par.kind is par.KEYWORD_ONLY and par.default is par.empty, fn.__name__
    par = inspect.signature(M.evaluate_views).parameters
    assert par["ssim_data_range"].default == 2.0 and par["stage"].default == "fine"
    par = inspect.signature(M.image_metrics).parameters
    assert [par[k].default for k in ("mask", "clamp", "quantize")] == [None, False, False]
    assert M.ImageMetrics._fields[:7] == MR.METRICS
    assert callable(M.aligned_test_pose)


def external(name):
    path = os.path.join(GOLDEN, "metrics_external", name + ".npz")
    if not os.path.exists(path):
        pytest.skip(f"no tests/golden/metrics_external/{name}.npz (run scripts/dump_metric_vectors.py where scikit-image "
                    "and jax are installed): the data range of metrics.py's SSIM call stays UNPINNED")
    return dict(np.load(path))


def test_restatement_against_scikit_image_vectors():
    """Present only after scripts/dump_metric_vectors.py ran elsewhere: pins R = 2 and the box arm to scikit-image itself."""
    ex = external("skimage")
    for n, i in enumerate(ex["case"].tolist()):
        c = MR.make_case(i)
        assert np.array_equal(MR.probe(c), ex["probe"][n])
        for r, key in ((1.0, "ssim_r1"), (2.0, "ssim_r2"), (2.0, "ssim_default")):
            got = MR.image_metrics(c["pred"], c["gt"], None, data_range=r, clamp=c["clamp"], quantize=c["quantize"],
                                   arms=("box",))
            assert MR.gap("ssim_box", got["ssim_box"][0], ex[key][n]) <= 1e-9, (MR.case_name(i), key)
        # peak_signal_noise_ratio without a data_range: 1 for a float image_true that is not negative, else 2
        r = 1.0 if MR.prepare(c["pred"], c["gt"], c["clamp"], c["quantize"])[1].min() >= 0 else 2.0
        assert MR.gap("psnr", got["psnr"][0] + 20 * math.log10(r), ex["psnr_default"][n]) <= 1e-9, MR.case_name(i)


def test_restatement_against_dycheck_vectors():
    ex = external("dycheck")
    gaps = MR.reference_gaps(load("metrics"))
    for n, i in enumerate(ex["case"].tolist()):
        c = MR.make_case(i)
        assert np.array_equal(MR.probe(c), ex["probe"][n])
        got = MR.image_metrics(c["pred"], c["gt"], c["mask"], data_range=c["data_range"], clamp=c["clamp"],
                               quantize=c["quantize"], arms=("gauss",))
        assert MR.gap("ssim_gauss", ex["ssim"][n], got["ssim_gauss"][0]) <= MR.tolerance("ssim_gauss", gaps), MR.case_name(i)
        assert MR.gap("psnr_masked", ex["psnr"][n], got["psnr_masked"][0]) <= MR.tolerance("psnr_masked", gaps), MR.case_name(i)
