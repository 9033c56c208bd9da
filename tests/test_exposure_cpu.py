"""The exposure-time estimate without a GPU: the fixture (tests/golden/exposure.npz, make_golden_exposure.py) replayed
through the restatement, the restatement's fp32 form against torch.quantile / torch.median themselves, the C ABI's
refusals and scratch sizes, and the wrappers' refusals of host tensors."""
import ctypes

import numpy as np
import pytest
import torch

import exposure_restatement as ER
from helpers import load

SIZES = [1, 2, 3, 63, 64, 65, 100, 101, 151, 255, 256, 257, 1024, 4097, 1024 * 256 + 131]


@pytest.fixture(scope="module")
def fx():
    return load("exposure")


def test_fixture_replays_through_the_restatement(fx):
    cam, lat = torch.from_numpy(fx["out_cam_flow"]), torch.from_numpy(fx["out_latent_flow"])
    assert cam.shape == lat.shape == (1, 48, 80, 2) and cam.dtype == torch.float32
    q = float(fx["q"][0])
    # the reference's own statements give what the fixture recorded, bit for bit
    assert np.array_equal(ER.reference_chain(cam, lat, q).numpy().reshape(1), fx["ref_value"])
    assert np.array_equal(ER.reference_chain(cam, lat, q, edge=True).numpy().reshape(1), fx["ref_value_edge"])
    assert fx["ref_value_edge"][0] == np.float32(0.5) * fx["ref_value"][0]
    f64 = ER.estimate(cam, lat, q, 1.0, torch.float64)
    assert f64["value"].dtype == torch.float64 and float(f64["value"]) == fx["f64_value"][0]
    assert f64["n_valid"] == fx["f64_n_valid"][0] and float(f64["threshold"]) == fx["f64_threshold"][0]
    f32 = ER.estimate(cam, lat, q, 1.0, torch.float32)
    assert f32["value"].dtype == torch.float32 and f32["value"].numpy() == fx["restated_value"][0]
    assert f32["n_valid"] == fx["restated_n_valid"][0] and 0 < f32["n_valid"] < cam.numel() // 2
    gap = abs(float(fx["ref_value"][0]) - fx["f64_value"][0])
    assert gap == fx["ref_gap"][0]
    bound = ER.fixture_bound(gap, fx["f64_value"][0])
    assert bound == max(3 * gap, 4 * 2.0 ** -25)            # the result lies in [0.25, 0.5): 1 ulp = 2^-25
    assert abs(float(f32["value"]) - fx["f64_value"][0]) <= bound


def same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))


@pytest.mark.parametrize("n", SIZES)
def test_restatement_is_bit_equal_to_torch(n):
    g = torch.Generator().manual_seed(n)
    cases = [ER.exact_case(n, 0, True), ER.exact_case(n, 1, False),
             (torch.randn(n, 2, generator=g) * 3, torch.randn(n, 2, generator=g))]
    for cam, lat in cases:
        for q, scale in ((0.01, 1.0), (0.01, 0.5), (0.0, 1.0), (0.37, 1.0), (1.0, 1.0)):
            got = ER.estimate(cam, lat, q, scale)
            thr, n_valid, value = ER.torch_judge(cam, lat, q, scale)
            assert torch.equal(got["threshold"], thr) and got["n_valid"] == n_valid, (n, q)
            assert same(got["value"], value), (n, q, scale)
            assert got["updated"] == (1 if n_valid else 0) and got["n_nonfinite"] == 0


def test_both_interpolation_branches_with_distinct_neighbours():
    for n, tail, branch in ((151, 2, "high"), (64, 1, "high"), (1024, 11, "low"), (3, 1, "low")):
        cam, lat = ER.exact_case(n, 2, True, tail=tail)
        pos = torch.tensor(0.01) * torch.tensor(float(n - 1))
        w = float(pos - torch.floor(pos))
        assert (w < 0.5) == (branch == "low") and int(torch.floor(pos)) == tail - 1
        s = torch.sort(ER.magnitudes(cam)).values
        assert float(s[tail - 1]) == 5.0 and float(s[tail]) == 10.0
        got = ER.estimate(cam, lat, 0.01)
        assert torch.equal(got["threshold"], torch.quantile(ER.magnitudes(cam), 0.01))
        assert 5.0 < float(got["threshold"]) < 10.0 and got["n_valid"] == n - tail
    assert float(torch.tensor(0.01) * torch.tensor(150.0)) == 1.5       # n = 151: w is exactly one half


def test_no_update_cases_of_the_restatement():
    cam = torch.tensor([[3.0, 4.0]] * 7)
    assert ER.estimate(cam, cam * 0.5)["updated"] == 0 and ER.estimate(cam[:1], cam[:1])["n_valid"] == 0
    cam, lat = ER.exact_case(100, 3)
    for bad in (float("nan"), float("inf")):
        for which in (0, 1):
            maps = [cam.clone(), lat.clone()]
            maps[which][17, 1] = bad
            r = ER.estimate(*maps)
            assert r["updated"] == 0 and r["value"] is None and r["n_nonfinite"] == 1
    # ... where the reference's statements give NaN
    assert torch.isnan(ER.reference_chain(torch.tensor([[3.0, 4.0]] * 7), cam[:7]))


def test_abi_entries_refusals_and_scratch():
    from mobgs_amd import _lib, build
    assert "exposure.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["exposure.hip"]
    h = _lib.load()
    assert _lib.ABI_VERSION >= 13 and h.mobgs_abi_version() == _lib.ABI_VERSION
    for name in ("mobgs_exposure_scratch_bytes", "mobgs_exposure_estimate"):
        assert name in _lib._SIGS and hasattr(h, name)
    ns = sorted(SIZES + [512 * 288, 1352 * 1014, 1 << 30])
    sizes = [h.mobgs_exposure_scratch_bytes(n) for n in ns]
    assert all(b > a for a, b in zip(sizes, sizes[1:])) and sizes[0] >= 8        # monotone in n
    assert all(s >= 8 * n for s, n in zip(sizes, ns))                             # two 4-byte keys per pixel
    assert h.mobgs_exposure_scratch_bytes(0) == 0 and h.mobgs_exposure_scratch_bytes(-5) == 0
    assert h.mobgs_exposure_scratch_bytes((1 << 30) + 1) == 0
    none = ctypes.c_void_p(None)
    buf = (ctypes.c_float * 64)()                      # host memory: every call below is refused before any launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert h.mobgs_exposure_estimate(0, p, p, 0.01, 1.0, p, p, p, none) == -1
    assert b"mobgs_exposure_estimate" in h.mobgs_last_error()
    assert h.mobgs_exposure_estimate(-3, p, p, 0.01, 1.0, p, p, p, none) == -1
    assert h.mobgs_exposure_estimate((1 << 30) + 1, p, p, 0.01, 1.0, p, p, p, none) == -1
    for k in range(5):
        args = [p] * 5
        args[k] = none
        assert h.mobgs_exposure_estimate(8, args[0], args[1], 0.01, 1.0, args[2], args[3], args[4], none) == -1
        assert b"mobgs_exposure_estimate: NULL" in h.mobgs_last_error()
    for q in (-0.01, 1.5, float("nan"), float("inf")):
        assert h.mobgs_exposure_estimate(8, p, p, q, 1.0, p, p, p, none) == -1
        assert b"mobgs_exposure_estimate: quantile" in h.mobgs_last_error()
    odd = ctypes.c_void_p(p.value + 4)                 # a flow map that is not 8-byte aligned
    assert h.mobgs_exposure_estimate(8, odd, p, 0.01, 1.0, p, p, p, none) == -1
    assert b"aligned" in h.mobgs_last_error()


def test_wrappers_refuse_host_tensors():
    from mobgs_amd.blce import blceKernel
    from mobgs_amd.gaussian_renderer import get_flow_static_pair  # noqa: F401  (the public name exists)
    from mobgs_amd.loss_utils import exposure_ratio
    cam, lat = ER.exact_case(64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        exposure_ratio(cam, lat)
    with pytest.raises(ValueError, match=r"\[...,2\]"):
        exposure_ratio(cam.reshape(-1), lat)
    with pytest.raises(ValueError, match=r"\[...,2\]"):
        exposure_ratio(cam[:0], lat[:0])
    kernel = blceKernel(num_views=3, num_warp=9)
    view = type("Cam", (), {"uid": 1})()
    with pytest.raises(RuntimeError, match="no CPU path"):
        kernel.estimate_exposure_time(view, view, view, None, None, None, None)
