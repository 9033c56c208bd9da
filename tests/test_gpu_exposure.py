"""Exposure-time estimation on the MI355X: the selection kernels (csrc/exposure.hip) through the C ABI and
loss_utils.exposure_ratio against the fp32 restatement (bit-equal) and the reference's fixture, the one-pass pair render
against two get_flow_static calls, blceKernel.estimate_exposure_time against the old composition, and the example."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import exposure_restatement as ER
from helpers import load

pytestmark = pytest.mark.gpu

GRID_TIMES_BLOCK = 1024 * 256          # csrc/exposure.hip EXPO_MAX_GRID x EXPO_BLOCK: beyond it, a second grid-stride trip
SIZES = [1, 2, 3, 63, 64, 65, 100, 101, 151, 255, 256, 257, 1024, 4097, GRID_TIMES_BLOCK + 131]
SENTINEL = -7.25


def _poison(dev, mb=64):
    """Fill free blocks of the caching allocator with 0xFF bytes: whatever a kernel reads without having written it shows
    as NaN in a float array and as -1 in the int32 control words and histogram tables."""
    t = torch.full((mb * 1024 * 1024,), 255, dtype=torch.uint8, device=dev)
    del t


def run_abi(cam, lat, q, scale, dev, scratch=None):
    """mobgs_exposure_estimate itself -> (slot value, stats list, scratch)."""
    from mobgs_amd import _lib
    from mobgs_amd._lib import check, ptr, stream
    h = _lib.load()
    cam_d, lat_d = cam.to(dev).contiguous(), lat.to(dev).contiguous()
    n = cam_d.numel() // 2
    slot = torch.full((1,), SENTINEL, dtype=torch.float32, device=dev)
    stats = torch.full((4,), -1, dtype=torch.int32, device=dev)
    if scratch is None:
        scratch = torch.empty(h.mobgs_exposure_scratch_bytes(n), dtype=torch.uint8, device=dev)
    check(h.mobgs_exposure_estimate(n, ptr(cam_d), ptr(lat_d), q, scale, ptr(slot), ptr(stats), ptr(scratch), stream()),
          "mobgs_exposure_estimate")
    torch.cuda.synchronize()
    for after, before in ((cam_d, cam), (lat_d, lat)):        # the inputs are only read (by bits: a NaN equals itself)
        assert torch.equal(after.cpu().view(torch.int32), before.contiguous().view(torch.int32))
    return slot.cpu()[0], stats.cpu().tolist(), scratch


def check_exact(cam, lat, q, scale, dev, what):
    want = ER.estimate(cam, lat, q, scale)
    value, stats, _ = run_abi(cam, lat, q, scale, dev)
    print(f"{what}: n_valid {stats[0]} (restated {want['n_valid']}), value {float(value)!r} "
          f"(restated {None if want['value'] is None else float(want['value'])!r})")
    assert stats[0] == want["n_valid"] and stats[1] == 0 and stats[2] == want["updated"] and stats[3] == 0, what
    if want["updated"]:
        assert value.view(torch.int32) == want["value"].view(torch.int32), what      # bit-equal
    else:
        assert float(value) == SENTINEL, what
    return want


@pytest.mark.parametrize("n", SIZES)
def test_exact_selection(n, hip_device):
    parities = set()
    for seed, ties in ((0, True), (1, False), (4, True)):
        cam, lat = ER.exact_case(n, seed, ties)
        for scale in (1.0, 0.5):
            want = check_exact(cam, lat, 0.01, scale, hip_device, f"n {n} seed {seed} scale {scale}")
        parities.add(want["n_valid"] % 2)
    if n in (1024, 4097):
        assert parities == {0, 1}, "an even and an odd n_valid are wanted among the cases of this size"
    g = torch.Generator().manual_seed(n)            # inexact arithmetic too: both sides round every operation alike
    check_exact(torch.randn(n, 2, generator=g) * 3, torch.randn(n, 2, generator=g), 0.01, 1.0, hip_device, f"n {n} random")


def test_interpolation_branches_and_other_quantiles(hip_device):
    for n, tail in ((151, 2), (64, 1), (1024, 11), (3, 1)):
        cam, lat = ER.exact_case(n, 2, True, tail=tail)
        want = check_exact(cam, lat, 0.01, 1.0, hip_device, f"lerp n {n}")
        assert 5.0 < float(want["threshold"]) < 10.0 and want["n_valid"] == n - tail
    cam, lat = ER.exact_case(4097, 5, False)
    for q in (0.0, 0.25, 0.37, 0.5, 0.999, 1.0):
        check_exact(cam, lat, q, 1.0, hip_device, f"q {q}")


def test_no_update_cases(hip_device):
    for n in (1, 7, 300):
        cam = torch.tensor([[3.0, 4.0]] * n)
        value, stats, _ = run_abi(cam, cam * 0.5, 0.01, 1.0, hip_device)
        assert float(value) == SENTINEL and stats[0] == 0 and stats[2] == 0, n
    cam, lat = ER.exact_case(1000, 3)
    for bad in (float("nan"), float("inf"), float("-inf")):
        for which in (0, 1):
            maps = [cam.clone(), lat.clone()]
            maps[which][617, 1] = bad
            value, stats, _ = run_abi(maps[0], maps[1], 0.01, 1.0, hip_device)
            assert float(value) == SENTINEL and stats[1] == 1 and stats[2] == 0, (bad, which)
    big = torch.tensor([[3e19, 4e19]] * 9 + [[3.0, 4.0]] * 91)      # finite flow whose squared magnitude overflows
    value, stats, _ = run_abi(big, cam[:100], 0.01, 1.0, hip_device)
    assert float(value) == SENTINEL and stats[1] == 9 and stats[2] == 0


def test_scratch_reuse_and_poisoned_allocator(hip_device):
    cam, lat = ER.exact_case(4097, 6)
    other = ER.exact_case(4097, 7, False)
    clean, stats, scratch = run_abi(cam, lat, 0.01, 1.0, hip_device)
    run_abi(other[0], other[1], 0.37, 1.0, hip_device, scratch=scratch)         # leaves its tables and prefixes behind
    again, stats2, _ = run_abi(cam, lat, 0.01, 1.0, hip_device, scratch=scratch)
    assert again.view(torch.int32) == clean.view(torch.int32) and stats2 == stats
    del scratch
    torch.cuda.empty_cache()
    _poison(hip_device)
    poisoned, stats3, _ = run_abi(cam, lat, 0.01, 1.0, hip_device)
    assert poisoned.view(torch.int32) == clean.view(torch.int32) and stats3 == stats
    assert clean.view(torch.int32) == ER.estimate(cam, lat)["value"].view(torch.int32)


def test_fixture_parity_and_wrapper(hip_device):
    from mobgs_amd.loss_utils import exposure_ratio
    fx = load("exposure")
    cam, lat = torch.from_numpy(fx["out_cam_flow"]), torch.from_numpy(fx["out_latent_flow"])
    q, f64 = float(fx["q"][0]), float(fx["f64_value"][0])
    bound = ER.fixture_bound(float(fx["ref_gap"][0]), f64)
    value, stats = exposure_ratio(cam.to(hip_device), lat.to(hip_device), q=q)
    stats = stats.cpu().tolist()
    err = abs(float(value) - f64)
    print(f"fixture: kernel {float(value)!r}, float64 {f64!r}, |diff| {err:.3e} (allowed {bound:.3e}, ref_gap "
          f"{float(fx['ref_gap'][0]):.3e}); n_valid {stats[0]}")
    assert err <= bound and stats[2] == 1 and stats[1] == 0
    assert float(value) == float(fx["restated_value"][0]) and stats[0] == int(fx["restated_n_valid"][0])
    # out=: a view into a larger tensor is written in place, its neighbours are not, the version counter moves
    table = torch.full((5,), 0.4, device=hip_device)
    v0 = table._version
    got, _ = exposure_ratio(cam.to(hip_device), lat.to(hip_device), q=q, scale=0.5, out=table[3])
    assert table._version > v0 and table.cpu().tolist() == [pytest.approx(0.4)] * 3 + [float(value) * 0.5, pytest.approx(0.4)]
    with pytest.raises(ValueError, match="one float32 element"):
        exposure_ratio(cam.to(hip_device), lat.to(hip_device), out=table)
    with pytest.raises(ValueError, match="outside"):
        exposure_ratio(cam.to(hip_device), lat.to(hip_device), q=1.5)


# ---- the pair render and the method ---------------------------------------------------------------------------------
W, H, NS, ND = 96, 64, 500, 200


@pytest.fixture(scope="module")
def scene(hip_device):
    """~500 static splats at 96 x 64 (24 tiles) and five nearby poses: previous / next view, the view, and the first /
    last camera of a short path around it."""
    from mobgs_amd.camera import PinholeCamera
    from mobgs_amd.gaussian_model import GaussianParams
    from mobgs_amd.helper_model import Sandwich
    from mobgs_amd.synth import SynthCamera, dynamic_extras, gaussian_cloud
    dev = hip_device
    scam = SynthCamera().scaled(W, H)
    torch.manual_seed(11)
    dec = Sandwich(9, 3).to(dev)
    sp, dp = gaussian_cloud(NS, scam, 11), gaussian_cloud(ND, scam, 12)
    stat = GaussianParams(sp, None, dec, dev, requires_grad=False)
    dyn = GaussianParams(dp, dynamic_extras(dp["xyz"], 11), dec, dev, requires_grad=False)

    def cam(f, uid):
        w2c = torch.eye(4)
        w2c[:3, 3] = f * torch.tensor([0.04, -0.02, 0.03])
        c = PinholeCamera(W, H, scam.K, w2c, time=scam.time, max_time=scam.max_time, device=dev)
        c.uid = uid
        c.image = torch.rand(3, H, W, generator=torch.Generator().manual_seed(uid)).to(dev)   # (BLCE's blur statistic)
        return c
    cams = {"bwd": cam(-1.0, 0), "view": cam(0.0, 1), "fwd": cam(1.0, 2), "start": cam(-0.35, 1), "end": cam(0.3, 1)}
    return stat, dyn, cams, torch.zeros(9, device=dev)


@pytest.fixture(scope="module")
def separate(scene):
    """The parent's route, computed once: two get_flow_static calls."""
    from mobgs_amd.gaussian_renderer import get_flow_static
    stat, dyn, c, bg = scene
    with torch.no_grad():
        cam_flow = get_flow_static(c["bwd"], c["fwd"], c["view"], stat, dyn, None, bg)[1]
        lat_flow = get_flow_static(c["start"], c["end"], c["view"], stat, dyn, None, bg)[1]
    return cam_flow, lat_flow


def torch_chain(cam_flow, lat_flow, q=0.01):
    """The old composition on the device: train.py:482-489 with sqrt(x x + y y) magnitudes."""
    cm = torch.sqrt(cam_flow[..., 0] * cam_flow[..., 0] + cam_flow[..., 1] * cam_flow[..., 1])
    lm = torch.sqrt(lat_flow[..., 0] * lat_flow[..., 0] + lat_flow[..., 1] * lat_flow[..., 1])
    valid = cm > torch.quantile(cm, q)
    return torch.median(lm[valid] / cm[valid])


def test_pair_render_is_the_two_separate_renders(scene, separate):
    from mobgs_amd.gaussian_renderer import get_flow_static_pair
    stat, dyn, c, bg = scene
    a, b = get_flow_static_pair(c["bwd"], c["fwd"], c["start"], c["end"], c["view"], stat, dyn, None, bg)
    assert a.shape == b.shape == (1, H, W, 2) and a.is_contiguous() and b.is_contiguous()
    da, db = float((a - separate[0]).abs().max()), float((b - separate[1]).abs().max())
    print(f"pair render: max |diff| camera flow {da:.3e}, latent flow {db:.3e}; covered pixels "
          f"{int((separate[0].abs().sum(-1) > 0).sum())} / {H * W}")
    assert float(separate[0].abs().max()) > 0.1 and float(separate[1].abs().max()) > 0.01
    assert torch.equal(a, separate[0]) and torch.equal(b, separate[1])


def test_estimate_exposure_time_end_to_end(scene, separate, hip_device):
    import types

    from mobgs_amd.blce import blceKernel
    stat, dyn, c, bg = scene
    torch.manual_seed(5)
    kernel = blceKernel(num_views=3, num_warp=9).to(hip_device)
    expo = kernel.model.exposure_time_expo
    warped = [c["start"]] + [None] * 7 + [c["end"]]      # only the first and the last latent camera are read
    old = torch_chain(*separate)
    ref_gap = float(load("exposure")["ref_gap"][0])
    v0 = expo._version
    before = expo.detach().clone()
    stats = kernel.estimate_exposure_time(c["view"], c["bwd"], c["fwd"], stat, dyn, None, bg, warped_cams=warped)
    got = expo.detach().cpu()
    bound = ER.fixture_bound(ref_gap, float(old))
    print(f"end to end: slot {float(got[1])!r}, old composition {float(old)!r}, |diff| {abs(float(got[1]) - float(old)):.3e} "
          f"(allowed {bound:.3e}); stats {stats.cpu().tolist()}")
    assert stats.cpu().tolist()[2] == 1 and stats.cpu().tolist()[1] == 0
    assert abs(float(got[1]) - float(old)) <= bound
    assert expo._version > v0
    assert torch.equal(got[[0, 2]], before.cpu()[[0, 2]])                 # the other views' entries: bit-unchanged
    full = got[1].clone()
    kernel.estimate_exposure_time(c["view"], c["bwd"], c["fwd"], stat, dyn, None, bg, edge=True, warped_cams=warped)
    assert expo.detach().cpu()[1] == full * 0.5 and torch.equal(expo.detach().cpu()[[0, 2]], before.cpu()[[0, 2]])
    # the latent cameras come from get_warped_cams when they are not handed in
    s2 = kernel.estimate_exposure_time(c["view"], c["bwd"], c["fwd"], stat, dyn, None, bg)
    assert s2.cpu().tolist()[1] == 0 and bool(torch.isfinite(expo).all())
    with pytest.raises(IndexError):
        kernel.estimate_exposure_time(types.SimpleNamespace(uid=7), c["bwd"], c["fwd"], stat, dyn, None, bg,
                                      warped_cams=warped)


def test_example_estimates_exposure(hip_device):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_deblur_synth as T
    history, stat, dyn, blce, _ = T.train(dev=str(hip_device), iters=4, ns=1500, nd=600, width=128, height=96, seed=2,
                                          estimate_exposure=2)
    expo = blce.model.exposure_time_expo.detach().cpu()
    print(f"example: exposure_time_expo {expo.tolist()}, losses {history}")
    assert len(history) == 4 and all(np.isfinite(history))
    assert bool(torch.isfinite(expo).all()) and bool((expo != 0.4).all())
