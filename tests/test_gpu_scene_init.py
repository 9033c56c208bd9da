"""Scene initialisation on the GPU: the exact 3-NN kernel (csrc/knn.hip) against a float64 brute force, and
TrainableGaussians.from_pcd / from_pcd_dynamic against the state the reference's create_from_pcd* left for the same
cloud (tests/golden/init.npz, make_golden_init.py).

Bound of the 3-NN result: relative 2^-20, derived.  One fp32 squared distance is three subtractions, three products
and two sums, each within 2^-24 relative (the sums are of non-negative terms), so within 8 x 2^-24 = 2^-21 of the
exact value; choosing among near-ties by the fp32 value instead of the exact one moves the chosen value by no more
than that again.  The mean of three such values and the division by 3 add 3 x 2^-24.  Together below 2^-20.

Times: scripts/knn_timing.py and test_timing_beats_cdist_topk (docs/MEASUREMENT_LOG.md)."""
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

from helpers import load

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 2.0 ** -20
N = 20000


def brute_force(points, chunk=2000):
    """float64, chunked: mean of the three smallest |p_i - p_j|^2 over j != i."""
    p = points.double()
    out = torch.empty(p.shape[0], dtype=torch.float64, device=p.device)
    for a in range(0, p.shape[0], chunk):
        b = min(a + chunk, p.shape[0])
        d = ((p[a:b, None, :] - p[None, :, :]) ** 2).sum(-1)
        d[torch.arange(b - a, device=p.device), torch.arange(a, b, device=p.device)] = float("inf")
        out[a:b] = d.topk(3, dim=1, largest=False).values.sum(1) / 3.0
    return out


def clouds():
    g = torch.Generator().manual_seed(41)
    uniform = torch.rand(N, 3, generator=g) * 4.0 - 2.0
    centres = torch.randn(40, 3, generator=g) * 3.0
    widths = 10.0 ** (-3.0 * torch.rand(40, 1, generator=g))
    which = torch.randint(0, 40, (N,), generator=g)
    clustered = centres[which] + widths[which] * torch.randn(N, 3, generator=g)
    dup = torch.rand(N, 3, generator=g)
    k = N // 20
    src = torch.randint(k, N, (k,), generator=g)
    dup[:k] = dup[src].clone()           # 5 % exact duplicates of other rows
    dup[k:k + 8] = dup[k + 8].clone()    # and one point nine times: all three neighbours at distance 0
    dup = dup[torch.randperm(N, generator=g)]
    t = torch.rand(N, 1, generator=g)
    line = torch.tensor([0.3, -1.2, 2.0]) + t * torch.tensor([1.0, 2.0, -0.5])   # all points on one line
    return {"uniform": uniform, "clustered": clustered, "duplicates": dup, "line": line}


@pytest.mark.parametrize("name", ["uniform", "clustered", "duplicates", "line"])
def test_knn3_against_float64_brute_force(hip_device, name):
    from mobgs_amd.scene_init import knn3_mean_dist2, knn3_sorted
    pts = clouds()[name].to(hip_device)
    ref = brute_force(pts)
    got = knn3_mean_dist2(pts)
    assert got.dtype == torch.float32 and got.shape == (N,)
    err = (got.double() - ref).abs()
    rel = float((err / ref.clamp_min(1e-300)).max())
    print(f"{name}: max relative error {rel:.3e} (allowed {REL:.3e}); zeros {int((ref == 0).sum())}")
    assert bool((err <= REL * ref).all()), rel
    assert torch.equal(got == 0, ref == 0)   # duplicates give exactly 0, nothing else does
    if name == "duplicates":
        assert int((ref == 0).sum()) >= 9
    # the kernel is exact for ANY row order: unsorted rows prune badly, and give the same bits
    assert torch.equal(knn3_sorted(pts), got)


@pytest.mark.parametrize("name", ["uniform", "clustered", "duplicates", "line"])
def test_knn3_permutation_invariance_and_repeatability(hip_device, name):
    from mobgs_amd.scene_init import knn3_mean_dist2
    pts = clouds()[name].to(hip_device)
    a = knn3_mean_dist2(pts)
    assert torch.equal(knn3_mean_dist2(pts), a)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(8)).to(hip_device)
    assert torch.equal(knn3_mean_dist2(pts[perm]), a[perm])
    # a size that fills neither the last wave nor the last box
    m = 64 * 137 + 21
    b = knn3_mean_dist2(pts[:m])
    assert torch.equal(knn3_mean_dist2(pts[:m].flip(0)), b.flip(0))
    ref = brute_force(pts[:m])
    assert bool(((b.double() - ref).abs() <= REL * ref).all())


def test_knn3_small_sizes(hip_device):
    from mobgs_amd.scene_init import knn3_mean_dist2
    from mobgs_amd.simple_knn._C import distCUDA2
    g = torch.Generator().manual_seed(2)
    for n in (4, 5, 63, 64, 65, 257):
        pts = torch.randn(n, 3, generator=g).to(hip_device)
        ref = brute_force(pts)
        got = distCUDA2(pts)
        assert bool(((got.double() - ref).abs() <= REL * ref).all()), n
    with pytest.raises(RuntimeError, match="mobgs_knn3_mean_dist2.*three neighbours"):
        knn3_mean_dist2(torch.randn(3, 3, generator=g).to(hip_device))
    with pytest.raises(RuntimeError, match="HIP device"):
        knn3_mean_dist2(torch.randn(8, 3, generator=g))


# ---- from_pcd / from_pcd_dynamic against the reference's state -------------------------------------------------------
CLOSED_FORM = {"_xyz": "xyz", "_rotation": "rotation", "_opacity": "opacity", "_features_dc": "f_dc",
               "_features_rest": "f_rest", "_features_t": "f_t", "_omega": "omega", "_zeta": "zeta", "_motion": "motion",
               "_trbf_center": "trbf_center", "_trbf_scale": "trbf_scale", "current_control_num": "current_control_num",
               "max_radii2D": "max_radii2D", "_deformation_table": "_deformation_table"}


def _pcd(fx):
    return types.SimpleNamespace(points=fx["points"], colors=fx["colors"], times=fx["times"])


def _check_state(pc, fx, tag):
    st = pc.table_state()
    for ref_name, field in CLOSED_FORM.items():
        ref = torch.from_numpy(fx[f"{tag}.{ref_name}"])
        got = st[field].cpu()
        assert got.shape == ref.shape and got.dtype == ref.dtype, (tag, ref_name, got.shape, ref.shape, got.dtype)
        assert torch.equal(got, ref), (tag, ref_name)
    # scaling = log(sqrt(dist2)) = ln(dist2) / 2: a relative 2^-20 in dist2 is an absolute 2^-21 (4.8e-7) here, plus one
    # ulp of the value for the two roundings of sqrt and log on either side
    ref = torch.from_numpy(fx[f"{tag}._scaling"])
    got = st["scaling"].cpu()
    assert got.shape == ref.shape
    err = (got - ref).abs()
    ulp = torch.abs(torch.nextafter(ref, torch.full_like(ref, float("inf"))) - ref)
    print(f"{tag} scaling: max |diff| {float(err.max()):.3e}, worst {float((err / (5e-7 + ulp)).max()):.3f} of the bound")
    assert bool((err <= 5e-7 + ulp).all())
    assert pc.spatial_lr_scale == float(fx["spatial_lr_scale"])


def test_from_pcd_matches_reference_state(hip_device):
    from mobgs_amd.densify import TrainableGaussians
    fx = load("init")
    pc = TrainableGaussians.from_pcd(_pcd(fx), 5.0, 0, device=hip_device, spatial_sort=False)
    _check_state(pc, fx, "static")
    # documented deviation: the reference's random control_xyz (:527) is not reproduced; GaussianParams' default stands
    assert torch.equal(pc.control_xyz.detach(), (pc._xyz.detach() * 100.0)[:, None, :].repeat(1, 12, 1))
    assert pc.pcd_order is None and pc.rows_coherent == -1 and not pc.is_dynamic
    pc2 = TrainableGaussians.from_pcd(_pcd(fx), 5.0, trbfslinit=0.25, sh_degree=1, device=hip_device, spatial_sort=False)
    assert float(pc2._trbf_scale.min()) == 0.25 == float(pc2._trbf_scale.max()) and pc2._features_rest.shape[1:] == (4, 3)


def test_from_pcd_dynamic_matches_reference_state(hip_device):
    from mobgs_amd.densify import TrainableGaussians
    fx = load("init")
    pc = TrainableGaussians.from_pcd_dynamic(_pcd(fx), 5.0, 0, torch.from_numpy(fx["traj"]), device=hip_device,
                                             spatial_sort=False)
    _check_state(pc, fx, "dynamic")
    # control points: the CPU test's tolerance (3 x the reference's own fp32 / float64 gap, per row and absolute)
    c64 = torch.from_numpy(fx["control_f64"])

    def gaps(c):
        err = (c.double() - c64).abs().reshape(c64.shape[0], -1).max(1).values
        return float(err.max()), float((err / c64.abs().reshape(c64.shape[0], -1).max(1).values).max())
    floor_abs, floor_rel = gaps(torch.from_numpy(fx["dynamic.control_xyz"]))
    got_abs, got_rel = gaps(pc.control_xyz.detach().cpu())
    print(f"control points vs float64: reference {floor_abs:.3e} / {floor_rel:.3e}, here {got_abs:.3e} / {got_rel:.3e}")
    assert pc.control_xyz.dtype == torch.float32 and got_abs <= 3 * floor_abs and got_rel <= 3 * floor_rel
    assert pc.is_dynamic


def test_spatial_sort_is_a_row_permutation(hip_device):
    from mobgs_amd.densify import TrainableGaussians
    fx = load("init")
    traj = torch.from_numpy(fx["traj"])
    for make in (lambda **k: TrainableGaussians.from_pcd(_pcd(fx), 5.0, device=hip_device, **k),
                 lambda **k: TrainableGaussians.from_pcd_dynamic(_pcd(fx), 5.0, 0, traj, device=hip_device, **k)):
        plain, srt = make(spatial_sort=False), make()
        order = srt.pcd_order
        assert srt.rows_coherent == order.numel() == plain.get_xyz.shape[0]
        assert torch.equal(torch.sort(order).values, torch.arange(order.numel(), device=order.device))
        a, b = plain.table_state(), srt.table_state()
        for k in a:
            assert torch.equal(a[k][order], b[k]), k


def test_models_from_the_fixture_cloud_render(hip_device):
    """End to end: both sets built from the fixture cloud go through one render(); the frame is finite, and the dynamic
    means the renderer's spline evaluator gives at every sample time lie within the fit residual of the trajectory."""
    from mobgs_amd.camera import PinholeCamera
    from mobgs_amd.densify import TrainableGaussians
    from mobgs_amd.gaussian_renderer import interpolate_cubic_hermite, render
    from mobgs_amd.synth import SynthCamera
    from oracle.render_torch import hermite
    fx = load("init")
    traj = torch.from_numpy(fx["traj"])
    stat = TrainableGaussians.from_pcd(_pcd(fx), 5.0, device=hip_device)
    dyn = TrainableGaussians.from_pcd_dynamic(_pcd(fx), 5.0, 0, traj, device=hip_device, spatial_sort=False)
    W, H = 160, 112
    scam = SynthCamera().scaled(W, H)
    w2c = torch.eye(4)
    w2c[2, 3] = 9.0
    cam = PinholeCamera(W, H, scam.K, w2c, 0.4, scam.max_time, device=hip_device)
    out = render(cam, stat, dyn, None, torch.zeros(9, device=hip_device))
    img = out["render"]
    assert img.shape[-2:] == (H, W) and bool(torch.isfinite(img).all()) and bool(torch.isfinite(out["depth"]).all())
    assert float(img.max()) > float(img.min())
    # the fit: residual of the float64 least-squares solution per point (CPU oracle's evaluator), and what the product
    # path's own evaluator makes of the fitted control points
    n = traj.shape[0]
    c64 = torch.from_numpy(fx["control_f64"])
    ncp = torch.full((n, 1), 12, dtype=torch.int64)
    target = traj.double() * 1e2
    ctrl = dyn.control_xyz.detach()
    scale_row = c64.abs().reshape(n, -1).max(1).values
    worst = 0.0
    for k, t in enumerate(torch.from_numpy(fx["t_step"])):
        floor = (hermite(c64, t.double(), ncp) - target[:, k]).norm(dim=1)
        times = t.to(hip_device)[None, None, None].expand(n, 3, 1)
        got = interpolate_cubic_hermite(ctrl.permute(0, 2, 1), times, dyn.current_control_num).detach().cpu().double()
        dev = (got - target[:, k]).norm(dim=1)
        # slack: the fp32 evaluation and the fp32 control points, ~16 roundings at the row's own scale (2^-20 relative),
        # doubled for the norm over three axes
        slack = 2.0 ** -19 * scale_row
        worst = max(worst, float(((dev - floor) / slack).max()))
        assert bool((dev <= floor + slack).all()), (k, float((dev - floor - slack).max()))
    print(f"dynamic means vs trajectory: worst excess over the fit residual {worst:.3f} of the rounding slack")


# ---- timing ------------------------------------------------------------------------------------------------------------
def _timing_module():
    spec = importlib.util.spec_from_file_location("knn_timing", os.path.join(ROOT, "scripts", "knn_timing.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_timing_beats_cdist_topk(hip_device):
    """HIP events after warm-up, median of 20 runs (the alternative: median of 3 -- one run of it takes seconds, so 20
    would cost the suite a minute, and the clock's noise is invisible at that length).  100 k, 300 k and 1 M points,
    uniform and clustered, are timed and printed (-s).  Asserted, one thing only: at 300 k points the whole
    knn3_mean_dist2 (Morton sort + kernel + scatter) is faster than a chunked torch.cdist + topk(3) in the same
    process on the same cloud.  No ratio is fixed in advance.
    Times on an MI355X: not measured yet (docs/MEASUREMENT_LOG.md, last section)."""
    T = _timing_module()
    for n in (100000, 300000, 1000000):
        for clustered in (False, True):
            rec = T.measure(n, clustered, runs=20, warmup=3, alt_runs=3 if (n == 300000 and not clustered) else 0)
            print(rec)
            if "cdist_topk" in rec:
                assert rec["knn3_mean_dist2"]["median_ms"] < rec["cdist_topk"]["median_ms"], rec
