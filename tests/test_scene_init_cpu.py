"""Host side of scene initialisation (mobgs_amd.scene_init): the spline fit against the control points the reference's
own inverse_cubic_hermite produced (tests/golden/init.npz, make_golden_init.py), and the simple_knn shim.

Tolerance of the fit: it cannot be derived -- it depends on the conditioning of the design matrix -- so
the fixture carries the reference's fit twice, in fp32 (what create_from_pcd_dynamic stored) and in float64.  Their gap
is the noise floor of the reference itself; 3 x that gap is allowed.  Measured in this fixture (printed by
test_fit_matches_reference_control_points): max |fp32 - f64| = 1.30e-2 at a control-point scale of 4.0e4 (the far
outlier), 5.9e-7 relative to each row's own largest coordinate; this implementation: 2.6e-3 and 9.6e-8 (it rounds
traj * 1e2 to fp32 as the reference's fp32 call does, then solves in float64).  Both measures are asserted."""
import numpy as np
import pytest
import torch

from helpers import load

N_PTS = 12


def _gaps(c, c64):
    """(max |c - c64|, max over rows of |c - c64| / the row's own largest |c64|)."""
    err = (c.double() - c64).abs().reshape(c64.shape[0], -1).max(1).values
    own = c64.abs().reshape(c64.shape[0], -1).max(1).values
    return float(err.max()), float((err / own).max())


def _fixture():
    fx = load("init")
    T = torch.from_numpy
    return fx, T(fx["traj"]), T(fx["t_step"]), T(fx["dynamic.control_xyz"]), T(fx["control_f64"])


def _evaluate(ctrl, t_step):
    """[N,T,3] float64: the spline of `ctrl` at the sample times (the CPU oracle's evaluator; the product path's is a
    GPU kernel, used by tests/test_gpu_scene_init.py)."""
    from oracle.render_torch import hermite
    n = ctrl.shape[0]
    ncp = torch.full((n, 1), N_PTS, dtype=torch.int64)
    return torch.stack([hermite(ctrl.double(), t.double(), ncp) for t in t_step], 1)


def test_fit_matches_reference_control_points():
    from mobgs_amd.scene_init import inverse_cubic_hermite
    fx, traj, t_step, c_ref, c64 = _fixture()
    times = t_step[None, :, None].expand(traj.shape[0], -1, -1)
    assert times.stride(0) == 0
    got = inverse_cubic_hermite(traj * 1e2, times, N_pts=N_PTS)
    assert got.dtype == torch.float32 and got.shape == c_ref.shape
    floor_abs, floor_rel = _gaps(c_ref, c64)
    got_abs, got_rel = _gaps(got, c64)
    print(f"control points vs the float64 fit: reference fp32 {floor_abs:.3e} abs / {floor_rel:.3e} of the row; "
          f"this implementation {got_abs:.3e} / {got_rel:.3e}")
    assert floor_abs > 0
    assert got_abs <= 3 * floor_abs and got_rel <= 3 * floor_rel
    # against the reference's own fp32 result: both sit within their gap to the float64 solution
    ref_abs, ref_rel = _gaps(got, c_ref.double())
    assert ref_abs <= 4 * floor_abs and ref_rel <= 4 * floor_rel


def test_fit_residual_not_above_the_reference_solution():
    """A least-squares minimiser cannot be beaten: only rounding separates the two residuals."""
    from mobgs_amd.scene_init import inverse_cubic_hermite
    fx, traj, t_step, c_ref, c64 = _fixture()
    target = traj.double() * 1e2
    got = inverse_cubic_hermite(traj * 1e2, t_step[None, :, None].expand(traj.shape[0], -1, -1), N_pts=N_PTS)
    res = float((_evaluate(got, t_step) - target).norm())
    res_ref = float((_evaluate(c_ref, t_step) - target).norm())
    print(f"fit residual: {res:.6e}, reference solution {res_ref:.6e}")
    assert res_ref > 1.0   # (noisy trajectories: the residual is far above rounding, so the comparison means something)
    assert res <= res_ref * (1 + 1e-4)


def test_per_row_times_agree_with_shared_times():
    from mobgs_amd.scene_init import inverse_cubic_hermite
    fx, traj, t_step, c_ref, c64 = _fixture()
    curves = traj[:64] * 1e2
    shared = inverse_cubic_hermite(curves, t_step[None, :, None].expand(64, -1, -1), N_pts=N_PTS)
    # the same times, but as a materialised batch with one row moved by less than rounding can see in the result: the
    # rows differ, so the batched least-squares path runs
    rows = t_step[None, :, None].repeat(64, 1, 1)
    rows[3, 5, 0] = torch.nextafter(rows[3, 5, 0], torch.tensor(1.0))
    per_row = inverse_cubic_hermite(curves, rows, N_pts=N_PTS)
    floor_abs, floor_rel = _gaps(c_ref, c64)
    d_abs, d_rel = _gaps(per_row, shared.double())
    print(f"per-row path vs shared path: {d_abs:.3e} abs / {d_rel:.3e} of the row")
    assert d_rel <= 3 * floor_rel
    # genuinely different times per row: every row solves its own system
    g = torch.Generator().manual_seed(3)
    tt = torch.sort((torch.linspace(0, 1, 24) + 0.01 * torch.randn(8, 24, generator=g)).clamp(0, 1), dim=1).values
    tt[:, 0], tt[:, -1] = 0.0, 1.0
    ctrl = torch.randn(8, N_PTS, 3, generator=g, dtype=torch.float64)
    from mobgs_amd.scene_init import hermite_design
    curves = (hermite_design(tt, N_PTS) @ ctrl).float()   # samples of known splines
    back = inverse_cubic_hermite(curves, tt[..., None], N_pts=N_PTS)
    A = hermite_design(tt, N_PTS)
    assert float((A @ back.double() - curves.double()).abs().max()) < 1e-4


def test_rank_deficient_input_raises():
    from mobgs_amd.scene_init import inverse_cubic_hermite
    curves = torch.randn(5, 8, 3)
    with pytest.raises(ValueError, match="rank-deficient"):   # T < N_pts
        inverse_cubic_hermite(curves, torch.linspace(0, 1, 8)[None, :, None].expand(5, -1, -1), N_pts=N_PTS)
    curves = torch.randn(5, 24, 3)
    with pytest.raises(ValueError, match="rank-deficient"):   # enough samples, all in the first two segments
        inverse_cubic_hermite(curves, (torch.linspace(0, 1, 24) * 0.15)[None, :, None].expand(5, -1, -1), N_pts=N_PTS)
    rows = (torch.linspace(0, 1, 24) * 0.15)[None, :, None].repeat(5, 1, 1)
    rows[1] *= 0.5
    with pytest.raises(ValueError, match="rank-deficient"):   # the per-row path
        inverse_cubic_hermite(curves, rows, N_pts=N_PTS)


def test_design_matrix_reproduces_the_spline_evaluator():
    """hermite_design row t = the weights of the evaluator render() uses (index clamping, one-sided end derivatives)."""
    from mobgs_amd.scene_init import hermite_design
    g = torch.Generator().manual_seed(5)
    ctrl = torch.randn(7, N_PTS, 3, generator=g, dtype=torch.float64)
    ts = torch.tensor([0.0, 1e-7, 0.04, 1.0 / 11.0, 0.25, 0.5, 10.0 / 11.0, 0.97, 0.999999, 1.0], dtype=torch.float64)
    A = hermite_design(ts, N_PTS)
    assert A.shape == (10, N_PTS) and float((A.sum(1) - 1).abs().max()) < 1e-12
    assert float((A @ ctrl - _evaluate(ctrl, ts)).abs().max()) < 1e-12


def test_simple_knn_shim_and_no_cpu_path():
    from mobgs_amd.simple_knn._C import distCUDA2
    import mobgs_amd.simple_knn as sk
    from mobgs_amd.scene_init import knn3_mean_dist2
    assert sk.distCUDA2 is distCUDA2 and callable(distCUDA2)
    with pytest.raises(RuntimeError, match="HIP device"):
        distCUDA2(torch.rand(16, 3))
    with pytest.raises(RuntimeError, match="HIP device"):
        knn3_mean_dist2(torch.rand(16, 3))


def test_knn_entry_points_refuse_bad_sizes_before_any_launch():
    """n < 4 and n above the 32-bit index range return MOBGS_E_INVALID with a message; no device is touched (this runs
    without one).  The scratch query reports 0 for them and 32 bytes per box / super-box otherwise."""
    import ctypes
    from mobgs_amd import _lib
    h = _lib.load()
    none = ctypes.c_void_p(None)
    for n in (3, 0, -1, (1 << 30) + 1, 2 ** 31 - 1):
        assert h.mobgs_knn3_scratch_bytes(n) == 0
        assert h.mobgs_knn3_mean_dist2(n, none, none, none, 0, none) == -1
        assert b"mobgs_knn3_mean_dist2" in h.mobgs_last_error()
    assert h.mobgs_knn3_scratch_bytes(4) == 2 * 32
    assert h.mobgs_knn3_scratch_bytes(1 << 20) == (4096 + 256) * 32
    assert h.mobgs_knn3_mean_dist2(100, none, none, none, 0, none) == -1   # NULL buffers


def test_fixture_is_small_and_complete():
    import os
    from helpers import GOLDEN
    assert os.path.getsize(os.path.join(GOLDEN, "init.npz")) < 420 * 1024
    fx = load("init")
    pts = fx["points"]
    assert len(np.unique(pts, axis=0)) < len(pts) and float(np.abs(pts).max()) > 100   # duplicates, far outlier
    assert "static.control_xyz" not in fx and fx["dynamic.control_xyz"].shape == (len(pts), 12, 3)
