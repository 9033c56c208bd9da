"""Scene seeding on the GPU (csrc/scene_seed.hip) against the float64 restatement tests/seed_restatement.py, on the
fixture the reference produced (tests/golden/seed.npz, make_golden_seed.py).

Tolerances are 3 x the reference's own fp32 / float64 gap stored in the fixture (`ref_gaps`): 3.9e-6 for
accum_error (values up to 2.5), 2.9e-8 for the per-view mean, 6.1e-7 for the world points (coordinates up to 3.5).  A pixel
is left out of the accum_error comparison only where a reprojection into another view lies within 1e-3 px of that view's
border (the in / out decision may then fall either way in fp32): at most 2 % of the pixels, and the restatement alone
must flag at most 1 %.  The thresholded masks must agree wherever |accum_error - mean| exceeds the accum_error + mean
tolerance; at most 0.1 % of the pixels may lie inside that margin.  Track indices and trajectories are exact: the
distances are formed in fp32 without contraction and the trajectory is a gather."""
import types

import numpy as np
import pytest
import torch

import seed_restatement as SR
from helpers import load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return load("seed")


def cameras(fx):
    V = fx["images"].shape[0]
    f, cx, cy = fx["intrinsics"]
    w2c = np.concatenate([fx["R"].transpose(0, 2, 1), fx["T"][:, :, None]], -1)
    K = np.tile(np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]]), (V, 1, 1))
    return w2c, K


@pytest.fixture(scope="module")
def restated(fx):
    """Computed once, shared, never written."""
    w2c, K = cameras(fx)
    accum, mean, near = SR.consistency(fx["images"], fx["depths"], w2c, K)
    inc, cls = SR.classify(accum, mean, fx["masks"])
    out = {"accum": accum, "mean": mean, "near": near, "inc": inc, "cls": cls,
           "points": SR.world_points(fx["depths"], w2c, K)}
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def maps(fx, hip_device):
    """One run of the two map launches on the fixture (+ view_consistency's mean), inputs checked for being unchanged."""
    from mobgs_amd.scene_init import seed_maps, view_consistency
    w2c, K = cameras(fx)
    dev = hip_device
    ins = [torch.from_numpy(fx[k]).to(dev) for k in ("images", "depths", "masks")]
    before = [t.clone() for t in ins]
    m = seed_maps(ins[0], ins[1], torch.from_numpy(w2c), torch.from_numpy(K), ins[2])
    accum, mean = view_consistency(ins[0], ins[1], torch.from_numpy(w2c), torch.from_numpy(K))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ins, before))
    assert torch.equal(accum, m.accum_error)          # deterministic: two runs, the same bits
    return m, mean


def _poison(dev, mb=64):
    """Fill free blocks of the caching allocator with 0xFF bytes: an output element that a kernel does not write shows
    as NaN in a float array, as 255 in the uint8 masks and as -1 in the int32 indices."""
    t = torch.full((mb * 1024 * 1024,), 255, dtype=torch.uint8, device=dev)
    del t


def test_accum_error_and_mean(fx, restated, maps):
    m, mean = maps
    gap_accum, gap_mean, _ = fx["ref_gaps"]
    near = restated["near"]
    assert near.mean() <= 0.01                         # the restatement alone
    err = np.abs(m.accum_error.cpu().numpy().astype(np.float64) - restated["accum"])
    err_mean = np.abs(mean.cpu().numpy().astype(np.float64) - restated["mean"])
    print(f"accum_error: max |diff| {err[~near].max():.3e} (allowed {3 * gap_accum:.3e}), at skipped pixels "
          f"{err[near].max() if near.any() else 0:.3e}; skipped {near.mean():.3%}; mean: {err_mean.max():.3e} (allowed "
          f"{3 * gap_mean:.3e})")
    assert near.mean() <= 0.02
    assert err[~near].max() <= 3 * gap_accum
    assert err_mean.max() <= 3 * gap_mean
    assert m.accum_error.dtype == torch.float32 and mean.shape == (fx["images"].shape[0],)


def test_inconsistent_and_class(fx, restated, maps):
    m, _ = maps
    gap_accum, gap_mean, _ = fx["ref_gaps"]
    margin = 3 * gap_accum + 3 * gap_mean
    out = (np.abs(restated["accum"] - restated["mean"][:, None, None]) <= margin) | restated["near"]
    inc, cls = m.inconsistent.cpu().numpy(), m.cls.cpu().numpy()
    print(f"left out {out.mean():.4%} (allowed 0.1 %); flips {int((inc != restated['inc'])[~out].sum())}")
    assert out.mean() <= 1e-3                          # everything left out, near-border pixels included
    assert inc.dtype == np.uint8 and cls.dtype == np.uint8
    assert np.array_equal(inc[~out], restated["inc"][~out]) and np.array_equal(cls[~out], restated["cls"][~out])
    assert set(np.unique(cls)) == {0, 1, 2}


def test_points(fx, restated, maps):
    m, _ = maps
    err = np.abs(m.points.cpu().numpy().astype(np.float64) - restated["points"])
    print(f"points: max |diff| {err.max():.3e} (allowed {3 * fx['ref_gaps'][2]:.3e})")
    assert err.max() <= 3 * fx["ref_gaps"][2]


def test_trajectories(fx, restated, maps, hip_device):
    from mobgs_amd.scene_init import track_trajectories
    m, _ = maps
    H, W = fx["images"].shape[2:]
    coords = fx["ref_dyn_coords"]
    index, pixel = SR.track_lookup(coords, fx["tracklet"], H, W)
    ins = [torch.from_numpy(coords).to(hip_device), torch.from_numpy(fx["tracklet"]).to(hip_device), m.points.clone()]
    before = [t.clone() for t in ins]
    got_index, got = track_trajectories(*ins)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ins, before))
    assert got_index.dtype == torch.int32 and np.array_equal(got_index.cpu().numpy(), index)
    for low, high in fx["planted"]:
        assert (index == low).any()                    # the planted ties went to the lower index (test_seed_cpu)
    want = SR.gather_trajectory(m.points.cpu().numpy(), pixel)
    assert np.array_equal(got.cpu().numpy(), want)     # a pure gather: bit-equal
    assert (pixel < 0).any() and (got.cpu().numpy()[pixel < 0] == 0).all()
    assert np.array_equal(index, fx["ref_track_index"])


@pytest.mark.parametrize("case", ["two_small_views", "second_chunk_one_track", "second_wave_one_lane"])
def test_launch_shapes(case, hip_device):
    """V = 2 at 17 x 33 (561 pixels: three workgroups per view, the last with 49 live lanes, and three partials for the
    mean); M = 1025 (the second LDS chunk holds one track, the nearest one); N = 65 (the second wave holds one lane).
    Outputs go into memory the allocator handed back with every byte 0xFF: NaN as a float, 255 as a class byte."""
    from mobgs_amd.scene_init import seed_maps, track_trajectories
    g = np.random.default_rng(11)
    V, H, W = (2, 17, 33) if case == "two_small_views" else (3, 20, 36)
    f = 30.0
    K = np.tile(np.array([[f, 0, W / 2 + 0.2], [0, f, H / 2 - 0.1], [0, 0, 1.0]]), (V, 1, 1))
    w2c = np.zeros((V, 3, 4))
    for i in range(V):
        a = 0.05 * i
        w2c[i, :, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        w2c[i, :, 3] = (0.1 * i, -0.05 * i, 0.02 * i)
    images = g.uniform(0.1, 0.9, (V, 3, H, W)).astype(np.float32)
    depths = g.uniform(2.0, 3.0, (V, H, W)).astype(np.float32)
    masks = (g.uniform(0, 1, (V, H, W)) < 0.3).astype(np.uint8)
    dev = hip_device
    ins = [torch.from_numpy(a).to(dev) for a in (images, depths, masks)]
    before = [t.clone() for t in ins]
    _poison(dev)
    m = seed_maps(ins[0], ins[1], torch.from_numpy(w2c), torch.from_numpy(K), ins[2])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ins, before))
    accum, mean, near = SR.consistency(images, depths, w2c, K)
    inc, cls = SR.classify(accum, mean, masks)
    pts = SR.world_points(depths, w2c, K)
    # random textures: a reprojected coordinate goes through ~10 fp32 operations at magnitude <= 36, so it is within
    # 10 x 2^-24 x 36 = 2.1e-5 px per axis; neighbouring pixels differ by <= 0.8, so a sample moves by <= 2 x 0.8 x 2.1e-5
    # = 3.4e-5 per view and accum_error by V times that.  Points: ~8 roundings at the largest coordinate.  (Derived, as
    # these inputs have no reference run; not taken from a measured gap.)
    tol = 3.4e-5 * V
    got = m.accum_error.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all() and np.abs(got - accum)[~near].max() <= tol
    sure = (np.abs(accum - mean[:, None, None]) > 2 * tol) & ~near
    assert np.array_equal(m.inconsistent.cpu().numpy()[sure], inc[sure]) and np.array_equal(m.cls.cpu().numpy()[sure], cls[sure])
    assert (m.cls.cpu().numpy() <= 2).all() and (m.inconsistent.cpu().numpy() <= 1).all()
    assert np.abs(m.points.cpu().numpy() - pts).max() <= 2.0 ** -21 * 4 * np.abs(pts).max()

    N, M = (65, 300) if case == "second_wave_one_lane" else (40, 1025 if case == "second_chunk_one_track" else 7)
    coords = np.stack([g.integers(0, W, N), g.integers(0, H, N)], 1).astype(np.float32)
    tracklet = np.stack([g.uniform(-3, W + 3, (V, M)), g.uniform(-3, H + 3, (V, M))], -1).astype(np.float32)
    if case == "second_chunk_one_track":
        tracklet[0, :1024] += 100.0                    # only the track alone in the second chunk is near anything
    tracklet = np.where(np.abs(tracklet - np.rint(tracklet)) < 2e-3, tracklet + np.float32(5e-3), tracklet).astype(np.float32)
    tins = [torch.from_numpy(coords).to(dev), torch.from_numpy(tracklet).to(dev), m.points]
    tbefore = [t.clone() for t in tins]
    _poison(dev)
    got_index, traj = track_trajectories(*tins)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(tins, tbefore))
    index, pixel = SR.track_lookup(coords, tracklet, H, W)
    assert np.array_equal(got_index.cpu().numpy(), index)
    if case == "second_chunk_one_track":
        assert (index == 1024).all()
    assert np.array_equal(traj.cpu().numpy(), SR.gather_trajectory(m.points.cpu().numpy(), pixel))


def test_end_to_end(fx, restated, hip_device):
    """scene_initialization with the reference's picks -> from_pcd / from_pcd_dynamic -> one render()."""
    from mobgs_amd.camera import PinholeCamera
    from mobgs_amd.densify import TrainableGaussians
    from mobgs_amd.gaussian_renderer import render
    from mobgs_amd.scene_init import scene_initialization
    dev = hip_device
    f, cx, cy = fx["intrinsics"]
    md = types.SimpleNamespace(principal_point_x=cx, principal_point_y=cy)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    V, _, H, W = fx["images"].shape
    vps = [types.SimpleNamespace(original_image=T(fx["images"][i]), depth=T(fx["depths"][i])[None], R=fx["R"][i],
                                 T=fx["T"][i], focal=float(f), metadata=md, mask=T(fx["masks"][i]).float()[None],
                                 time=float(fx["times"][i]), tracklet=T(fx["tracklet"])) for i in range(V)]
    stat_pc, dyn_pc, traj = scene_initialization(vps, int(fx["npts"][0]), int(fx["npts"][1]),
                                                 select=(fx["stat_idx"], fx["dyn_idx"]))
    assert stat_pc.points.is_cuda and traj.is_cuda and stat_pc.normals is None
    tol = 3 * fx["ref_gaps"][2]
    assert np.abs(stat_pc.points.cpu().numpy() - fx["f64_stat_points"]).max() <= tol
    assert np.abs(dyn_pc.points.cpu().numpy() - fx["f64_dyn_points"]).max() <= tol
    assert np.abs(traj.cpu().numpy() - fx["f64_traj"]).max() <= tol
    for k, got in (("stat_colors", stat_pc.colors), ("dyn_colors", dyn_pc.colors), ("stat_times", stat_pc.times),
                   ("dyn_times", dyn_pc.times)):
        assert np.array_equal(got.cpu().numpy(), fx["ref_" + k]), k
    stat = TrainableGaussians.from_pcd(stat_pc, 5.0, device=dev)
    # the spline fit determines 12 control points and refuses fewer samples than that (scene_init.inverse_cubic_hermite);
    # the fixture has 6 views, so its trajectories are resampled to 12 uniform times (linear, end points kept) first
    with pytest.raises(ValueError, match="rank-deficient"):
        TrainableGaussians.from_pcd_dynamic(dyn_pc, 5.0, 0, traj, device=dev)
    traj12 = torch.nn.functional.interpolate(traj.permute(0, 2, 1), size=12, mode="linear", align_corners=True)
    traj12 = traj12.permute(0, 2, 1).contiguous()
    assert torch.equal(traj12[:, 0], traj[:, 0]) and torch.equal(traj12[:, -1], traj[:, -1])
    dyn = TrainableGaussians.from_pcd_dynamic(dyn_pc, 5.0, 0, traj12, device=dev)
    w2c = torch.eye(4)
    w2c[:3, :3] = torch.from_numpy(fx["R"][2].T.copy())
    w2c[:3, 3] = torch.from_numpy(fx["T"][2])
    K = torch.tensor([[f, 0, cx], [0, f, cy], [0, 0, 1.0]], dtype=torch.float32)
    cam = PinholeCamera(W, H, K, w2c, float(fx["times"][2]), V, device=dev)
    out = render(cam, stat, dyn, None, torch.zeros(9, device=dev))
    img = out["render"]
    assert img.shape[-2:] == (H, W) and bool(torch.isfinite(img).all())
    assert float(img.max()) > float(img.min())


def test_example_from_views(hip_device):
    """examples/train_deblur_synth.py --from-views: both sets come out of scene_initialization on 12 synthetic views
    (enough samples for the spline fit as they are) with the sizes asked for, lie on the views' plane, and the miniature
    training loop runs on them with finite losses and gradients on both sets."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_deblur_synth as T
    history, stat, dyn, _, _ = T.train(dev=str(hip_device), iters=3, ns=1500, nd=600, width=128, height=96, seed=2,
                                       from_views=True)
    assert len(history) == 3 and all(h == h for h in history)        # finite
    assert stat.get_xyz.shape == (1500, 3) and dyn.get_xyz.shape == (600, 3)
    n = torch.tensor([0.15, -0.1, 1.0], device=hip_device)
    # on the plane normal . X = 3.5 of the views, up to three Adam steps on the positions (a few 1e-3 each at most)
    assert float((stat.get_xyz.detach() @ n - 3.5).abs().max()) < 0.02
    assert int(dyn.current_control_num.min()) == 12 and bool(torch.isfinite(dyn.control_xyz).all())
    assert float(stat.xyz_gradient_accum.abs().max()) > 0 and float(dyn.denom.max()) > 0
