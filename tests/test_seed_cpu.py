"""Scene seeding without a GPU: the float64 restatement against what the reference computed for the fixture
(tests/golden/seed.npz, make_golden_seed.py), the pair table, the sampling and tie rules, every refusal, the C ABI, and
scene_initialization on host tensors (its float64 composition) against the fixture's point clouds."""
import ctypes
import types

import numpy as np
import pytest
import torch

import seed_restatement as SR
from helpers import load


@pytest.fixture(scope="module")
def fx():
    return load("seed")


def cameras(fx):
    V = fx["images"].shape[0]
    f, cx, cy = fx["intrinsics"]
    w2c = np.concatenate([fx["R"].transpose(0, 2, 1), fx["T"][:, :, None]], -1)
    K = np.tile(np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]]), (V, 1, 1))
    return w2c, K


def viewpoints(fx, n=None, device="cpu"):
    f, cx, cy = fx["intrinsics"]
    md = types.SimpleNamespace(principal_point_x=cx, principal_point_y=cy)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    V = fx["images"].shape[0] if n is None else n
    return [types.SimpleNamespace(original_image=T(fx["images"][i]), depth=T(fx["depths"][i])[None], R=fx["R"][i],
                                  T=fx["T"][i], focal=float(f), metadata=md, mask=T(fx["masks"][i]).float()[None],
                                  time=float(fx["times"][i]), tracklet=T(fx["tracklet"])) for i in range(V)]


@pytest.fixture(scope="module")
def restated(fx):
    w2c, K = cameras(fx)
    accum, mean, near = SR.consistency(fx["images"], fx["depths"], w2c, K)
    inc, cls = SR.classify(accum, mean, fx["masks"])
    return {"accum": accum, "mean": mean, "near": near, "inc": inc, "cls": cls,
            "points": SR.world_points(fx["depths"], w2c, K)}


def test_restatement_matches_the_reference(fx, restated):
    gap_accum, gap_mean, gap_points = fx["ref_gaps"]
    assert np.array_equal(restated["accum"], fx["f64_accum"]) and np.array_equal(restated["mean"], fx["f64_mean"])
    keep = ~restated["near"]
    assert restated["near"].mean() <= 0.01
    assert np.abs(restated["accum"] - fx["ref_accum"])[keep].max() <= gap_accum
    assert np.abs(restated["mean"] - fx["ref_mean"]).max() <= gap_mean
    assert np.array_equal(restated["cls"], fx["ref_cls"]) and np.array_equal(restated["inc"], fx["ref_inconsistent"])
    c = SR.clouds(fx["images"], restated["points"], restated["cls"], fx["times"], fx["stat_idx"], fx["dyn_idx"])
    assert np.abs(c["stat_points"] - fx["ref_stat_points"]).max() <= gap_points
    assert np.abs(c["dyn_points"] - fx["ref_dyn_points"]).max() <= gap_points
    for k in ("stat_colors", "stat_times", "dyn_colors", "dyn_times", "dyn_coords"):
        assert np.array_equal(c[k], fx["ref_" + k]), k
    H, W = fx["images"].shape[2:]
    index, pixel = SR.track_lookup(c["dyn_coords"], fx["tracklet"], H, W)
    assert np.array_equal(index, fx["ref_track_index"])
    assert np.abs(SR.gather_trajectory(restated["points"], pixel) - fx["ref_traj"]).max() <= gap_points
    assert (fx["ref_traj"][pixel < 0] == 0).all() and (pixel < 0).any()
    assert len(fx["dyn_idx"]) == fx["npts"][1] > (restated["cls"][0] == 1).sum()    # the with-replacement branch


def test_pair_table_against_the_step_by_step_product(fx):
    from mobgs_amd.scene_init import pair_table, unproject_table
    w2c, K = cameras(fx)
    V = w2c.shape[0]
    w, k = torch.from_numpy(w2c), torch.from_numpy(K)
    table = pair_table(w, k).double().reshape(V, V, 3, 4)
    unproj = unproject_table(w, k).double().reshape(V, 3, 4)
    assert pair_table(w, k).dtype == torch.float32
    g = np.random.default_rng(3)
    for i in range(V):
        for j in range(V):
            u, v, d = g.uniform(0, 79), g.uniform(0, 47), g.uniform(2, 6)
            cam = d * (np.linalg.inv(K[i]) @ np.array([u, v, 1.0]))
            world = w2c[i][:, :3].T @ cam - w2c[i][:, :3].T @ w2c[i][:, 3]
            pix = K[j] @ (w2c[j][:, :3] @ world + w2c[j][:, 3])
            h = np.array([d * u, d * v, d, 1.0])
            got = table[i, j].numpy() @ h
            assert np.abs(got - pix).max() <= 4 * 2.0 ** -24 * np.abs(table[i, j].numpy() * h).sum(1).max()
            if j == i:
                assert np.abs(got / got[2] - np.array([u, v, 1.0])).max() < 1e-4
            gotw = unproj[i].numpy() @ h
            assert np.abs(gotw - world).max() <= 4 * 2.0 ** -24 * np.abs(unproj[i].numpy() * h).sum(1).max()


def test_nearest_sample_rule():
    from mobgs_amd.scene_init import nearest_pixel
    u = np.array([0.0, 0.49, 0.5, 0.99, 1.0, 1.5, 2.0, 2.5, 3.0, 3.49, 79.5, 80.0, 80.01, -0.01, 1e-9])
    want = np.array([-0.0, -0.0, 0.0, 0.0, 0.0, 1.0, 2.0, 2.0, 2.0, 3.0, 79.0, 80.0, 80.0, -1.0, -0.0])
    assert np.array_equal(SR.nearest_pixel(u), want)                  # integers are the half-way cases: ties to even
    assert np.array_equal(nearest_pixel(torch.from_numpy(u)).numpy(), want)
    # ... and it is what grid_sample(nearest, align_corners=False) reads after / W * 2 - 1, away from the half-way cases
    W = 8
    img = torch.arange(W, dtype=torch.float32).reshape(1, 1, 1, W)
    us = torch.tensor([0.3, 0.7, 1.2, 3.6, 6.9, 7.4, 7.9])
    grid = torch.stack([us / W * 2 - 1, torch.zeros_like(us)], -1).reshape(1, 1, -1, 2)
    got = torch.nn.functional.grid_sample(img, grid, mode="nearest", align_corners=False)[0, 0, 0]
    assert torch.equal(got, nearest_pixel(us))
    _, pixel = SR.track_lookup(np.zeros((1, 2), np.float32), np.array([[[8.2, 0.6]], [[7.9, 0.6]]], np.float32), 1, W)
    assert pixel.tolist() == [[-1, 7]]


def test_tie_rule(fx):
    from mobgs_amd.scene_init import track_trajectories
    coords = np.array([[5.0, 5.0], [9.0, 2.0]], np.float32)
    tr = np.full((2, 6, 2), 40.0, np.float32)
    tr[0, 4], tr[0, 1] = (5.25, 5.0), (4.75, 5.0)       # equal distance: index 1 wins
    tr[0, 2], tr[0, 5] = (9.0, 2.5), (9.0, 1.5)         # equal distance: index 2 wins
    index, _ = SR.track_lookup(coords, tr, 48, 80)
    assert index.tolist() == [1, 2]
    got, traj = track_trajectories(torch.from_numpy(coords), torch.from_numpy(tr), torch.ones(2, 48, 80, 3))
    assert got.tolist() == [1, 2] and got.dtype == torch.int32 and traj.shape == (2, 2, 3)
    # the planted ties of the fixture
    H, W = fx["images"].shape[2:]
    idx, _ = SR.track_lookup(fx["ref_dyn_coords"], fx["tracklet"], H, W)
    for low, high in fx["planted"]:
        start = fx["tracklet"][0]
        rows = [n for n, c in enumerate(fx["ref_dyn_coords"])
                if ((c - start[low]) ** 2).sum() == ((c - start[high]) ** 2).sum() == ((c - start) ** 2).sum(-1).min()]
        assert rows and (idx[rows] == low).all()


def test_refusals(fx):
    from mobgs_amd import scene_init as SI
    vps = viewpoints(fx)
    with pytest.raises(ValueError, match="at least 2"):
        SI.scene_initialization(vps[:1], 10, 10)
    bad = viewpoints(fx)
    bad[0].tracklet = bad[0].tracklet[:5]
    with pytest.raises(ValueError, match="one frame per view"):
        SI.scene_initialization(bad, 10, 10)
    bad = viewpoints(fx)
    bad[2].original_image = bad[2].original_image[:, :, :-1]
    with pytest.raises(ValueError, match="one image size"):
        SI.scene_initialization(bad, 10, 10)
    for value in (float("nan"), float("inf"), 0.0, -1.0):
        bad = viewpoints(fx)
        bad[3].depth = bad[3].depth.clone()
        bad[3].depth[0, 7, 9] = value
        with pytest.raises(ValueError, match="finite and positive"):
            SI.scene_initialization(bad, 10, 10)
    with pytest.raises(ValueError, match="static candidates"):
        SI.scene_initialization(vps, 10 ** 6, 10)
    still = viewpoints(fx)
    for v in still:
        v.mask = torch.zeros_like(v.mask)
    with pytest.raises(ValueError, match="no dynamic candidate"):
        SI.scene_initialization(still, 10, 10)
    pts = torch.zeros(6, 48, 80, 3)
    with pytest.raises(ValueError, match="one frame per view"):
        SI.track_trajectories(torch.zeros(3, 2), torch.zeros(5, 9, 2), pts)
    w2c, K = cameras(fx)
    img, dep = torch.from_numpy(fx["images"]), torch.from_numpy(fx["depths"])
    with pytest.raises(ValueError, match="at least 2 views"):
        SI.view_consistency(img[:1], dep[:1], torch.from_numpy(w2c[:1]), torch.from_numpy(K[:1]))


def test_abi_entries_and_sources():
    from mobgs_amd import _lib, build
    assert "scene_seed.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["scene_seed.hip"]
    h = _lib.load()
    assert _lib.ABI_VERSION >= 12
    for name in ("mobgs_seed_scratch_bytes", "mobgs_seed_consistency", "mobgs_seed_classify", "mobgs_seed_trajectories"):
        assert name in _lib._SIGS and hasattr(h, name)
    assert h.mobgs_seed_scratch_bytes(6, 48, 80) == 6 * 15 * 4
    assert h.mobgs_seed_scratch_bytes(2, 17, 33) == 2 * 3 * 4
    assert h.mobgs_seed_scratch_bytes(1, 48, 80) == 0 and h.mobgs_seed_scratch_bytes(2, 1, 80) == 0
    none = ctypes.c_void_p(None)
    assert h.mobgs_seed_consistency(1, 48, 80, none, none, none, none, none, 0, none) == -1
    assert b"mobgs_seed_consistency" in h.mobgs_last_error()
    assert h.mobgs_seed_consistency(6, 48, 80, none, none, none, none, none, 0, none) == -1
    assert h.mobgs_seed_classify(6, 48, 80, none, none, 0, none, none, none, none, none, none, none, none) == -1
    assert h.mobgs_seed_trajectories(4, 5, 9, 6, 48, 80, none, none, none, none, none, none) == -1
    assert b"5 frames" in h.mobgs_last_error()
    assert h.mobgs_seed_trajectories(4, 6, 0, 6, 48, 80, none, none, none, none, none, none) == -1
    assert h.mobgs_seed_trajectories(0, 6, 9, 6, 48, 80, none, none, none, none, none, none) == 0   # nothing to do
    assert h.mobgs_seed_trajectories(4, 6, 9, 6, 48, 80, none, none, none, none, none, none) == -1  # NULL buffers


def test_scene_initialization_on_host_tensors_reproduces_the_fixture(fx):
    from mobgs_amd.scene_init import scene_initialization, seed_maps
    _, _, gap_points = fx["ref_gaps"]
    stat_pc, dyn_pc, traj = scene_initialization(viewpoints(fx), int(fx["npts"][0]), int(fx["npts"][1]),
                                                 select=(fx["stat_idx"], fx["dyn_idx"]))
    assert stat_pc.normals is None and dyn_pc.normals is None
    assert stat_pc.points.shape == (fx["npts"][0], 3) and dyn_pc.points.shape == (fx["npts"][1], 3)
    tol = 3 * gap_points
    assert np.abs(stat_pc.points.numpy() - fx["f64_stat_points"]).max() <= tol
    assert np.abs(dyn_pc.points.numpy() - fx["f64_dyn_points"]).max() <= tol
    assert np.array_equal(stat_pc.colors.numpy(), fx["ref_stat_colors"])
    assert np.array_equal(dyn_pc.colors.numpy(), fx["ref_dyn_colors"])
    assert np.array_equal(stat_pc.times.numpy(), fx["ref_stat_times"])
    assert np.array_equal(dyn_pc.times.numpy(), fx["ref_dyn_times"])
    assert np.abs(traj.numpy() - fx["f64_traj"]).max() <= tol
    assert np.array_equal(traj.numpy() == 0, fx["ref_traj"] == 0)
    # the draw: seeded, inside the candidate lists, without / with replacement
    g = torch.Generator().manual_seed(5)
    a = scene_initialization(viewpoints(fx), 500, 300, generator=g)
    b = scene_initialization(viewpoints(fx), 500, 300, generator=torch.Generator().manual_seed(5))
    assert torch.equal(a[0].points, b[0].points) and torch.equal(a[2], b[2])
    assert len(torch.unique(a[0].points, dim=0)) == 500 and len(torch.unique(a[1].points, dim=0)) < 300
    w2c, K = cameras(fx)
    maps = seed_maps(torch.from_numpy(fx["images"]), torch.from_numpy(fx["depths"]), torch.from_numpy(w2c),
                     torch.from_numpy(K), torch.from_numpy(fx["masks"]))
    assert np.array_equal(maps.cls.numpy(), fx["ref_cls"]) and maps.inconsistent.dtype == torch.uint8
