"""Report sheets without a GPU: the float64 restatement and the numpy path of mobgs_amd.flow_vis against the fixture the
reference's own render_training_image produced (tests/golden/make_golden_report.py), the colour wheel's anchors, what
can be said about the flow colours without remembering the flow_vis package, shapes, refusals."""
import os

import numpy as np
import pytest
import torch

import report_cases as RC
import report_restatement as R
from helpers import GOLDEN, load

CASES = ("test", "train", "train_blur")


@pytest.fixture(scope="module")
def fx():
    return load("report_sheets")


def inputs(fx, case):
    r = {k: fx[f"{case}_{k}"] for k in ("render", "d_render", "s_render", "d_alpha", "depth")}
    r.update(gt=fx["gt"], gt_normal=fx["gt_normal"], gt_depth=fx["gt_depth"])
    if case == "train_blur":
        r["blurry"] = fx[f"{case}_blurry"]
    return r


def expected(panels, cam):
    xs = [R.panel(p[0], p[1], p[2] if len(p) > 2 else None, cam) for p in panels]
    bs = [RC.band(p[0], p[1], p[2] if len(p) > 2 else None, cam) for p in panels]
    return R.level(np.concatenate(xs, axis=1)), np.concatenate(bs, axis=1)


@pytest.mark.parametrize("case", CASES)
def test_restatement_against_the_references_sheets(fx, case):
    """The reference's own uint8 arrays (captured before JPEG coding) obey the one-level rule around the restatement."""
    cam = tuple(fx["cam"])
    r = inputs(fx, case)
    for name, panels in (("image", R.image_panels(case, r)), ("decomp", R.decomp_panels(case, r))):
        L, b = expected(panels, cam)
        RC.check_bytes(fx[f"{case}_{name}"], L, b, f"{case} {name}")
    if case == "train_blur":
        for k in range(9):
            L, b = expected([("RGB", fx[f"{case}_latent_{k}"])], cam)
            RC.check_bytes(fx[f"{case}_latent_img_{k}"], L, b, f"latent {k}")
        ten = np.stack([fx[f"{case}_latent_{k}"] for k in range(9)] + [fx[f"{case}_render"]])
        assert np.abs(ten.astype(np.float64).mean(0) - fx[f"{case}_blurry"]).max() < 1e-6     # the mean of TEN images


def test_sheet_shapes(fx):
    H, W = fx["gt"].shape[-2:]
    assert (H, W) == (48, 80)
    for case, n_image, n_decomp in (("test", 6, 2), ("train", 5, 4), ("train_blur", 4, 4)):
        r = inputs(fx, case)
        assert fx[f"{case}_image"].shape == (H, n_image * W, 3) and fx[f"{case}_image"].dtype == np.uint8
        assert fx[f"{case}_decomp"].shape == (H, n_decomp * W, 3)
        assert R.sheet(R.image_panels(case, r)).shape == (H, n_image * W, 3)
        assert R.sheet(R.decomp_panels(case, r), tuple(fx["cam"])).shape == (H, n_decomp * W, 3)
    from mobgs_amd.scene_utils import ReportSheets
    assert ReportSheets._fields[:4] == ("image", "decomp", "flows", "latents")


def test_numpy_flow_path_against_fixture_and_restatement(fx):
    """The fixture's flow images are UNPINNED (the generator's flow_vis is the restatement); the numpy path of
    mobgs_amd.flow_vis, float32 as the package computes, is held to the one-level rule around it."""
    from mobgs_amd import flow_vis
    assert set(fx["unpinned"]) == {f"train_blur_flow_img_{k}" for k in (0, 4, 8)}
    for k in (0, 4, 8):
        flow = fx[f"train_blur_flow_{k}"]
        assert flow.shape == (48, 80, 2) and flow.dtype == np.float32
        assert np.array_equal(R.flow_to_color(flow), fx[f"train_blur_flow_img_{k}"])
        got = flow_vis.flow_to_color(flow)
        assert got.dtype == np.uint8 and got.shape == (48, 80, 3)
        RC.check_bytes(got, R.level(R.flow(flow)), RC.band("FLOW", flow), f"numpy flow_to_color {k}")
        assert np.array_equal(flow_vis.flow_to_color(torch.from_numpy(flow)), got)          # a host tensor: the numpy path
        assert np.array_equal(flow_vis.flow_to_color(flow, convert_to_bgr=True), got[..., ::-1])
    flow = RC.source("FLOW", 13, 17, 5)[1]
    RC.check_bytes(flow_vis.flow_to_color(flow, clip_flow=1.5), R.level(R.flow(flow, 1.5)), RC.band("FLOW", flow, clip=1.5),
                   "numpy flow_to_color, clip_flow")
    with pytest.raises(ValueError):
        flow_vis.flow_to_color(np.zeros((4, 4, 3), np.float32))


def test_wheel_anchors():
    from mobgs_amd import flow_vis
    w = R.wheel()
    assert w.shape == (55, 3)
    for k, rgb in ((0, (255, 0, 0)), (15, (255, 255, 0)), (21, (0, 255, 0)), (25, (0, 255, 255)), (36, (0, 0, 255)),
                   (49, (255, 0, 255))):
        assert tuple(w[k]) == rgb, k
    assert np.array_equal(flow_vis.make_colorwheel(), w.astype(np.float64))
    assert np.abs(np.diff(np.concatenate([w, w[:1]]), axis=0)).max() <= 64     # the slope bound tests/report_cases.py uses
    # the `* 0.75` arm exists in the numpy path and the restatement only
    u, v = np.array([[1.5, 0.3]], np.float32), np.array([[0.5, -0.2]], np.float32)
    assert np.abs(flow_vis.flow_uv_to_colors(u, v).astype(np.int64) - R.to_bytes(R.flow_uv_to_colors(u, v))).max() <= 1
    unit = np.hypot(u, v)[0, 0]             # at radius 1 the colour is the wheel's own: beyond, 0.75 of it
    assert np.allclose(R.flow_uv_to_colors(u, v)[0, 0], 0.75 * R.flow_uv_to_colors(u / unit, v / unit)[0, 0], atol=1e-6)


def test_flow_colour_facts_that_need_no_memory_of_the_package():
    one = np.zeros((1, 2, 2))
    one[0, 0] = (3.0, 0.0)                       # to the right; the second pixel is a zero flow
    img = R.flow_to_color(one.astype(np.float32))
    assert img[0, 0, 0] == 255 and img[0, 0, 1] == img[0, 0, 2] < 30, img[0, 0]     # red
    assert tuple(img[0, 1]) == (255, 255, 255)                                       # white
    assert tuple(R.flow_to_color(np.zeros((3, 4, 2), np.float32)).reshape(-1, 3).max(0)) == (255, 255, 255)
    assert R.flow_to_color(np.zeros((3, 4, 2), np.float32)).min() == 255
    # continuous in the angle, except across the wrap at v = 0, u > 0 (theta = 0)
    n = 7200
    theta = (np.arange(n) + 0.5) * 2 * np.pi / n
    ring = R.flow_uv_to_colors(0.8 * np.cos(theta)[None], 0.8 * np.sin(theta)[None])[0]
    step = np.abs(np.diff(ring, axis=0)).max(1)
    assert step.max() <= 0.8 * (64 / 255) * 54 / n + 1e-12        # slope in fk times the step in fk, times the radius
    assert np.abs(ring[0] - ring[-1]).max() > 0.1                # the wrap: entry 0 against entry 54
    # saturation grows with the radius: along a direction every channel falls (or stays) as the radius rises
    for ang in (0.3, 1.9, 3.0, 4.4, 5.9):
        rad = np.linspace(0.0, 0.99, 50)
        line = R.flow_uv_to_colors((rad * np.cos(ang))[None], (rad * np.sin(ang))[None])[0]
        assert (np.diff(line, axis=0) <= 1e-12).all() and line[0].min() == 1.0
        assert (line.max(1) - line.min(1))[-1] > (line.max(1) - line.min(1))[1]


def test_sizes_below_two_by_two_are_refused():
    from mobgs_amd.scene_utils import compose_sheet
    cam = RC.camera(1, 5)
    for H, W in ((1, 5), (5, 1), (1, 1)):
        with pytest.raises(ValueError, match="NORMALS_FD"):
            compose_sheet([("NORMALS_FD", torch.ones(1, H, W))], H, W, camera=cam)
        with pytest.raises(ValueError):
            R.normals_fd(np.ones((1, H, W), np.float32), cam)
    with pytest.raises(ValueError, match="unknown panel kind"):
        compose_sheet([("HSV", torch.ones(3, 2, 2))], 2, 2)
    with pytest.raises(RuntimeError, match="HIP device"):          # no CPU path for the kernels
        compose_sheet([("RGB", torch.ones(3, 2, 2))], 2, 2)
    from mobgs_amd.scene_utils import render_training_image, report_sheets
    with pytest.raises(NotImplementedError):
        report_sheets(None, None, None, None, None, None, None, None, stage="warm")
    with pytest.raises(NotImplementedError):
        render_training_image(None, None, None, [], None, None, None, "warm", 0, 0.0, "dycheck")


def test_entry_points_and_build_flags():
    from mobgs_amd import _lib, build
    assert "report.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["report.hip"]
    P = _lib.c_void_p
    assert _lib._SIGS["mobgs_report_stats"] == (_lib.c_int, [_lib.c_int, P, P, P])
    assert _lib._SIGS["mobgs_report_stats_floats"] == (_lib.c_size_t, [_lib.c_int])
    assert len(_lib._SIGS["mobgs_report_compose"][1]) == 14
    h = _lib.load()
    none = P(None)
    assert h.mobgs_report_stats_floats(3) == 15 and h.mobgs_report_stats_floats(0) == 0
    assert h.mobgs_report_stats(0, none, none, none) == -1 and b"mobgs_report_stats" in h.mobgs_last_error()
    assert h.mobgs_report_compose(4, 4, 1, none, none, 0, 1.0, 0.0, 0.0, 0.0, 0.5, 0, none, none) == -1
    assert b"mobgs_report_compose" in h.mobgs_last_error()
    assert _lib._DEFINES["MOBGS_REPORT_WHEEL"] == R.NCOLS


def test_flowvis_vectors():
    """Present only after scripts/dump_flowvis_vectors.py ran where the flow_vis package is installed; skipped otherwise
    (README, "The flow colour wheel is UNPINNED")."""
    path = os.path.join(GOLDEN, "flowvis_external", "flow_to_color.npz")
    if not os.path.exists(path):
        pytest.skip("no tests/golden/flowvis_external/flow_to_color.npz (scripts/dump_flowvis_vectors.py): UNPINNED")
    from mobgs_amd import flow_vis
    ex = dict(np.load(path))
    assert np.array_equal(ex["colorwheel"], R.wheel().astype(np.float64))
    assert np.array_equal(flow_vis.make_colorwheel(), ex["colorwheel"])
    for name in (k[:-5] for k in ex if k.endswith("_flow")):
        clip = float(ex[name + "_clip"]) if name + "_clip" in ex else None
        flow = ex[name + "_flow"]
        assert np.array_equal(flow_vis.flow_to_color(flow, clip_flow=clip), ex[name + "_color"]), name
        RC.check_bytes(ex[name + "_color"], R.level(R.flow(flow, clip)), RC.band("FLOW", flow, clip=clip), name)
