"""tests/refcam_cases.py without a GPU: RefCamera is the documented interface and nothing more, its map is the one the
oracle expects for the fixtures' cameras, the renderer's ray selection sends it down the ray-map arm, and the pixel filter
of the map-gradient comparison holds its caps on the two oracles alone."""
import numpy as np
import pytest
import torch

import refcam_cases as C
from helpers import load, scene_from_fixture


def _fixture_camera(name):
    cam, stat, dyn, bg, w2c = scene_from_fixture(load(name), device="cpu", requires_grad=False)
    return cam, stat, dyn, bg


def test_refcamera_has_exactly_the_documented_attributes():
    import mobgs_amd.camera as camera_module
    pin, *_ = _fixture_camera("render_lean")
    for kw in ({}, {"pose_leaf": True}, {"ray_leaf": True}):
        cam, leaf = C.ref_camera(pin, **kw)
        public = {n for n in dir(cam) if not n.startswith("__")}
        assert public == set(C.CAMERA_ATTRIBUTES), public
        assert set(vars(cam)) | {"get_pixels"} == set(C.CAMERA_ATTRIBUTES)
        for n in C.PINHOLE_ONLY:
            assert not hasattr(cam, n), n
        assert (leaf is None) == (not kw)
    for n in C.CAMERA_ATTRIBUTES:   # the list is the docstring's
        assert n in camera_module.__doc__, n
    assert tuple(cam.cam_ray.shape) == (1, 6, pin.image_height, pin.image_width)
    assert np.array_equal(cam.get_pixels(7, 5, use_center=False), pin.get_pixels(7, 5, use_center=False))


def test_leaf_options_build_the_graph_the_issue_names():
    pin, *_ = _fixture_camera("render_lean")
    cam, c2w = C.ref_camera(pin, pose_leaf=True)
    assert c2w.is_leaf and c2w.requires_grad and tuple(c2w.shape) == (3, 4)
    assert not cam.cam_ray.is_leaf and cam.cam_ray.requires_grad          # a non-leaf with a graph into the pose
    assert torch.equal(cam.cam_ray.detach(), C.ref_camera(pin)[0].cam_ray)  # the same numbers as the plain camera
    g, = torch.autograd.grad(cam.cam_ray.sum(), c2w)
    assert float(g.abs().max()) > 0
    cam, ray = C.ref_camera(pin, ray_leaf=True)
    assert ray is cam.cam_ray and ray.is_leaf and ray.requires_grad


@pytest.mark.parametrize("name", ["render_lean", "render_train", "render_train_delta_flow", "get_flow"])
def test_map_is_what_the_oracle_expects_for_the_fixture_cameras(name):
    """The fixtures were produced by the reference with its own cam_ray: the oracle, fed the RefCamera, reproduces the
    fixture's decoded image (the only output the map enters) as it does with the PinholeCamera, bit for bit."""
    from oracle import render_torch as R
    fx = load(name)
    pin, stat, dyn, bg = _fixture_camera(name)
    cam, _ = C.ref_camera(pin)
    assert torch.equal(cam.cam_ray, pin.cam_ray)
    # ... and the float64 restatement of the map's construction agrees with the fp32 one to fp32 rounding
    c2w = torch.inverse(pin._w2c.double())[:3, :]
    m64 = C.ray_map_from_c2w(pin.image_width, pin.image_height, pin.K, c2w)
    assert float((m64 - cam.cam_ray.double()).abs().max()) <= 8 * 2.0 ** -24 * float(m64.abs().max())
    c2w32 = torch.inverse(pin._w2c)[:3, :]
    assert torch.equal(C.ray_map_from_c2w(pin.image_width, pin.image_height, pin.K, c2w32),
                       type(pin).build_cam_ray_c2w(pin.image_width, pin.image_height, pin.K, c2w32))
    with torch.no_grad():
        if name == "get_flow":
            d = torch.tensor(float(fx["opt"][0]))
            a, b = R.get_flow(cam, stat, dyn, bg, d)[2], R.get_flow(pin, stat, dyn, bg, d)[2]
            ref = fx["out_latent_img"]
        else:
            a, b = R.render(cam, stat, dyn, bg)["render"], R.render(pin, stat, dyn, bg)["render"]
            ref = None if bool(fx["opt"][2]) else fx["out_render"]   # (a delta-exposure fixture: another instant)
    assert torch.equal(a, b)
    if ref is not None:
        assert float((a - torch.from_numpy(ref)).abs().max()) <= 3e-5   # (tests/test_oracle_cpu.py's figure for this image)


def test_ray_selection_takes_the_map_arm():
    import mobgs_amd.gaussian_renderer as GR
    pin, *_ = _fixture_camera("render_lean")
    cam, _ = C.ref_camera(pin)
    assert GR.INKERNEL_RAYS
    assert GR._rays_of(cam) is cam.cam_ray
    assert GR._rays_of_many([cam, cam]) is None and GR._rays_of_many([pin, cam]) is None
    assert isinstance(GR._rays_of(pin), tuple) and GR._rays_of_many([pin, pin]) is not None
    GR.INKERNEL_RAYS = False
    try:
        assert GR._rays_of(pin) is pin.cam_ray and GR._rays_of_many([pin, pin]) is None
    finally:
        GR.INKERNEL_RAYS = True


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("size", C.SIZES)
def test_filter_caps_hold_on_the_oracles_alone(size, mode, capsys):
    case = C.oracle_case(size, mode)
    with capsys.disabled():
        print()
        C.report("oracles", case)
    assert case["excluded"] <= C.CAP_ORACLE, case["excluded"]
    # the per-pair bounds the margins are multiples of really bound the fp32 oracle's own error, on every pair
    assert case["worst_a"] <= 1.0 and case["worst_t"] <= 1.0, (case["worst_a"], case["worst_t"])
    assert float(case["map64"].abs().max()) > 0 and float(case["c2w64"].abs().max()) > 0
    # the fp32 oracle meets its own yardstick (trivially: the allowed distance is 3 x its gap) and the gap is rounding
    assert case["gap_map"] <= 1e-5 * float(case["map64"].abs().max())
    assert case["gap_c2w"] <= 1e-5 * float(case["c2w64"].abs().max())
