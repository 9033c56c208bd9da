"""The render entry points one level above the kernels: the ray-map camera arm (any object with the reference camera's
read-side attributes, tests/refcam_cases.RefCamera), the Python host bodies at the entry points that never ran them, and
the two A/B switches no test switched (LAZY_AUX, BATCH_FLOW_EXPOSURES).

Tolerances: the reference-fixture comparisons are the shared checkers of tests/helpers.py and tests/test_gpu_config4.py
(the numbers of the pinhole tests); batched-against-separate gradients use the yardsticks of tests/test_gpu_render_many.py,
tests/test_gpu_render_parity.py and tests/test_gpu_zero_gate.py, imported; gradients against float64 follow DESIGN.md 3a
(refcam_cases.tolerance: 3 x the fp32 oracle's own distance, at least 8 x 2^-24 of the largest entry)."""
import contextlib

import pytest
import torch

import refcam_cases as C
from helpers import (check_get_flow_fixture_outputs, check_get_flow_static_fixture_outputs, check_render_fixture_gradients,
                     check_render_fixture_outputs, check_separate_calls_gradients, leaf_map, load, render_fixture_options,
                     render_loss, same_bits, scene_from_fixture)
from test_gpu_config4 import blce_mode, blurry_view_run, check_blurry_view_fixture  # noqa: F401  (blce_mode: a fixture)
from test_gpu_render_many import assert_grads_of_the_batch
from test_gpu_zero_gate import assert_grads_of_shared_mid_state

pytestmark = pytest.mark.gpu

NINE = C.NINE


@contextlib.contextmanager
def switches(fast=None, inkernel_rays=None, lazy_aux=None, batch_flow=None):
    """Module switches for the body, every one put back afterwards."""
    import mobgs_amd.gaussian_renderer as GR
    from mobgs_amd import _fast
    saved = (GR.INKERNEL_RAYS, GR.LAZY_AUX, GR.BATCH_FLOW_EXPOSURES)
    try:
        if fast is not None:
            _fast.reset(bool(fast))
            assert (_fast.get() is not None) == bool(fast), _fast.load_error
        if inkernel_rays is not None:
            GR.INKERNEL_RAYS = inkernel_rays
        if lazy_aux is not None:
            GR.LAZY_AUX = lazy_aux
        if batch_flow is not None:
            GR.BATCH_FLOW_EXPOSURES = batch_flow
        GR.invalidate_flow_cache()
        yield GR
    finally:
        GR.INKERNEL_RAYS, GR.LAZY_AUX, GR.BATCH_FLOW_EXPOSURES = saved
        _fast.reset(None)
        GR.invalidate_flow_cache()


def _tensors(d):
    return {k: v.detach().clone() for k, v in d.items() if torch.is_tensor(v)}


def _grads(stat, dyn, **extra):
    g = {k: t.grad.detach().clone() for k, t in leaf_map(stat, dyn).items() if t.grad is not None}
    g.update({k: v.detach().clone() for k, v in extra.items() if v is not None})
    return g


def _assert_same_bits(a, b, what):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k in a:
        assert same_bits(a[k], b[k]), f"{what}: {k} differs"


# ---- 1. the reference's fixtures through the ray-map arm -----------------------------------------------------------------
def _fixture_render(fx, dev, as_refcam):
    from mobgs_amd.gaussian_renderer import render
    pin, stat, dyn, bg, _ = scene_from_fixture(fx, device=dev)
    cam = C.ref_camera(pin)[0] if as_refcam else pin
    kw, w2c_leaf = render_fixture_options(fx, dev)
    out = render(cam, stat, dyn, None, bg, **kw)
    check_render_fixture_outputs(out, fx, dyn)
    render_loss(out, fx, dev).backward()
    check_render_fixture_gradients(out, fx, stat, dyn, w2c_leaf)
    return _tensors(out), _grads(stat, dyn, w2c=None if w2c_leaf is None else w2c_leaf.grad,
                                 viewspace=out["viewspace_points"].grad)


@pytest.mark.parametrize("fast", [True, False], ids=["extension", "python"])
@pytest.mark.parametrize("name", ["render_lean", "render_train", "render_train_delta_flow"])
def test_render_fixture_through_the_ray_map_arm(hip_device, kernel_selection, name, fast):
    """The fixtures were produced by the reference with its own cam_ray, so the pinhole tests' numbers apply unchanged.
    The arm is asserted from rendering.path_log; a PinholeCamera under INKERNEL_RAYS = False is the same arm reached
    another way and gives the same bits."""
    from mobgs_amd import rendering
    fx = load(name)
    with switches(fast=fast):
        out_a, grad_a = _fixture_render(fx, hip_device, as_refcam=True)
        log = list(rendering.path_log)
        kernel_selection.check()
        assert [e for e in log if e["dir"] == "fwd"] and not any(e.get("decode") for e in log if e["dir"] == "fwd"), log
        assert not any(e.get("decode_bwd") for e in log), log
        prep = [e for e in log if e["dir"] == "prep"]
        assert len(prep) == 1
        if name == "render_lean":   # the ray map changes the decoder's arm, not the prep's
            assert prep[0]["fused"] == bool(fast)
        with switches(fast=fast, inkernel_rays=False):
            out_b, grad_b = _fixture_render(fx, hip_device, as_refcam=False)
        assert not any(e.get("decode") for e in rendering.path_log if e["dir"] == "fwd")
    _assert_same_bits(out_a, out_b, "outputs")
    _assert_same_bits(grad_a, grad_b, "gradients")


@pytest.mark.parametrize("fast", [True, False], ids=["extension", "python"])
def test_get_flow_fixture_through_the_ray_map_arm(hip_device, kernel_selection, fast):
    from mobgs_amd import rendering
    from mobgs_amd.camera import PinholeCamera
    from mobgs_amd.gaussian_renderer import get_flow, get_flow_static
    fx = load("get_flow")
    dev = hip_device

    def run(as_refcam):
        pin, stat, dyn, bg, _ = scene_from_fixture(fx, device=dev, requires_grad=False)
        pin_b = PinholeCamera(pin.image_width, pin.image_height, pin.K, torch.from_numpy(fx["in_w2c_b"]), pin.time,
                              pin.max_time, device=dev)
        cam, cam_b = (C.ref_camera(pin)[0], C.ref_camera(pin_b)[0]) if as_refcam else (pin, pin_b)
        with torch.no_grad():
            maps = get_flow(cam, stat, dyn, None, bg, delta_exposure=torch.tensor(float(fx["opt"][0]), device=dev))
            f2d, fimg = get_flow_static(cam, cam_b, cam, stat, dyn, None, bg)
        check_get_flow_fixture_outputs(fx, *maps)
        check_get_flow_static_fixture_outputs(fx, f2d, fimg)
        return dict(zip(("e2m", "m2e", "img", "alpha", "f2d", "fimg"), [t.clone() for t in maps] + [f2d, fimg]))

    with switches(fast=fast):
        a = run(True)
        kernel_selection.check(need_bwd=False)
        assert not any(e.get("decode") for e in rendering.path_log if e["dir"] == "fwd")
        with switches(fast=fast, inkernel_rays=False):
            b = run(False)
    _assert_same_bits(a, b, "get_flow / get_flow_static")


# ---- 2. the gradient into the map, and through it into a pose, against float64 ------------------------------------------
@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("size", C.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_map_and_pose_gradients_match_float64(hip_device, size, mode, capsys):
    """render() with a RefCamera whose map is a leaf (per-pixel gradient, decision and kink pixels left out by the oracles'
    filter of tests/refcam_cases.py) and with one whose map is built from a c2w leaf (the twelve numbers of c2w.grad: sums
    over all pixels, no exclusion), against oracle/render_torch.render in float64 on the CPU; c2w.grad also against the
    in-kernel arm's g_c2w for the same pose.  Train mode: three decodes add into the one map."""
    from mobgs_amd.gaussian_renderer import render
    dev = hip_device
    W, H = size
    train = mode == "train"
    case = C.oracle_case(size, mode)
    cot = C.cotangents(W, H)
    bg = torch.zeros(9, device=dev)

    def run(make_camera):
        scam, stat, dyn = C.scene(dev, W, H)
        cam, leaf = make_camera(C.pinhole(scam, W, H, dev))
        out = render(cam, stat, dyn, None, bg, get_static=train, get_dynamic=train)
        C.loss_of(out, cot, train).backward()
        return leaf.grad.detach().cpu().double()

    def inkernel(pin):
        pin.ray_c2w = pin.ray_c2w.detach().clone().requires_grad_(True)
        return pin, pin.ray_c2w

    v_map = run(lambda pin: C.ref_camera(pin, ray_leaf=True))[0].permute(1, 2, 0).reshape(H * W, 6)
    g_map_arm = run(lambda pin: C.ref_camera(pin, pose_leaf=True))
    g_kernel = run(inkernel)
    keep = case["keep"]
    obs_map = float((v_map - case["map64"])[keep].abs().max())
    obs_c2w = float((g_map_arm - case["c2w64"]).abs().max())
    obs_kernel = float((g_kernel - case["c2w64"]).abs().max())
    obs_arms = float((g_map_arm - g_kernel).abs().max())
    with capsys.disabled():
        print()
        C.report("MI355X", case, obs_map, obs_c2w)
        left_out = float((v_map - case["map64"])[~keep].abs().max()) if bool((~keep).any()) else 0.0
        print(f"[refcam]   in-kernel arm's g_c2w against float64: {obs_kernel:.3e}; the two arms apart: {obs_arms:.3e} "
              f"(allowed {2 * case['tol_c2w']:.3e}); worst left-out pixel {left_out:.3e}")
    assert case["excluded"] <= C.CAP_EXCLUDED
    assert obs_map <= case["tol_map"], (obs_map, case["tol_map"])
    assert obs_c2w <= case["tol_c2w"], (obs_c2w, case["tol_c2w"])
    assert obs_kernel <= case["tol_c2w"], (obs_kernel, case["tol_c2w"])
    assert obs_arms <= 2 * case["tol_c2w"]   # (both within tol of the same float64 numbers)


# ---- 3. render_many with three RefCameras --------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False], ids=["extension", "python"])
def test_render_many_of_reference_cameras_equals_separate_renders(hip_device, fast):
    """_rays_of_many() returns None for them: the batch is composited once and decoded image by image.  Images and depths
    bit-identical to three render() calls (render_many's docstring), gradients to the order of the sums."""
    from mobgs_amd import rendering
    from mobgs_amd.gaussian_renderer import render, render_many, viewspace_grad
    dev = hip_device
    W, H = 50, 37
    deltas = (None, 0.25, -0.3)
    g = torch.Generator().manual_seed(1)
    v3 = [torch.randn(3, H, W, generator=g).to(dev) for _ in deltas]
    v1 = [torch.randn(1, H, W, generator=g).to(dev) for _ in deltas]
    bg = torch.zeros(9, device=dev)

    def run(many):
        scam, stat, dyn = C.scene(dev, W, H)
        cams = [C.ref_camera(C.pinhole(scam, W, H, dev, k))[0] for k in range(3)]
        if many:
            outs = render_many(cams, stat, dyn, None, bg, deltas)
        else:
            outs = [render(c, stat, dyn, None, bg, delta_exposure=d) for c, d in zip(cams, deltas)]
        torch.autograd.backward([o["render"] for o in outs] + [o["depth"] for o in outs], v3 + v1)
        return ([(o["render"].detach().clone(), o["depth"].detach().clone(), o["radii"].clone()) for o in outs],
                _grads(stat, dyn), [viewspace_grad(o).clone() for o in outs])

    saved = rendering.path_log
    rendering.path_log = []
    try:
        with switches(fast=fast):
            ref_out, ref_g, ref_vs = run(False)
            del rendering.path_log[:]
            out, got_g, got_vs = run(True)
            assert not any(e.get("decode") for e in rendering.path_log if e["dir"] == "fwd"), rendering.path_log
    finally:
        rendering.path_log = saved
    for k, ((r, d, rad), (r0, d0, rad0)) in enumerate(zip(out, ref_out)):
        assert torch.equal(rad, rad0) and torch.equal(r, r0) and torch.equal(d, d0), f"sub-frame {k}"
    assert set(got_g) == set(ref_g) and len(ref_g) >= 13
    for k in ref_g:
        assert_grads_of_the_batch(got_g[k], ref_g[k], f"leaf {k}")
    for k, (a, b) in enumerate(zip(got_vs, ref_vs)):
        assert_grads_of_the_batch(a, b, f"viewspace gradient of sub-frame {k}")


# ---- 4. get_flow / get_flow_many ------------------------------------------------------------------------------------------
def _flow_run(dev, W, H, ws, many, pose_leaf=False):
    import mobgs_amd.gaussian_renderer as GR
    scam, stat, dyn = C.scene(dev, W, H)
    cam, c2w = C.ref_camera(C.pinhole(scam, W, H, dev), pose_leaf=pose_leaf)
    bg = torch.zeros(9, device=dev)
    if many:
        outs = GR.get_flow_many(cam, stat, dyn, None, bg, NINE)
    else:
        outs = [GR.get_flow(cam, stat, dyn, None, bg, delta_exposure=d) for d in NINE]
    loss = sum((t * w).sum() for o, row in zip(outs, ws) for t, w in zip(o, row))
    loss.backward()
    return [t.detach().clone() for o in outs for t in o], _grads(stat, dyn), (c2w.grad.clone() if pose_leaf else None)


@pytest.mark.parametrize("batch", [True, False], ids=["batched-exposures", "exposure-by-exposure"])
def test_get_flow_many_with_a_reference_camera(hip_device, batch, capsys):
    """Nine exposures through a RefCamera, BATCH_FLOW_EXPOSURES on and off: the four maps of every call are bit-identical to
    the single get_flow() calls (get_flow_many's docstring), leaf gradients of a loss that reads all of them equal the
    per-call loop's up to summation order.

    Then the same with a map that carries a graph into a pose (pose_leaf).  Before this test the batched-exposure path
    raised NotImplementedError there (ops._decode_args refuses a shared map that needs a gradient, and so does the kernel's
    launcher).  The fix chosen: gaussian_renderer._get_flow_exposures gives every one of the G images its own copy of the
    map -- expand + contiguous, as ops._decode_args does for a shared c2w -- and autograd sums the G map gradients.
    c2w.grad against the per-call loop, and both against float64: DESIGN.md 3a from the two oracles' c2w gradient of the
    same nine-call loss (refcam_cases.oracle_flow_pose_case), at 50 x 37."""
    dev = hip_device
    W, H = C.SIZES[1]
    ws = [[w.to(dev) for w in row] for row in C.flow_weights(W, H)]
    with switches(batch_flow=batch):
        ref_maps, ref_g, _ = _flow_run(dev, W, H, ws, many=False)
        maps, got_g, _ = _flow_run(dev, W, H, ws, many=True)
        ref_maps_p, _, ref_c2w = _flow_run(dev, W, H, ws, many=False, pose_leaf=True)
        maps_p, _, got_c2w = _flow_run(dev, W, H, ws, many=True, pose_leaf=True)   # must not raise
    assert len(maps) == 36
    for i, (a, b) in enumerate(zip(maps, ref_maps)):
        assert torch.equal(a, b), f"map {i % 4} of call {i // 4}"
    for i, (a, b) in enumerate(zip(maps_p, ref_maps_p)):
        assert torch.equal(a, b) and torch.equal(a, maps[i]), f"pose_leaf: map {i % 4} of call {i // 4}"
    check_separate_calls_gradients(got_g, ref_g)
    names = sorted(ref_g)
    assert_grads_of_shared_mid_state([got_g[k] for k in names], [ref_g[k] for k in names])
    case = C.oracle_flow_pose_case((W, H))
    ref64 = case["c2w64"]
    observed = float((got_c2w - ref_c2w).abs().max())
    many64, loop64 = (float((t.cpu().double() - ref64).abs().max()) for t in (got_c2w, ref_c2w))
    with capsys.disabled():
        print(f"\n[refcam] get_flow_many {'batched' if batch else 'per exposure'} {W}x{H}: c2w.grad against the per-call "
              f"loop: observed {observed:.3e}; against float64: get_flow_many {many64:.3e}, the loop {loop64:.3e}; fp32 "
              f"oracle {case['gap']:.3e}, allowed {case['tol']:.3e} (largest {float(ref64.abs().max()):.3e})")
    assert float(ref_c2w.abs().max()) > 0
    assert observed <= case["tol"], (observed, case["tol"])
    assert many64 <= case["tol"] and loop64 <= case["tol"], (many64, loop64, case["tol"])


# ---- 5. a blurry view through BLCE with ray-map latent cameras -----------------------------------------------------------
@pytest.mark.parametrize("blce_mode", ["fused", "graph"], indirect=True)
def test_blurry_view_k9_blce_with_ray_map_latent_cameras(hip_device, blce_mode):
    """tests/golden/blurry_view.npz with INKERNEL_RAYS off: the nine cameras hand over their maps, so the pose gradient
    reaches BLCE's parameters through v_rays and torch's ray construction instead of g_c2w.  Same assertions and
    tolerances as the in-kernel test (tests/test_gpu_config4.py); render_many against render() for the latent frames."""
    from mobgs_amd import rendering
    dev = hip_device
    saved = rendering.path_log
    rendering.path_log = []
    try:
        with switches(inkernel_rays=False):
            fx, cam, stat, dyn, kern, idx, pred, mid = blurry_view_run(dev)
            assert not any(e.get("decode") for e in rendering.path_log if e["dir"] == "fwd")
            check_blurry_view_fixture(fx, dev, cam, stat, dyn, kern, pred, mid)
            *_, pred_one_by_one, _ = blurry_view_run(dev, batched_latent=False)
    finally:
        rendering.path_log = saved
    g = kern._graphed.get(idx)
    assert (g is not None and g is not False) if blce_mode == "graph" else g is None
    assert torch.equal(pred, pred_one_by_one), "render_many and nine render() calls must give the same prediction"


# ---- 6. LAZY_AUX ----------------------------------------------------------------------------------------------------------
def test_lazy_aux_off_changes_no_bit(hip_device):
    """render_train with the auxiliary images computed eagerly: every key of the result and every gradient of the fixture's
    loss has the bits of the default (lazy) run."""
    from mobgs_amd.gaussian_renderer import render
    fx = load("render_train")
    res = {}
    for lazy in (True, False):
        with switches(lazy_aux=lazy) as GR:
            cam, stat, dyn, bg, _ = scene_from_fixture(fx, device=hip_device)
            kw, _ = render_fixture_options(fx, hip_device)
            out = render(cam, stat, dyn, None, bg, **kw)
            pending = [k for k in out.keys() if dict.__getitem__(out, k) is GR._PENDING]
            assert ("s_render" in pending) == lazy and ("visibility_filter" in pending) == lazy, pending
            render_loss(out, fx, hip_device).backward()
            res[lazy] = (_tensors(out), _grads(stat, dyn, viewspace=out["viewspace_points"].grad))
    assert len(res[True][0]) == len({k for k in fx if k.startswith("out_")})
    _assert_same_bits(res[True][0], res[False][0], "outputs")
    _assert_same_bits(res[True][1], res[False][1], "gradients")


# ---- 7. the Python host bodies at the entry points that never ran them --------------------------------------------------
def _entry(name, dev):
    """One entry point with PinholeCameras on the 80 x 64 scene -> {name: tensor} of its outputs and gradients."""
    import mobgs_amd.gaussian_renderer as GR
    W, H = C.SIZES[0]
    scam, stat, dyn = C.scene(dev, W, H)
    cams = [C.pinhole(scam, W, H, dev, k) for k in range(5)]
    bg = torch.zeros(9, device=dev)
    g = torch.Generator().manual_seed(9)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)   # noqa: E731
    res = {}
    if name == "render_many":
        outs = GR.render_many(cams[:3], stat, dyn, None, bg, (None, 0.25, -0.3))
        torch.autograd.backward([o["render"] for o in outs] + [o["depth"] for o in outs],
                                [rnd(3, H, W) for _ in outs] + [rnd(1, H, W) for _ in outs])
        for k, o in enumerate(outs):
            res.update({f"render{k}": o["render"], f"depth{k}": o["depth"], f"radii{k}": o["radii"]})
        res["viewspace"] = outs[0]["viewspace_points"].grad
    elif name in ("get_flow", "get_flow_many"):
        deltas = NINE if name == "get_flow_many" else [0.25]
        outs = GR.get_flow_many(cams[0], stat, dyn, None, bg, deltas) if name == "get_flow_many" else \
            [GR.get_flow(cams[0], stat, dyn, None, bg, delta_exposure=deltas[0])]
        sum((t * rnd(*t.shape)).sum() for o in outs for t in o).backward()
        res.update({f"map{i}_{j}": t for i, o in enumerate(outs) for j, t in enumerate(o)})
    elif name == "get_flow_static_pair":
        a, b = GR.get_flow_static_pair(cams[0], cams[1], cams[2], cams[3], cams[4], stat, dyn, None, bg)
        return {"flow_a": a.clone(), "flow_b": b.clone()}
    else:   # train-mode render with an exposure offset and the original-time flow
        out = GR.render(cams[0], stat, dyn, None, bg, get_static=True, get_dynamic=True,
                        delta_exposure=torch.tensor(0.25, device=dev), get_flow=True)
        keys = ("render", "depth", "s_render", "d_render", "d_alpha", "s_alpha", "d_depth", "ori_flow", "ori_coord_map")
        sum((out[k] * rnd(*out[k].shape)).sum() for k in keys).backward()
        res.update(_tensors(out))
        res["viewspace"] = out["viewspace_points"].grad
    res = {k: v.detach().clone() for k, v in res.items()}
    res.update({"grad_" + k: v for k, v in _grads(stat, dyn).items()})
    return res


@pytest.mark.parametrize("name", ["render_many", "get_flow", "get_flow_many", "get_flow_static_pair", "render_train_flow"])
def test_python_bodies_equal_the_extension_at_every_entry_point(hip_device, name):
    """Both host bodies end in the same C-ABI calls: outputs and gradients bit for bit, as tests/test_gpu_fastpath.py asserts
    for render()."""
    with switches(fast=True):
        a = _entry(name, hip_device)
    with switches(fast=False):
        b = _entry(name, hip_device)
    assert len(a) > 1 and all(torch.isfinite(v.float()).all() for v in a.values())
    if name != "get_flow_static_pair":
        assert any(k.startswith("grad_") and float(v.abs().max()) > 0 for k, v in a.items())
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
