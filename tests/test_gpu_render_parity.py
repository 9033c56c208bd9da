"""GPU parity of the render API (B1) against the golden fixtures produced by the reference's own
render()/get_flow()/interpolate_cubic_hermite()/Sandwich (tests/golden/make_golden.py)."""
import numpy as np
import pytest
import torch

from helpers import (check_get_flow_fixture_outputs, check_get_flow_static_fixture_outputs,
                     check_render_fixture_gradients, check_render_fixture_outputs, check_separate_calls_gradients, close,
                     leaf_map, load, render_fixture_options, render_loss, scene_from_fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["render_lean", "render_train", "render_train_delta_flow"])
def test_render_matches_reference_fixture(hip_device, name, kernel_selection):
    """Twice: under the library's default selection for the fixture's small grid (four waves per tile, matrix-pipe
    backward) and under the BENCHMARK's selection (conftest.kernel_selection "headline": one wave per tile
    raster_fwd_blocks<10, ., DECODE> with the decoder epilogue, quadrant raster_bwd_kernel<10> with the static-row blend
    body, project_fwd<PREP> / project_bwd<PREPB>) -- asserted from rendering.path_log, not assumed."""
    from mobgs_amd.gaussian_renderer import render
    fx = load(name)
    cam, stat, dyn, bg, w2c = scene_from_fixture(fx, device=hip_device)
    get_static, get_dynamic, has_delta, delta, get_flow, use_w2c = fx["opt"]
    kw, w2c_leaf = render_fixture_options(fx, hip_device)
    out = render(cam, stat, dyn, None, bg, **kw)
    # (the per-key comparison with its derived flip bounds, and the gradient loop: helpers, shared with the ray-map arm's
    # tests in tests/test_gpu_reference_cameras.py)
    check_render_fixture_outputs(out, fx, dyn)
    render_loss(out, fx, hip_device).backward()
    check_render_fixture_gradients(out, fx, stat, dyn, w2c_leaf)
    ps = kernel_selection.check()
    from mobgs_amd import _fast, rendering
    if _fast.get() is not None and not (has_delta and get_flow):
        # the whole-set pass: prep inside the projection kernels, decoder inside the forward compositor
        assert any(e.get("decode") for e in ps if e["dir"] == "fwd" and not e["class_filter"]), ps
        assert [e for e in rendering.path_log if e["dir"] == "prep"][-1]["fused"], "fused prep -> project path not taken"
    if rendering.STATIC_ROWS:
        ns = stat.get_xyz.shape[0]
        assert any(e["dir"] == "bwd" and e.get("static_rows") == ns for e in ps), ps


def test_get_flow_matches_reference_fixture(hip_device, kernel_selection):
    from mobgs_amd.camera import PinholeCamera
    from mobgs_amd.gaussian_renderer import get_flow, get_flow_static
    fx = load("get_flow")
    cam, stat, dyn, bg, w2c = scene_from_fixture(fx, device=hip_device, requires_grad=False)
    with torch.no_grad():
        e2m, m2e, img, alpha = get_flow(cam, stat, dyn, None, bg,
                                        delta_exposure=torch.tensor(float(fx["opt"][0]), device=hip_device))
    check_get_flow_fixture_outputs(fx, e2m, m2e, img, alpha)
    cam_b = PinholeCamera(cam.image_width, cam.image_height, cam.K, torch.from_numpy(fx["in_w2c_b"]), cam.time,
                          cam.max_time, device=hip_device)
    with torch.no_grad():
        f2d, fimg = get_flow_static(cam, cam_b, cam, stat, dyn, None, bg)
    check_get_flow_static_fixture_outputs(fx, f2d, fimg)
    kernel_selection.check(need_bwd=False)


def test_get_flow_gradients_match_reference_fixture(hip_device, kernel_selection):
    """get_flow() / get_flow_static() forward AND backward against the reference's own autograd result (the only
    reference check the 12-channel compositor backward, raster_bwd<12>, gets) -- under both kernel selections
    (conftest.kernel_selection: "headline" = one wave per tile, quadrant backward with the static-row blend body)."""
    from test_oracle_cpu import _flow_grad_check
    from mobgs_amd.gaussian_renderer import get_flow, get_flow_static
    _flow_grad_check(load("get_flow_grad"), lambda cam, s, d, bg, dl: get_flow(cam, s, d, None, bg, delta_exposure=dl),
                     lambda a, b, c, s, d, bg: get_flow_static(a, b, c, s, d, None, bg), hip_device, 2e-3, 2e-4,
                     flip={"flip_frac": 2e-4, "flip_atol": "derived"})
    ps = kernel_selection.check()
    assert any(e["D"] == 12 and e["dir"] == "bwd" for e in ps), ps


def test_hermite_wrapper_matches_reference_fixture(hip_device):
    from mobgs_amd.gaussian_renderer import interpolate_cubic_hermite
    fx = load("hermite")
    ncp = torch.from_numpy(fx["ncp"]).to(hip_device)
    cot = torch.from_numpy(fx["cot"]).to(hip_device)
    for i, t in enumerate(fx["ts"]):
        ctrl = torch.from_numpy(fx["control"]).to(hip_device).requires_grad_(True)
        n = ctrl.shape[0]
        tt = torch.tensor(float(t), dtype=torch.float32, device=hip_device)[None, None].expand(n, 3, 1)
        out = interpolate_cubic_hermite(ctrl.permute(0, 2, 1), tt, ncp)
        close(out, fx["out"][i], 2e-5, 2e-5, f"hermite(t={t})")
        (out * cot).sum().backward()
        close(ctrl.grad, fx["grad"][i], 2e-5, 2e-5, f"hermite grad(t={t})")


def test_sandwich_module_matches_reference_fixture(hip_device):
    from mobgs_amd.helper_model import Sandwich
    fx = load("sandwich")
    dec = Sandwich(9, 3).to(hip_device)
    with torch.no_grad():
        dec.mlp1.weight.copy_(torch.from_numpy(fx["w1"]))
        dec.mlp2.weight.copy_(torch.from_numpy(fx["w2"]))
    feat = torch.from_numpy(fx["feat"]).to(hip_device).requires_grad_(True)
    rays = torch.from_numpy(fx["rays"]).to(hip_device).requires_grad_(True)
    out = dec(feat, rays)
    close(out, fx["out"], 1e-5, 1e-6, "sandwich")
    (out * torch.from_numpy(fx["cot"]).to(hip_device)).sum().backward()
    close(feat.grad, fx["grad_feat"], 1e-4, 1e-6, "grad feat")
    close(rays.grad, fx["grad_rays"], 1e-4, 1e-6, "grad rays")
    close(dec.mlp1.weight.grad, fx["grad_w1"], 1e-4, 1e-5, "grad w1")
    close(dec.mlp2.weight.grad, fx["grad_w2"], 1e-4, 1e-5, "grad w2")


@pytest.mark.parametrize("class_passes", [True, False])
def test_layered_render_equals_separate_passes(hip_device, class_passes):
    """Train-mode render(): the static-only / dynamic-only images from the shared lists -- two class-restricted
    passes of the single-set compositor (default) or the generic 3-layer kernel -- reproduce the five separate
    rasterizations: images bit for bit (same per-pixel operation sequence), gradients up to summation order."""
    import mobgs_amd.gaussian_renderer as GR
    from mobgs_amd import rendering
    fx = load("render_train")
    res = {}
    for fuse in (False, True):
        GR.FUSE_LAYERS = fuse
        rendering.CLASS_PASSES = class_passes
        try:
            cam, stat, dyn, bg, _ = scene_from_fixture(fx, device=hip_device)
            out = GR.render(cam, stat, dyn, None, bg, get_static=True, get_dynamic=True)
            render_loss(out, fx, hip_device).backward()
            res[fuse] = ({k: v.detach().cpu() for k, v in out.items() if isinstance(v, torch.Tensor)},
                         {k: t.grad.cpu() for k, t in leaf_map(stat, dyn).items() if t.grad is not None},
                         out["viewspace_points"].grad.cpu())
        finally:
            GR.FUSE_LAYERS = True
            rendering.CLASS_PASSES = True
    for k in ("render", "depth", "s_render", "d_render", "d_depth", "radii"):
        assert torch.equal(res[True][0][k], res[False][0][k]), f"{k} differs"
    for k in ("s_alpha", "d_alpha"):  # (1 - T) + T bg  vs  sum_i w_i + T bg: telescoping sum, fp32 rounding
        close(res[True][0][k], res[False][0][k], 0, 2e-6, k)
    for k, g in res[False][1].items():
        close(res[True][1][k], g, 1e-4, 1e-5 * float(g.abs().max()) + 1e-8, f"grad[{k}]")
    g = res[False][2]
    close(res[True][2], g, 1e-4, 1e-5 * float(g.abs().max()), "viewspace_points.grad")


def test_auxiliary_outputs_are_lazy(hip_device):
    """render(get_static=True, get_dynamic=True) as the 8 latent sub-frame renders of train.py:512-516 use it
    (only "render"/"depth" are read): the static / dynamic images are never composited."""
    import mobgs_amd.gaussian_renderer as GR
    from mobgs_amd import profiler
    fx = load("render_train")
    cam, stat, dyn, bg, _ = scene_from_fixture(fx, device=hip_device)
    profiler.enable(True)
    try:
        out = GR.render(cam, stat, dyn, None, bg, get_static=True, get_dynamic=True)
        (out["render"].sum() + out["depth"].sum()).backward()
        assert "raster_class_fwd" not in profiler.summary() and "raster_layers_fwd" not in profiler.summary()
        assert dict.__getitem__(out, "s_render") is GR._PENDING and "s_render" in out and len(out) == 22
        s_render = out["s_render"]  # first access: one call (two class-restricted passes) produces all five images
        assert profiler.summary()["raster_class_fwd"]["calls"] == 1
        assert torch.is_tensor(out["d_alpha"]) and torch.is_tensor(out["d_render"]) and torch.is_tensor(out["s_alpha"])
        assert profiler.summary()["raster_class_fwd"]["calls"] == 1
        # one blend step through the decoder, derived (helpers.decoded_flip_bound), for <= 2e-4 of the elements -- the
        # allowance of test_render_matches_reference_fixture (was a flat 0.01 for 2e-3 of them)
        from helpers import decoded_flip_bound
        fb = decoded_flip_bound(dyn.rgbdecoder, float(np.abs(fx["out_colors_precomp_final"]).max()))
        close(s_render, fx["out_s_render"], 0, 3e-5, "s_render", flip_frac=2e-4, flip_atol=fb)
    finally:
        profiler.enable(False)


def test_inkernel_rays_match_ray_map_and_reach_the_pose(hip_device):
    """Decoder with in-kernel pinhole rays == decoder fed the [1,6,H,W] map; the ray gradient reaches c2w."""
    from mobgs_amd.camera import PinholeCamera
    from mobgs_amd.ops import decode
    H, W = 40, 56
    g = torch.Generator().manual_seed(3)
    K = torch.tensor([[60.0, 0, 27.5], [0, 58.0, 20.5], [0, 0, 1]])
    w2c = torch.eye(4)
    a = 0.2
    w2c[:3, :3] = torch.tensor([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]])
    w2c[:3, 3] = torch.tensor([0.3, -0.1, 0.4])
    feat = torch.randn(H, W, 10, generator=g).to(hip_device)
    alphas = torch.rand(H, W, generator=g).to(hip_device)
    w1 = torch.randn(6, 12, generator=g).to(hip_device)
    w2 = torch.randn(3, 6, generator=g).to(hip_device)
    cot = torch.randn(3, H, W, generator=g).to(hip_device)

    c2w = torch.inverse(w2c)[:3, :]
    c2w_a = c2w.to(hip_device).requires_grad_(True)
    rays = PinholeCamera.build_cam_ray_c2w(W, H, K.to(hip_device), c2w_a)
    rgb_map, d_map = decode(feat, alphas, rays, w1, w2, True)
    (rgb_map * cot).sum().backward()

    c2w_b = c2w.to(hip_device).requires_grad_(True)
    intr = torch.stack([K[0, 0], K[1, 1], K[0, 2], K[1, 2]]).to(hip_device)
    rgb_k, d_k = decode(feat, alphas, (intr, c2w_b), w1, w2, True)
    (rgb_k * cot).sum().backward()
    close(rgb_k, rgb_map, 0, 2e-6, "rgb")
    assert torch.equal(d_k, d_map)
    gref = c2w_a.grad
    close(c2w_b.grad, gref, 1e-3, 1e-4 * float(gref.abs().max()), "grad c2w through the rays")
    assert float(gref.abs().max()) > 0
    # and the map itself equals the w2c-based construction the fixtures were generated with
    close(rays, PinholeCamera.build_cam_ray(W, H, K.to(hip_device), w2c.to(hip_device)), 0, 1e-6, "ray map")


import math  # noqa: E402


def test_get_flow_many_equals_separate_calls(hip_device):
    """get_flow_many shares the mid-exposure projection / lists between the calls: outputs bit-identical to separate
    get_flow calls, summed gradients equal up to fp32 accumulation order."""
    from mobgs_amd.gaussian_renderer import get_flow, get_flow_many
    fx = load("get_flow")
    deltas = [(k - 4) / 4.0 for k in range(9)]  # train.py:571-573; nine calls: one 16-channel walk + one 2-channel
    res = {}
    for many in (False, True):
        cam, stat, dyn, bg, _ = scene_from_fixture(fx, device=hip_device)
        if many:
            outs = get_flow_many(cam, stat, dyn, None, bg, deltas)
        else:
            outs = [get_flow(cam, stat, dyn, None, bg, delta_exposure=d) for d in deltas]
        loss = sum((t * (i + 1)).sum() for i, o in enumerate(outs) for t in o)
        loss.backward()
        res[many] = ([t.detach().cpu() for o in outs for t in o],
                     {k: t.grad.cpu() for k, t in leaf_map(stat, dyn).items() if t.grad is not None})
    for a, b in zip(res[True][0], res[False][0]):
        assert torch.equal(a, b)
    check_separate_calls_gradients(res[True][1], res[False][1])


def test_leaf_grad_sink_equals_autograd_accumulation(hip_device):
    """LeafGradSink: several render() calls back-propagated with their leaf gradients accumulated in-kernel give the
    same .grad as autograd's own accumulation (same sums, same order), also on top of an existing .grad."""
    import mobgs_amd.gaussian_renderer as GR
    from mobgs_amd.ops import LeafGradSink
    fx = load("render_train")
    res = {}
    for sink in (False, True):
        cam, stat, dyn, bg, _ = scene_from_fixture(fx, device=hip_device)
        for rep in range(2):  # second round: .grad already exists
            outs = [GR.render(cam, stat, dyn, None, bg, delta_exposure=d)["render"] for d in (None, 0.2, -0.3)]
            loss = sum((o * (i + 1)).sum() for i, o in enumerate(outs))
            if sink:
                with LeafGradSink(stat, dyn):
                    loss.backward()
            else:
                loss.backward()
        res[sink] = {k: t.grad.cpu() for k, t in leaf_map(stat, dyn).items() if t.grad is not None}
    assert set(res[True]) == set(res[False])
    for k, g in res[False].items():
        close(res[True][k], g, 1e-6, 1e-7 * float(g.abs().max()) + 1e-12, f"grad[{k}]")


def test_train_mode_render_block_walk_equals_quadrant_kernel(hip_device):
    """Regression (round 3, found by scripts/soak_render.py): the static-only and dynamic-only passes of a train-mode
    render() share ONE array of per-entry reach bytes, each pass owning the bytes of its class.  The class-restricted
    block-walk forward used to write (zero) bytes for the OTHER class's entries too, wiping what the first pass had
    left there -- the backward pass of that class then skipped everything and its gradients came out zero.  With the
    block walk on and off, every output and every leaf gradient of a train-mode render must agree bit for bit."""
    import bench as B
    from mobgs_amd import rendering
    from mobgs_amd.gaussian_renderer import render
    dev = hip_device
    W, H = 232, 120
    res = {}
    try:
        for bw in (1, 0):
            rendering.tuning.block_walk = bw
            rendering.tuning.heavy_tile_len = 0   # one wave per tile: the block-walk path on this small grid
            scam, cam, stat, dyn, _ = B.build_scene(dev, 300, 200, W, H, seed=5)
            g = torch.Generator().manual_seed(3)
            v3, v1 = torch.randn(3, H, W, generator=g).to(dev), torch.randn(1, H, W, generator=g).to(dev)
            out = render(cam, stat, dyn, None, torch.zeros(9, device=dev), get_static=True, get_dynamic=True)
            outs = [out[k] for k in ("render", "depth", "s_render", "d_render", "d_alpha", "s_alpha", "d_depth")]
            cots = [v3, v1, v3, v3, v1, v1, v1]
            torch.autograd.backward(outs, cots)
            res[bw] = ([o.detach().clone() for o in outs], [p.grad.clone() for p in B.leaves(stat, dyn)])
    finally:
        rendering.tuning.block_walk = -1
        rendering.tuning.heavy_tile_len = -1
    for i, (a, b) in enumerate(zip(res[1][0], res[0][0])):
        assert torch.equal(a, b), f"output {i}"
    assert float(res[1][1][0].abs().max()) > 0, "the static set must receive a gradient"
    for i, (a, b) in enumerate(zip(res[1][1], res[0][1])):
        assert torch.equal(a, b), f"gradient of leaf {i}"
