"""The Sandwich decoder's kernels against float64: the stand-alone arms (`ops.decode`, `ops.decode_with_channels`:
csrc/decoder.hip) and the fused arms (the epilogue of the forward compositor and the prologue of the backward compositor
with its two weight-gradient reductions: csrc/raster.hip through `SharedProjection.composite_decode`).

Cases, the restatement and the comparison are tests/decoder_cases.py (tests/test_decoder_cases_cpu.py shows from the
restatement alone that each case reaches its edge).  Every pixel is kept away from the six ReLU kinks by the float64
restatement (min |s| >= 2^-10), so fp32 and float64 take the same branch everywhere: every output and every gradient is
compared in full, the 12 (16) pose entries included.  Per tensor:
    max |got - ref64| <= k max |ref32 - ref64| + 2^-23 max |ref64|,  ref32 = the same statements in fp32 on the CPU,
and got == 0 wherever ref64 == 0 exactly (alpha == 0, channels the decoder does not read, channel 9 and the alphas
without a depth cotangent, the fourth pose row).  The fused arms are evaluated on the fp32 image and alphas the
compositing node returned, so the reference is the decoder's alone.

k per tensor family = twice the worst k any tensor of the family needed on an MI355X (all 158 cases, 1255 tensors),
rounded up (docs/MEASUREMENT_LOG.md, "Decoder kernels against float64"); decoder_cases.K holds them:

    family                  worst k needed (case, tensor)                                       k
    outputs                 0.72  (one image, P = 1537, [4,4] pose, rgb)                        2
    per-pixel cotangents    1.61  (one image, P = 1, v_feat)                                    4
    weight gradients        2.12  (one image, P = 64, g_w2)                                     5
    pose gradient           3.58  (fused, 250x170, one wave per tile, first weight set)         8

By arm, worst of any family: one image 2.90 (pose, P = 63), batch 0.91, channels 0.58, sink 0.19, forward grid-stride loop
0.42; fused 3.58 (pose), 1.18 (weights), 0.59 (cotangents of the separate chain on the same inputs), 0.31 (outputs).  No
family came near 8, so the kernels' `__expf` against torch's sigmoid needs no term of its own: rgb needed 0.72 at most.
The pose gradient is a sum of signed terms over all pixels whose result is a small fraction of the terms' magnitudes; what
it needed above 2 are one case of 42 500 pixels summed per tile (3.58; 1.64 with four waves per tile) and cases of 1 and 63
pixels, where kernel error and reference gap are single draws (2.53, 2.90, 2.24); every other pose tensor needed at most 1.9.
"""
import contextlib
from types import SimpleNamespace

import pytest
import torch

import decoder_cases as C

pytestmark = pytest.mark.gpu

K = C.K


@contextlib.contextmanager
def _host_path(host):
    """"extension": the C++ bodies of the autograd nodes (csrc/fastpath.cpp); "ctypes": the Python bodies."""
    from mobgs_amd import _fast
    try:
        _fast.reset(host == "extension")
        assert (_fast.get() is not None) == (host == "extension"), _fast.load_error
        yield
    finally:
        _fast.reset(None)


def _leaf(t, dev, grad=True):
    return t.to(dev).clone().requires_grad_(grad)


def _inputs(case, dev, map_grad=True):
    """The case's tensors on the device in the shapes ops.decode takes: one image without a batch dimension."""
    C_, H, W, CF = case.C, case.H, case.W, case.CF
    lead = (C_,) if C_ > 1 else ()
    t = SimpleNamespace(lead=lead, feat=_leaf(case.feat.reshape(*lead, H, W, CF), dev), alphas=None, rays=None, c2w=None,
                        w1=_leaf(case.w1, dev), w2=_leaf(case.w2, dev))
    if case.has_depth:
        t.alphas = _leaf(case.alphas.reshape(*lead, H, W), dev)
    if case.ray == "map":
        t.rays = _leaf(case.rays.reshape(-1, 6, H, W), dev, map_grad)
        t.src = t.rays
    else:
        intr = case.intr.to(dev) if case.intr.shape[0] > 1 else case.intr[0].to(dev)
        t.c2w = _leaf(case.c2w if (case.c2w.shape[0] == C_ and C_ > 1) else case.c2w[0], dev)
        t.src = (intr, t.c2w)
    t.v_rgb = case.v_rgb.reshape(*lead, 3, H, W).to(dev)
    t.v_depth = case.v_depth.reshape(*lead, H, W).to(dev) if case.v_depth is not None else None
    return t


def _gathered(case, t, rgb, depth):
    """What the kernels returned, shaped as decoder_cases.evaluate shapes its results."""
    C_, P, CF = case.C, case.P, case.CF
    got = {"rgb": rgb.detach().reshape(C_, 3, P), "v_feat": t.feat.grad.reshape(C_, P, CF), "g_w1": t.w1.grad, "g_w2": t.w2.grad}
    if case.has_depth:
        got["depth"] = depth.detach().reshape(C_, P)
        got["v_alphas"] = t.alphas.grad.reshape(C_, P) if t.alphas.grad is not None else None
    if t.rays is not None and t.rays.requires_grad:
        got["v_rays"] = t.rays.grad.reshape(C_, 6, P) if t.rays.grad is not None else None
    if t.c2w is not None:
        got["g_c2w"] = t.c2w.grad.reshape(-1, *case.c2w.shape[-2:]) if t.c2w.grad is not None else None
    return got


def _decode_and_compare(case, ref64, ref32, dev, tag):
    from mobgs_amd.ops import decode
    t = _inputs(case, dev, map_grad=not (case.ray == "map" and case.C > 1 and case.rays.shape[0] == 1))
    rgb, depth = decode(t.feat, t.alphas, t.src, t.w1, t.w2, case.has_depth)
    assert rgb.shape == (*t.lead, 3, case.H, case.W) and (depth is None) == (not case.has_depth)
    outs, cots = [rgb], [t.v_rgb]
    if t.v_depth is not None:
        outs.append(depth)
        cots.append(t.v_depth)
    torch.autograd.backward(outs, cots)
    torch.cuda.synchronize()
    got = _gathered(case, t, rgb, depth)
    return C.compare(case, got, ref64, ref32, K, tag, list(got))


# ---- stand-alone arms --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", C.DEPTH_FORMS, ids=lambda f: f"depth{int(f[0])}-CF{f[1]}-cot{int(f[2])}")
@pytest.mark.parametrize("ray", C.RAY_FORMS)
@pytest.mark.parametrize("P", C.SINGLE_P)
def test_one_image_matches_float64(hip_device, P, ray, form):
    """Both ray sources; with pinhole rays the pose is a leaf, as [3,4] and as [4,4], and its gradient compared in full."""
    case = C.synth_case(P, ray, *form)
    ref64, ref32 = C.synth_reference(P, ray, *form)
    needs = _decode_and_compare(case, ref64, ref32, hip_device, f"single {case.name}")
    assert ("g_c2w" in needs) == (ray != "map") and ("v_rays" in needs) == (ray == "map")
    assert ("v_alphas" in needs) == form[0]


def test_forward_grid_stride_loop_matches_float64(hip_device):
    """More than 4096 x 256 pixels: every thread of the forward kernel decodes a second pixel, the last workgroups a ragged
    tail of them.  Forward only (the backward grid is capped at 4096 x 768 pixels: not reached)."""
    from mobgs_amd.ops import decode
    case = C.synth_case(C.BIG_P, "pin34")
    ref64, ref32 = C.synth_reference(C.BIG_P, "pin34", forward_only=True)
    dev = hip_device
    with torch.no_grad():
        rgb, depth = decode(case.feat.reshape(case.H, case.W, 10).to(dev), case.alphas.reshape(case.H, case.W).to(dev),
                            (case.intr[0].to(dev), case.c2w[0].to(dev)), case.w1.to(dev), case.w2.to(dev), True)
    got = {"rgb": rgb.reshape(1, 3, case.P), "depth": depth.reshape(1, case.P)}
    C.compare(case, got, ref64, ref32, K, "forward grid-stride", ["rgb", "depth"])
    tail = slice(4096 * 256, None)       # the pixels of the second trip, by themselves
    C.close_to_f64(got["rgb"][..., tail], ref64["rgb"][..., tail], ref32["rgb"][..., tail], K["outputs"], "second trip rgb")


BATCHED = [("pin34", ""), ("pin44", ""), ("pin34", "intr"), ("pin34", "c2w"), ("map", ""), ("map", "map")]


@pytest.mark.parametrize("ray,share,host", [(*b, "extension") for b in BATCHED] + [("pin34", "", "ctypes")])
def test_batch_matches_float64(hip_device, ray, share, host):
    """grid.y = 3 images of 769 pixels (two partial rows each): per-image and shared strides, weight gradients summed over
    all images, pose gradients over each image's own rows -- and, for a shared pose that requires grad (decode expands it),
    the sum of the three per-image float64 pose gradients."""
    Cn, P = C.BATCH
    case = C.synth_case(P, ray, C=Cn, share=share)
    ref64, ref32 = C.synth_reference(P, ray, C=Cn, share=share)
    if share == "c2w":
        ref64, ref32 = C.summed_pose(ref64), C.summed_pose(ref32)
    with _host_path(host):
        needs = _decode_and_compare(case, ref64, ref32, hip_device, f"batch {case.name} {host}")
    assert ("g_c2w" in needs) == (ray != "map") and ("v_rays" in needs) == (ray == "map" and share != "map")


def test_shared_ray_map_with_gradient_is_refused(hip_device):
    from mobgs_amd.ops import decode
    Cn, P = C.BATCH
    case = C.synth_case(P, "map", C=Cn, share="map")
    t = _inputs(case, hip_device, map_grad=True)
    with pytest.raises(NotImplementedError):
        decode(t.feat, t.alphas, t.rays, t.w1, t.w2, True)


CHANNELS = [(CF, c0, Cn, ray, "extension") for CF, c0 in ((11, 9), (12, 9), (12, 10)) for Cn in (1, 2) for ray in ("map", "pin34")]


@pytest.mark.parametrize("CF,c0,Cn,ray,host", CHANNELS + [(12, 10, 2, "pin34", "ctypes")])
def test_channel_hand_off(hip_device, CF, c0, Cn, ray, host):
    """decode_with_channels: the channels handed out are the slice, bit for bit; their cotangent arrives in those channels of
    the image's gradient bit for bit, the other channels the decoder does not read get exact zeros, channels 0..8 match
    float64."""
    from mobgs_amd.ops import decode_with_channels
    n, P, dev = 2, 769, hip_device
    case = C.synth_case(P, ray, False, CF, False, Cn)
    ref64, ref32 = C.synth_reference(P, ray, False, CF, False, Cn)
    v_chan = torch.randn(*((Cn,) if Cn > 1 else ()), case.H, case.W, n, generator=torch.Generator().manual_seed(CF + c0)).to(dev)
    with _host_path(host):
        t = _inputs(case, dev)
        rgb, chan = decode_with_channels(t.feat, None, t.src, t.w1, t.w2, c0, n)
        assert chan.shape == v_chan.shape and chan.is_contiguous()
        assert torch.equal(chan, t.feat.detach()[..., c0:c0 + n])
        torch.autograd.backward([rgb, chan], [t.v_rgb, v_chan])
        torch.cuda.synchronize()
    assert torch.equal(t.feat.grad[..., c0:c0 + n], v_chan)
    got = _gathered(case, t, rgb, None)
    got["v_feat"] = got["v_feat"].clone()
    got["v_feat"][..., c0:c0 + n] = 0.0          # (compared bit for bit above): what is left is zero from channel 9 on
    assert not ref64["v_feat"][..., 9:].any()
    C.compare(case, got, ref64, ref32, K, f"channels CF{CF} c0{c0} C{Cn} {ray} {host}", list(got))


@pytest.mark.parametrize("ray", ["map", "pin34"])
def test_weight_gradients_accumulate_in_a_sink(hip_device, ray):
    """Two backward passes with cotangents of scale 1 and 3 under ops.LeafGradSink: the first writes the sink's buffers,
    the second adds to them in the reduction kernel (accumulate_wgrad); against the float64 sum."""
    from mobgs_amd.ops import LeafGradSink, decode
    dev, P = hip_device, 1537
    case = C.synth_case(P, ray)
    refs = [C.synth_reference(P, ray, cot_scale=s) for s in (1.0, 3.0)]
    t = _inputs(case, dev)
    dummy = torch.zeros(1, device=dev)
    pcs = SimpleNamespace(_xyz=dummy, _scaling=dummy, _rotation=dummy, _opacity=dummy, _features_dc=dummy, _features_t=dummy,
                          get_control_xyz=dummy, _omega=dummy, rgbdecoder=SimpleNamespace(
                              mlp1=SimpleNamespace(weight=t.w1), mlp2=SimpleNamespace(weight=t.w2)))
    with LeafGradSink(pcs, pcs) as sink:
        for scale in (1.0, 3.0):
            rgb, depth = decode(t.feat, t.alphas, t.src, t.w1, t.w2, True)
            torch.autograd.backward([rgb, depth], [scale * t.v_rgb, scale * t.v_depth])
        assert sink.dec_buffers is not None
    torch.cuda.synchronize()
    for i, key in enumerate(("g_w1", "g_w2")):
        got = (t.w1, t.w2)[i].grad
        assert got is not None
        C.close_to_f64(got, refs[0][0][key] + refs[1][0][key], refs[0][1][key] + refs[1][1][key], K["weights"],
                       f"sink {ray} [weights] {key}")


@pytest.mark.parametrize("host", ["extension", "ctypes"])
def test_single_image_on_both_host_paths(hip_device, host):
    case = C.synth_case(769, "pin44")
    ref64, ref32 = C.synth_reference(769, "pin44")
    with _host_path(host):
        _decode_and_compare(case, ref64, ref32, hip_device, f"host path {host} {case.name}")


# ---- fused arms --------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _fused_arms(heavy_len=None, wgrad_in_reduce=None):
    """Both halves of the decoder fusion on, the quadrant kernel whatever the grid; every global restored."""
    import mobgs_amd.rendering as R
    saved = (R.FUSE_DECODER, R.FUSE_DECODER_BWD, R.WGRAD_IN_REDUCE, R.tuning.heavy_tile_len, R.tuning.bwd_mfma, R.path_log)
    try:
        R.FUSE_DECODER = R.FUSE_DECODER_BWD = True
        R.tuning.bwd_mfma = 0
        if heavy_len is not None:
            R.tuning.heavy_tile_len = heavy_len
        if wgrad_in_reduce is not None:
            R.WGRAD_IN_REDUCE = wgrad_in_reduce
        R.path_log = []
        yield R
    finally:
        R.FUSE_DECODER, R.FUSE_DECODER_BWD, R.WGRAD_IN_REDUCE, R.tuning.heavy_tile_len, R.tuning.bwd_mfma, R.path_log = saved


def _composite_decode_and_compare(dev, grid, sign, heavy_len=None, wgrad_in_reduce=None):
    from mobgs_amd import ops
    from mobgs_amd.synth import SynthCamera, splat_inputs
    W, H, ns, nd, Cn = C.FUSED_GRIDS[grid]
    tag = f"fused {grid} sign{sign:+.0f} heavy{heavy_len} reduce{wgrad_in_reduce}"
    scam = SynthCamera().scaled(W, H)
    a, b = splat_inputs(ns, scam, 0, 9), splat_inputs(nd, scam, 1, 9)
    s = {k: torch.cat([a[k], b[k]]).to(dev) for k in ("means", "quats", "scales", "opacities")}
    g = torch.Generator().manual_seed(17)
    colors = (1.2 * torch.rand(ns + nd, 9, generator=g)).to(dev)      # composited over a zero background: [0, 1.2]
    vm = torch.eye(4).expand(Cn, 4, 4).clone()
    vm[:, 0, 3] = -0.02 * torch.arange(Cn)
    Ks = scam.K.expand(Cn, 3, 3).contiguous()
    intr = torch.tensor([[scam.focal * (1.0 + 0.05 * c), scam.focal, W / 2.0 + c, H / 2.0] for c in range(Cn)])
    poses = torch.stack([C.pose(c, 3, (C.T_BIAS[0] + 0.05 * c, C.T_BIAS[1], C.T_BIAS[2])) for c in range(Cn)])
    w1c, w2c = C.bias_weights(sign)
    c2w = _leaf(poses if Cn > 1 else poses[0], dev)       # a leaf of its own: its gradient is the decoder's alone
    w1, w2 = _leaf(w1c, dev), _leaf(w2c, dev)
    intr_d = (intr if Cn > 1 else intr[0]).to(dev)
    with _fused_arms(heavy_len, wgrad_in_reduce) as R:
        sp = R.SharedProjection(s["means"], s["quats"], s["scales"], s["opacities"], vm.to(dev), Ks.to(dev), W, H)
        img, alphas, rgb, depth = sp.composite_decode(colors, torch.zeros(Cn, 9, device=dev), (intr_d, c2w), w1, w2)
        case = C.rendered_case(tag, img.detach().cpu().reshape(Cn, H, W, 10), alphas.detach().cpu(), intr, poses, w1c, w2c, 0)
        print(f"MARGIN {tag}: min |s| {case.margin:.3f}, max |z| {case.z_max:.2f}, holes {float(case.hole.float().mean()):.1%}")
        assert case.margin >= C.MARGIN and case.z_max < C.Z_MAX and torch.equal(*case.signs)
        assert torch.equal(case.signs[0], sign * torch.tensor([1.0, -1, 1, -1, 1, -1], dtype=torch.float64))
        assert float(case.hole.float().mean()) < 0.5
        v_rgb, v_depth = case.v_rgb.to(dev), case.v_depth.to(dev)
        torch.autograd.backward([rgb, depth], [v_rgb.reshape(rgb.shape), v_depth.reshape(depth.shape)])
        torch.cuda.synchronize()
        log_f = [e for e in R.path_log if e["dir"] == "fwd" and e["D"] == 10][-1]
        log_b = [e for e in R.path_log if e["dir"] == "bwd" and e["D"] == 10][-1]
        # the separate chain on the same inputs: the image cotangent the compositing loop is handed
        lead = (Cn,) if Cn > 1 else ()
        sep = ops.decode_backward((img.detach().reshape(*lead, H, W, 10), alphas.detach().reshape(*lead, H, W), None, intr_d,
                                   c2w.detach(), w1.detach(), w2.detach()), True, (w1, w2), (*lead, H, W, 10), False, True,
                                  v_rgb.reshape(*lead, 3, H, W), v_depth.reshape(*lead, H, W))
        torch.cuda.synchronize()
    assert log_f["decode"] and log_b.get("decode_bwd") and log_b["bwd_kernel"] == "quadrant"
    assert log_f["n_tiles"] == Cn * C.tiles(W, H)[0] * C.tiles(W, H)[1]
    ref64, ref32 = C.evaluate(case, torch.float64), C.evaluate(case, torch.float32)
    P = H * W
    got = {"rgb": rgb.detach().reshape(Cn, 3, P), "depth": depth.detach().reshape(Cn, P), "g_w1": w1.grad, "g_w2": w2.grad,
           "g_c2w": c2w.grad.reshape(Cn, 3, 4)}
    C.compare(case, got, ref64, ref32, K, tag, list(got))
    got = {"v_feat": sep[0].reshape(Cn, P, 10), "v_alphas": sep[1].reshape(Cn, P), "g_c2w": sep[4].reshape(Cn, 3, 4),
           "g_w1": sep[5], "g_w2": sep[6]}
    C.compare(case, got, ref64, ref32, K, tag + " separate", list(got))
    return log_b


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_fused_arms_on_a_grid_of_six_ragged_tiles(hip_device, sign):
    _composite_decode_and_compare(hip_device, "tiny", sign)


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("heavy_len", [0, 1])
def test_fused_arms_with_one_and_with_four_waves_per_tile(hip_device, heavy_len, sign):
    """heavy_tile_len = 0: one wave per tile; 1: every tile four waves, whose partial rows meet in LDS."""
    log_b = _composite_decode_and_compare(hip_device, "small", sign, heavy_len=heavy_len)
    assert (log_b["heavy_tiles"] > 0) == (heavy_len == 1)


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("in_reduce", [True, False])
def test_fused_arms_on_more_than_2048_tiles_with_both_reductions(hip_device, in_reduce, sign):
    """2070 partial rows: the column sums inside the slot reduction (True) and the chunked, ticketed finish kernel (False)."""
    _composite_decode_and_compare(hip_device, "large", sign, wgrad_in_reduce=in_reduce)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_fused_arms_with_three_cameras(hip_device, sign):
    """One partial row per (camera, tile); the pose gradient of a camera sums its own rows."""
    _composite_decode_and_compare(hip_device, "cams", sign, heavy_len=0)
