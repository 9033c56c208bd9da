"""The Farneback kernels on the MI355X (csrc/tof.hip through the C ABI of include/mobgs_hip.h K25 and mobgs_amd.metrics)
against the float64 restatement tests/tof_restatement.py: stage by stage, each stage fed the restatement's own input for it
(rounded to fp32 first, so that the error shown is the kernel's arithmetic alone), then end to end.

Shapes (W x H), the smallest that reach every branch: 75x50 is one level with tile tails on both axes; 136x72 two levels;
262x259 all four, with half-to-even size rounding (65.5 -> 66, 129.5 -> 130) and non-integer resize ratios.  F = 3 frames of
a seeded smooth texture under a smooth, spatially varying motion of at most 4 px.

Tolerances: OBSERVED holds, per stage, the largest error relative to the array's largest magnitude that the
MI355X showed over all shapes and levels (docs/MEASUREMENT_LOG.md, "Farneback kernels against float64"); a test allows three
times that, with no element allowance.  That holds for the update matrices too, although their in-bounds test is a genuine
discontinuity: for an fp32 flow handed in both sides decide it on exact integers (the kernel splits u into floor(u) and
u - floor(u), the restatement adds the fp32 u to an integer in float64), so every pixel is compared."""
import ctypes

import numpy as np
import pytest
import torch

import tof_restatement as TR
from helpers import same_bits

pytestmark = pytest.mark.gpu

SHAPES = [(50, 75), (72, 136), (259, 262)]                           # (H, W)
F = 3
OBSERVED = {
    "pyramid": 2.83e-7,              # 33x32 of 262x259, 19 taps
    "polyexp": 4.94e-6,              # r_yy at 262x259: b_1 ig03 + b_yy ig33 cancels
    "update": 1.95e-7,               # G22 at 136x72
    "update_flow": 1.69e-7,          # 131x130 -> 262x259
    "solve": 4.86e-8,                # 75x50, round 0
    "score": 1.48e-16,               # 75x50, no mask
    "flow": 3.79e-7,                 # 136x72
    "tof": 4.75e-7,                  # 75x50
}


def allowed(stage):
    return 3.0 * OBSERVED[stage]


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.fixture(scope="module")
def lib():
    from mobgs_amd import _lib
    return _lib.load(build_if_missing=False)


class Trace:
    """The restatement run once on one shape, every stage's input and output kept (float64), never modified."""

    def __init__(self, H, W):
        self.H, self.W = H, W
        self.rgb = TR.moving_frames(F, H, W, seed=H)
        self.grey = TR.grey(self.rgb)
        self.levels = TR.levels(H, W)
        self.img, self.R, self.first_flow, self.M, self.flow = [], [], [], [], []
        flow = None
        for lv in self.levels:
            w, h = lv[:2]
            img = np.stack([TR.pyramid_level(g, lv) for g in self.grey])
            R = np.stack([TR.poly_exp(i) for i in img])
            flow = np.zeros((F - 1, h, w, 2)) if flow is None else np.stack([TR.resize_bilinear(f, h, w) * 2.0 for f in flow])
            self.first_flow.append(flow)
            Ms = []
            M = np.stack([TR.update_matrices(R[p], R[p + 1], flow[p]) for p in range(F - 1)])
            for i in range(TR.ITERATIONS):
                Ms.append(M)
                flow = np.stack([TR.blur_solve(m) for m in M])
                if i < TR.ITERATIONS - 1:
                    M = np.stack([TR.update_matrices(R[p], R[p + 1], flow[p]) for p in range(F - 1)])
            self.img.append(img)
            self.R.append(R)
            self.M.append(Ms)
            self.flow.append(flow)


_traces = {}


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def trace(request):
    if request.param not in _traces:
        _traces[request.param] = Trace(*request.param)
    return _traces[request.param]


def dev32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def call(lib, name, *args):
    from mobgs_amd._lib import check, ptr, stream
    conv = [ptr(a) if torch.is_tensor(a) else a for a in args]
    check(getattr(lib, name)(*conv, stream()), name)


def level_record(lv):
    from mobgs_amd import _lib
    return _lib.MobgsTofLevel(lv[0], lv[1], lv[2], lv[3])


def test_levels_agree(trace, lib):
    from mobgs_amd import _lib
    out = (_lib.MobgsTofLevel * 4)()
    n = lib.mobgs_tof_levels(trace.H, trace.W, ctypes.cast(out, ctypes.c_void_p))
    assert [(out[i].width, out[i].height, out[i].taps, out[i].sigma) for i in range(n)] == trace.levels
    assert n == {50: 1, 72: 2, 259: 4}[trace.H]


def test_grey_bit_exact(trace, lib, hip_device):
    from mobgs_amd.metrics import grey_frames
    rgb = torch.from_numpy(trace.rgb).to(hip_device)
    got = grey_frames(rgb)
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().astype(np.float64), trace.grey)
    assert len(np.unique(trace.grey)) > 100
    # values outside [0, 1], exact k / 255 and values just around them, under every flag
    rng = np.random.default_rng(1)
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    edge = np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1)), [-0.3, 1.2, 1.0, 0.0]])
    x = rng.uniform(-0.2, 1.2, size=(2, 3, trace.H, trace.W)).astype(np.float32)
    x.reshape(-1)[:3 * len(edge)] = np.tile(edge, 3)
    for clamp in (False, True):
        for quantize in (False, True):
            got = grey_frames(torch.from_numpy(x).to(hip_device), clamp=clamp, quantize=quantize).cpu().numpy()
            assert np.array_equal(got.astype(np.float64), TR.grey(x, clamp, quantize)), (clamp, quantize)


def test_grey_table_of_all_256_values(lib, hip_device):
    from mobgs_amd.metrics import grey_frames
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    img = np.broadcast_to(k[None, None, None, :], (1, 3, 48, 256)).copy()
    got = grey_frames(torch.from_numpy(img).to(hip_device)).cpu().numpy()
    want = TR.round_trip_table().astype(np.float32)                   # (equal channels: the grey value is the channel's)
    assert np.array_equal(got[0], np.broadcast_to(want, (48, 256)))


def test_pyramid_level(trace, lib, hip_device):
    grey = dev32(trace.grey, hip_device)
    for i, lv in enumerate(trace.levels):
        w, h = lv[:2]
        out = torch.full((F, h, w), float("nan"), device=hip_device)
        rec = level_record(lv)
        call(lib, "mobgs_tof_pyramid_level", F, trace.H, trace.W, grey, ctypes.cast(ctypes.pointer(rec), ctypes.c_void_p), out)
        err = rel_err(out.cpu().numpy(), trace.img[i])
        print(f"[tof] pyramid {trace.W}x{trace.H} level {w}x{h} ({lv[2]} taps): relative error {err:.2e} "
              f"(allowed {allowed('pyramid'):.2e})")
        assert err <= allowed("pyramid")


def test_polynomial_expansion(trace, lib, hip_device):
    for i, lv in enumerate(trace.levels):
        w, h = lv[:2]
        img32 = np.ascontiguousarray(trace.img[i], dtype=np.float32)
        want = np.stack([TR.poly_exp(a.astype(np.float64)) for a in img32])
        R = torch.full((F, 5, h, w), float("nan"), device=hip_device)
        call(lib, "mobgs_tof_polyexp", F, h, w, torch.from_numpy(img32).to(hip_device), R)
        got = R.cpu().numpy()
        for c, name in enumerate(("r_x", "r_y", "r_xx", "r_yy", "r_xy")):
            err = rel_err(got[:, c], want[:, c])
            print(f"[tof] polyexp {trace.W}x{trace.H} level {w}x{h} {name}: relative error {err:.2e} "
                  f"(allowed {allowed('polyexp'):.2e})")
            assert err <= allowed("polyexp")


def test_update_matrices(trace, lib, hip_device):
    i = len(trace.levels) - 1
    w, h = trace.levels[i][:2]
    R32 = np.ascontiguousarray(trace.R[i], dtype=np.float32)
    flow32 = TR.update_test_flows(h, w, F - 1)
    share = np.mean([TR.out_of_bounds_share(f) for f in flow32])
    assert 0.05 <= share <= 0.2, share
    want = np.stack([TR.update_matrices(R32[p].astype(np.float64), R32[p + 1].astype(np.float64), flow32[p])
                     for p in range(F - 1)])
    M = torch.full((F - 1, 5, h, w), float("nan"), device=hip_device)
    flow = torch.from_numpy(flow32).to(hip_device)
    used = torch.full_like(flow, float("nan"))
    call(lib, "mobgs_tof_update_matrices", F - 1, h, w, torch.from_numpy(R32).to(hip_device), flow, h, w, used, M)
    assert same_bits(used, flow)
    got = M.cpu().numpy()
    assert np.isfinite(got).all()
    for c, name in enumerate(("G11", "G12", "G22", "h1", "h2")):
        err = rel_err(got[:, c], want[:, c])
        print(f"[tof] update matrices {w}x{h} {name}: relative error {err:.2e} (allowed {allowed('update'):.2e}), "
              f"{share:.1%} of the samples out of bounds, every pixel compared")
        assert err <= allowed("update")
    # a NULL flow is the zero flow; flow_out may be NULL
    zero = torch.full_like(M, float("nan"))
    call(lib, "mobgs_tof_update_matrices", F - 1, h, w, torch.from_numpy(R32).to(hip_device), None, 0, 0, None, zero)
    want0 = np.stack([TR.update_matrices(R32[p].astype(np.float64), R32[p + 1].astype(np.float64), np.zeros((h, w, 2)))
                      for p in range(F - 1)])
    for c in range(5):
        assert rel_err(zero.cpu().numpy()[:, c], want0[:, c]) <= allowed("update")


def test_update_matrices_from_the_coarser_flow(trace, lib, hip_device):
    if len(trace.levels) < 2:
        pytest.skip("one level: no coarser flow to start from")
    for i in range(1, len(trace.levels)):
        w, h = trace.levels[i][:2]
        sw, sh = trace.levels[i - 1][:2]
        coarse32 = np.ascontiguousarray(trace.flow[i - 1], dtype=np.float32)
        R32 = np.ascontiguousarray(trace.R[i], dtype=np.float32)
        want_flow = np.stack([TR.resize_bilinear(f.astype(np.float64), h, w) * 2.0 for f in coarse32])
        used = torch.full((F - 1, h, w, 2), float("nan"), device=hip_device)
        M = torch.full((F - 1, 5, h, w), float("nan"), device=hip_device)
        call(lib, "mobgs_tof_update_matrices", F - 1, h, w, torch.from_numpy(R32).to(hip_device),
             torch.from_numpy(coarse32).to(hip_device), sh, sw, used, M)
        err = rel_err(used.cpu().numpy(), want_flow)
        print(f"[tof] upsampled flow {sw}x{sh} -> {w}x{h}: relative error {err:.2e} (allowed {allowed('update_flow'):.2e})")
        assert err <= allowed("update_flow")
        # the matrices are those of the flow the kernel formed, bit for bit
        again = torch.full_like(M, float("nan"))
        call(lib, "mobgs_tof_update_matrices", F - 1, h, w, torch.from_numpy(R32).to(hip_device), used, h, w, None, again)
        assert same_bits(M, again)


def test_box_mean_and_solve(trace, lib, hip_device):
    for i, lv in enumerate(trace.levels):
        w, h = lv[:2]
        R = dev32(trace.R[i], hip_device)
        for r, M64 in enumerate(trace.M[i]):
            M32 = np.ascontiguousarray(M64, dtype=np.float32)
            want = np.stack([TR.blur_solve(m.astype(np.float64)) for m in M32])
            flow = torch.full((F - 1, h, w, 2), float("nan"), device=hip_device)
            M_in = torch.from_numpy(M32).to(hip_device)
            call(lib, "mobgs_tof_blur_solve", F - 1, h, w, M_in, flow, None, None)
            err = rel_err(flow.cpu().numpy(), want)
            print(f"[tof] box mean + solve {trace.W}x{trace.H} level {w}x{h} round {r}: relative error {err:.2e} "
                  f"(allowed {allowed('solve'):.2e})")
            assert err <= allowed("solve")
            # the fused form: the same flow, and the update matrices of that flow, bit for bit
            flow2, M_out = torch.full_like(flow, float("nan")), torch.full_like(M_in, float("nan"))
            call(lib, "mobgs_tof_blur_solve", F - 1, h, w, M_in, flow2, R, M_out)
            separate = torch.full_like(M_in, float("nan"))
            call(lib, "mobgs_tof_update_matrices", F - 1, h, w, R, flow, h, w, None, separate)
            assert same_bits(flow, flow2) and same_bits(M_out, separate)


def test_score(trace, lib, hip_device):
    from mobgs_amd.metrics import flow_distance
    rng = np.random.default_rng(trace.H)
    fa = np.ascontiguousarray(trace.flow[-1], dtype=np.float32)
    fb = (fa + rng.normal(size=fa.shape) * 0.3).astype(np.float32)
    mask = (rng.uniform(size=fa.shape[:3]) < 0.4).astype(np.float32)
    a, b, m = (torch.from_numpy(t).to(hip_device) for t in (fa, fb, mask))
    for name, mk, mt in (("no mask", None, None), ("mask", mask, m)):
        got = flow_distance(a, b, mt)
        assert got.dtype == torch.float64 and got.shape == (F - 1,) and got.is_cuda
        want = np.array([TR.score(fa[p], fb[p], None if mk is None else mk[p]) for p in range(F - 1)])
        err = float(np.abs(got.cpu().numpy() - want).max() / np.abs(want).max())
        print(f"[tof] score {trace.W}x{trace.H} {name}: {got.tolist()}, float64 {want.tolist()}, relative error {err:.2e} "
              f"(allowed {allowed('score'):.2e})")
        assert err <= allowed("score")
    assert torch.equal(flow_distance(a, a), torch.zeros(F - 1, dtype=torch.float64, device=hip_device))
    assert torch.isnan(flow_distance(a, b, torch.zeros_like(m))).all()        # the reference's 0 / 0


def test_flow_and_tof_end_to_end(trace, lib, hip_device):
    from mobgs_amd.metrics import TofTarget, farneback_flow, grey_frames, temporal_of
    grey = dev32(trace.grey, hip_device)
    flow = farneback_flow(grey)
    assert flow.shape == (F - 1, trace.H, trace.W, 2) and flow.dtype == torch.float32
    want = trace.flow[-1]
    err = rel_err(flow.cpu().numpy(), want)
    print(f"[tof] flow {trace.W}x{trace.H} end to end: largest flow {np.abs(want).max():.3f} px, relative error {err:.2e} "
          f"(allowed {allowed('flow'):.2e})")
    assert np.abs(want).max() > 1.0 and err <= allowed("flow")
    assert same_bits(flow, farneback_flow(grey))                              # run to run
    # tOF of a perturbed prediction against these frames
    rng = np.random.default_rng(5)
    pred = np.clip(trace.rgb + rng.normal(size=trace.rgb.shape).astype(np.float32) * 0.02, -0.05, 1.05).astype(np.float32)
    p, g = torch.from_numpy(pred).to(hip_device), torch.from_numpy(trace.rgb).to(hip_device)
    for clamp, quantize in ((False, False), (True, True)):
        got = temporal_of(p, g, clamp=clamp, quantize=quantize)
        assert got.shape == (F - 1,) and got.dtype == torch.float64
        if quantize:
            # (the saturating 8-bit conversion makes the clamp a no-op on the ground truth: its flows are the trace's)
            assert np.array_equal(TR.grey(trace.rgb, clamp=True), trace.grey)
            want_tof = np.array([TR.score(a, b) for a, b in zip(want, TR.flows(TR.grey(pred, True, True)))])
            e = float(np.abs(got.cpu().numpy() - want_tof).max() / np.abs(want_tof).max())
            print(f"[tof] tOF {trace.W}x{trace.H} of the quantised prediction: {got.tolist()}, float64 "
                  f"{want_tof.tolist()}, relative error {e:.2e} (allowed {allowed('tof'):.2e})")
            assert e <= allowed("tof")
        # the cached target, bit for bit; the flows of the prediction's grey frames, scored directly
        target = TofTarget.from_frames(g, clamp=clamp)
        assert target.frames == F and same_bits(temporal_of(p, target, clamp=clamp, quantize=quantize), got)
    assert same_bits(target.flows, farneback_flow(grey_frames(g, clamp=True)))


def test_batch_identity_and_pieces(trace, hip_device, monkeypatch):
    from mobgs_amd import metrics as M
    rgb5 = TR.moving_frames(5, trace.H, trace.W, seed=trace.W, amplitude=2.0)
    grey5 = M.grey_frames(torch.from_numpy(rgb5).to(hip_device))
    all4 = M.farneback_flow(grey5)
    one = M.farneback_flow(grey5[2:4])
    assert same_bits(one[0], all4[2])
    # a scratch budget that forces pieces of two and three frames changes nothing
    lib = M._lib.load()
    monkeypatch.setattr(M, "TOF_SCRATCH_BUDGET", int(lib.mobgs_tof_scratch_bytes(3, trace.H, trace.W)))
    assert same_bits(M.farneback_flow(grey5), all4)
    monkeypatch.setattr(M, "TOF_SCRATCH_BUDGET", 1)
    assert same_bits(M.farneback_flow(grey5), all4)


def test_identical_and_flat_frames(hip_device):
    """Equal frames: exactly 0 wherever no window reaches the last row or column, whose pixels take the out-of-bounds arm
    (tests/test_tof_cpu.py test_identical_frames); a flat sequence is exactly 0 everywhere; equal sequences score exactly 0."""
    from mobgs_amd import metrics as M
    a = torch.from_numpy(TR.texture(50, 75, 5).astype(np.float32)).to(hip_device)
    flow = M.farneback_flow(torch.stack([a, a]))
    assert torch.all(flow[0, :50 - 22, :75 - 22] == 0) and float(flow.abs().max()) > 1e-3
    flat = torch.full((2, 259, 262), 77.0, device=hip_device)
    assert torch.all(M.farneback_flow(flat) == 0)
    rgb = torch.from_numpy(TR.moving_frames(3, 259, 262, seed=1)).to(hip_device)
    assert torch.equal(M.temporal_of(rgb, rgb.clone()), torch.zeros(2, dtype=torch.float64, device=hip_device))
    g = M.grey_frames(rgb)
    assert M.get_tOF(g[0], g[1], g[0], g[1]) == 0.0
    assert M.get_tOF(g[0].cpu().numpy(), g[1], g[0], g[2], mask=torch.ones(259, 262, 1, device=hip_device)) > 0.0


def test_python_refusals(hip_device):
    from mobgs_amd import metrics as M
    dev = hip_device
    with pytest.raises(ValueError, match="H, W >= 48"):
        M.grey_frames(torch.rand(2, 3, 47, 64, device=dev))
    with pytest.raises(ValueError, match=r"\[F,3,H,W\]"):
        M.grey_frames(torch.rand(2, 1, 64, 64, device=dev))
    with pytest.raises(ValueError, match="two frames"):
        M.farneback_flow(torch.rand(1, 64, 64, device=dev))
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.farneback_flow(torch.rand(2, 64, 64))
    with pytest.raises(ValueError, match="one shape"):
        M.temporal_of(torch.rand(3, 3, 64, 64, device=dev), torch.rand(2, 3, 64, 64, device=dev))
    target = M.TofTarget.from_frames(torch.rand(2, 3, 64, 64, device=dev))
    with pytest.raises(ValueError, match="target holds"):
        M.temporal_of(torch.rand(3, 3, 64, 64, device=dev), target)
    with pytest.raises(ValueError, match="mask"):
        M.flow_distance(target.flows, target.flows, torch.ones(1, 64, 63, device=dev))


def test_evaluate_views_tof(hip_device):
    """evaluate_views(..., tof=True) on the synthetic scene of tests/test_gpu_metrics.py (at a size tOF accepts) equals
    temporal_of of its "images"; without tof nothing is added."""
    from mobgs_amd import _lib
    from mobgs_amd.camera import PinholeCamera
    from mobgs_amd.gaussian_model import GaussianParams
    from mobgs_amd.helper_model import Sandwich
    from mobgs_amd.metrics import TofTarget, evaluate_views, temporal_of
    from mobgs_amd.synth import SynthCamera, dynamic_extras, gaussian_cloud
    dev = hip_device
    _lib.load(build_if_missing=False)
    W, H = 80, 64
    scam = SynthCamera().scaled(W, H)
    torch.manual_seed(0)
    dec = Sandwich(9, 3).to(dev)
    stat_p, dyn_p = gaussian_cloud(1500, scam, 0), gaussian_cloud(700, scam, 1)
    stat = GaussianParams(stat_p, None, dec, dev, requires_grad=False)
    dyn = GaussianParams(dyn_p, dynamic_extras(dyn_p["xyz"], 0), dec, dev, requires_grad=False)
    cams = []
    for k in range(3):
        w2c = torch.eye(4)
        w2c[0, 3] = 0.05 * (k - 1)
        cams.append(PinholeCamera(W, H, scam.K, w2c, (3 + 8 * k) / 23.0, scam.max_time, device=dev))
    bg = torch.zeros(9, device=dev)
    g = torch.Generator().manual_seed(11)
    plain = evaluate_views(cams, stat, dyn, None, bg, torch.zeros(3, 3, H, W, device=dev))
    assert "tof" not in plain and "tof_per_pair" not in plain
    gt = (plain["images"].cpu() + 0.2 * torch.randn(3, 3, H, W, generator=g)).clamp(-0.1, 1.1).to(dev)
    rep = evaluate_views(cams, stat, dyn, None, bg, gt, tof=True)
    want = temporal_of(rep["images"], gt, clamp=True)
    assert same_bits(rep["tof_per_pair"], want) and rep["tof_per_pair"].shape == (2,)
    assert rep["tof"] == float(want.mean()) and rep["tof"] > 0.0
    assert rep["psnr"] == evaluate_views(cams, stat, dyn, None, bg, gt)["psnr"]
    cached = evaluate_views(cams, stat, dyn, None, bg, gt, tof=TofTarget.from_frames(gt, clamp=True))
    assert same_bits(cached["tof_per_pair"], want)
