"""CPU checks around LPIPS (include/mobgs_hip.h K24, mobgs_amd.lpips): the restatement against itself and against
tests/golden/lpips.npz, the state-dict checks, the packed weight layout, the size queries and the refusals of the C ABI.
Nothing here launches a kernel."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_restatement as LR
from helpers import GOLDEN, load


@pytest.fixture(scope="module")
def fx():
    return load("lpips")


@pytest.fixture(scope="module")
def nets():
    return LR.seeded_trunk(), LR.reference_heads()


def test_heads_fixture_is_the_published_shape():
    heads = LR.reference_heads()
    assert [heads[f"lin{l}.model.1.weight"].shape[1] for l in range(5)] == list(LR.COUT)
    assert sum(v.numel() for v in heads.values()) == 1152
    assert all(v.dtype == torch.float32 and float(v.min()) >= 0.0 and float(v.max()) > 0.1 for v in heads.values())


def test_the_two_convolutions_of_the_restatement_agree():
    g = torch.Generator().manual_seed(3)
    for cin, cout, k, stride, pad, H, W in ((3, 8, 11, 4, 2, 31, 37), (6, 5, 5, 1, 2, 7, 4), (4, 7, 3, 1, 1, 1, 1)):
        x = torch.randn(2, cin, H, W, generator=g, dtype=torch.float64)
        w = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64)
        b = torch.randn(cout, generator=g, dtype=torch.float64)
        want = LR.conv_torch(x, w, b, stride, pad)
        got = LR.conv_sequential(x, w, b, stride, pad)
        assert got.shape == want.shape
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
        got32 = LR.conv_sequential(x.float(), w.float(), b.float(), stride, pad)
        assert got32.dtype == torch.float32 and float((got32.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())


@pytest.mark.parametrize("i", (0, 2, 5))
def test_fixture_reproduces(fx, nets, i):
    c = LR.make_case(i)
    assert np.array_equal(LR.probe(c), fx["probe"][i])
    rows = slice(int(fx["first"][i]), int(fx["first"][i + 1]))
    v64, t64 = LR.evaluate(c, *nets, torch.float64)
    assert np.allclose(v64.numpy(), fx["f64"][rows], rtol=1e-12, atol=0)
    v32, t32 = LR.evaluate(c, *nets, torch.float32)
    # (a torch build may order an fp32 sum differently: the stored fp32 run is a sample of the reference's error, the gaps
    # it implies must stay of the stored size)
    assert np.allclose(v32.double().numpy(), fx["f32"][rows], rtol=2e-6, atol=0)
    assert (LR.taps_gap(t32, t64) <= 4 * fx["tap_gap_f32"].max(0)).all()
    if LR.CASES[i][3] == "identical":
        assert (v64 == 0).all() and (v32 == 0).all()


def test_fixture_is_not_degenerate(fx):
    assert len(fx["probe"]) == len(LR.CASES) == 9 and fx["first"][-1] == fx["f64"].shape[0] == 21
    for i, (H, W, B, what) in enumerate(LR.CASES):
        v = fx["f64"][int(fx["first"][i]):int(fx["first"][i + 1])]
        if what == "identical":
            assert (v == 0).all()
        elif what != "flat":
            assert (v[:, 1:] > 2e-4).all() and (v[:, 1:] < 1e-2).all() and (v[:, 0] > 3e-3).all() and (v[:, 0] < 3e-2).all()
        else:
            assert (v[:, 0] > 0).all()
    gaps = LR.reference_gaps(fx)
    assert set(gaps) == set(LR.QUANTITIES) | set(LR.TAPS)
    assert all(1e-8 < g < 1e-5 for g in gaps.values()), gaps
    assert all(LR.tolerance(k, gaps) >= LR.FLOOR for k in gaps)


def test_state_dict_checks_name_the_key(nets):
    from mobgs_amd import lpips as L
    trunk, heads = nets
    ws, bs, ls = L.check_state_dicts(trunk, heads)
    assert [tuple(w.shape) for w in ws] == [(L.COUT[l], L.CIN[l], L.KS[l], L.KS[l]) for l in range(5)]
    assert [v.shape for v in ls] == [(c,) for c in L.COUT] and [b.shape for b in bs] == [(c,) for c in L.COUT]
    # other keys (the classifier's) are ignored; float64 is converted
    L.check_state_dicts({**{k: v.double() for k, v in trunk.items()}, "classifier.1.weight": torch.zeros(2)}, heads)
    for key in ("features.6.weight", "features.10.bias"):
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            L.check_state_dicts({k: v for k, v in trunk.items() if k != key}, heads)
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            L.check_state_dicts({**trunk, key: trunk[key][:-1]}, heads)
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            L.check_state_dicts({**trunk, key: trunk[key].to(torch.int32)}, heads)
    with pytest.raises(ValueError, match=r"lin3\.model\.1\.weight"):
        L.check_state_dicts(trunk, {k: v for k, v in heads.items() if not k.startswith("lin3")})
    with pytest.raises(ValueError, match=r"lin0\.model\.1\.weight"):
        L.check_state_dicts(trunk, {**heads, "lin0.model.1.weight": heads["lin0.model.1.weight"].reshape(-1)})
    with pytest.raises(ValueError, match=r"features\.0\.weight"):
        L.check_state_dicts(None, heads)
    # the checks come first, then the device: no model on the host
    with pytest.raises(ValueError, match=r"features\.0\.weight"):
        L.LpipsAlex({}, heads, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        L.LpipsAlex(trunk, heads, device="cpu")


def test_packer_round_trips_and_is_the_layout_the_kernel_documents(nets):
    """pack_conv_weight: [Kpad, Cout] with zero padding rows, unpack_conv_weight its inverse; and the packed matrix times
    the patch matrix in the K order of include/mobgs_hip.h K24 -- (ky, kx, ci) over a channel-last input for layers 2 .. 5,
    (ci, ky, kx) over the channel-first image for layer 1 -- is the convolution."""
    from mobgs_amd import _lib, lpips as L
    trunk, _ = nets
    h = _lib.load()
    g = torch.Generator().manual_seed(5)
    for layer in range(1, 6):
        l = layer - 1
        w = trunk[f"features.{L.TRUNK_INDEX[l]}.weight"]
        K = L.CIN[l] * L.KS[l] ** 2
        packed = L.pack_conv_weight(w, layer)
        assert packed.shape == (L.pack_k(layer), L.COUT[l]) == (h.mobgs_lpips_pack_k(layer), L.COUT[l])
        assert packed.shape[0] % L.K_STEP == 0 and packed.shape[0] - K < L.K_STEP and packed.is_contiguous()
        assert (packed[K:] == 0).all() and torch.equal(L.unpack_conv_weight(packed, layer), w)
        x = torch.randn(1, L.CIN[l], 9 if layer > 1 else 31, 7 if layer > 1 else 35, generator=g, dtype=torch.float64)
        want = F.conv2d(x, w.double(), None, stride=L.STRIDE[l], padding=L.PAD[l])
        k, s, p = L.KS[l], L.STRIDE[l], L.PAD[l]
        xp = F.pad(x, (p, p, p, p))[0]                                  # [Cin, H + 2p, W + 2p]
        ho, wo = want.shape[2:]
        patches = torch.zeros(ho * wo, packed.shape[0], dtype=torch.float64)
        for oy in range(ho):
            for ox in range(wo):
                win = xp[:, oy * s:oy * s + k, ox * s:ox * s + k]      # [Cin, ky, kx]
                patches[oy * wo + ox, :K] = (win if layer == 1 else win.permute(1, 2, 0)).reshape(-1)
        got = (patches @ packed.double()).t().reshape(1, L.COUT[l], ho, wo)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), layer
    assert [L.pack_k(i) for i in range(1, 6)] == [384, 1600, 1728, 3456, 2304]
    assert h.mobgs_lpips_pack_k(0) == 0 and h.mobgs_lpips_pack_k(6) == 0
    with pytest.raises(ValueError, match="layer 2"):
        L.pack_conv_weight(trunk["features.0.weight"], 2)


def test_size_queries_and_the_minimum_size():
    from mobgs_amd import _lib, build, lpips as L
    h = _lib.load()
    assert "lpips.hip" in build.SOURCES
    assert _lib._SIGS["mobgs_lpips_scratch_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    P = ctypes.c_void_p
    assert _lib._SIGS["mobgs_lpips_alex"] == (ctypes.c_int, [ctypes.c_int] * 3 + [P] * 3 + [ctypes.c_int, P, ctypes.c_size_t,
                                                                                      P, P, P])
    assert [n for n, _ in _lib.MobgsLpipsWeights._fields_] == [f"{p}{l}" for p in ("w", "b", "lin") for l in range(1, 6)]
    assert _lib.ABI_VERSION == 16
    # 30 is refused, 31 accepted
    assert h.mobgs_lpips_scratch_bytes(1, 30, 64) == 0 and h.mobgs_lpips_scratch_bytes(1, 64, 30) == 0
    assert h.mobgs_lpips_scratch_bytes(1, 31, 31) > 0
    assert h.mobgs_lpips_scratch_bytes(0, 64, 64) == 0 and h.mobgs_lpips_scratch_bytes(4097, 64, 64) == 0
    assert h.mobgs_lpips_scratch_bytes(1, 16385, 64) == 0
    assert h.mobgs_lpips_scratch_bytes(4096, 4096, 4096) == 0          # 2 B h1 w1 beyond 2^30
    with pytest.raises(ValueError, match=">= 31"):
        L.tap_sizes(30, 64)
    # the sizes torch gives, and a scratch that holds the two largest maps of 2 B images plus the partial sums
    for H, W in ((31, 31), (31, 48), (64, 97), (130, 67), (288, 512), (1014, 1352)):
        x = torch.zeros(1, 3, H, W)
        t = LR.trunk_taps(x, LR.seeded_trunk(), torch.float32) if H < 200 else None
        sizes = L.tap_sizes(H, W)
        if t is not None:
            assert [tuple(m.shape[2:]) for m in t] == sizes
        for B in (1, 3):
            tap1 = 2 * B * sizes[0][0] * sizes[0][1] * 64 * 4
            got = h.mobgs_lpips_scratch_bytes(B, H, W)
            assert tap1 < got < 2 * tap1 + (1 << 16) and got % 256 == 0
    assert L.tap_sizes(1014, 1352)[0] == (252, 337)                     # 21.7 MB per image at fp32 x 64 channels
    assert 10 * h.mobgs_lpips_scratch_bytes(1, 1014, 1352) < L.LpipsAlex.max_scratch_bytes


def test_bad_arguments_are_refused_before_any_launch():
    from mobgs_amd import _lib
    h = _lib.load()
    none = ctypes.c_void_p(None)
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p((base + 255) & ~255)                            # a 256-byte aligned host address: never dereferenced
    rec = _lib.MobgsLpipsWeights(**{n: p.value for n, _ in _lib.MobgsLpipsWeights._fields_})
    ok = ctypes.byref(rec)
    big = 1 << 40
    INVALID = _lib._DEFINES["MOBGS_E_INVALID"]

    def call(B=1, H=64, W=64, img0=p, img1=p, weights=ok, flags=1, scratch=p, nbytes=big, out=p, taps=none):
        h.mobgs_raster_bwd_reduce(0, 5, 3, 0, *[none] * 12)            # leaves another entry point's message behind
        rc = h.mobgs_lpips_alex(B, H, W, img0, img1, weights, flags, scratch, nbytes, out, taps, none)
        assert b"mobgs_lpips_alex" in h.mobgs_last_error(), h.mobgs_last_error()
        return rc

    for kw in (dict(B=0), dict(B=4097), dict(H=30), dict(W=30), dict(H=16385), dict(img0=none), dict(img1=none),
               dict(weights=none), dict(scratch=none), dict(out=none), dict(flags=8), dict(flags=-1),
               dict(nbytes=h.mobgs_lpips_scratch_bytes(1, 64, 64) - 1), dict(scratch=ctypes.c_void_p(p.value + 16)),
               dict(out=ctypes.c_void_p(p.value + 4)), dict(img0=ctypes.c_void_p(p.value + 2))):
        assert call(**kw) == INVALID, kw
    for field in ("w3", "b1", "lin5"):
        broken = _lib.MobgsLpipsWeights(**{n: (0 if n == field else p.value) for n, _ in _lib.MobgsLpipsWeights._fields_})
        assert call(weights=ctypes.byref(broken)) == INVALID, field
    misaligned = _lib.MobgsLpipsWeights(**{n: p.value + (4 if n == "w2" else 0) for n, _ in _lib.MobgsLpipsWeights._fields_})
    assert call(weights=ctypes.byref(misaligned)) == INVALID
    taps = (ctypes.c_void_p * 5)(p.value, p.value, 0, p.value, p.value)
    assert call(taps=taps) == INVALID
    with pytest.raises(RuntimeError, match="mobgs_lpips_alex"):
        _lib.check(call(H=30), "mobgs_lpips_alex")


def test_python_refusals_need_no_gpu():
    from mobgs_amd import lpips as L
    model = object.__new__(L.LpipsAlex)                                 # no device, no weights: the checks come first
    a = torch.rand(1, 3, 40, 40)
    with pytest.raises(RuntimeError, match="no CPU path"):
        model(a, a)
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.forward(a, a)
    with pytest.raises(NotImplementedError):
        model.forward(a, a, mask=torch.ones(1, 1, 40, 40))
    with pytest.raises(NotImplementedError):
        model.forward(a, a, spatial=True)
    with pytest.raises(TypeError):
        model(a.numpy(), a)


def test_external_vectors():
    """Present only after scripts/dump_lpips_vectors.py ran where torchvision, its AlexNet file and the reference are
    installed; skipped otherwise (README, "UNPINNED").  Checks the restatement, the thing every GPU test trusts, against
    what the reference's own PerceptualLoss returned for the recorded trunk checksum and images."""
    path = os.path.join(GOLDEN, "lpips_external", "perceptual_loss.npz")
    if not os.path.exists(path):
        pytest.skip("no tests/golden/lpips_external/perceptual_loss.npz (scripts/dump_lpips_vectors.py): UNPINNED")
    ex = dict(np.load(path))
    trunk_path = os.environ.get("MOBGS_ALEXNET_TRUNK")
    if not trunk_path or not os.path.exists(trunk_path):
        pytest.skip("MOBGS_ALEXNET_TRUNK does not name torchvision's alexnet-owt-7be5be79.pth")
    trunk = torch.load(trunk_path, map_location="cpu")
    assert abs(float(trunk["features.0.weight"].double().sum()) - float(ex["trunk_checksum"])) <= 1e-9
    heads = LR.reference_heads()
    for n, i in enumerate(ex["case"].tolist()):
        c = LR.make_case(i)
        assert np.array_equal(LR.probe(c), ex["probe"][n])
        v, _ = LR.evaluate(c, trunk, heads, torch.float64)
        want = ex["lpips"][int(ex["first"][n]):int(ex["first"][n + 1])]
        assert np.allclose(v[:, 0].numpy(), want, rtol=1e-4, atol=1e-7), LR.case_name(i)
