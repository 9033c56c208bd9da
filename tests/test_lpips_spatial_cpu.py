"""CPU checks around the spatial and masked forms of LPIPS (include/mobgs_hip.h K24, mobgs_lpips_alex_spatial): the
nearest-neighbour rule and the upsample-size quirk against torch, the empty-mask conventions, tests/golden/lpips_spatial.npz,
the refusals of the C ABI and of the Python wrappers.  Nothing here launches a kernel."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_restatement as LR
import lpips_spatial_restatement as LS
from helpers import load


@pytest.fixture(scope="module")
def fx():
    return load("lpips_spatial")


@pytest.fixture(scope="module")
def nets():
    return LR.seeded_trunk(), LR.reference_heads()


def test_nearest_rule_is_torch_and_the_integer_rule_is_not():
    """min((int)floorf(i sH), H - 1) with sH = (float)H / (float)h and an fp32 product is what F.interpolate samples, for
    every tap edge of every image edge in 31 .. 699; the exact integer rule (i H) // h is not."""
    integer_differs = 0
    for H in range(31, 700):
        src = torch.arange(H, dtype=torch.float32).reshape(1, 1, H, 1)
        for h in sorted(set(LS.tap_edges(H))):
            want = F.interpolate(src, size=(h, 1))[0, 0, :, 0].long().numpy()
            assert np.array_equal(LS.nearest_index(h, H), want), (H, h)
            integer_differs += not np.array_equal(np.arange(h) * H // h, want)
    assert integer_differs == 77


def test_quirk_sizes_and_the_size_form():
    """Where floor(h (H / h)) = H the reference's scale_factor form gives an H-row map that agrees with the size= form;
    elsewhere it gives H - 1 rows, and the reference cannot add its five maps."""
    pairs = [(H, h) for H in range(31, 1500) for h in sorted(set(LS.tap_edges(H)))]
    bad = [p for p in pairs if LS.quirk(*p)]
    assert len(bad) == 403 and {(49, 11), (61, 14), (98, 11)} <= set(bad)
    assert not any(LS.quirk(H, h) for H in (288, 512, 1014, 1352) for h in LS.tap_edges(H))
    assert LS.quirk(49, LS.tap_edges(49)[0]) and LS.quirk(61, LS.tap_edges(61)[0])          # the fixture's quirk case
    g = torch.Generator().manual_seed(1)
    for H, h in ((49, 11), (61, 14), (98, 11)):
        d = torch.rand(1, 1, h, 5, generator=g, dtype=torch.float64)
        assert LS.reference_upsample(d, H, 5 * 7).shape[2] == H - 1
    for H, W in ((64, 97), (130, 67), (288, 512), (33, 35)):
        hs, ws = LS.tap_edges(H), LS.tap_edges(W)
        if any(LS.quirk(H, h) for h in hs) or any(LS.quirk(W, w) for w in ws):
            continue
        for h, w in zip(hs, ws):
            d = torch.rand(2, 1, h, w, generator=g, dtype=torch.float64)
            want = LS.reference_upsample(d, H, W)
            got = F.interpolate(d, size=(H, W), mode="bilinear", align_corners=False)
            # the two forms round the scale differently (1 / (H / h) against h / H): a source coordinate up to max(h, w)
            # moves by a few of its float64 ulps, and so does the weight of a neighbour, on values in [0, 1)
            assert got.shape == want.shape and float((got - want).abs().max()) <= 16 * max(h, w) * 2.0 ** -53


def test_bilinear_statement_is_torch():
    """The kernel's statement of the upsample (src = max(s (dst + 0.5) - 0.5, 0), i1 = i0 + (i0 < h - 1)) in float64 against
    F.interpolate(size=), on the quirk size too."""
    g = torch.Generator().manual_seed(2)
    for H, W, h, w in ((49, 61, 11, 14), (31, 31, 1, 1), (130, 67, 7, 3), (64, 97, 15, 23)):
        d = torch.rand(h, w, generator=g, dtype=torch.float64)

        def axis(n_out, n_in):
            src = np.maximum(n_in / n_out * (np.arange(n_out) + 0.5) - 0.5, 0)
            i0 = src.astype(np.int64)
            return i0, i0 + (i0 < n_in - 1), torch.from_numpy(src - i0)

        (y0, y1, ty), (x0, x1, tx) = axis(H, h), axis(W, w)
        ty, tx = ty[:, None], tx[None, :]
        got = (1 - ty) * ((1 - tx) * d[y0][:, x0] + tx * d[y0][:, x1]) + ty * ((1 - tx) * d[y1][:, x0] + tx * d[y1][:, x1])
        want = F.interpolate(d[None, None], size=(H, W), mode="bilinear", align_corners=False)[0, 0]
        assert float((got - want).abs().max()) <= 1e-14


def test_empty_mask_conventions():
    g = torch.Generator().manual_seed(4)
    ds = [torch.rand(2, 1, h, w, generator=g, dtype=torch.float64) for h, w in ((7, 9), (3, 4), (1, 1), (1, 1), (1, 1))]
    val = LS.spatial_map(ds, 35, 43)
    empty = torch.zeros(2, 35, 43)
    assert (LS.dycheck_mean(val, empty) == 0).all()
    layers, num, den = LS.masked_layers(ds, empty)
    assert (layers == 0).all() and (num == 0).all() and (den == 0).all()
    v = LS.values(ds, val, empty)
    assert torch.isfinite(v).all() and (v[:, 0] > 0).all() and (v[:, 1:] == 0).all()
    # one pixel: dycheck's mean is the map there; the reference's average is d at the tap pixels that sample it
    one = empty.clone()
    one[:, 0, 0] = 1
    assert torch.equal(LS.dycheck_mean(val, one), val[:, 0, 0, 0])
    layers, num, den = LS.masked_layers(ds, one)
    assert (den == 1).all() and torch.equal(num, torch.stack([d[:, 0, 0, 0] for d in ds], 1))


@pytest.mark.parametrize("i", (0, 5))
def test_fixture_reproduces(fx, nets, i):
    c = LS.make_case(i)
    masks = [LS.make_mask(i, n) for n in LS.MASKS]
    assert np.array_equal(LS.probe(c, masks), fx["probe"][i])
    m64, v64 = LS.evaluate(c, masks, *nets, torch.float64)
    assert np.allclose(v64.numpy(), LS.rows(fx, i), rtol=1e-12, atol=0)
    m32, v32 = LS.evaluate(c, masks, *nets, torch.float32)
    assert np.allclose(v32.double().numpy(), LS.rows(fx, i, "f32"), rtol=2e-5, atol=0)
    assert LS.map_gap(m32, m64) <= 4 * max(fx["map_gap_f32"].max(), fx["map_gap_seq"].max())
    if i in LS.CL_CASES:
        n = LS.CL_CASES.index(i)
        for k, name in enumerate(LS.CL_MASKS):
            got = LS.compute_lpips(c, LS.make_mask(i, name), *nets, torch.float64)
            assert np.allclose(got.numpy(), fx["cl_f64"][n, k], rtol=1e-12, atol=0), name


def test_fixture_is_not_degenerate(fx):
    assert len(fx["probe"]) == len(LS.CASES) == 7
    assert fx["first"][-1] == fx["f64"].shape[0] == len(LS.MASKS) * sum(c[2] for c in LS.CASES)
    assert fx["cl_f64"].shape == (len(LS.CL_CASES), len(LS.CL_MASKS)) and (fx["cl_f64"] > 1e-3).all()
    for i, (H, W, B, what) in enumerate(LS.CASES):
        v = LS.rows(fx, i)
        if what == "identical":
            assert (v == 0).all()
            continue
        k = {n: j for j, n in enumerate(LS.MASKS)}
        assert (v[:, :, 0] > 3e-3).all() and (v[:, :, 0] < 3e-2).all()                    # the map's mean
        assert np.array_equal(v[k["ones"], :, 1], v[k["ones"], :, 0])                      # all ones: the masked mean is the mean
        for n in ("bernoulli", "rect", "soft", "first", "last"):
            assert (v[k[n], :, 1] > 1e-4).all(), n
        assert (v[k["empty"], :, 1:] == 0).all()
        for n in ("ones", "soft"):                       # (a 1 x 1 tap samples mask pixel (0, 0), outside the rectangle)
            assert (v[k[n], :, 2:] > 0).all(), n
        assert (v[k["rect"], :, 2:4] > 0).all()
        assert (v[k["first"], :, 3:] > 0).all()          # tap pixel (0, 0) samples mask pixel (0, 0)
    # the trap: some masks are empty at a tap, and the layer value is then exactly 0
    assert (fx["f64"][:, 3:] == 0).sum() > (fx["f64"][:, 0] == 0).sum() * 5
    gaps = LS.reference_gaps(fx)
    assert set(gaps) == set(LS.QUANTITIES)
    assert all(1e-8 < g < 2e-5 for g in gaps.values()), gaps
    assert all(LS.tolerance(q, gaps) >= LS.FLOOR for q in gaps)


def test_abi_declares_the_spatial_entry_points():
    from mobgs_amd import _lib, lpips as L
    h = _lib.load()
    P = ctypes.c_void_p
    assert _lib._SIGS["mobgs_lpips_spatial_scratch_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    assert _lib._SIGS["mobgs_lpips_alex_spatial"] == (ctypes.c_int, [ctypes.c_int] * 3 + [P] * 4 +
                                                      [ctypes.c_int, P, ctypes.c_size_t, P, P, P])
    assert _lib.ABI_VERSION == 16 and L.SPATIAL_COLUMNS == 21
    for B, H, W in ((1, 31, 31), (3, 64, 97), (2, 1014, 1352)):
        plain, spatial = h.mobgs_lpips_scratch_bytes(B, H, W), h.mobgs_lpips_spatial_scratch_bytes(B, H, W)
        pixels = sum(a * b for a, b in L.tap_sizes(H, W))
        assert spatial % 256 == 0 and plain + 4 * B * pixels < spatial < plain + 8 * B * pixels + 32 * B * (H * W // 1024 + 8) + 4096
    for bad in ((0, 64, 64), (4097, 64, 64), (1, 30, 64), (1, 64, 30), (1, 16385, 64), (4096, 4096, 4096)):
        assert h.mobgs_lpips_spatial_scratch_bytes(*bad) == 0, bad


def test_bad_arguments_are_refused_before_any_launch():
    from mobgs_amd import _lib
    h = _lib.load()
    none = ctypes.c_void_p(None)
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)         # a 256-byte aligned host address: never dereferenced
    fields = [n for n, _ in _lib.MobgsLpipsWeights._fields_]
    rec = _lib.MobgsLpipsWeights(**{n: p.value for n in fields})
    INVALID = _lib._DEFINES["MOBGS_E_INVALID"]

    def call(B=1, H=64, W=64, img0=p, img1=p, weights=ctypes.byref(rec), mask=none, flags=1, scratch=p, nbytes=1 << 40,
             fmap=none, out=p):
        h.mobgs_lpips_alex(0, 64, 64, *[none] * 3, 0, none, 0, none, none, none)      # leaves another entry point's message
        rc = h.mobgs_lpips_alex_spatial(B, H, W, img0, img1, weights, mask, flags, scratch, nbytes, fmap, out, none)
        assert b"mobgs_lpips_alex_spatial" in h.mobgs_last_error(), h.mobgs_last_error()
        return rc

    off = lambda k: ctypes.c_void_p(p.value + k)  # noqa: E731
    for kw in (dict(B=0), dict(B=4097), dict(H=30), dict(W=30), dict(H=16385), dict(img0=none), dict(img1=none),
               dict(weights=none), dict(scratch=none), dict(out=none), dict(flags=8), dict(flags=-1),
               dict(nbytes=h.mobgs_lpips_spatial_scratch_bytes(1, 64, 64) - 1),
               dict(nbytes=h.mobgs_lpips_scratch_bytes(1, 64, 64)),             # the plain call's scratch is too short
               dict(scratch=off(16)), dict(out=off(4)), dict(img0=off(2)), dict(mask=off(2)), dict(fmap=off(1))):
        assert call(**kw) == INVALID, kw
    for field in ("w3", "b1", "lin5"):
        broken = _lib.MobgsLpipsWeights(**{n: (0 if n == field else p.value) for n in fields})
        assert call(weights=ctypes.byref(broken)) == INVALID, field
    misaligned = _lib.MobgsLpipsWeights(**{n: p.value + (4 if n == "w2" else 0) for n in fields})
    assert call(weights=ctypes.byref(misaligned)) == INVALID
    assert b"mobgs_lpips_spatial_scratch_bytes(1, 64, 64)" in (call(nbytes=16) and h.mobgs_last_error())
    with pytest.raises(RuntimeError, match="mobgs_lpips_alex_spatial"):
        _lib.check(call(H=30), "mobgs_lpips_alex_spatial")


def test_python_refusals_need_no_gpu():
    from mobgs_amd import lpips as L
    from mobgs_amd.metrics import compute_lpips
    model = object.__new__(L.LpipsAlex)                                 # no device, no weights: the checks come first
    a = torch.rand(1, 3, 40, 40)
    for call in (lambda: model.spatial(a, a), lambda: model.forward_spatial(a, a),
                 lambda: model.forward_masked(a, a, torch.ones(1, 1, 40, 40)),
                 lambda: compute_lpips(model, a[0].permute(1, 2, 0), a[0].permute(1, 2, 0))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    with pytest.raises(TypeError):
        model.spatial(a.numpy(), a)
    # forward keeps refusing both, and names the calls that do them
    with pytest.raises(NotImplementedError, match="forward_masked"):
        model.forward(a, a, mask=torch.ones(1, 1, 40, 40))
    with pytest.raises(NotImplementedError, match="forward_spatial"):
        model.forward(a, a, spatial=True)
    assert L.LpipsSpatial._fields[:7] == ("map", "mean", "masked_mean", "masked_total", "masked_per_layer", "numerators",
                                          "denominators")
    like = torch.empty(2, 3, 40, 41, device="meta")
    assert L._mask("x", None, like) is None
