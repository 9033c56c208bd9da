"""The cases of the LPIPS gradient tests, checked where no GPU is needed: every committed seed passes the kink vetting of
lpips_grad_cases (so the GPU test is not the first place a bad case shows), the probes, margins and reference gaps of
tests/golden/lpips_grad.npz describe these cases, the restated model has the bits of lpips_restatement.lpips, the float64
truth has the zeros the issue's cases are about, and the host side of the backward call -- the backward weight packing, the
header's entry points, the refusals that come before any launch -- works."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_grad_cases as G
import lpips_restatement as LR
from helpers import load, same_bits


@pytest.fixture(scope="module")
def fx():
    return load("lpips_grad")


@pytest.fixture(scope="module")
def nets():
    return LR.seeded_trunk(), LR.reference_heads()


def test_the_cases_are_the_issue_s():
    assert [c[:3] for c in G.CASES[:6]] == [(31, 31, 1), (31, 48, 2), (35, 33, 1), (38, 34, 1), (64, 97, 2), (130, 67, 2)]
    assert all(c[3] == "noisy" for c in G.CASES[:6])
    assert [c for c in G.CASES[6:]] == [(64, 97, 2, k) for k in ("identical", "clamp", "flat")]
    assert set(G.SEEDS) == {G.case_name(i) for i, c in enumerate(G.CASES) if c[3] != "flat"}
    assert G.MARGIN_FACTOR == 4.0


@pytest.mark.parametrize("i", range(len(G.CASES)))
def test_every_committed_case_passes_the_vetting(fx, nets, i):
    c = G.make_case(i)
    H, W, B, what = G.CASES[i]
    assert c["gt"].shape == c["pred"].shape == (B, 3, H, W) and c["gt"].dtype == c["pred"].dtype == np.float32
    assert np.array_equal(G.probe(c), fx["probe"][i])
    ok, reports = G.vet_case(c, nets[0], flat=what == "flat")
    tol = G.forward_tolerances()
    for b, pair in enumerate(reports):
        for side, r in zip(("gt", "pred"), pair):
            print(f"[lpips-grad-cases] {G.case_name(i)} pair {b} {side}: min |z| / margin {r['min_abs_z'] / r['margin']}, "
                  f"min pool gap / margin {r['min_pool_gap'] / r['margin'][:2]}")
            assert r["ok"] and r["zero_vectors"] == 0, (G.case_name(i), b, side, r)
            assert (r["min_abs_z"] >= r["margin"]).all() and (r["min_pool_gap"] >= r["margin"][:2]).all()
            assert (r["margin"] > 0).all() and (tol >= LR.FLOOR).all()
    assert ok
    # (float64 sums of another torch build may differ in their last bits; min |z| is a difference of terms ~1e5 x itself)
    assert np.allclose(fx["margin"][i], np.max([r[s]["margin"] for r in reports for s in (0, 1)], 0), rtol=1e-9)
    assert np.allclose(fx["min_abs_z"][i], np.min([r[s]["min_abs_z"] for r in reports for s in (0, 1)], 0), rtol=1e-3)
    if what == "identical":
        assert np.array_equal(c["gt"], c["pred"])
    if what == "clamp":
        for k in ("gt", "pred"):
            assert (c[k] < 0).sum() > 1000 and (c[k] > 1).sum() > 1000 and (c[k] == 0).sum() > 50 and (c[k] == 1).sum() > 50
    if what == "flat":
        assert len(np.unique(c["gt"])) == 1 and len(np.unique(c["pred"])) == 1 and c["gt"][0, 0, 0, 0] != c["pred"][0, 0, 0, 0]


def test_an_unvetted_image_is_refused(nets):
    """The vetting is no formality: 0.5, the constant of lpips_restatement's flat case, has a unit inside the margin, and a
    flat image without the same-chain rule fails on its ties."""
    x = torch.full((1, 3, 64, 97), 0.5, dtype=torch.float64)
    r = G.vet_image(x, nets[0], flat=True)
    assert not r["ok"] and (r["min_abs_z"] < r["margin"]).any()
    good = torch.full((1, 3, 64, 97), G.FLAT[0], dtype=torch.float64)
    assert G.vet_image(good, nets[0], flat=True)["ok"]
    r = G.vet_image(good, nets[0], flat=False)
    assert not r["ok"] and (r["min_pool_gap"] < r["margin"][:2]).all()      # (0, or a last bit where F.conv2d rounds unevenly)


def test_border_signatures():
    sigs = G.border_signatures(64, 97)
    from mobgs_amd.lpips import tap_sizes
    assert [tuple(s.shape) for s in sigs] == tap_sizes(64, 97)
    s = sigs[0]                                              # tap 1: 15 x 23; window rows 4 oy - 2 .. 4 oy + 8 of 64, columns of 97
    assert len(torch.unique(s[1:14, 1:22])) == 1            # the interior is one pattern
    assert s[0, 5] == s[0, 9] and s[5, 0] == s[9, 0]        # along a border the clipping repeats
    assert s[0, 5] != s[1, 5] and s[5, 0] != s[5, 1] and s[0, 0] != s[0, 5] and s[0, 5] != s[5, 0]


def test_model_has_the_bits_of_the_restatement(nets):
    for i in (G.CASES.index((31, 48, 2, "noisy")), G.CASES.index(G.EXTRA_SIZE + ("clamp",))):
        c = G.make_case(i)
        with torch.no_grad():
            want, (t0, t1) = LR.lpips(c["gt"], c["pred"], *nets, dtype=torch.float64, clamp=c["clamp"])
            total, _, (m0, m1) = G.model(torch.from_numpy(c["gt"]).double(), torch.from_numpy(c["pred"]).double(), *nets,
                                         clamp=c["clamp"])
        assert same_bits(total, want[:, 0])
        assert all(same_bits(a, b) for a, b in zip(t0 + t1, m0 + m1))


def test_truth_has_the_zeros_and_the_fixture_the_gaps(fx, nets):
    gaps = G.reference_gaps(fx)
    assert fx["gap_f32"].shape == fx["gap_seq"].shape == (len(G.CASES), len(G.QUANTITIES))
    for q in G.QUANTITIES:
        tol = G.tolerance(q, gaps)
        print(f"[lpips-grad-cases] {q}: reference gap {gaps[q]:.2e}, tolerance {tol:.2e}")
        assert LR.FLOOR <= tol == max(3 * gaps[q], LR.FLOOR) and 1e-7 < gaps[q] < 1e-4
    i = G.CASES.index((38, 34, 1, "noisy"))
    t = G.gradients(G.make_case(i), *nets)
    for s in (0, 1):
        g = t["image"][s]
        assert float(g[:, :, -1, :].abs().max()) == 0 and float(g[:, :, :, -1].abs().max()) == 0
        assert float(g[:, :, :-1, :-1].abs().min()) > 0
    # the fixture's gap of this case, measured again through F.conv2d in fp32
    got = G.gradients(G.make_case(i), *nets, dtype=torch.float32)
    row = [max(float(G.pair_gap(got[q][s], t[q][s]).max()) for s in (0, 1)) for q in G.QUANTITIES]
    for q, gap in zip(G.QUANTITIES, row):                    # (another build of torch may order its sums differently: the
        assert 0 < gap <= G.tolerance(q, gaps), (q, gap)     # reference's own fp32 run must pass the test it sets the bar for)
    i = G.CASES.index(G.EXTRA_SIZE + ("identical",))
    t = G.gradients(G.make_case(i), *nets)
    assert all(float(t[q][s].abs().max()) == 0 for q in G.QUANTITIES for s in (0, 1))
    assert (fx["gap_f32"][i] == 0).all() and (fx["gap_seq"][i] == 0).all()


def test_backward_weight_packing_is_the_backward_data_convolution():
    """conv(g, unpacked backward weight, pad) is autograd's gradient of the layer's input, for layers 2 .. 5."""
    from mobgs_amd.lpips import CIN, COUT, KS, PAD, bwd_pack_k, pack_conv_weight_bwd
    gen = torch.Generator().manual_seed(5)
    for layer in range(2, 6):
        cout, cin, k, pad = COUT[layer - 1], CIN[layer - 1], KS[layer - 1], PAD[layer - 1]
        w = torch.randn(cout, cin, k, k, generator=gen, dtype=torch.float64)
        x = torch.randn(1, cin, 6, 7, generator=gen, dtype=torch.float64, requires_grad=True)
        g = torch.randn(1, cout, 6, 7, generator=gen, dtype=torch.float64)
        (want,) = torch.autograd.grad(F.conv2d(x, w, padding=pad), x, g)
        packed = pack_conv_weight_bwd(w, layer)
        assert packed.shape == (bwd_pack_k(layer), cin) and bwd_pack_k(layer) % 32 == 0 and cin % 64 == 0
        # row (ky k + kx) Cout + co, column ci -> a [Cin, Cout, k, k] kernel over g
        as_conv = packed.reshape(k, k, cout, cin).permute(3, 2, 0, 1)
        got = F.conv2d(g, as_conv, padding=pad)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    with pytest.raises(ValueError):
        pack_conv_weight_bwd(torch.zeros(64, 3, 11, 11), 1)


def test_the_entry_point_is_declared_bound_and_refuses_before_any_launch():
    from mobgs_amd import _lib, loss_utils
    from mobgs_amd.lpips import LpipsAlex
    P = ctypes.c_void_p
    S = _lib._SIGS
    assert S["mobgs_lpips_alex_bwd"] == (ctypes.c_int, [ctypes.c_int] * 3 + [P] * 4 + [ctypes.c_int, P, P, P, ctypes.c_size_t]
                                         + [P] * 4)
    assert S["mobgs_lpips_bwd_scratch_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    assert S["mobgs_lpips_bwd_pack_k"] == (ctypes.c_int, [ctypes.c_int])
    assert [n for n, _ in _lib.MobgsLpipsBwdWeights._fields_] == ["w2", "w3", "w4", "w5"]
    assert callable(loss_utils.lpips_loss) and callable(LpipsAlex.loss)
    h = _lib.load()
    assert [h.mobgs_lpips_bwd_pack_k(l) for l in range(7)] == [0, 0, 4800, 3456, 2304, 2304, 0]
    assert h.mobgs_lpips_bwd_scratch_bytes(1, 30, 64) == 0 and h.mobgs_lpips_bwd_scratch_bytes(0, 64, 64) == 0
    one, two = h.mobgs_lpips_bwd_scratch_bytes(1, 64, 97), h.mobgs_lpips_bwd_scratch_bytes(2, 64, 97)
    assert 0 < one < two <= 2 * one and one % 256 == 0
    # refusals that need no device: host values that look like aligned device pointers are never dereferenced
    fake = P(1 << 20)
    rec, brec = _lib.MobgsLpipsWeights(), _lib.MobgsLpipsBwdWeights()
    ptrs = (P * 5)(*[1 << 20] * 5)
    invalid = _lib._DEFINES["MOBGS_E_INVALID"]

    def call(B, H, flags, g0, g1):
        return h.mobgs_lpips_alex_bwd(B, H, 64, fake, fake, ctypes.byref(rec), ctypes.byref(brec), flags, ptrs, fake, fake,
                                      1 << 30, g0, g1, None, None)
    assert call(1, 64, 1, None, None) == invalid and b"mobgs_lpips_alex_bwd" in h.mobgs_last_error()
    assert b"both NULL" in h.mobgs_last_error()
    assert call(1, 64, 1 | 4, None, fake) == invalid and b"QUANTIZE" in h.mobgs_last_error()
    assert call(1, 64, 8, fake, None) == invalid and b"unknown bits" in h.mobgs_last_error()
    assert call(1, 30, 1, fake, None) == invalid and b"below 31" in h.mobgs_last_error()
    assert call(0, 64, 1, fake, None) == invalid
    assert call(1, 64, 1, fake, None) == invalid and b"layer 1" in h.mobgs_last_error()   # the records hold NULL weights
