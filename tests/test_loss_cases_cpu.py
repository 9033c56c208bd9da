"""tests/loss_cases.py checked from the oracles alone (no GPU): every SSIM / L1 and normals case reaches the edge it is named
after, the restatements the planted errors are built from are the oracle's own statements, the window allowance is what
the module says it is, and the comparators at k = 3 accept the fp32 oracle and reject each planted error in a named case."""
import functools

import pytest
import torch

import loss_cases as C
from oracle import loss_torch as L
from oracle import normals_torch as N


# ---- SSIM + L1 ---------------------------------------------------------------------------------------------------------
def _tiles(n):
    return (n + C.TILE - 1) // C.TILE


def test_sizes_reach_the_tile_edges():
    assert C.SSIM_SIZES == ((1, 1), (5, 6), (16, 16), (17, 16), (16, 17), (15, 33), (48, 48))
    have = {(C.ssim_case(n).H, C.ssim_case(n).W) for n in C.SSIM_CASES}
    assert have == set(C.SSIM_SIZES)
    R = C.RADIUS
    # (5, 6): no pixel whose window lies inside the image in either axis; over both ends in every row position
    assert all(y - R < 0 and y + R >= 5 for y in range(5)) and all(x - R < 0 or x + R >= 6 for x in range(6))
    assert (_tiles(16), _tiles(17), _tiles(15), _tiles(33), _tiles(48)) == (1, 2, 1, 3, 3)
    assert 17 - C.TILE == 1 and 33 % C.TILE == 1 and 15 % C.TILE != 0  # one live row / column in the last tile; ragged
    lo, hi = C.TILE - R, 2 * C.TILE + R  # the 26-wide patch of the centre tile of 48 x 48
    assert 0 <= lo and hi <= 48 and hi - lo == 26
    assert {C.ssim_case(n).B for n in C.SSIM_CASES} == {0, 1, 2}
    for content in C.CONTENTS:
        assert f"{content}_48x48" in C.SSIM_CASES and f"{content}_17x16" in C.SSIM_CASES


def test_layouts():
    c = C.ssim_case("noisy_16x17_permuted")
    assert not c.img.is_contiguous() and tuple(c.img.shape) == (2, 3, 16, 17) and c.img.stride(1) == 1
    c = C.ssim_case("noisy_15x33_nobatch")
    assert tuple(c.img.shape) == (3, 15, 33) and C.calls_of(c) == ("photo_0.2", "photo_1.0", "photo_0", "ssim_mean")
    assert C.calls_of(C.ssim_case("noisy_1x1")) == C.CALLS


@pytest.mark.parametrize("size", ["48x48", "17x16"])
def test_contents_reach_their_regime(size):
    H, W = (int(v) for v in size.split("x"))
    flat = C.ssim_case(f"flat_{size}")
    assert torch.equal(flat.gt, torch.full_like(flat.gt, 0.7)) and 0 < float((flat.img - flat.gt).abs().max()) < 0.01
    r64, r32, _ = C.ssim_reference(flat.name, "ssim_mean")
    m64 = C.ssim_map(flat.img.double(), flat.gt.double(), C.oracle_window())
    m32 = C.ssim_map(flat.img, flat.gt, C.oracle_window())
    gap = float((m32.double() - m64).abs().max())
    print(f"flat {size}: the fp32 oracle's SSIM map is {gap:.2e} from float64 (mean: {C.rel_gap(r32['value'], r64['value']):.2e})")
    assert gap > 1e-6  # the cancellation of E[x^2] - mu^2 against C2 = 9e-4: far above one fp32 rounding of a value near 1
    black = C.ssim_case(f"black_{size}")
    assert not black.img.any() and not black.gt.any()
    for call in ("photo_0.2", "photo_0"):
        r64, r32, _ = C.ssim_reference(black.name, call)
        assert float(r64["value"]) == 0.0 and not r64["grad"].any() and not r32["grad"].any()
    eq = C.ssim_case(f"equal_block_{size}")
    same = (eq.img == eq.gt).all(dim=1)[0]
    r0, r1 = C.BLOCK[0], min(C.BLOCK[1], H)
    c0, c1 = C.BLOCK[0], min(C.BLOCK[1], W)
    assert same[r0:r1, c0:c1].all() and r0 < C.TILE < r1  # ... on both sides of a tile edge
    if size == "48x48":
        assert (r1 - r0, c1 - c0) == (20, 20) and c0 < C.TILE < c1  # around the tile corner (16, 16)
    assert int(same.sum()) < (r1 - r0) * (c1 - c0) + 0.02 * H * W  # and (clamped pixels aside) nowhere else
    g0 = C.ssim_reference(eq.name, "photo_0")[0]["grad"]
    assert not g0[..., r0:r1, c0:c1].any() and g0[..., :r0, :].abs().min() > 0  # lambda = 0: exactly 0 on the block only
    assert C.ssim_reference(eq.name, "photo_0.2")[0]["grad"][..., r0:r1, c0:c1].abs().min() > 0
    oor = C.ssim_case(f"out_of_range_{size}")
    assert float(oor.img.min()) <= -0.2 and float(oor.img.max()) >= 1.3
    noisy = C.ssim_case(f"noisy_{size}")
    assert 0.0 <= float(noisy.img.min()) and float(noisy.img.max()) <= 1.0


def test_per_image_cotangents_put_both_arms_in_one_launch():
    for name in ("noisy_48x48", "noisy_17x16", "noisy_16x17_permuted"):
        r64 = C.ssim_reference(name, "per_image_b")[0]
        assert r64["grad"][0].abs().min() > 0 and not r64["grad"][1].any()
        ra = C.ssim_reference(name, "per_image_a")[0]
        assert ra["grad"][0].abs().min() > 0 and ra["grad"][1].abs().min() > 0 and tuple(ra["value"].shape) == (2,)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_ssim_map_restates_the_oracle_bit_for_bit(dtype):
    g = C.taps().unsqueeze(1)
    assert torch.equal(C.oracle_window(), g.mm(g.t()).float())
    for name in ("noisy_48x48", "noisy_15x33_nobatch", "flat_17x16"):
        case = C.ssim_case(name)
        a, b = case.img.to(dtype), case.gt.to(dtype)
        assert torch.equal(C.ssim_map(a, b, C.oracle_window()).mean(), L.ssim(a, b))
    case = C.ssim_case("noisy_17x16")
    m = C.ssim_map(case.img.to(dtype), case.gt.to(dtype), C.oracle_window())
    assert torch.equal(m.mean(1).mean(1).mean(1), L.ssim(case.img.to(dtype), case.gt.to(dtype), size_average=False))


def test_window_allowance_is_small_against_the_fp32_gap():
    """max |ref64_separable - ref64| comes from references alone; it is far below the fp32 oracle's own gap, so it cannot
    carry an error of the kernel."""
    w, s = C.oracle_window().double(), C.separable_window()
    assert s.dtype == torch.float64 and 0 < float((w - s).abs().max()) <= 2.0 ** -24 * float(s.max())
    worst = (0.0, None)
    for name in C.SSIM_CASES:
        case = C.ssim_case(name)
        for call in C.calls_of(case):
            r64, r32, sep = C.ssim_reference(name, call)
            extra, gap = C.window_extra(r64, sep, "grad"), float((r32["grad"].double() - r64["grad"]).abs().max())
            vextra = float((sep["value"] - r64["value"]).abs().max())
            if call == "photo_0" or case.content == "black":
                assert extra == 0.0 and vextra == 0.0
                continue
            assert vextra <= 1e-8, (name, call, vextra)
            if gap > 0 and extra / gap > worst[0]:
                worst = (extra / gap, f"{name} {call}: window {extra:.2e} gap {gap:.2e}")
    print(f"largest window allowance in units of the fp32 gap of the same gradient: {worst[0]:.3f} ({worst[1]})")
    assert worst[0] <= 0.5


def _scales(case, call, dtype):
    return C.call_scales(case, call, dtype)


def test_term_allowance_is_the_cancellation_of_the_gradients_terms():
    """One-pixel planes: the terms of the SSIM gradient are 3 to 165 times their sum.  On images the floor stays within a few
    times 2^-23 max |gradient|."""
    r64 = C.ssim_reference("noisy_1x1", "per_image_a")[0]
    ratio = (C.term_magnitude("noisy_1x1", "per_image_a") / r64["grad"].abs()).reshape(-1)
    print("noisy_1x1: terms / gradient per plane", [round(float(v), 1) for v in ratio])
    assert float(ratio.min()) > 2 and float(ratio.max()) > 100
    for name in C.SSIM_CASES:
        case = C.ssim_case(name)
        for call in C.calls_of(case):
            r64 = C.ssim_reference(name, call)[0]
            t = C.term_magnitude(name, call)
            assert t.shape == r64["grad"].shape and bool((t >= r64["grad"].abs() * (1 - 1e-9)).all()), (name, call)
            if call == "photo_0":
                assert C.term_extra(name, call, r64) == 0.0  # |sign| is the gradient
    big = C.ssim_reference("noisy_48x48", "photo_0.2")[0]
    assert C.term_extra("noisy_48x48", "photo_0.2", big) <= 4 * 2.0 ** -23 * float(big["grad"].abs().max())


@pytest.mark.parametrize("call", ["photo_0.2", "photo_0", "per_image_a"])
def test_manual_backward_is_the_oracles_gradient(call):
    """The formula the planted errors are applied to: equal to autograd through the oracle in float64, and accepted by the
    comparator in fp32."""
    for name in ("noisy_48x48", "equal_block_17x16", "flat_48x48", "out_of_range_17x16"):
        case = C.ssim_case(name)
        r64, r32, _ = C.ssim_reference(name, call)
        g64 = C.manual_grad(case.img.double(), case.gt.double(), *_scales(case, call, torch.float64), C.oracle_window())
        assert float((g64 - r64["grad"]).abs().max()) <= 1e-10 * float(r64["grad"].abs().max()), (name, call)
        g32 = C.manual_grad(case.img, case.gt, *_scales(case, call, torch.float32), C.oracle_window())
        C.compare_ssim(case, call, r32["value"], g32, f"manual fp32 {name} {call}")


def _rejected(case, call, grad, what):
    with pytest.raises(AssertionError):
        C.compare_ssim(case, call, C.ssim_reference(case.name, call)[1]["value"], grad, what)


def test_planted_error_missing_factor_two_is_rejected():
    for name in ("noisy_48x48", "noisy_17x16", "noisy_5x6"):
        case = C.ssim_case(name)
        bad = C.manual_grad(case.img, case.gt, *_scales(case, "photo_0.2", torch.float32), C.oracle_window(), e11_factor=1.0)
        _rejected(case, "photo_0.2", bad, f"planted (a) {name}")


def test_planted_error_padding_at_the_tile_edge_is_rejected():
    for name in ("noisy_48x48", "noisy_17x16", "noisy_16x17", "noisy_15x33", "flat_48x48"):
        case = C.ssim_case(name)
        _rejected(case, "photo_0.2", C.tiled_grad(case, 0.2, torch.float32), f"planted (b) {name}")
    one = C.ssim_case("noisy_16x16")  # one tile: the tile edge IS the image edge, and the same statement is accepted
    C.compare_ssim(one, "photo_0.2", C.ssim_reference(one.name, "photo_0.2")[1]["value"], C.tiled_grad(one, 0.2, torch.float32),
                   "tiled 16x16")


def test_planted_error_sign_of_zero_is_rejected():
    for name, call in (("equal_block_48x48", "photo_0"), ("equal_block_17x16", "photo_0.2"), ("black_48x48", "photo_0.2"),
                       ("black_17x16", "photo_0")):
        case = C.ssim_case(name)
        bad = C.manual_grad(case.img, case.gt, *_scales(case, call, torch.float32), C.oracle_window(), sign_of_zero=1.0)
        _rejected(case, call, bad, f"planted (c) {name}")


def test_scalar_rule_has_teeth():
    case = C.ssim_case("noisy_48x48")
    r64, r32, _ = C.ssim_reference(case.name, "photo_0.2")
    C.compare_ssim(case, "photo_0.2", r32["value"], r32["grad"], "fp32 oracle")
    with pytest.raises(AssertionError):
        C.compare_ssim(case, "photo_0.2", r32["value"] * (1 + 2e-5), r32["grad"], "value off by 2e-5")
    with pytest.raises(AssertionError):
        C.compare_ssim(case, "photo_0.2", r32["value"] * float("nan"), r32["grad"], "NaN value")


# ---- normals -----------------------------------------------------------------------------------------------------------
def test_normals_sizes_and_cameras():
    sizes = {(C.normals_case(n).H, C.normals_case(n).W) for n in C.NORMALS_CASES}
    assert sizes == {(1, 1), (1, 7), (2, 5), (3, 3), (3, 300), (16, 16), (17, 16), (20, 24)}
    blocks = lambda h, w: (h * w + 255) // 256
    assert blocks(3, 300) == 4 and blocks(16, 16) == 1 and blocks(17, 16) == 2 and 17 * 16 - 256 == 16
    assert not any(C.normals_case(f"smooth_{s}").interior for s in ("1x1", "1x7", "2x5"))
    assert C.normals_case("smooth_3x3").interior
    c1, c2 = C.cameras()
    assert c1.use_center and c1.skew != 0
    assert not c2.use_center and c2.skew == 0 and c2.principal_point_x < 0 and c2.principal_point_y > 20
    assert tuple(N.get_normals(torch.ones(1, 1, 7), *C.oracle_args(c1)).shape) == (1, 3, 2, 7)  # no reference for H = 1
    for s in ("1x1", "1x7", "2x5"):
        r64, r32 = C.normals_reference(f"smooth_{s}")
        H, W = (int(v) for v in s.split("x"))
        assert tuple(r64["normals"].shape) == (1, 3, H, W) and not r64["normals"].any() and not r64["grad"].any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_restated_normals_are_the_oracles(dtype):
    for name in C.NORMALS_CASES:
        case = C.normals_case(name)
        if not case.interior:
            continue
        a = C.normals_eval(case, dtype)
        b = C.normals_eval(case, dtype, fn=C.restated_normals)
        assert torch.equal(a["normals"], b["normals"]), name
        # (F.normalize and n / |n|.clamp_min(eps) differentiate to the same formula in a different order)
        assert float((a["grad"] - b["grad"]).abs().max()) <= 64 * torch.finfo(dtype).eps * float(a["grad"].abs().max()), name


@pytest.mark.parametrize("name", [n for n in C.NORMALS_CASES if C.normals_case(n).interior])
def test_no_raw_length_near_the_clamp_and_exact_zeros(name):
    case = C.normals_case(name)
    r64, r32 = C.normals_reference(name)
    raw64 = C.raw_normals(case.z.double(), C.oracle_args(case.cam)).norm(dim=-1)
    raw32 = C.raw_normals(case.z, C.oracle_args(case.cam)).norm(dim=-1)
    assert not ((raw64 >= 1e-13) & (raw64 <= 1e-11)).any() and not ((raw32 >= 1e-13) & (raw32 <= 1e-11)).any()
    assert torch.equal(raw64 < 1e-12, raw32 < 1e-12)  # both precisions on the same side of the clamp: no flip allowance
    fwd, bwd = C.normals_strata(name)
    assert torch.equal(fwd["hole"][1:-1, 1:-1], raw64 < 1e-12)
    n = r64["normals"][0]
    assert not n[:, fwd["border"]].any()
    assert float((n[:, fwd["unit"]].norm(dim=0) - 1).abs().max()) < 1e-12
    g = r64["grad"][0]
    H, W = case.H, case.W
    assert all(float(g[i, j]) == 0.0 for i in (0, H - 1) for j in (0, W - 1)) and not r32["grad"][0][bwd["corner"]].any()
    frame = torch.ones(H, W, dtype=torch.bool)
    frame[1:-1, 1:-1] = False
    for i in (0, H - 1):
        for j in (0, W - 1):
            frame[i, j] = False
    assert frame.any() and g[frame].abs().min() > 0  # each border pixel is a neighbour of one interior centre
    assert torch.isfinite(r32["normals"]).all() and torch.isfinite(r32["grad"]).all()
    if case.content == "smooth":
        assert not fwd["hole"].any() and float(case.z.min()) >= 2.0
        return
    assert float(case.depth.min()) == 0.0 and float(case.z.min()) == float(torch.tensor(1e-6))
    (r0, r1, c0, c1), (s0, s1, d0, d1) = C.HOLES
    assert fwd["hole"][r0 + 1:r1 - 1, c0 + 1:c1 - 1].all() and fwd["hole"][1:s1 - 1, d0 + 1:d1 - 1].all()
    assert int(fwd["hole"].sum()) == (r1 - r0 - 2) * (c1 - c0 - 2) + (s1 - 2) * (d1 - d0 - 2)
    assert d1 == W and s0 == 0  # the second hole touches the border: its border pixels carry a clamped centre's gradient
    assert bwd["hole"][0, d0 + 1:d1 - 1].all() and bwd["hole"][1:s1 - 1, W - 1].all()
    length = n[:, fwd["hole"]].norm(dim=0)
    inside, outside = float(g[bwd["hole"]].abs().max()), float(g[bwd["unit"]].abs().max())
    rel = float((r32["grad"][0].double() - g)[bwd["hole"]].abs().max()) / inside
    print(f"{name}: |n| in the hole {float(length.min()):.2e} .. {float(length.max()):.2e}; |gradient| {inside:.2e} in the "
          f"hole, {outside:.2e} outside; the fp32 oracle's relative gradient gap in the hole {rel:.2e}")
    assert 1e-5 < float(length.min()) and float(length.max()) < 1e-1  # n / 1e-12: not a unit vector
    assert inside > 1e4 * outside


def test_two_dimensional_input_is_part_of_the_contract():
    case = C.normals_case("smooth_20x24")
    a = N.get_normals(case.z.double(), *C.oracle_args(case.cam))
    assert tuple(a.shape) == (1, 3, 20, 24) and tuple(case.z[0].shape) == (20, 24)


def _normals_rejected(name, what, **kw):
    case = C.normals_case(name)
    bad = C.normals_eval(case, torch.float32, **kw)
    with pytest.raises(AssertionError):
        C.compare_normals(name, bad["normals"], bad["grad"], what)


def test_normals_comparator_accepts_the_fp32_oracle():
    for name in C.NORMALS_CASES:
        r32 = C.normals_reference(name)[1]
        C.compare_normals(name, r32["normals"], r32["grad"], f"fp32 oracle {name}")


def test_planted_error_use_center_ignored_is_rejected():
    for name in ("smooth_17x16_cam2", "smooth_3x300_cam2", "holes_20x24_cam2"):
        args = C.oracle_args(C.normals_case(name).cam)
        _normals_rejected(name, f"planted (a) {name}", cam_args=args[:5] + (0.5,))


def test_planted_error_clamp_dropped_is_rejected():
    for name in ("holes_20x24", "holes_20x24_cam2"):
        _normals_rejected(name, f"planted (b) {name}", fn=functools.partial(C.restated_normals, eps=0.0))
    ok = C.normals_eval(C.normals_case("smooth_20x24"), torch.float32, fn=functools.partial(C.restated_normals, eps=0.0))
    C.compare_normals("smooth_20x24", ok["normals"], ok["grad"], "no clamp, no hole")  # only a hole reaches the clamp


def test_planted_error_rows_and_columns_swapped_is_rejected():
    for name in ("smooth_17x16", "smooth_20x24", "smooth_3x300", "holes_20x24_cam2"):
        _normals_rejected(name, f"planted (c) {name}", fn=functools.partial(C.restated_normals, swap=True))
