"""tests/decoder_cases.py from the restatement alone: every case of tests/test_gpu_decoder_kernels.py reaches the edge it is
named after -- the kink margin and the redraw share, which entries are exactly zero (so that the comparator's exact-zero
rule is seen to cover them), where the pixel counts sit against the wave, the workgroup and the backward's 768 pixels per
workgroup, how many images and partial rows the batched and the fused cases have, and ref32 close to ref64."""
from types import SimpleNamespace

import pytest
import torch

import decoder_cases as C

SINGLE = [(P, ray, form) for P in C.SINGLE_P for ray in C.RAY_FORMS for form in C.DEPTH_FORMS]
BATCHED = [("pin34", ""), ("pin44", ""), ("pin34", "intr"), ("pin34", "c2w"), ("map", ""), ("map", "map")]


def test_every_synthetic_case_keeps_its_margin_and_redraws_few_pixels():
    shares, draws = [], []
    cases = [C.synth_case(P, ray, *form) for P, ray, form in SINGLE]
    cases += [C.synth_case(C.BATCH[1], ray, C=C.BATCH[0], share=share) for ray, share in BATCHED]
    cases += [C.synth_case(769, ray, False, CF, False, Cn) for ray in ("map", "pin34") for CF in (11, 12) for Cn in (1, 2)]
    cases.append(C.synth_case(C.BIG_P, "pin34"))
    for case in cases:
        s, z = C.pre_activations(case)     # float64, from the case as it stands
        assert float(s.abs().min()) == case.margin >= C.MARGIN, case.name
        assert float(z.abs().max()) == case.z_max < C.Z_MAX, case.name
        assert case.redrawn <= C.MAX_REDRAW and case.draws <= 4, case.name
        if case.has_depth:
            assert bool(((case.alphas == 0) == case.hole).all()) and float(case.alphas[~case.hole].min()) >= C.ALPHA_MIN
            assert not case.feat[..., 9][case.hole].any() and bool((case.feat[..., 9][~case.hole] > 0).all())
        shares.append((case.redrawn, case.P * case.C))
        draws.append(case.draws)
    pixels = sum(n for _, n in shares)
    print(f"REDRAW {len(cases)} cases: worst share {max(s for s, _ in shares):.2%}, "
          f"over all {sum(s * n for s, n in shares) / pixels:.2%} of {pixels} pixels, "
          f"large case {cases[-1].redrawn:.2%}; cases drawn again whole: {sum(d > 1 for d in draws)}")
    # both branches of every unit are taken somewhere in every case of some size
    for case in cases:
        if case.P * case.C >= 256:
            s, _ = C.pre_activations(case)
            assert bool(((s > 0).any(dim=2) & (s < 0).any(dim=2)).all()), case.name


def test_pixel_counts_sit_around_the_wave_the_workgroup_and_the_backward_grid():
    res = {P: (P % 64, P % 256, P % 768) for P in C.SINGLE_P}
    assert res[63] == (63, 63, 63) and res[64] == (0, 64, 64) and res[65] == (1, 65, 65)
    assert res[256][:2] == (0, 0) and res[257][:2] == (1, 1)
    assert res[767][2] == 767 and res[768][2] == 0 and res[769][2] == 1 and res[1537][2] == 1
    assert [C.bwd_rows(P) for P in (1, 767, 768, 769, 1537)] == [1, 1, 1, 2, 3]
    # a ragged last wave whose software-pipelined prefetch reads past the end: more than one workgroup, last wave partial
    for P in (769, 1537):
        assert C.bwd_rows(P) > 1 and P % 64 == 1
    for P, (H, W) in C.SHAPES.items():
        assert H * W == P
    assert C.BIG_P > 4096 * 256 and C.BIG_P % 256 == 65       # the forward grid-stride loop, with a ragged tail
    assert C.BIG_P <= 4096 * 768                               # ... below the backward grid cap, which is out of scope
    assert max(H for H, W in C.SHAPES.values()) > 1 and C.SHAPES[767][0] > 1 and C.SHAPES[1537][0] > 1


def test_batched_and_fused_cases_have_the_images_and_rows_they_claim():
    Cn, P = C.BATCH
    assert Cn == 3 and C.bwd_rows(P) == 2              # 3 images x 2 partial rows: an image's rows are not the first ones
    for ray, share in BATCHED:
        case = C.synth_case(P, ray, C=Cn, share=share)
        assert case.feat.shape == (Cn, P, 10) and case.v_rgb.shape == (Cn, 3, P)
        if ray == "map":
            assert case.rays.shape[0] == (1 if share == "map" else Cn)
        else:
            assert case.intr.shape == (1 if share == "intr" else Cn, 4)
            assert case.c2w.shape == (1 if share == "c2w" else Cn, 4 if ray == "pin44" else 3, 4)
        scales = case.v_rgb.abs().amax(dim=(1, 2))
        assert scales[1] > 1.5 * scales[0] > 2.0 * scales[2]      # a row credited to the wrong image shows
    ref64, _ = C.synth_reference(P, "pin34", C=Cn)
    g = ref64["g_c2w"]
    assert g.shape == (Cn, 3, 4) and float((g[0] - g[1]).abs().max()) > 0.1 * float(g.abs().max())
    grids = {k: C.tiles(W, H) for k, (W, H, _, _, _) in C.FUSED_GRIDS.items()}
    assert grids["tiny"] == (3, 2) and 37 % 16 and 21 % 16
    assert grids["small"] == grids["cams"] == (16, 11) and 250 % 16 == 170 % 16 == 10
    assert grids["large"] == (46, 45) and 46 * 45 == 2070 > max(1024, 64 * 32) and 728 % 16 == 712 % 16 == 8
    assert C.FUSED_GRIDS["cams"][4] == 3 and all(v[4] == 1 for k, v in C.FUSED_GRIDS.items() if k != "cams")


@pytest.mark.parametrize("P", [65, 769, 1537])
@pytest.mark.parametrize("ray", C.RAY_FORMS)
@pytest.mark.parametrize("form", C.DEPTH_FORMS)
def test_the_exact_zeros_of_the_reference_are_where_the_comparator_must_find_them(P, ray, form):
    has_depth, CF, depth_cot = form
    case = C.synth_case(P, ray, *form)
    ref64, ref32 = C.synth_reference(P, ray, *form)
    vf = ref64["v_feat"]
    assert vf.shape == (1, P, CF) and bool((vf[..., :3] != 0).all())
    dark = (C.pre_activations(case)[0] < 0).all(dim=1)      # all six units inactive: nothing reaches the layer's inputs
    assert bool(((vf[..., 3:9] == 0).all(dim=-1) == dark).all()) and bool(((vf[..., 3:9] != 0).all(dim=-1) == ~dark).all())
    if CF > 10:
        assert not vf[..., 10:].any()                       # channels the decoder does not read
    if has_depth:
        hole = case.hole
        assert int(hole.sum()) >= 3 and bool(hole[0, 0]) and bool(hole[0, P - 1])
        assert not ref64["depth"][hole].any() and bool((ref64["depth"][~hole] > 0).all())
        assert not ref64["v_alphas"][hole].any()            # alpha == 0: the clamp passes nothing on
        if depth_cot:
            assert bool((ref64["v_alphas"][~hole] != 0).all()) and bool((vf[..., 9] != 0).all())
            assert float(vf[..., 9][hole].abs().min()) > 1e6     # g / 1e-10: compared apart from everything else
        else:
            assert not ref64["v_alphas"].any() and not vf[..., 9].any()
    if ray == "map":
        assert "g_c2w" not in ref64 and bool(((ref64["v_rays"] != 0).all(dim=1) == ~dark).all())
    else:
        g = ref64["g_c2w"]
        assert g.shape == (1, 4 if ray == "pin44" else 3, 4) and bool((g[:, :3] != 0).all())
        if ray == "pin44":
            assert not g[:, 3].any()                        # the fourth pose row
    # the parts as they are compared carry those zeros, and ref32 has them too
    p64, p32 = C.parts(case, ref64), C.parts(case, ref32)
    assert set(p64) == set(p32)
    for name, (family, t) in p64.items():
        assert family in C.FAMILIES
        assert bool(((t == 0) == (p32[name][1] == 0)).all()), name


def test_ref32_is_close_to_ref64_everywhere():
    """The comparator's unit, max |ref32 - ref64|, is fp32 rounding and nothing else: below 64 ulp of each tensor's
    largest value in the per-pixel tensors and below 2^-16 of it in the sums over pixels."""
    worst = {f: 0.0 for f in C.FAMILIES}
    for P, ray, form in SINGLE:
        case = C.synth_case(P, ray, *form)
        ref64, ref32 = C.synth_reference(P, ray, *form)
        p64, p32 = C.parts(case, ref64), C.parts(case, ref32)
        for name, (family, t) in p64.items():
            _, gap, floor, _ = C.needed_k(t, t, p32[name][1])
            if floor > 0:
                worst[family] = max(worst[family], gap / floor)
    print("GAP in units of 2^-23 max |ref64|:", {k: round(v, 2) for k, v in worst.items()})
    assert worst["outputs"] < 64 and worst["cots"] < 64 and worst["weights"] < 128 and worst["pose"] < 128
    assert all(v > 0 for v in worst.values())


def test_forward_only_reference_of_the_large_case():
    case = C.synth_case(C.BIG_P, "pin34")
    ref64, ref32 = C.synth_reference(C.BIG_P, "pin34", forward_only=True)
    assert set(ref64) == {"rgb", "depth"} and ref64["rgb"].shape == (1, 3, C.BIG_P)
    assert not ref64["depth"][case.hole].any()
    assert float((ref64["rgb"] - ref32["rgb"].double()).abs().max()) < 1e-6
    # the direction differs from pixel to pixel all the way to the last one (W = 349547: fx grows with the width)
    rays = C.pinhole_rays(case.intr[0].double(), case.c2w[0].double(), case.H, case.W)
    assert float((rays[3:, -1] - rays[3:, -2]).abs().max()) > 1e-7


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_bias_weights_hold_every_unit_on_one_side(sign):
    """Features in [0, 1.2], unit directions, origin T_BIAS: no pixel near a kink, each unit on one side, the two weight
    sets on opposite sides."""
    w1, w2 = C.bias_weights(sign)
    t = torch.tensor(C.T_BIAS, dtype=torch.float64)
    assert float((w1[:, 6:9].double() @ t - sign * torch.tensor([3.0, -3, 3, -3, 3, -3])).abs().max()) < 1e-5
    g = torch.Generator().manual_seed(9)
    n = 200_000
    d = torch.randn(3, n, generator=g, dtype=torch.float64)
    x = torch.cat([1.2 * torch.rand(6, n, generator=g, dtype=torch.float64), t[:, None].expand(3, n), d / d.norm(dim=0)])
    s = w1.double() @ x
    print(f"BIAS sign {sign:+.0f}: min |s| = {float(s.abs().min()):.3f}")
    assert float(s.abs().min()) >= 0.5
    assert torch.equal(torch.sign(s).amin(dim=1), torch.sign(s).amax(dim=1))
    assert torch.equal(torch.sign(s[:, 0]), sign * torch.tensor([1.0, -1, 1, -1, 1, -1], dtype=torch.float64))
    img = torch.cat([x[:6].t().float(), torch.rand(n, 4, generator=g)], dim=1)[:, [6, 7, 8, 0, 1, 2, 3, 4, 5, 9]]
    case = C.rendered_case("bias", img.reshape(1, 400, 500, 10), torch.rand(1, 400, 500, generator=g), torch.tensor(
        [300.0, 300.0, 250.0, 200.0]), C.pose(0, 3, C.T_BIAS), w1, w2, 0)
    assert case.margin >= 0.5 and case.z_max < C.Z_MAX and torch.equal(*case.signs)
    assert bool((case.v_depth[case.hole] == 0).all()) and bool(case.hole.any()) and bool((case.v_depth[~case.hole] != 0).all())


# ---- the comparison notices the errors it is there for -------------------------------------------------------------------
def _with_cotangents_on(case, keep):
    """The case with its cotangents zeroed outside the pixels `keep` [C, P]: gradients are linear in the cotangents, so its
    weight and pose gradients are the contribution of those pixels."""
    sub = SimpleNamespace(**vars(case))
    sub.v_rgb = case.v_rgb * keep[:, None, :]
    sub.v_depth = case.v_depth * keep if case.v_depth is not None else None
    return sub


def _fails(case, got, ref64, ref32, names):
    """Every tensor of `names` fails the comparison with the k of the GPU tests; the other tensors of `got` pass."""
    for name in got:
        one = {name: got[name]}
        if name in names:
            with pytest.raises(AssertionError):
                C.compare(case, one, ref64, ref32, C.K, "mutant " + name, [name])
        else:
            C.compare(case, one, ref64, ref32, C.K, "mutant " + name, [name])


def test_a_wrong_relu_mask_on_one_hidden_unit_fails():
    """fp32 statements whose backward pass lets unit 3 through where it is inactive (the forward pass is untouched)."""
    def leaky_backward(s):
        e = torch.zeros_like(s)
        e[3] = torch.where(s[3] < 0, s[3], e[3])
        return torch.relu(s) + (e - e.detach())
    case = C.synth_case(769, "pin34")
    ref64, ref32 = C.synth_reference(769, "pin34")
    got = C.evaluate(case, torch.float32, relu=leaky_backward)
    assert torch.equal(got["rgb"], ref32["rgb"]) and torch.equal(got["g_w2"], ref32["g_w2"])
    _fails(case, got, ref64, ref32, {"v_feat", "g_w1", "g_c2w"})


def test_a_wrong_loc_term_in_the_pose_chain_fails():
    """The pose gradient's loc factor taken at the pixel's corner instead of its centre -- in the BACKWARD chain only, so
    that nothing but g_c2w can tell."""
    def corner_loc_backward(intr, c2w, H, W):
        right = C.pinhole_rays(intr, c2w, H, W)
        shifted = torch.stack([intr[0], intr[1], intr[2] + 0.5, intr[3] + 0.5])
        wrong = C.pinhole_rays(shifted, c2w, H, W)
        return right.detach() + (wrong - wrong.detach())
    for P in (769, 1537):
        case = C.synth_case(P, "pin34")
        ref64, ref32 = C.synth_reference(P, "pin34")
        got = C.evaluate(case, torch.float32, rays_fn=corner_loc_backward)
        _fails(case, got, ref64, ref32, {"g_c2w"})


def test_a_partial_row_credited_to_the_wrong_image_fails():
    """Batch of 3 x 769 pixels, two partial rows per image: the second row of image 1 (pixels 256..511 and 768, as the
    kernel's grid-stride loop deals them out) summed into image 0's pose gradient."""
    Cn, P = C.BATCH
    case = C.synth_case(P, "pin34", C=Cn)
    ref64, ref32 = C.synth_reference(P, "pin34", C=Cn)
    keep = torch.zeros(Cn, P)
    keep[1, 256:512] = keep[1, 768] = 1.0
    row = C.evaluate(_with_cotangents_on(case, keep), torch.float32)["g_c2w"][1]
    got = dict(ref32, g_c2w=ref32["g_c2w"].clone())
    got["g_c2w"][0] += row
    got["g_c2w"][1] -= row
    _fails(case, got, ref64, ref32, {"g_c2w"})


def test_a_tile_row_dropped_on_a_ragged_border_fails():
    """37 x 21 pixels = 3 x 2 tiles: the weight and pose sums without the 5 x 5 pixels of the last, ragged tile."""
    W, H = C.FUSED_GRIDS["tiny"][:2]
    g = torch.Generator().manual_seed(3)
    w1, w2 = C.bias_weights(1.0)
    img = 1.2 * torch.rand(1, H, W, 10, generator=g)
    case = C.rendered_case("tiny", img, 0.1 + 0.9 * torch.rand(1, H, W, generator=g), torch.tensor([32.0, 32.0, W / 2, H / 2]),
                           C.pose(0, 3, C.T_BIAS), w1, w2, 0)
    assert case.margin >= C.MARGIN
    ref64, ref32 = C.evaluate(case, torch.float64), C.evaluate(case, torch.float32)
    keep = torch.ones(H, W)
    keep[16:, 32:] = 0.0
    assert int((keep == 0).sum()) == 25
    got = C.evaluate(_with_cotangents_on(case, keep.reshape(1, -1)), torch.float32)
    got = {k: got[k] for k in ("g_w1", "g_w2", "g_c2w")}
    _fails(case, got, ref64, ref32, {"g_w1", "g_w2", "g_c2w"})
