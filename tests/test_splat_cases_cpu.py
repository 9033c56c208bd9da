"""tests/splat_cases.py checked from the oracles alone (no GPU): every case keeps its near-kink filter under the 5 % cap and
reaches the edge it is named after, fp32 and float64 agree on every discrete decision of the kept rows, the prep restatement
reproduces a render fixture of the reference, and the per-row comparator rejects a wrong backward term that the per-tensor
max-scaled rule of the end-to-end tests lets through."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import splat_cases as S
from helpers import close, load
from oracle.render_torch import hermite


# ---- projection --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.PROJ_CASES)
def test_projection_case_filter_strata_and_branches(name):
    case = S.proj_case(name)
    code = S.proj_strata(case)
    counts = {s: int((code == i).sum()) for i, s in enumerate(S.STRATA)}
    print(f"projection {name}: N {case.N} C {case.C}, dropped {case.dropped:.2%} of the candidates, culled "
          f"{int((code < 0).sum())}, visible {counts}")
    assert case.dropped <= S.MAX_DROP
    geom = (case.C, case.N) if case.own else (case.N,)
    assert case.means.shape == geom + (3,) and case.quats.shape == geom + (4,) and case.scales.shape == (case.N, 3)
    assert case.viewmats.shape == (case.C, 4, 4) and case.Ks.shape == (case.C, 3, 3)
    T = S.proj_terms_of(case)
    assert not S.proj_near_kink(T, case.W, case.H, case.near_plane, case.far_plane, case.radius_clip).any()
    # the restatement that the filter and the strata read IS the oracle (float64; einsum orders differ in the last bits)
    ref64, ref32 = S.proj_reference(name)
    assert torch.equal(T.radii, ref64["radii"])
    for key in S.PROJ_OUTPUTS:
        assert torch.allclose(getattr(T, key), ref64[key], rtol=1e-12, atol=1e-12), key
    # after the filter fp32 and float64 decide alike on every row: radii, and with them every cull
    assert torch.equal(ref32["radii"], ref64["radii"])
    T32 = S.proj_terms_of(case, torch.float32)
    for axis in ("x_clamped", "y_clamped"):
        assert torch.equal(getattr(T32, axis) | ~T.zok, getattr(T, axis) | ~T.zok)
    # un-normalised quaternions, anisotropic scales, fx != fy, off-centre principal point, a camera away from the origin
    qn = case.quats.norm(dim=-1)
    assert float(qn.min()) < 0.5 < 2.0 < float(qn.max()) or case.N < 63
    K = case.Ks[0]
    assert K[0, 0] != K[1, 1] and K[0, 2] != case.W / 2 and K[1, 2] != case.H / 2
    assert not torch.equal(case.viewmats[0], torch.eye(4))
    assert [c is None for c in case.cots] == [not u for u in S._ONLY.get(name, (True, True, True))]


@pytest.mark.parametrize("name", ["n1100", "n1100_only2d", "n1100_onlydepth", "n1100_onlyconic", "clip", "c3_shared",
                                  "c3_own"])
def test_every_visible_stratum_is_populated(name):
    case = S.proj_case(name)
    code = S.proj_strata(case)
    for key in ("means2d", "v_means", "v_scales"):
        rows = S.proj_row_strata(case, key)
        assert set(rows) == set(S.STRATA)
        least = 30 if name == "clip" else 50
        assert all(r.numel() >= least for r in rows.values()), (key, {s: r.numel() for s, r in rows.items()})
    if name == "clip":  # (its culls take rows of every stratum away)
        return
    vis = code[0][code[0] >= 0]  # camera 0 (the further cameras stand back and see more of the rows inside the image)
    assert vis.numel() >= 0.25 * case.N  # a quarter and more of the rows is visible ...
    assert float((vis > 0).double().mean()) >= 0.5  # ... and of those half and more lie beyond a frustum limit


def test_wave_and_workgroup_tails():
    assert [S.PROJ_SHAPES[f"n{n}"] for n in (1, 63, 64, 65, 255, 256, 257)] == [(n, 1) for n in (1, 63, 64, 65, 255, 256, 257)]
    one = S.proj_case("n1")
    assert int(S.proj_strata(one)[0, 0]) == 3  # the only row is visible and clamped in x and in y
    n = S.proj_case("many_rows").N
    assert -(-n // 256) == 258 > 256 and n % 256 == 1  # viewmat_reduce_kernel's strided loop runs twice for 2 threads
    assert -(-S.proj_case("n256").N // 256) == 1 and -(-S.proj_case("n257").N // 256) == 2


def test_near_plane_rows_cross_the_plane():
    case = S.proj_case("n1100")
    z = S.proj_terms_of(case).z[0]
    sweep = z[(z > -0.25) & (z < 0.035)]
    print(f"n1100: {sweep.numel()} rows within the sweep, {int((sweep >= case.near_plane).sum())} in front of the near plane")
    assert sweep.numel() >= 50 and (sweep < case.near_plane).sum() >= 40 and (sweep >= case.near_plane).sum() >= 2


def test_clip_case_populates_both_culls():
    case = S.proj_case("clip")
    assert case.radius_clip == 4.0 and case.far_plane == 5.0
    T = S.proj_terms_of(case)
    near, far = T.z < case.near_plane, T.z > case.far_plane
    mx, my, r = T.mean2d[..., 0], T.mean2d[..., 1], T.radius
    inside = T.zok & ~((mx + r <= 0) | (mx - r >= case.W) | (my + r <= 0) | (my - r >= case.H))
    small = inside & (r <= case.radius_clip)
    print(f"clip: culled by the near plane {int(near.sum())}, by the far plane {int(far.sum())}, by radius_clip alone "
          f"{int(small.sum())}, visible {int((T.radii > 0).sum())}")
    assert near.sum() >= 20 and far.sum() >= 100 and small.sum() >= 10
    assert not T.radii[near | far | small].any() and (T.radii[inside & ~small] > case.radius_clip).all()


def test_all_culled_is_all_zero_in_the_reference():
    case = S.proj_case("all_culled")
    assert (S.proj_terms_of(case).z < 0).all() and case.C == 2
    for ref in S.proj_reference("all_culled"):
        for key, t in ref.items():
            assert not t.any(), key


def test_per_camera_geometry_and_camera_poses():
    own, shared = S.proj_case("c3_own"), S.proj_case("c3_shared")
    assert own.means.dim() == 3 and own.quats.dim() == 3 and shared.means.dim() == 2
    assert not torch.equal(own.means[0], own.means[1]) and not torch.equal(own.quats[1], own.quats[2])
    for case in (own, shared):
        for c in range(1, case.C):
            assert not torch.allclose(case.viewmats[c, :3, :3], case.viewmats[0, :3, :3], atol=1e-2)
            assert not torch.allclose(case.viewmats[c, :3, 3], case.viewmats[0, :3, 3], atol=1e-2)
    # per-camera geometry: one oracle call per camera, the scale gradient is the sum over the cameras
    ref64, _ = S.proj_reference("c3_own")
    assert ref64["v_means"].shape == own.means.shape and ref64["v_scales"].shape == own.scales.shape
    assert ref64["v_viewmats"].shape == (3, 4, 4) and not ref64["v_viewmats"][:, 3].any()


# ---- prep --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.PREP_CASES)
def test_prep_case_shapes_and_knot_counts(name):
    case = S.prep_case(name)
    present = sorted(set(case.d_ncp.reshape(-1).tolist()))
    print(f"prep {name}: Ns {case.Ns} Nd {case.Nd} K {case.K}, times {case.times.tolist()}, knot counts {present}")
    if case.Nd >= 9:
        assert present == list(S.KNOTS)  # every count in every case that has room for them
    assert case.leaves["d_control"].shape == (case.Nd, 12, 3) and case.d_ncp.dtype == torch.int64
    assert set(case.leaves) == set(S.LEAVES) and len(case.cots) == 5
    ref64, ref32 = S.prep_reference(name)
    lead = (case.K,) if case.times.dim() == 2 else ()
    N = case.Ns + case.Nd
    assert [tuple(ref64[k].shape) for k in S.PREP_OUTPUTS] == [lead + (N, 3), lead + (N, 4), (N, 3), (N,), lead + (N, 9)]
    # knots beyond a row's count take no gradient, and the static f_t none either
    for j, n in enumerate(case.d_ncp.reshape(-1).tolist()):
        assert not ref64["d_control"][j, n:].any()
    assert not ref64["s_ft"].any() and not ref64["colors"][..., :case.Ns, 6:].any()
    if case.half:
        for k in S.HALF_LEAVES:
            assert torch.equal(case.leaves[k].half().float(), case.leaves[k])


def test_prep_shapes_straddle_the_wave_and_the_workgroup():
    sizes = {n: S.PREP_SHAPES[n][0] for n in S.PREP_CASES}
    assert sizes["s0_d1"] == (0, 1) and sizes["s1_d0"] == (1, 0) and sizes["d257"] == (0, 257) and sizes["s300"] == (300, 0)
    assert sizes["wave_63_2"][0] % 64 == 63  # the dynamic rows start inside a wave: prep_bwd_clear_rows clears 1 + 1 rows
    assert sizes["wave_64_64"] == (64, 64)  # ... exactly at a wave
    ns, nd = sizes["wave_100_157"]
    assert ns % 64 and ns < 256 < ns + nd == 257  # ... inside a wave, and the rows run into a second workgroup
    assert S.prep_case("k3").times.shape == (3, 2) and sizes["accumulate"] == sizes["half"] == sizes["k3"] == (100, 157)


def test_times_at_the_ends_on_knots_and_outside():
    assert S.prep_case("ends_0").times.tolist() == [0.0, 0.0] and S.prep_case("ends_1").times.tolist() == [1.0, 1.0]
    lo, hi = S.prep_case("outside_lo").times.tolist(), S.prep_case("outside_hi").times.tolist()
    assert lo[0] < 0 == lo[1] and hi[0] > 1 == hi[1]  # t_feat outside [0, 1], t_curve clamped: an exposure offset
    k3 = S.prep_case("k3").times
    assert k3[2, 0] > 1 and k3[2, 1] == 1
    for name, (q, counts) in S.ON_KNOTS.items():
        t = S.prep_case(name).times
        assert t[0] == t[1] == np.float32(1.0 / q)
        for n in S.KNOTS:
            on_knot = (Fraction(1, q) * (n - 1)).denominator == 1
            assert on_knot == (n in counts), (name, n)
            if on_knot:  # in fp32 the product lands on the knot or one ulp beside it: either segment may be taken
                ts = float(np.float32(t[1].item()) * np.float32(n - 1))
                assert abs(ts - round(ts)) <= 2.0 ** -22 * ts


def test_spline_and_its_control_gradient_are_continuous_across_a_knot():
    """Why times on knots are not filtered: u = 1 of one segment gives the value and the control-point gradient of
    u = 0 of the next, so the two branches of floor(t (n - 1)) agree at the knot -- shown from the oracle in float64."""
    case = S.prep_case("on_knots_2")
    ctrl = case.leaves["d_control"].double()
    cot = torch.randn(case.Nd, 3, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    for n in S.KNOTS:
        ncp = torch.full((case.Nd, 1), n)
        for k in range(1, n - 1):
            res = []
            for dt in (-1e-10, 1e-10):  # the segment left of the knot, the segment right of it
                c = ctrl.clone().requires_grad_(True)
                t = torch.tensor(k / (n - 1) + dt, dtype=torch.float64)
                assert int(torch.floor(t * (n - 1))) == (k - 1 if dt < 0 else k)
                out = hermite(c, t, ncp)
                g, = torch.autograd.grad((out * cot).sum(), c)
                res.append((out.detach(), g))
            assert (res[0][0] - res[1][0]).abs().max() <= 1e-6 * ctrl.abs().max()
            assert (res[0][1] - res[1][1]).abs().max() <= 1e-6 * cot.abs().max()
    # and the fp32 evaluation AT the knots is as close to float64 as at interior times
    for name in S.ON_KNOTS:
        ref64, ref32 = S.prep_reference(name)
        for key in ("means", "d_control"):
            rows = S.prep_row_strata(S.prep_case(name), key)["dynamic"]
            mx, med = S.row_stats(ref32[key], ref64[key], rows, S.COLS[key])
            print(f"{name} {key}: fp32 against float64 max {mx:.2e} median {med:.2e}")
            assert mx <= 1e-5


def test_prep_restatement_reproduces_the_reference_render_fixture():
    """The dynamic positions and all colour features of tests/golden/render_train.npz (written by the reference's own
    render()) from the restatement in fp32; the fixture stores no rotations: those are the closed form r + tfp w."""
    fx = load("render_train")
    T = torch.from_numpy
    L = {"s_xyz": T(fx["in_s_xyz"]), "s_scaling": T(fx["in_s_scaling"]), "s_rotation": T(fx["in_s_rotation"]),
         "s_opacity": T(fx["in_s_opacity"]), "s_fdc": T(fx["in_s_features_dc"]), "s_ft": T(fx["in_s_features_t"]),
         "d_control": T(fx["in_d_control_xyz"]), "d_scaling": T(fx["in_d_scaling"]), "d_rotation": T(fx["in_d_rotation"]),
         "d_omega": T(fx["in_d_omega"]), "d_opacity": T(fx["in_d_opacity"]), "d_fdc": T(fx["in_d_features_dc"]),
         "d_ft": T(fx["in_d_features_t"])}
    time = float(fx["in_cam"][2])
    means, quats, scales, opac, colors = S.prep_state(L, T(fx["in_d_current_control_num"]), T(fx["in_d_trbf_center"]),
                                                      torch.tensor([time, time]))
    ns = L["s_xyz"].shape[0]
    close(means[ns:], fx["out_means_3d"], 1e-6, 1e-6, "dynamic means")
    close(colors, fx["out_colors_precomp_final"], 1e-6, 1e-6, "colour features")
    tfp = time - T(fx["in_d_trbf_center"])
    assert torch.equal(quats[ns:], L["d_rotation"] + tfp * L["d_omega"]) and torch.equal(quats[:ns], L["s_rotation"])
    close(scales[ns:], torch.exp(L["d_scaling"]), 1e-6, 0, "dynamic scales")
    close(opac[:ns], torch.sigmoid(L["s_opacity"])[:, 0], 1e-6, 0, "static opacities")


# ---- the comparators ---------------------------------------------------------------------------------------------------
def _rejected(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def test_row_comparator_sees_a_wrong_clamp_term_that_the_max_scaled_rule_does_not():
    """A backward pass that takes the UNCLAMPED branch of persp_setup's vector-Jacobian product for the rows clamped in x
    (fp32, otherwise the oracle): the per-tensor rule of the end-to-end tests passes its position gradient, the per-row
    comparator at the widest k the GPU tests may use rejects it in the two strata that clamp in x, and nowhere else."""
    case = S.proj_case("n1100_onlyconic")  # (next to a means2d cotangent the Jacobian's own path is a 1e-6 of the row)
    ref64, ref32 = S.proj_reference("n1100_onlyconic")

    def wrong(means, quats, scales, V, Ks):
        return S.project_terms(means, quats, scales, V, Ks, case.W, case.H, case.near_plane, case.far_plane,
                               case.radius_clip, torch.float32, straight_x=True)
    swapped = S.proj_eval(case, torch.float32, project=wrong)
    for key in S.PROJ_OUTPUTS:  # the forward pass is untouched
        assert torch.allclose(swapped[key], ref32[key], rtol=1e-5, atol=1e-6)
    key, strata = "v_means", S.proj_row_strata(case, "v_means")
    norm = ref64[key].abs().amax(1)
    # the rows a per-tensor bound cannot see: clamped in x, own gradient below 1e-4 of the tensor's largest entry
    hit = torch.cat([strata["x-clamped"], strata["both"]])
    hit = hit[norm[hit] < 1e-4 * norm.max()]
    bad = {key: ref32[key].clone()}
    bad[key][hit] = swapped[key][hit]
    rel = (bad[key].double() - ref64[key]).abs().amax(1) / norm.clamp_min(1e-300)
    print(f"wrong clamp term in {hit.numel()} of {strata['x-clamped'].numel() + strata['both'].numel()} rows clamped in x: "
          f"relative row error median {float(rel[hit].median()):.2e}, largest |row| / max |tensor| "
          f"{float(norm[hit].max() / norm.max()):.2e}")
    assert hit.numel() >= 20 and float(rel[hit].median()) > 1e-2  # wrong by far more than rounding in those rows ...
    assert S.max_scaled_close(bad[key], ref64[key])  # ... and still inside atol = 5e-4 max |grad|
    for name, rows in strata.items():
        one = {name: rows}
        assert _rejected(S.rows_close_to_f64, bad[key], ref64[key], ref32[key], one, 3, 8, "wrong " + name) == \
            (name in ("x-clamped", "both")), name
        S.rows_close_to_f64(ref32[key], ref64[key], ref32[key], one, 3, 1, "fp32 reference " + name)  # accepts the honest one


def test_row_comparator_sees_one_knot_count_off_by_1e4():
    """Prep: the control-point gradients of the rows with 7 knots scaled by 1 + 1e-4."""
    case = S.prep_case("wave_100_157")
    ref64, ref32 = S.prep_reference("wave_100_157")
    key, strata = "d_control", S.prep_row_strata(case, "d_control")
    bad = ref32[key].clone()
    bad[strata["knots7"]] *= 1.0 + 1e-4
    assert S.max_scaled_close(bad, ref64[key])
    assert _rejected(S.rows_close_to_f64, bad, ref64[key], ref32[key], strata, 36, 8, "wrong knots7")
    for name, rows in strata.items():
        assert _rejected(S.rows_close_to_f64, bad, ref64[key], ref32[key], {name: rows}, 36, 8, "wrong " + name) == \
            (name in ("knots7", "dynamic")), name
    S.rows_close_to_f64(ref32[key], ref64[key], ref32[key], strata, 36, 1, "fp32 reference")
    # one rounding to half is what `shrink` takes off, and no more
    g = ref64["d_scaling"]
    assert torch.equal(S.shrink(g.half(), g, S.half_allowance(g)), g)
    assert not torch.equal(S.shrink(g * (1 + 2.0 ** -9), g, S.half_allowance(g)), g)
