"""The cases of tests/tof_cases.py are what they claim, from the references alone (numpy, tests/tof_restatement.py): the fp32
twin of the restatement stays inside the per-element bounds with the recorded factors, every case reaches the edge it is
named after, the comparator rejects five planted errors (and today's relative-to-maximum rule of tests/test_gpu_tof.py is
recorded beside it), and every end-to-end case keeps its sample positions away from the in-bounds test's jump by 100 times
the fp32 twin's own flow error.  No kernel runs here."""
import numpy as np
import pytest

import tof_cases as TC
import tof_restatement as TR
from test_gpu_tof import allowed as old_allowed       # the relative-to-maximum allowances, for the record of what they accept


def test_float64_is_the_default_and_fp32_is_fp32():
    rng = np.random.default_rng(0)
    img = np.rint(rng.uniform(0, 255, size=(50, 75)))
    lv = TR.levels(50, 75)[0]
    a = TR.pyramid_level(img, lv)
    assert a.dtype == np.float64 and np.array_equal(a, TR.pyramid_level(img, lv, np.float64))
    R = TR.poly_exp(a[:20, :24])
    R32 = TR.poly_exp(a[:20, :24], np.float32)
    assert R.dtype == np.float64 and R32.dtype == np.float32 and 0 < np.abs(R32 - R).max() < 1e-3
    flow = TR.smooth_flow(20, 24, 1, 2.0)
    M = TR.update_matrices(R, R[:, ::-1].copy(), flow)
    M32 = TR.update_matrices(R, R[:, ::-1].copy(), flow, np.float32)
    assert M.dtype == np.float64 and M32.dtype == np.float32 and TR.resize_bilinear(flow, 40, 48, np.float32).dtype == np.float32
    # the solve keeps its float64 sums: only the result is rounded
    assert np.array_equal(TR.blur_solve(M32, np.float32), TR.blur_solve(M32.astype(np.float64)).astype(np.float32))
    assert TR.pyramid_level(img, lv, np.float32).dtype == np.float32


def test_fp32_twin_stays_within_the_bounds():
    """For every case, stage and stratum: the fp32 twin against float64 with the recorded C, k <= 1, and the share of the
    bound it uses; the smallest factor that would do is measured per stage and must be the recorded one."""
    used = {s: 0.0 for s in TC.STAGES}
    for shape, kind in TC.stage_cases():
        c = TC.stage_case(shape, kind)
        for stage, st in c.stage.items():
            for _, _, _, stratum, k in TC.compare(c, stage, st.twin, "fp32 twin", limit=1.0):
                used[stage] = max(used[stage], k * TC.C[stage])
    for stage in TC.STAGES:
        print(f"[tof] fp32 twin, {stage}: smallest factor {used[stage]:.3f}, recorded C = {TC.C[stage]:g} "
              f"({used[stage] / TC.C[stage]:.0%} of the bound)")
        assert used[stage] <= TC.C[stage] and TC.C[stage] >= 1.0
        assert TC.C[stage] <= max(1.0, 1.1 * used[stage]), f"{stage}: C is not the smallest factor"


def test_cases_reach_their_edges():
    for shape in TC.SHAPES:
        h, w = TC.LEVEL_HW[shape]
        c = TC.stage_case(shape, "smooth")
        assert (c.h, c.w) == (h, w) and set(c.stage) == set(TC.STAGES) - (set() if c.image else {"pyramid"})
        for stage in c.stage:
            tags = TC.case_strata(c, stage)
            covered = np.zeros((h, w), bool)
            for m in tags.values():
                covered |= m
            assert covered.all()
    tags = TC.case_strata(TC.stage_case("48x48", "smooth"), "solve")
    assert not tags["tail"].any() and tags["seams"].sum() == 48 * 48 - 44 * 44 and tags["interior"].any()
    assert tags["corners"].sum() == 4 * 49
    y, x = np.mgrid[0:49, 0:65]
    tags = TC.case_strata(TC.stage_case("49x65", "smooth"), "polyexp")
    assert np.array_equal(tags["tail"], (x == 64) | (y == 48)) and tags["interior"].any()      # one-pixel tails on both axes
    y, x = np.mgrid[0:32, 0:33]
    assert np.array_equal(TC.case_strata(TC.stage_case("32x33", "smooth"), "polyexp")["tail"], x == 32)
    assert TC.stage_case("32x33", "smooth").level[2:] == (19, 3.5) and TC.stage_case("49x65", "smooth").level[2:] == (3, 0.5)
    # 7x13 is narrower than every window, and its border bands overlap: rows 2 to 4 carry the factor of both sides
    small = TC.stage_case("7x13", "smooth")
    for stage in ("polyexp", "update", "solve"):
        tags = TC.case_strata(small, stage)
        assert tags["tail"].all() and not tags["interior"].any() and not tags["seams"].any()
    assert 7 < 2 * len(TR.BORDER) and 7 < 2 * TR.POLY_N + 1 and 13 < TR.WINSIZE
    s = TR.border_factor(7, 13)
    both = [y for y in range(7) if y < 5 and y >= 7 - 5]
    assert both == [2, 3, 4] and abs(s[3, 6] - 0.4472 ** 2) < 1e-18 and abs(s[2, 0] - 0.4472 ** 2 * 0.14) < 1e-18
    assert abs(s[0, 12] - 0.14 * 0.14) < 1e-18 and abs(TR.border_factor(2, 2)[0, 1] - 0.14 ** 4) < 1e-18
    assert TC.case_strata(TC.stage_case("2x2", "smooth"), "update")["corners"].all()
    # the update flows leave the image somewhere, and some sample lands in the last column, where `<` and `<=` part
    for shape in ("48x48", "49x65", "32x33"):
        flow = TC.stage_case(shape, "smooth").stage["update"].inp[1][0]
        h, w = flow.shape[:2]
        fx, fy = TR.sample_positions(flow)
        assert 0.02 <= TR.out_of_bounds_share(flow) <= 0.3
        assert ((np.floor(fx) == w - 1) & (np.floor(fy) >= 0) & (np.floor(fy) < h - 1)).any()


def test_contents_are_what_they_are_named():
    """Every shape, the two small ones included (their texture is a finer one, tof_cases.SMALL; at 2x2 the properties are
    those of the case's two frames together, eight pixels): 8-bit values; 25 - 40 % of the saturated content at 0 or 255;
    at least four grey levels within 126 .. 130 in the low-contrast one; a flat left half beside a textured right one;
    and no content whose expansion coefficients vanish."""
    for shape in TC.SHAPES:
        cases = {k: TC.stage_case(shape, k) for k in TC.CONTENTS}
        imgs = {k: np.asarray(c.grey if c.image else c.stage["polyexp"].inp, np.float64) for k, c in cases.items()}
        for k, a in imgs.items():
            assert np.array_equal(a, np.rint(a)) and a.min() >= 0 and a.max() <= 255, (shape, k)      # 8-bit valued
            R = cases[k].stage["polyexp"].ref
            assert all(np.abs(R[f, ch]).max() > 1e-3 for f in range(2) for ch in range(5)), (shape, k)
            assert np.abs(cases[k].stage["update"].ref).max() > 0 and np.abs(cases[k].stage["solve"].ref).max() > 0
        low, share = imgs["low_contrast"], TC.saturated_share(imgs["saturated"])
        print(f"[tof] {shape}: saturated share {share:.1%}, low-contrast values {np.unique(low).tolist()}, smooth std "
              f"{imgs['smooth'].std():.1f}")
        assert 0.25 <= share <= 0.40, (shape, share)
        assert low.min() >= 126 and low.max() <= 130 and len(np.unique(low)) >= 4
        assert imgs["smooth"].std() > 20
        half = cases["const_half"]
        W = imgs["const_half"].shape[-1]
        assert np.all(imgs["const_half"][:, :, :W // 2] == 128) and imgs["const_half"][:, :, W // 2:].std() > 10
        if half.image:
            assert 5 < half.edge < half.w - 5
            assert TC.case_strata(half, "polyexp")["const"].any() and TC.case_strata(half, "update")["const"].any()
            assert TC.case_strata(half, "polyexp")["const_edge"].any()
        else:
            assert half.edge == W // 2


def test_closed_form_is_the_normal_equations():
    """The sum of absolute terms of the expansion uses the closed form of the 6x6 solve: with signs it IS that solve."""
    for shape in ("49x65", "7x13", "2x2"):
        img = TC.stage_case(shape, "saturated").stage["polyexp"].inp[0].astype(np.float64)
        want, got = TR.poly_exp(img), TC.polyexp_closed_form(img)
        T = TC.polyexp_closed_form(img, absolute=True)
        assert np.abs(got - want).max() <= 1e-10 and np.all(T >= np.abs(want) - 1e-10)


def test_exact_facts_of_the_references():
    """The finest level in fp32 equals float64 bit for bit (sigma 0: taps 1/4, 1/2, 1/4, identity resize, every intermediate
    a multiple of 1/16 below 256); a flat region's update matrices and flow are exactly 0 given exactly zero coefficients."""
    for shape in ("48x48", "49x65", "32x33"):
        for kind in TC.CONTENTS:
            c = TC.stage_case(shape, kind)
            H, W = c.image
            finest = TR.levels(H, W)[-1]
            assert finest == (W, H, 3, 0.0)
            a64 = TR.pyramid_level(c.grey[0], finest)
            assert np.array_equal(TR.pyramid_level(c.grey[0], finest, np.float32).astype(np.float64), a64)
            assert np.array_equal(a64 * 16, np.rint(a64 * 16)) and a64.max() <= 255
    R = np.zeros((2, 5, 20, 24))
    R[:, :, :, 16:] = np.random.default_rng(3).normal(size=(2, 5, 20, 8))
    flow = TR.smooth_flow(20, 24, 2, 1.5)
    M = TR.update_matrices(R[0], R[1], flow)
    assert np.all(M[:, :, :13] == 0) and np.all(TR.blur_solve(M)[:, :6] == 0)


# ---- planted errors --------------------------------------------------------------------------------------------------------
def _pyramid_with_replicate(grey, level):
    w, h, taps, sigma = level
    g = TR.gaussian_taps(taps, sigma)
    return TR.resize_bilinear(TR.correlate_axis(TR.correlate_axis(grey, g, 1, "edge"), g, 0, "edge"), h, w)


def _update_with(R0, R1, flow, monkeypatch, no_bottom=False, inclusive=False):
    """TR.update_matrices with the border factor's bottom side dropped, or with `x1 <= w - 1` (the tap x1 + 1 then read from
    the clamped column, where a kernel would read the next row)."""
    if no_bottom:
        h, w = flow.shape[:2]
        top = TR.border_factor(2 * h, w)[:h]
        monkeypatch.setattr(TR, "border_factor", lambda hh, ww: top)
        try:
            return TR.update_matrices(R0, R1, flow)
        finally:
            monkeypatch.undo()
    assert inclusive
    h, w = flow.shape[:2]
    pad = np.pad(R1, ((0, 0), (0, 0), (0, 1)), mode="edge")
    wide = np.pad(flow, ((0, 0), (0, 1), (0, 0)))
    wide[:, w] = 1e6                                              # (the added column itself is cut off again)
    R0w = np.pad(R0, ((0, 0), (0, 0), (0, 1)))
    s = TR.border_factor(h, w)
    monkeypatch.setattr(TR, "border_factor", lambda hh, ww: np.pad(s, ((0, 0), (0, 1))))
    try:
        return TR.update_matrices(R0w, pad, wide)[:, :, :w]      # in a level one column wider, x1 = w - 1 IS in bounds
    finally:
        monkeypatch.undo()


def _solve_with_short_window(M):
    """TR.blur_solve whose horizontal window misses its last tap in the last column of every tile."""
    box = np.full(TR.WINSIZE, 1.0 / TR.WINSIZE)
    out = []
    for m in M:
        rows = TR.correlate_axis(m, box, 1, "edge")
        p = np.pad(m, ((0, 0), (TR.WINSIZE // 2,) * 2), mode="edge")
        x = np.arange(m.shape[1])
        last = x[x % TC.TILE == TC.TILE - 1]
        rows[:, last] -= p[:, last + TR.WINSIZE - 1] / TR.WINSIZE
        out.append(TR.correlate_axis(rows, box, 0, "edge"))
    G11, G12, G22, h1, h2 = out
    det = G11 * G22 - G12 * G12 + 1e-3
    return np.stack([(G22 * h1 - G12 * h2) / det, (G11 * h2 - G12 * h1) / det], -1)


def _verdict(c, stage, planted):
    """(worst k of the comparator over the strata, worst relative-to-maximum error of the old rule over the channels)."""
    with pytest.raises(AssertionError):
        TC.compare(c, stage, planted, "planted")
    st = c.stage[stage]
    flow = stage == "solve"
    g, ref, T = (TC.planes(a) if flow else a for a in (planted, st.ref, st.T))
    k = TC.needed_k(g, ref, T, TC.C[stage])
    old = max(TC.rel_to_max(planted[:, ch], st.ref[:, ch]) for ch in range(st.ref.shape[1])) if stage in (
        "polyexp", "update") else TC.rel_to_max(planted, st.ref)
    return k, old


def test_planted_errors_are_rejected(monkeypatch):
    rows = []
    c = TC.stage_case("32x33", "smooth")
    planted = np.stack([_pyramid_with_replicate(g, c.level) for g in c.grey])
    rows.append(("replicate for reflect-101 in the pyramid blur", "pyramid") + _verdict(c, "pyramid", planted))
    c = TC.stage_case("49x65", "smooth")
    R, flow = (a.astype(np.float64) for a in c.stage["update"].inp)
    planted = _update_with(R[0], R[1], flow[0], monkeypatch, no_bottom=True)[None]
    assert np.array_equal(planted[:, :, :44], c.stage["update"].ref[:, :, :44])
    rows.append(("border factor without the bottom side", "update") + _verdict(c, "update", planted))
    planted = _update_with(R[0], R[1], flow[0], monkeypatch, inclusive=True)[None]
    changed = np.any(planted != c.stage["update"].ref, axis=(0, 1))
    assert changed.any() and changed.sum() <= 49                    # only pixels that sample the last column
    rows.append(("<= w - 1 in the in-bounds test", "update") + _verdict(c, "update", planted))
    planted = _solve_with_short_window(c.stage["solve"].inp[0][0].astype(np.float64))[None]
    rows.append(("box window of 14 in a tile's last column", "solve") + _verdict(c, "solve", planted))
    c = TC.stage_case("49x65", "const_half")
    st = c.stage["polyexp"]
    flat = TC.case_strata(c, "polyexp")["const"]
    planted = st.ref.copy()
    for ch in range(5):
        planted[:, ch][:, flat] += 1e-5 * np.abs(st.ref[:, ch]).max()
    rows.append(("flat half of the expansion off by 1e-5 of the largest value", "polyexp") + _verdict(c, "polyexp", planted))
    for what, stage, k, old in rows:
        print(f"[tof] PLANTED {what}: comparator k = {k:.3g} (allowed {TC.K}: rejected); relative to the maximum "
              f"{old:.2e} (allowed {old_allowed(stage):.2e}: {'accepted' if old <= old_allowed(stage) else 'rejected'})")
        assert k > TC.K
    assert rows[-1][3] <= old_allowed("polyexp")                    # the old rule lets the low-contrast error through


# ---- kink margins ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TC.END_TO_END) + list(TC.OLD_END_TO_END))
def test_kink_margins(name):
    """The smallest distance of any sample position of the float64 trace from x = 0, x = w - 1, y = 0, y = h - 1 (every
    update of every level and pair but the zero-flow first one) is at least 100 times the fp32 twin's largest flow error.
    The three cases of tests/test_gpu_tof.py are measured and recorded; they do not keep the margin, which is why each
    has a twin with a searched seed among the asserted ones."""
    margin, err = TC.kink_margin(name)
    H, W, F, seed = {**TC.OLD_END_TO_END, **TC.END_TO_END}[name]
    old = name in TC.OLD_END_TO_END
    print(f"[tof] KINK {name} (seed {seed}, {F} frames): margin {margin:.3e} px, fp32 twin's flow error {err:.3e} px, "
          f"ratio {margin / err:.0f} ({'recorded only' if old else f'asked {TC.MARGIN_RATIO:.0f}'})")
    assert seed not in (64, 257) and margin > 0 and len(TR.levels(H, W)) == {48: 1, 50: 1, 64: 2, 72: 2, 256: 4, 259: 4}[H]
    if not old:
        assert margin >= TC.MARGIN_RATIO * err
