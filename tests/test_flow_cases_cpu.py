"""tests/flow_cases.py checked from the references alone (no GPU): every case is kink-free with the stated margins, the margins
are at least 100 x the fp32 reference's own error, every case reaches the edge it is named after, one dropped or doubled
contribution cannot hide under a tensor's maximum, and the comparator at k = 3 accepts the fp32 reference and rejects each
planted error at a strip end."""
import time

import pytest
import torch

import flow_cases as C

# the table of the change that introduced these cases: name -> (B, K, H, W)
TABLE = {"min_2x2": (1, 1, 2, 2), "row_pair_2x70": (1, 2, 2, 70), "col_pair_70x2": (1, 2, 70, 2), "w64": (1, 2, 9, 64),
         "w65": (1, 2, 9, 65), "w129": (2, 2, 19, 129), "rows_tail4": (1, 3, 37, 70), "tall8_a": (32, 2, 500, 70),
         "tall8_b": (256, 1, 33, 65), "below_tall": (255, 1, 33, 65), "white_noise_4": (2, 3, 37, 70),
         "white_noise_8": (32, 1, 500, 70), "pile_up": (1, 2, 37, 70), "shift": (1, 2, 37, 70), "clamp_left": (1, 1, 19, 70),
         "clamp_right": (1, 1, 19, 70), "clamp_top": (1, 1, 19, 70), "clamp_bottom": (1, 1, 19, 70),
         "clamp_corner": (1, 1, 19, 70), "holes": (2, 2, 37, 70), "smooth_a": (2, 3, 37, 70), "smooth_b": (1, 9, 67, 129)}


def _rows(c, combine=True):
    return C.expected_rows(c.B, c.H, c.W, combine)


# ---- the table and the builds ------------------------------------------------------------------------------------------
def test_case_table_and_builds():
    assert {n: (C.case(n).B, C.case(n).K, C.case(n).H, C.case(n).W) for n in C.CASES} == TABLE
    assert {C.case(n).v for n in C.CASES} == {1.0, 0.37, -2.5}
    # the rule, restated by hand: ceil(W / 64) ceil(H / 32) B >= 1024 and combine_taps
    assert C.expected_rows(32, 500, 70, True) == 8 and 2 * 16 * 32 == 1024
    assert C.expected_rows(256, 33, 65, True) == 8 and 2 * 2 * 256 == 1024
    assert C.expected_rows(255, 33, 65, True) == 4 and 2 * 2 * 255 == 1020
    assert C.expected_rows(2, 1014, 1352, True) == 8 and C.expected_rows(1, 1014, 1352, True) == 4  # training; the old test
    assert all(C.expected_rows(B, H, W, False) == 4 for B, _, H, W in TABLE.values())
    tall = [n for n in C.CASES if _rows(C.case(n)) == 8]
    assert tall == ["tall8_a", "tall8_b", "white_noise_8"]
    assert _rows(C.case("below_tall")) == 4
    # each of the three builds -- <true, 8>, <true, 4>, <false, 4> -- is reached by at least three cases
    assert len(tall) >= 3 and len(C.CASES) - len(tall) >= 3 and len(C.CASES) >= 3
    # tall8_a: H % 32 = 20 -- in the last workgroup two whole strips, one cut after 4 rows, one dead wave
    assert 500 % 32 == 20 and 20 == 2 * 8 + 4
    # tall8_b: a workgroup with ONE live row and a strip with ONE live lane; w65 the same lane in the 4-row build
    assert 33 % 32 == 1 and 65 % C.TX == 1 and C.case("w65").W - C.TX == 1
    # rows_tail4: H % 16 = 5 -- the last workgroup has one whole strip, one of a single row and two dead waves
    assert 37 % 16 == 5


# ---- kinks -------------------------------------------------------------------------------------------------------------
def _fp32_errors(c):
    """(largest |ix32 - ix64| over the positions within one pixel of the image, largest |d32 - d64|)."""
    ex = 0.0
    for key in ("e2m", "m2e"):
        for i, size in ((0, c.W), (1, c.H)):
            p64 = C.sample_pos(c.inputs[key][..., i].double(), size)
            p32 = C.sample_pos(c.inputs[key][..., i], size).double()
            near = (p64 >= -1) & (p64 <= size)  # farther out the clamp decides, whatever the rounding
            if near.any():
                ex = max(ex, float((p32 - p64)[near].abs().max()))
    d64, d32 = C.differences(c.inputs, torch.float64), C.differences(c.inputs, torch.float32)
    return ex, max(float((a.double() - b).abs().max()) for a, b in zip(d32, d64))


def test_margins_are_100_times_the_fp32_references_own_error():
    worst_x, worst_d = (0.0, ""), (0.0, "")
    for name in C.CASES:
        ex, ed = _fp32_errors(C.case(name))
        worst_x, worst_d = max(worst_x, (ex, name)), max(worst_d, (ed, name))
    print(f"fp32 reference's own error: ix {worst_x[0]:.3e} px ({worst_x[1]}), difference {worst_d[0]:.3e} ({worst_d[1]}); "
          f"MARGIN_X {C.MARGIN_X} = {C.MARGIN_X / worst_x[0]:.0f} x, MARGIN_D {C.MARGIN_D} = {C.MARGIN_D / worst_d[0]:.0f} x")
    assert C.MARGIN_X >= 100 * worst_x[0] and C.MARGIN_D >= 100 * worst_d[0]
    assert 2 * C.MARGIN_X < C.NUDGE < 0.5 - 2 * C.MARGIN_X


@pytest.mark.parametrize("name", C.CASES)
def test_case_is_kink_free(name):
    c = C.case(name)
    inp, H, W = c.inputs, c.H, c.W
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in inp.values())
    assert tuple(inp["la"].shape) == (c.B, c.K, 1, H, W) and tuple(inp["da"].shape) == (c.B, 1, H, W)
    for key in ("e2m", "m2e"):
        assert not C.near_kink(inp[key], H, W).any(), key
        # ... so fp32 lands in the same cell, on the same side of both clamps
        for i, size in ((0, W), (1, H)):
            p64, p32 = C.sample_pos(inp[key][..., i].double(), size), C.sample_pos(inp[key][..., i], size)
            assert torch.equal(p64 <= 0, p32 <= 0) and torch.equal(p64 >= size - 1, p32 >= size - 1)
            assert torch.equal(p64.clamp(0, size - 1).floor(), p32.clamp(0, size - 1).floor().double())
    d1, d2 = C.differences(inp, torch.float64)
    s1, s2 = C.differences(inp, torch.float32)
    la, da = inp["la"].expand_as(d1) != 0, inp["da"].unsqueeze(1).expand_as(d2) != 0
    assert float(d1[la].abs().min()) >= C.MARGIN_D and float(d2[da].abs().min()) >= C.MARGIN_D
    assert torch.equal(torch.sign(s1[la]).double(), torch.sign(d1[la])) and torch.equal(torch.sign(s2[da]).double(), torch.sign(d2[da]))
    for m in (inp["la"], inp["da"]):
        live = m[m != 0]
        assert 0.25 <= float(live.min()) and float(live.max()) <= 1.0
    zeros = (float((inp["la"] == 0).double().mean()), float((inp["da"] == 0).double().mean()))
    print(f"{name}: nudged {c.nudged:.2%} of the coordinates, zeroed {c.zeroed:.2%} of a mask for a near-zero difference; "
          f"zero share of latent_alpha {zeros[0]:.1%}, of d_alpha {zeros[1]:.1%}")
    # (zeroed: 3 K differences share one d_alpha entry -- 27 at K = 9, smooth_b, where it reaches 12.5 %)
    assert c.nudged <= 0.03 and c.zeroed <= 0.15


# ---- edges -------------------------------------------------------------------------------------------------------------
def _adjacent(tp, W):
    """bool [B,K,H,W]: lane l < 63 of a strip has a right neighbour in the image that samples the cell to the right."""
    x = torch.arange(W)
    has = ((x % C.TX) < C.TX - 1) & (x + 1 < W)
    adj = torch.zeros_like(tp.x0, dtype=torch.bool)
    adj[..., :-1] = (tp.x0[..., 1:] == tp.x0[..., :-1] + 1) & (tp.y0[..., 1:] == tp.y0[..., :-1])
    return adj & has, has


def test_white_noise_has_no_neighbour_structure():
    for name in ("white_noise_4", "white_noise_8"):
        c = C.case(name)
        for key in ("e2m", "m2e"):
            tp = C.taps(c.inputs[key], c.H, c.W)
            adj, _ = _adjacent(tp, c.W)
            per_strip_row = [int(adj[..., s:s + C.TX].sum(dim=-1).max()) for s in range(0, c.W, C.TX)]
            below = (tp.y0[:, :, 1:] == tp.y0[:, :, :-1] + 1) & (tp.x0[:, :, 1:] == tp.x0[:, :, :-1])
            outside = float(tp.clamped.double().mean())
            print(f"{name} {key}: at most {max(per_strip_row)} of 64 lanes with a neighbour to give to, "
                  f"{float(below.double().mean()):.2%} of the rows continue a carried row, {outside:.1%} clamped")
            assert max(per_strip_row) < 4 and float(below.double().mean()) < 0.01
            assert tp.left.any() and tp.right.any() and tp.top.any() and tp.bottom.any()
    # three pushes of up to 64 per row against the queue's 192 entries: it drains in the middle of a row


def test_shift_is_the_ideal_pattern():
    c = C.case("shift")
    for which, key in enumerate(("e2m", "m2e")):
        tp = C.taps(c.inputs[key], c.H, c.W)
        adj, has = _adjacent(tp, c.W)
        assert torch.equal(adj, has.expand_as(adj))                    # every lane gives its right-hand column away
        assert bool((tp.y0[:, :, 1:] == tp.y0[:, :, :-1] + 1).all()) and bool((tp.x0[:, :, 1:] == tp.x0[:, :, :-1]).all())
        x = torch.arange(c.W).expand_as(tp.x0)
        y = torch.arange(c.H).reshape(c.H, 1).expand_as(tp.y0)
        assert torch.equal(tp.x0, x) and torch.equal(tp.y0, y)        # ... across every strip end of either build
        inside = ~tp.clamped
        sx, sy = C.SHIFT[which]
        assert float((tp.ix - x - sx)[inside].abs().max()) < 1e-4 and float((tp.iy - y - sy)[inside].abs().max()) < 1e-4


def test_pile_up_is_one_cell():
    c = C.case("pile_up")
    for which, key in enumerate(("e2m", "m2e")):
        tp = C.taps(c.inputs[key], c.H, c.W)
        assert len(torch.unique(tp.y0 * c.W + tp.x0)) == 1 and not tp.clamped.any()
        assert 0 < int(tp.x0.flatten()[0]) < c.W - 2 and 0 < int(tp.y0.flatten()[0]) < c.H - 2
    # the four cells around each sample carry a sum of thousands of terms: what the term allowance is for
    for key, live in (("ori", c.inputs["la"]), ("latent", c.inputs["da"].unsqueeze(1).expand(c.B, c.K, 1, c.H, c.W))):
        T, n = C.term_magnitude("pile_up")[key]
        sources = int((live != 0).sum()) // (1 if key == "ori" else c.K)
        assert int((n > 100).sum()) == 4 * n.shape[0] * (n.shape[1] if key == "latent" else 1) and float(n.max()) >= sources > 1000
        assert float(T.max()) > 100 * float(T.median())


@pytest.mark.parametrize("name", sorted(C.CLAMP_SIDES))
def test_clamp_cases_clamp_exactly_the_named_side(name):
    c = C.case(name)
    r64 = C.reference(name)[0]
    for key in ("e2m", "m2e"):
        tp = C.taps(c.inputs[key], c.H, c.W)
        have = {s for s in ("left", "right", "top", "bottom") if getattr(tp, s).any()}
        assert have == C.CLAMP_SIDES[name], (key, have)
        x_out, y_out = tp.left | tp.right, tp.top | tp.bottom
        assert bool(((tp.ix <= -1) | (tp.ix >= c.W))[x_out].all()) and bool(((tp.iy <= -1) | (tp.iy >= c.H))[y_out].all())
        n = int(tp.clamped.sum())
        assert n >= (C.BAND * C.BAND if name == "clamp_corner" else C.BAND * min(c.H, c.W))
        # the coordinate gradient is exactly zero on the clamped axis and (where the mask is not 0) lives on the other
        g = r64[key]
        assert not g[..., 0][x_out].any() and not g[..., 1][y_out].any()
        if name != "clamp_corner":
            other = g[..., 1][x_out] if x_out.any() else g[..., 0][y_out]
            assert other.any()


def test_holes_cover_a_strip_end_and_a_whole_batch_entry():
    c = C.case("holes")
    la, da = c.inputs["la"], c.inputs["da"]
    assert not la[..., 0:8, 0:8].any() and not da[0, :, 0:8, 0:8].any()      # rows 3 | 4: a strip end of the 4-row builds
    assert _rows(c) == 4 and not da[c.B - 1].any() and da[0].any()
    r64 = C.reference("holes")[0]
    # no second term in the last batch entry: its latent gradient is the direct term alone, exactly 0 under a zero mask
    assert torch.equal(r64["latent"][c.B - 1] == 0, (la[c.B - 1] == 0).expand(c.K, 3, c.H, c.W))
    assert not r64["m2e"][c.B - 1].any() and not r64["e2m"][:, :, 0:8, 0:8].any()
    # g_la and g_da carry 3 dS under a zero mask: not zero
    assert float(r64["la"][la == 0].abs().min()) > 0 and float(r64["da"][da == 0].abs().min()) > 0
    tags = C.strata("holes", 4)
    assert tags["latent"]["zero_mask"].any() and tags["ori"]["zero_mask"].any() and tags["e2m"]["zero_mask"].any()


def test_smallest_sizes_have_gradients_that_are_zero_everywhere():
    """size - 1 = 1: every sample of min_2x2 is clamped or lies in the one cell.  A tensor whose float64 gradient is zero
    everywhere compares as exact zeros: nothing divides by its maximum."""
    r64, r32 = C.reference("min_2x2")
    tags = C.strata("min_2x2", 4)
    zero = {k: torch.zeros_like(r64[k]) for k in C.NAMES}
    fake64 = dict(zero, loss=r64["loss"])
    got = dict(zero, loss=r32["loss"])
    C.compare("min_2x2", 4, got, "all-zero gradients", refs=(fake64, got))
    got["e2m"] = zero["e2m"].clone()
    got["e2m"][0, 0, 1, 1, 0] = 1e-30
    with pytest.raises(AssertionError, match="not 0 where"):
        C.compare("min_2x2", 4, got, "a stray value", refs=(fake64, dict(zero, loss=r32["loss"])))
    assert all(m.shape[-2:] == (2, 2) for m in tags["ori"].values())
    for name in ("row_pair_2x70", "col_pair_70x2"):
        c = C.case(name)
        assert min(c.H, c.W) == 2 and torch.isfinite(C.reference(name)[0]["loss"])


def test_strata_tag_the_walk_of_each_build():
    tags4, tags8 = C.strata("tall8_b", 4), C.strata("tall8_b", 8)
    rows = lambda m: sorted(set(torch.nonzero(m.reshape(-1, 33, 65)[0].any(dim=1)).flatten().tolist()))
    assert rows(tags4["la"]["strip_last"]) == [3, 7, 11, 15, 19, 23, 27, 31, 32]
    assert rows(tags8["la"]["strip_last"]) == [7, 15, 23, 31, 32] and rows(tags8["la"]["strip_first"]) == [8, 16, 24, 32]
    cols = sorted(set(torch.nonzero(tags8["ori"]["col63_64"].reshape(-1, 33, 65)[0].any(dim=0)).flatten().tolist()))
    assert cols == [63, 64]
    assert sorted(set(torch.nonzero(C.strata("w129", 4)["da"]["col63_64"][0, 0].any(dim=0)).flatten().tolist())) == [63, 64, 127, 128]
    for name in C.CASES:
        c = C.case(name)
        for rows_ in sorted({4, _rows(c)}):
            for key, t in C.strata(name, rows_).items():
                union = torch.zeros_like(t["interior"])
                for s in C.STRATA:
                    union |= t[s]
                assert union.all(), (name, key)
                assert tuple(t["interior"].expand(C.planes(key, c.inputs[key]).shape).shape) == tuple(C.planes(key, c.inputs[key]).shape)


# ---- sensitivity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.CASES)
def test_sensitivity(name):
    """At least 99 % of the non-zero float64 entries of every gradient tensor exceed 10 x the bound they are held to -- in
    the tensor as a whole (against the largest bound of its strata) and in each strip-end and column-63/64 stratum (against
    that stratum's own): one dropped, doubled or misplaced contribution there is ten bounds away from passing."""
    c = C.case(name)
    r64 = C.reference(name)[0]
    lowest = (1.0, "")
    for rows in sorted({4, _rows(c)}):
        tags = C.strata(name, rows)
        for key in C.NAMES:
            r = C.planes(key, r64[key])
            if not r.any():
                continue
            bounds = {s: C.bound(name, key, rows, s) for s in C.STRATA}
            whole = max(b for b in bounds.values() if b is not None)
            checks = [("whole", torch.ones_like(r, dtype=torch.bool), whole)]
            checks += [(s, tags[key][s].expand(r.shape), bounds[s]) for s in C.EDGE_STRATA if bounds[s] is not None]
            for s, m, b in checks:
                e = r[m]
                e = e[e != 0].abs()
                if e.numel() == 0:
                    continue
                share = float((e > 10 * b).double().mean())
                lowest = min(lowest, (share, f"g_{key} [{s}] rows {rows}: {e.numel()} entries, bound {b:.2e}, max {float(e.max()):.2e}"))
                assert share >= 0.99, (name, key, s, rows, share, e.numel())
    print(f"{name}: lowest share of entries above 10 x their bound {lowest[0]:.4f} ({lowest[1]})")


# ---- the comparator ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.CASES)
def test_comparator_accepts_the_fp32_reference(name):
    c = C.case(name)
    for rows in sorted({4, _rows(c)}):
        needs = C.compare(name, rows, C.reference(name)[1], f"fp32 reference {name} rows {rows}")
        assert all(k <= 1.0 and plain <= 1.0 for _, _, _, k, plain in needs)  # the gap is its own distance


def _strip_end_entry(name, key, rows):
    """Index (into planes(key, .)) of the SMALLEST entry of the strip_last stratum above 10 x that stratum's bound that has
    a lower neighbour, and the bound."""
    r = C.planes(key, C.reference(name)[0][key])
    b = C.bound(name, key, rows, "strip_last")
    m = C.strata(name, rows)[key]["strip_last"].expand(r.shape).clone()
    m[..., -1, :] = False
    m &= r.abs() > 10 * b
    idx = torch.nonzero(m)
    assert idx.numel(), (name, key)
    pick = idx[torch.argmin(r[m].abs())]
    return tuple(int(i) for i in pick), b


PLANTED = ("zeroed", "negated", "doubled", "moved down")


@pytest.mark.parametrize("name,rows", [("rows_tail4", 4), ("tall8_b", 8), ("holes", 4), ("shift", 4)])
def test_planted_errors_at_a_strip_end_are_rejected(name, rows):
    """What a carried row lost in flush(), a stray dropped by drain() or a strip walked from the wrong row would do to ONE
    entry: set to 0, negated, doubled, added to the entry below instead -- in each of the two scatter targets and each of
    the four plain-store gradients, at the smallest strip-end entry that is above 10 x its bound."""
    assert C.expected_rows(*[getattr(C.case(name), a) for a in ("B", "H", "W")], True) == rows
    r32 = C.reference(name)[1]
    for key in C.NAMES:
        at, b = _strip_end_entry(name, key, rows)
        below = at[:-2] + (at[-2] + 1, at[-1])
        for what in PLANTED:
            got = dict(r32)
            got[key] = r32[key].clone()
            p = C.planes(key, got[key])  # a view: writes reach got[key]
            v = float(p[at])
            if what == "zeroed":
                p[at] = 0.0
            elif what == "negated":
                p[at] = -v
            elif what == "doubled":
                p[at] = 2 * v
            else:
                p[at] = 0.0
                p[below] += v
            with pytest.raises(AssertionError, match=r"strip_last"):
                C.compare(name, rows, got, f"planted {what} g_{key}{list(at)}", keys=(key,), loss=False)
    print(f"{name}: {len(PLANTED)} planted errors x {len(C.NAMES)} tensors rejected at a strip end of the {rows}-row build")


def test_planted_nonzero_where_float64_is_exactly_zero_is_rejected():
    r64, r32 = C.reference("holes")
    for key in C.NAMES:
        zeros = torch.nonzero(r64[key] == 0)
        if key in ("la", "da"):
            assert zeros.numel() == 0  # 3 dS everywhere: no exact zero to plant in
            continue
        assert zeros.numel() > 0, key
        got = dict(r32)
        got[key] = r32[key].clone()
        got[key][tuple(int(i) for i in zeros[len(zeros) // 2])] = 1e-30
        with pytest.raises(AssertionError, match="not 0 where"):
            C.compare("holes", 4, got, f"planted stray g_{key}", keys=(key,), loss=False)
    with pytest.raises(AssertionError, match="loss"):
        C.compare("holes", 4, dict(r32, loss=r32["loss"] * (1 + 2e-5)), "loss off by 2e-5", keys=())
    with pytest.raises(AssertionError):
        C.compare("holes", 4, dict(r32, loss=r32["loss"] * float("nan")), "NaN loss", keys=())


def test_scatter_sums_in_another_order_pass():
    """The two scatter targets are sums in an order that is not fixed.  The fp32 reference on the images and maps mirrored
    in both axes visits the same samples from the far end (torch's scatter walks them in memory order), so the terms of a
    cell are added in another order, and the mirrored coordinates size - 1 - c are rounded once more: it stays inside the
    bound on the case whose cells collect their terms from all over the image."""
    c = C.case("white_noise_4")
    t = {k: x.clone().requires_grad_(True) for k, x in c.inputs.items()}
    flip = lambda x: x.flip(-1).flip(-2)
    size = torch.tensor([c.W - 1.0, c.H - 1.0])
    loss = C.RT.flow_warp_loss(flip(t["ori"]), flip(t["latent"]), size - t["e2m"].flip(2).flip(3),
                               size - t["m2e"].flip(2).flip(3), flip(t["la"]), flip(t["da"]))
    loss.backward(torch.tensor(c.v))
    C.compare(c.name, 4, {k: t[k].grad for k in C.SCATTER}, "mirrored fp32 white_noise_4", keys=C.SCATTER, loss=False)
    T, n = C.term_magnitude("pile_up")["ori"]
    print(f"pile_up g_ori: up to {int(n.max())} terms per cell, allowance {float((n.sqrt() * T).max()) / float(T.max()) / 2:.1f} x 2^-23 T")
    assert int(n.max()) > 3000
    T, n = C.term_magnitude("shift")["latent"]
    live = n[..., 1:-1, 1:-1][n[..., 1:-1, 1:-1] > 1]
    assert float(live.max()) == 5.0 and float(live.median()) == 5.0  # four taps and the direct term


# ---- cost --------------------------------------------------------------------------------------------------------------
def test_references_are_cheap():
    worst = (0.0, "")
    for name in C.CASES:
        c = C.case(name)
        for dtype in (torch.float64, torch.float32):
            t0 = time.perf_counter()
            C.evaluate(c, dtype)
            worst = max(worst, (time.perf_counter() - t0, f"{name} {dtype}"))
    print(f"slowest reference: {worst[0]:.2f} s ({worst[1]})")
    assert worst[0] < 2.0
