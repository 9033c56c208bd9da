"""tests/raster_cases.py without a GPU: the dense reference equals oracle/gsplat_torch.py on the oracle's own lists, every
case reaches the edge it is named after (list lengths from tests/isect_cases.py's numpy restatement of the lists, stop
indices, which quadrant finishes first, the two sides of the clamp), the near-kink filter dropped at most 10 % of the
candidates and each of its margins is at least 16 x the fp32 reference's own relative error of the quantity it guards.
Run with -s to see the figures per case."""
import numpy as np
import pytest
import torch

import isect_cases as I
import raster_cases as R
from oracle import gsplat_torch as G


def _lists(cs, cull):
    return I.reference(R.isect_case(cs), cull)


def _tile(cs, tx, ty, cam=0):
    tw, th = -(-cs.W // 16), -(-cs.H // 16)
    return (cam * th + ty) * tw + tx


def _list_of(ref, tile):
    off = ref["tile_offsets"]
    return ref["flatten_ids"][off[tile]:off[tile + 1]]


def _walk64(cs):
    return R.walk(R.arrays_of(cs), cs.W, cs.H, torch.float64, cs.boxcut)


# ---- every case --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASES)
def test_filter_drop_share_and_margins(name):
    cs = R.case(name)
    e_raw, e_T = R.margins(name)
    m_t = R.M_T_OF.get(name, R.M_T)
    print(f"\nCASE {name}: N {cs.N}, dropped {cs.dropped:.1%} of {cs.candidates} candidates; fp32 reference error raw "
          f"{e_raw:.2e} (margin {R.M_A:.0e} = {R.M_A / max(e_raw, 1e-300):.0f} x), T {e_T:.2e} (margin {m_t:.0e} = "
          f"{m_t / max(e_T, 1e-300):.0f} x)")
    assert cs.dropped <= R.MAX_DROP
    assert R.M_A >= R.MARGIN_FACTOR * e_raw, (e_raw, R.M_A)
    assert m_t >= R.MARGIN_FACTOR * e_T, (e_T, m_t)
    assert not R.near_kink(R.arrays_of(cs), cs.W, cs.H, cs.boxcut, m_t).any()
    # fp32 and float64 take the same branch at every pair
    a = R.arrays_of(cs)
    for w64, w32 in zip(_walk64(cs), R.walk(a, cs.W, cs.H, torch.float32, cs.boxcut)):
        assert torch.equal(w64.valid, w32.valid) and torch.equal(w64.contrib, w32.contrib)


@pytest.mark.parametrize("name", R.CASES)
def test_inputs_are_what_the_reference_assumes(name):
    cs = R.case(name)
    assert cs.radii.dtype == torch.int32 and cs.means2d.dtype == torch.float32
    for c in range(cs.C):
        d = cs.depths[c].numpy().view(np.uint32)
        assert len(np.unique(d)) == cs.N, "depths: distinct fp32 values"
    a, b, c = cs.conics.double().unbind(-1)
    assert (a > 0).all() and (a * c - b * b > 0).all(), "conics: positive definite"
    # radius = ceil(k x the larger standard deviation), from the fp32 conic the device gets
    lam_min = 0.5 * (a + c) - torch.sqrt(0.25 * (a - c) ** 2 + b * b)
    smax = 1.0 / torch.sqrt(lam_min)
    k = R.K_BOXCUT if cs.boxcut else R.K_RADIUS
    seen = cs.radii > 0
    assert ((cs.radii.double() - k * smax)[seen] > -1e-4).all() and ((cs.radii.double() - k * smax)[seen] < 1 + 1e-4).all()
    if not cs.boxcut:   # list-free is legitimate: every passing pair lies inside the splat's tile rectangle
        for w in _walk64(cs):
            assert not (w.valid & ~w.inside).any()


@pytest.mark.parametrize("name", ["stop_mid", "two_cams", "boxcut"])
def test_dense_reference_equals_the_oracle_on_its_own_lists(name):
    cs = R.case(name)
    tw, th = -(-cs.W // 16), -(-cs.H // 16)
    ch, has_extra = R.layout_of(10)
    cot = R.cotangents(cs, 10)
    mine = R.dense_eval(cs, torch.float64, ch, has_extra, cot=cot)
    leaves = dict(m=cs.means2d.double().requires_grad_(True), con=cs.conics.double().requires_grad_(True),
                  op=cs.opacities.double().requires_grad_(True), col=cs.colors[..., :ch].double().requires_grad_(True),
                  ex=cs.depths.double().requires_grad_(True), bg=cs.backgrounds[:, :10].double().requires_grad_(True))
    _, isect_ids, flatten_ids = G.isect_tiles(cs.means2d, cs.radii, cs.depths, 16, tw, th)
    offsets = G.isect_offset_encode(isect_ids, cs.C, tw, th)
    col = leaves["col"] if leaves["col"].dim() == 3 else leaves["col"][None].expand(cs.C, -1, -1)
    op = leaves["op"] if leaves["op"].dim() == 2 else leaves["op"][None].expand(cs.C, -1)
    render, alpha = G.rasterize_to_pixels(leaves["m"], leaves["con"], torch.cat([col, leaves["ex"][..., None]], -1), op,
                                          cs.W, cs.H, 16, offsets, flatten_ids, backgrounds=leaves["bg"])
    torch.autograd.backward([render, alpha], [cot[0].double(), cot[1].double()])
    pairs = [("render", render.detach()), ("alpha", alpha.detach()), ("v_means2d", leaves["m"].grad),
             ("v_conics", leaves["con"].grad), ("v_opacities", leaves["op"].grad), ("v_colors", leaves["col"].grad),
             ("v_extra", leaves["ex"].grad), ("v_backgrounds", leaves["bg"].grad)]
    for key, theirs in pairs:
        scale = float(theirs.abs().max())
        assert scale > 0, key
        assert float((mine[key] - theirs).abs().max()) <= 1e-12 * scale, key


@pytest.mark.parametrize("name,kw", [("stop_mid", {}), ("two_cams", {}), ("boxcut", {}), ("classes", dict(rows=slice(64, 130))),
                                     ("centre", dict(ch=1, has_extra=False, ones=True, only="render"))])
def test_kernel_form_evaluation_is_the_same_function(name, kw):
    """raster_cases.kernel_form_eval -- exponent-form alpha, upstream's backward walk from the stored alpha, raw-sum position
    gradients -- in float64 equals the dense autograd reference: the second fp32 reference differs from the first in
    rounding alone."""
    cs = R.case(name)
    kw = dict(dict(ch=9, has_extra=True), **kw)
    D = (1 if kw.get("ones") else kw["ch"]) + (1 if kw["has_extra"] else 0)
    cot = R.cotangents(cs, D)
    a = R.dense_eval(cs, torch.float64, cot=cot, **kw)
    for moments in (False, True):
        b = R.kernel_form_eval(cs, torch.float64, cot=cot, moments=moments, **kw)
        assert a.keys() == b.keys()
        for key in a:
            assert float((a[key] - b[key]).abs().max()) <= 1e-11 * float(a[key].abs().max()), (key, moments)


# ---- the edge of each case ---------------------------------------------------------------------------------------------
def test_len0_1_has_an_empty_and_a_single_entry_list():
    cs = R.case("len0_1")
    for cull in (0, 1):
        lens = _lists(cs, cull)["lens"]
        assert lens[_tile(cs, *cs.edge["empty_tile"])] == 0 and lens[_tile(cs, *cs.edge["single_tile"])] == 1, lens
        assert 0 < lens[2:].min() and lens.max() <= 8, lens
    untouched = R.no_contributor("len0_1")[0]
    assert untouched[:16, :16].all() and not untouched[:16, 16:32].all()


@pytest.mark.parametrize("name", sorted(R.SEAM_TILE))
def test_seam_lists_have_exactly_their_length_and_no_pixel_stops(name):
    cs = R.case(name)
    n = int(name[4:])
    for cull in (0, 1):
        lens = _lists(cs, cull)["lens"]
        assert lens[_tile(cs, *cs.edge["target"])] == n, (cull, lens)
    for w in _walk64(cs):
        assert torch.equal(w.valid, w.contrib), "a pixel stops"
        tx, ty = cs.edge["target"]
        inside = w.contrib.reshape(cs.H, cs.W, -1)[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16]
        assert int(inside.any(dim=0).any(dim=0).sum()) >= n, "entries of the target list that blend nowhere in it"


def test_stop_mid_stops_in_both_batches_quadrant_first_tile_before_its_end():
    cs = R.case("stop_mid")
    w = _walk64(cs)[0]
    lst = {}
    for cull in (0, 1):
        lst[cull] = _list_of(_lists(cs, cull), _tile(cs, 0, 0))
        assert len(lst[cull]) == sum(cs.edge["groups"]) == 152
    assert np.array_equal(lst[0], lst[1])
    pos_of_row = {int(r): i for i, r in enumerate(lst[0])}
    stopped = w.valid & ~w.contrib                       # the stopping pair and every passing pair behind it
    assert stopped.any(dim=1).all(), "every pixel of the image ends at the walls at the latest"
    first = stopped.int().argmax(dim=1)                  # position (in depth order) of the stopping pair
    rows = w.idx[first].reshape(cs.H, cs.W)[:16, :16]
    pos = torch.tensor([[pos_of_row[int(r)] for r in line] for line in rows])
    quads = [pos[8 * (q >> 1):8 * (q >> 1) + 8, 8 * (q & 1):8 * (q & 1) + 8] for q in range(4)]
    print(f"\nstop_mid: stop index per quadrant min/max {[(int(q.min()), int(q.max())) for q in quads]}, list {len(lst[0])}")
    assert int(pos.min()) < 64 and bool(((pos >= 64) & (pos < 128)).any())
    assert int(quads[0].max()) < 64 and all(int(quads[0].max()) < int(q.max()) for q in quads[1:])
    assert all(len(torch.unique(q)) >= 4 for q in quads), "pixels of one wave stop at different indices"
    assert int(pos.max()) < len(lst[0]) - 20, "the whole tile finishes before its list ends"
    # splats wholly behind the stop: the reference's gradients are exactly 0 (what the comparator's zero rule enforces)
    ref64 = R.reference("stop_mid", *R.layout_of(10))[0]
    tail = slice(122, 152)
    assert not w.contrib[:, torch.isin(w.idx, torch.arange(122, 152))].any()
    assert not ref64["v_means2d"][0, tail].any() and not ref64["v_opacities"][tail].any()
    assert not ref64["v_colors"][tail].any()


def test_quadrant_splats_reach_one_quadrant_each_and_the_corner_splat_four_tiles():
    cs = R.case("quadrant")
    w = _walk64(cs)[0]
    py, px = torch.meshgrid(torch.arange(cs.H), torch.arange(cs.W), indexing="ij")
    quad = ((py // 8) * 64 + (px // 8)).reshape(-1)
    tile = ((py // 16) * 64 + (px // 16)).reshape(-1)
    for j, row in enumerate(w.idx.tolist()):
        hit = w.valid[:, j]
        assert hit.any()
        if row < cs.edge["small"]:
            assert len(torch.unique(quad[hit])) == 1, row
        else:
            assert len(torch.unique(tile[hit])) == 4, row
    assert cs.N == cs.edge["small"] + 1


def test_span_has_full_strip_and_empty_spans_and_culling_thins_some():
    cs = R.case("span")
    tw, th = 3, 3
    x0, y0, x1, y1 = I.tile_rects(cs.means2d[0].numpy(), cs.radii[0].numpy(), tw, th)
    shapes = {(int(a), int(b)) for a, b, r in zip(x1 - x0, y1 - y0, cs.radii[0]) if r > 0}
    assert {(3, 3), (3, 1), (1, 3)} <= shapes, shapes
    assert int(cs.radii[0, cs.edge["unseen_row"]]) == 0 and int((cs.radii == 0).sum()) == 1
    ref = _lists(cs, 1)
    kept_per_owner = np.bincount(ref["owner"][ref["keep"]], minlength=cs.N)
    thinned = (kept_per_owner < ref["tiles_per_gauss"]) & (kept_per_owner > 0)
    print(f"\nspan: rectangles {sorted(shapes)}, {int(thinned.sum())} splats keep only part of their rectangle under culling")
    assert thinned.sum() >= 4
    ref64 = R.reference("span", *R.layout_of(10))[0]
    u = cs.edge["unseen_row"]
    assert not ref64["v_means2d"][0, u].any() and not ref64["v_colors"][u].any() and not ref64["v_opacities"][u].any()


def test_centre_means_sit_on_pixel_centres_on_both_sides_of_the_clamp():
    cs = R.case("centre")
    assert torch.equal(cs.means2d, cs.means2d.floor() + 0.5)
    a = R.arrays_of(cs)
    sides = {True: 0, False: 0}
    for dtype in (torch.float64, torch.float32):
        w = R.walk(a, cs.W, cs.H, dtype)[0]
        for j, row in enumerate(w.idx.tolist()):
            p = int(cs.means2d[0, row, 1]) * cs.W + int(cs.means2d[0, row, 0])
            assert float(w.sigma[p, j]) == 0.0 and bool(w.valid[p, j])
            assert float(w.raw[p, j]) == float(cs.opacities[row].to(dtype))
            if dtype == torch.float64 and bool(w.contrib[p, j]):
                sides[float(w.raw[p, j]) > R.ALPHA_MAX] += 1
    print(f"\ncentre: contributing centre pixels clamped {sides[True]}, not clamped {sides[False]}")
    assert sides[True] >= 2 and sides[False] >= 2
    assert set(np.round(cs.opacities.numpy().astype(np.float64), 4)) == {0.9985, 0.9995}
    # a cotangent at one clamped centre pixel alone: the slope is zero there, so the splat's geometry and opacity gradients
    # are exactly 0 in the reference (the comparator then demands exact zeros of the kernels) while its colours' are not
    row = R.clamped_front_row(cs)
    for ref in R.reference("centre", *R.layout_of(10), tag="one clamped pixel")[:2]:
        assert not ref["v_means2d"][0, row].any() and not ref["v_conics"][0, row].any() and not ref["v_opacities"][row].any()
        assert ref["v_colors"][row].all() and ref["v_extra"][0, row] != 0


def test_narrow_two_cams_boxcut_heavy_shapes():
    cs = R.case("narrow")
    assert (cs.W, cs.H) == (12, 40) and _lists(cs, 0)["tile_w"] == 1
    cs = R.case("two_cams")
    assert cs.C == 2 and cs.colors.dim() == 3 and cs.opacities.dim() == 2
    assert not torch.equal(cs.means2d[0], cs.means2d[1])
    cs = R.case("boxcut")
    assert cs.boxcut and (cs.opacities == 0.9).all()
    edges = torch.stack([cs.means2d[0, :, a].double() + s * cs.radii[0] for a in (0, 1) for s in (-1.0, 1.0)], 1) / 16
    assert ((edges - edges.round()).abs() >= 1e-3).all()
    free = R.walk(R.arrays_of(cs), cs.W, cs.H, torch.float64, boxcut=False)[0]
    cut = free.valid & ~free.inside
    print(f"\nboxcut: {int(cut.sum())} pairs pass outside their rectangle (largest alpha {float(free.raw[cut].max()):.4f})")
    assert int(cut.sum()) >= 40, "the rectangle cuts nothing"
    cs = R.case("heavy")
    for cull in (0, 1):
        lens = _lists(cs, cull)["lens"]
        t = _tile(cs, *cs.edge["target"])
        assert lens[t] == R.HEAVY_LEN and np.delete(lens, t).max() < R.HEAVY_REST_MAX and (np.delete(lens, t) > 0).sum() >= 6


def test_classes_one_batch_of_one_class_and_one_that_alternates():
    cs = R.case("classes")
    assert cs.N == 130 and cs.Ns == 64
    for cull in (0, 1):
        ref = _lists(cs, cull)
        la, lb = _list_of(ref, _tile(cs, *cs.edge["tile_a"])), _list_of(ref, _tile(cs, *cs.edge["tile_b"]))
        assert len(la) == 64 and (la >= cs.Ns).all(), "tile A: one batch, dynamic rows only"
        assert len(lb) == 64 and np.array_equal(lb < cs.Ns, np.arange(64) % 2 == 0), "tile B alternates"
    assert not cs.colors[:cs.Ns, 6:11].any() and cs.colors[:cs.Ns, :6].all() and cs.colors[cs.Ns:, 6:11].all()
    for w in _walk64(cs):
        assert torch.equal(w.valid, w.contrib)
