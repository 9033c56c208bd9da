"""The compositors, each kernel by itself, against the dense float64 reference of tests/raster_cases.py at list seams,
mid-batch stops, single quadrants, tile spans and class batches: csrc/raster.hip (forward quadrant / block-walk kernels,
backward quadrant / block-walk kernels, the class-filtered builds), csrc/raster_bwd_mfma.hip (mfma, mfma_team) and
csrc/raster_layers.hip, through rendering.build_tile_lists + rasterize_to_pixels / _RasterizeLayers / _RasterizeClasses /
_RasterizeClassAlpha with the 2D tensors SharedProjection would pass.

Cases, references and the comparator are tests/raster_cases.py (tests/test_raster_cases_cpu.py shows from the reference
alone that each case reaches its edge).  Every evaluated (pixel, splat) pair is kept away from the alpha cut, the clamp and
the transmittance stop by the float64 walk, so fp32 and float64 take the same branch everywhere: every pixel and every
gradient element is compared, there is no flip allowance anywhere.  Per tensor (deform_cases.close_to_f64):
    max |got - ref64| <= k max |ref32 - ref64| + 2^-23 max |ref64|,
ref32 = the reference's statements in fp32 on the CPU, and got == 0 wherever ref64 == 0 exactly (alpha of untouched pixels,
gradients of splats that blend nowhere or lie behind every stop, the clamped side of `centre`, dead channels); at pixels
without a contributor the render equals the background bit for bit.  Every case runs with tile culling on and off, every
row asserts its kernels from rendering.path_log, as tests/test_gpu_compositor_matrix.py does (_check_arms).

The yardstick is the dense fp32 reference alone.  Gradients take three DERIVED terms for arithmetic that reference does not
share (raster_cases.py holds the derivations); outputs take none:
  * the stored alpha (every arm, every gradient; signed, not a bound): the backward kernels start from T' = 1 - alpha32,
    upstream's way.  Every gradient share of a pixel is proportional to that T', so its effect is the float64 gradient of
    the same loss with cotangents eps x v, eps = T' / T - 1 per pixel from the alpha image the forward kernel wrote
    (raster_cases.stored_alpha_shift); it is taken off the result before the comparison.  eps is 3e-4 at a pixel that
    stopped just above T = 1e-4 and below 1e-7 at a translucent one;
  * v_exp_f32 and v_rcp_f32 at 1 ulp (every arm, every gradient; additive, per element): alpha (1 + 2^-23) makes 1 - alpha
    wrong by 2^-23 alpha / (1 - alpha) and every transmittance behind it with it (kernel_form_eval(ulp_bound=True));
    at most 1.3e-4 of a tensor's maximum (stop_mid, opacities), 1e-6 .. 3e-5 elsewhere;
  * tile moments (mfma and mfma_team only, conics and positions only; additive): raster_cases.moment_term, 26 roundings of
    2^-24 sum |vs| (|m| + |c|)^2; at most 6.7e-4 of the maximum (seam128 conics), the largest residual measured is 7 such
    roundings.

k needed on an MI355X, all 376 parameters with both culling settings, without the terms and with them
(docs/MEASUREMENT_LOG.md, "K32"); k = twice the worst need with the terms, rounded up, at least 1, at most 8:

    family        dense reference alone                          with the terms                            k
    outputs       1.72  (stop_mid class_alpha1 over bg, render)  (no term)                                 4
    colour        3742  (stop_mid classes mask2, v_extra)        0: inside floor + terms                   1
    opacity       2562  (stop_mid D12 default, v_opacities)      0                                         1
    geometry      1394  (stop_mid D3 default, v_means2d)         0                                         1
    background    62.9  (stop_mid D3 default, v_backgrounds)     0                                         1

The reference clamps alpha at the fp32 constant 0.999f, as upstream and the kernels do: against 0.999 in float64 the
transmittance behind a clamped splat is off by 1.3e-5 of itself (`centre` needed k = 626 on its colours for that alone).

Found by this file and fixed with it: MobgsTuning.static_rows promises zeros for the static rows' dead colour channels, but
only the quadrant backward kernel wrote them; the mfma, mfma_team and block_walk arms returned the real gradient
(rendering._zero_dead_channels).
"""

import pytest
import torch

import raster_cases as R
from test_gpu_compositor_matrix import _lens, _tuned

pytestmark = pytest.mark.gpu

K = {"outputs": 4, "colour": 1, "opacity": 1, "geometry": 1, "background": 1}
FAMILY = {"render": "outputs", "alpha": "outputs", "v_colors": "colour", "v_extra": "colour", "v_opacities": "opacity",
          "v_means2d": "geometry", "v_means2d_view": "geometry", "v_conics": "geometry", "v_backgrounds": "background"}
HEAVY_MIXED = 100   # between the other tiles (< 40 entries) and the 300-entry tile of `heavy`

# ---- arms: knobs of test_gpu_compositor_matrix._tuned ("bw" block_walk, "bb" bwd_block_walk, "m" bwd_mfma, "h"
# heavy_tile_len), every one set explicitly, and the kernels they must select per build ---------------------------------
_BLOCK_FWD, _WALK_BWD, _MFMA_BWD = (9, 10, 12), (9, 10), (1, 3, 4, 9, 10)


def _expected(D, knobs):
    k = {s.rstrip("0123456789"): int(s[len(s.rstrip("0123456789")):]) for s in knobs.split()}
    fwd = "blocks" if k["bw"] == 1 and D in _BLOCK_FWD else "quadrant"
    if k["bb"] == 1:
        bwd = "block_walk" if D in _WALK_BWD else "quadrant"
    else:
        bwd = ("quadrant", "mfma", "mfma_team")[k["m"]] if D in _MFMA_BWD else "quadrant"
    heavy = "none" if k["h"] == 0 else "all" if k["h"] == 1 else "mixed"
    return fwd, bwd, heavy, k["h"]


# D = 10: each forward arm with the default backward (mfma), each backward arm with the default forward (blocks); the
# quadrant backward with COVER_SLOTS on and off.  (name, knobs, cover_slots)
ARMS_10 = [(f"fwd_{f}_h{h}", f"bw{bw} bb0 m1 h{h}", True) for f, bw in (("blocks", 1), ("quadrant", 0)) for h in (0, 1)]
ARMS_10 += [(f"bwd_{b}_h{h}", f"bw1 {kn} h{h}", cover)
            for b, kn, cover in (("quadrant_cover", "bb0 m0", True), ("quadrant_fill", "bb0 m0", False),
                                 ("mfma_team", "bb0 m2", True), ("block_walk", "bb1 m1", True)) for h in (0, 1)]
ARMS_HEAVY = [(f"fwd_{f}_mixed", f"bw{bw} bb0 m1 h{HEAVY_MIXED}", True) for f, bw in (("blocks", 1), ("quadrant", 0))]
ROWS_10 = [(c, a) for c in R.CASES for a in ARMS_10] + [("heavy", a) for a in ARMS_HEAVY]

OTHER_BUILDS = (1, 2, 3, 4, 9, 12, 16, 26, 5)   # 5: padded up to the 9-channel build
OTHER_CASES = ("seam65", "stop_mid", "span", "narrow")
ARMS_OTHER = [("default", "bw1 bb0 m1 h1", True), ("all_quadrant", "bw0 bb0 m0 h0", True)]
ROWS_OTHER = [(c, D, a) for D in OTHER_BUILDS for c in OTHER_CASES for a in ARMS_OTHER]

CLASS_CASES = ("classes", "stop_mid", "seam65", "narrow")
ARMS_CLASS = [("default", "bw1 bb0 m1 h1"), ("all_quadrant", "bw0 bb0 m0 h0"), ("team", "bw1 bb0 m2 h0")]


# ---- helpers -----------------------------------------------------------------------------------------------------------
def _dev_inputs(cs, dev, ch, has_extra, use_bg=True, D=None):
    t = dict(means2d=cs.means2d, conics=cs.conics, opacities=cs.opacities)
    if ch:
        t["colors"] = cs.colors[..., :ch]
    if has_extra:
        t["extra"] = cs.depths
    if use_bg:
        t["backgrounds"] = cs.backgrounds[:, :(ch + (1 if has_extra else 0)) if D is None else D]
    return {k: v.to(dev).clone().contiguous().requires_grad_(True) for k, v in t.items()}


def _lists(cs, dev, t, cull):
    from mobgs_amd import rendering
    rendering.set_tile_culling(cull)
    radii, depths = cs.radii.to(dev).contiguous(), cs.depths.to(dev).contiguous()
    tl = rendering.build_tile_lists(t["means2d"].detach(), radii, depths, t["conics"].detach(), t["opacities"].detach(),
                                    R.tiles_per_gauss(cs).to(dev).contiguous(), cs.W, cs.H)
    return radii, tl


class _culling:
    """Both settings of tile culling in turn; the previous one is restored."""

    def __iter__(self):
        from mobgs_amd import rendering
        prev = rendering.get_tile_culling()
        try:
            for cull in (True, False):
                yield cull
        finally:
            rendering.set_tile_culling(prev)


def _flat(refs):
    """raster_cases.reference's (float64, fp32, terms) as four name -> tensor dicts: float64, fp32, the ulp bound and the
    moment term (conics and positions only)."""
    ref64, ref32, terms = refs
    mc, mm = R.moment_term(terms["moment_mass"])
    return ref64, ref32, terms["ulp_bound"], {"v_conics": mc, "v_means2d": mm}


def _compare(tag, got, refs, bwd="quadrant", shift=None):
    """Every tensor of `got` (name -> device tensor) against refs (four dicts, _flat).  Outputs: close_to_f64 against the
    dense references as they are.  Gradients: raster_cases.close_with_terms -- the same yardstick after the stored-alpha
    `shift` (name -> tensor) and the ulp bound; the moment term only where the matrix-pipe backward ran (bwd "mfma" /
    "mfma_team")."""
    ref64, ref32, ulp, mom = refs
    for key, g in got.items():
        assert g is not None, f"{tag}: {key} received no gradient"
        fam = FAMILY[key]
        r64 = ref64[key].double()
        what = f"{tag} [{fam}] {key}"
        if not key.startswith("v_"):
            R.close_to_f64(g.reshape(r64.shape), r64, ref32[key], K[fam], what)
            continue
        bound = ulp[key].double()
        if bwd.startswith("mfma") and key in mom:
            bound = bound + mom[key]
        R.close_with_terms(g, r64, ref32[key], shift["v_means2d" if key == "v_means2d_view" and key not in shift else key].double(), bound,
                           K[fam], what)


def _check_arms(log, cs, D, class_filter, fwd, bwd, heavy, heavy_len, lens, directions=("fwd", "bwd")):
    """test_gpu_compositor_matrix._check_path's statements, exact for these small grids: the logged passes of D channels
    took the expected kernels, and the schedule marked heavy exactly the tiles whose list lies in a longer length class
    than heavy_tile_len (csrc/isect.hip tile_scan_kernel: classes of 1/255 of the longest list; a one-entry list shares
    the class of heavy_tile_len = 1)."""
    es = [e for e in log if e["D"] == D and e["class_filter"] == class_filter]
    assert sorted({e["dir"] for e in es}) == sorted(directions), es
    longest = int(lens.max())
    marked = torch.zeros_like(lens, dtype=torch.bool)
    if heavy != "none" and longest >= heavy_len:
        marked = (lens * 255) // longest > (heavy_len * 255) // longest
    for e in es:
        assert e["n_tiles"] == lens.numel(), e
        assert (e["fwd_kernel"] if e["dir"] == "fwd" else e["bwd_kernel"]) == (fwd if e["dir"] == "fwd" else bwd), e
        assert e["heavy_len"] == heavy_len and e["heavy_tiles"] == int(marked.sum()), (e, int(marked.sum()))
    if heavy == "mixed":
        assert 0 < int(marked.sum()) < int((lens > 0).sum())
    if heavy == "all":
        assert int(marked.sum()) >= int((lens > 1).sum()) > 0


def _background_is_exact(tag, render, bg, untouched):
    """At pixels no splat contributes to, the render IS the background, bit for bit."""
    r = render.detach().cpu()
    want = bg.detach().cpu()[:, None, None, :].expand_as(r)
    assert torch.equal(r[untouched], want[untouched]), f"{tag}: the render of a pixel without contributors is not the background"


def _grads(t):
    names = {"means2d": "v_means2d", "conics": "v_conics", "opacities": "v_opacities", "colors": "v_colors",
             "extra": "v_extra", "backgrounds": "v_backgrounds"}
    return {names[k]: v.grad for k, v in t.items()}


def _plain(cs, dev, D, arm, static_rows=0, depth_channel=None, tag="", zero_dead=None):
    """One plain pass of D channels under `arm`, culling on and off, against the reference."""
    from mobgs_amd import rendering
    name, knobs, cover = arm
    ch, has_extra = R.layout_of(D, depth_channel)
    refs = _flat(R.reference(cs.name, ch, has_extra, tag=tag))
    if zero_dead is not None:   # static rows: the dead channels' gradient is returned as exactly 0
        refs = tuple({**r, "v_colors": r["v_colors"].clone()} for r in refs[:2]) + refs[2:]
        for r in refs[:2]:
            r["v_colors"][zero_dead] = 0.0
    v_r, v_a = (v.to(dev) for v in R.cotangents(cs, D, tag))
    untouched = R.no_contributor(cs.name)
    Dp = rendering._pad_channels(D)
    fwd, bwd, heavy, heavy_len = _expected(Dp, knobs)
    saved_cover = rendering.COVER_SLOTS
    try:
        rendering.COVER_SLOTS = cover
        for cull in _culling():
            t = _dev_inputs(cs, dev, ch, has_extra)
            with _tuned(knobs) as log:
                radii, tl = _lists(cs, dev, t, cull)
                render, alpha = rendering.rasterize_to_pixels(t["means2d"], t["conics"], t["colors"], t["opacities"], radii,
                                                              tl, cs.W, cs.H, backgrounds=t["backgrounds"],
                                                              extra=t.get("extra"), static_rows=static_rows)
                torch.autograd.backward([render, alpha], [v_r, v_a])
                torch.cuda.synchronize()
                log = list(log)
            lens = _lens(tl.tile_offsets[:-1], tl.n_isects)
            _check_arms(log, cs, Dp, False, fwd, bwd, heavy, heavy_len, lens)
            what = f"{cs.name} D{D} {name} cull{int(cull)}"
            got = {"render": render, "alpha": alpha, **_grads(t)}
            _compare(what, got, refs, bwd, R.stored_alpha_shift(cs.name, ch, has_extra, tag=tag, stored=alpha))
            _background_is_exact(what, render, t["backgrounds"], untouched)
    finally:
        rendering.COVER_SLOTS = saved_cover


# ---- 1. plain passes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,arm", ROWS_10, ids=[f"{c}-{a[0]}" for c, a in ROWS_10])
def test_training_build_matches_float64(hip_device, case, arm):
    cs = R.case(case)
    static = dict(static_rows=cs.Ns, zero_dead=(slice(0, cs.Ns), slice(6, 9))) if case == "classes" else {}
    _plain(cs, hip_device, 10, arm, **static)


@pytest.mark.parametrize("case,D,arm", ROWS_OTHER, ids=[f"{c}-D{D}-{a[0]}" for c, D, a in ROWS_OTHER])
def test_other_builds_match_float64(hip_device, case, D, arm):
    _plain(R.case(case), hip_device, D, arm)


@pytest.mark.parametrize("arm", ARMS_OTHER, ids=[a[0] for a in ARMS_OTHER])
def test_twelve_channel_build_with_static_rows(hip_device, arm):
    """D = 12 = 11 colours + depth (get_flow()'s layout): the static rows' channels 6 .. 10 are dead."""
    cs = R.case("classes")
    _plain(cs, hip_device, 12, arm, static_rows=cs.Ns, depth_channel=True, zero_dead=(slice(0, cs.Ns), slice(6, 11)))


@pytest.mark.parametrize("arm", ARMS_10, ids=[a[0] for a in ARMS_10])
def test_clamped_alpha_has_zero_slope(hip_device, arm):
    """`centre` with a cotangent at ONE pixel, the centre of a splat whose alpha is clamped to 0.999 there: the reference's
    geometry and opacity gradients of that splat are exactly 0 and the comparator's zero rule demands the same of the
    kernel; its colour gradient is not 0."""
    cs = R.case("centre")
    _plain(cs, hip_device, 10, arm, tag="one clamped pixel")


# ---- 2. layered and class kernels --------------------------------------------------------------------------------------
def _class_rows(cs):
    return {0: None, 1: (0, cs.Ns), 2: (cs.Ns, cs.N)}


def _layer_refs(cs, layers, use_bg=True):
    tags = ("all", "static", "dynamic")
    return {ly: _flat(R.reference(cs.name, 9, True, rows=_class_rows(cs)[ly], use_bg=use_bg, tag=tags[ly])) for ly in layers}


def _sum_refs(refs, layers, key, like):
    """Sums over `layers` of the dicts' tensor `key` (as float64: gradients, shifts and bounds all add); zeros for no
    layer or where a dict has no such tensor."""
    out = []
    for i in range(5):
        parts = [refs[ly][i][key].double() for ly in layers if i < len(refs[ly]) and key in refs[ly][i]]
        out.append(sum(parts) if parts else torch.zeros_like(like, dtype=torch.float64))
    return out


@pytest.mark.parametrize("mask", (1, 6, 7))
@pytest.mark.parametrize("heavy", (0, 1))
@pytest.mark.parametrize("case", CLASS_CASES)
def test_layers_match_float64(hip_device, case, heavy, mask):
    """_RasterizeLayers: the combined, static and dynamic layers of one walk; all requested layers are back-propagated at
    once.  The view alias receives the position gradient of the combined layer alone, means2d that of the other two.
    The layered node has one forward and one backward kernel and logs no selection: there is no arm to assert, only the
    tile schedule (heavy_tile_len) varies."""
    from mobgs_amd import rendering
    cs, dev = R.case(case), hip_device
    layers = [ly for ly in range(3) if (mask >> ly) & 1]
    refs = _layer_refs(cs, layers)
    cots = {ly: [v.to(dev) for v in R.cotangents(cs, 10, ("all", "static", "dynamic")[ly])] for ly in layers}
    for cull in _culling():
        t = _dev_inputs(cs, dev, 9, True)
        bg = t.pop("backgrounds").detach()
        view = t["means2d"].detach().clone().requires_grad_(True)   # same values; a leaf, so that its gradient stays apart
        with _tuned(f"h{heavy}"):
            radii, tl = _lists(cs, dev, t, cull)
            outs = rendering._RasterizeLayers.apply(t["means2d"], view, t["conics"], t["colors"], t["opacities"], t["extra"],
                                                    bg, radii, tl, cs.W, cs.H, cs.Ns, mask)
            torch.autograd.backward([outs[2 * ly + i] for ly in layers for i in (0, 1)],
                                    [cots[ly][i].reshape(outs[2 * ly + i].shape) for ly in layers for i in (0, 1)])
            torch.cuda.synchronize()
        what = f"{case} layers mask{mask} h{heavy} cull{int(cull)}"
        for ly in range(3):
            if ly not in layers:
                assert outs[2 * ly].numel() == 0 and outs[2 * ly + 1].numel() == 0
                continue
            tag = f"{what} layer{ly}"
            _compare(tag, {"render": outs[2 * ly], "alpha": outs[2 * ly + 1]}, refs[ly])
            _background_is_exact(tag, outs[2 * ly], bg, R.no_contributor(case, _class_rows(cs)[ly]))
        full = {ly: refs[ly] + (R.stored_alpha_shift(case, 9, True, _class_rows(cs)[ly], tag=("all", "static", "dynamic")[ly],
                                                     stored=outs[2 * ly + 1]),) for ly in layers}
        got = _grads(t)   # (the node returns no background gradient: the background is passed detached)
        got["v_means2d_view"] = view.grad if view.grad is not None else torch.zeros_like(view)
        sums = ({}, {}, {}, {}, {})   # float64, fp32, ulp bound, moment term, stored-alpha shift
        for key, g in got.items():
            src = "v_means2d" if key == "v_means2d_view" else key
            over = [ly for ly in layers if ly == 0] if key == "v_means2d_view" else \
                [ly for ly in layers if ly != 0] if key == "v_means2d" else layers
            for d, v in zip(sums, _sum_refs(full, over, src, g.detach().cpu())):
                d[key] = v
        _compare(what, got, sums[:4], shift=sums[4])


@pytest.mark.parametrize("mask", (2, 4, 6))
@pytest.mark.parametrize("arm", ARMS_CLASS, ids=[a[0] for a in ARMS_CLASS])
@pytest.mark.parametrize("case", CLASS_CASES)
def test_class_passes_match_float64(hip_device, case, arm, mask):
    """_RasterizeClasses (the class-filtered 10-channel builds) over the lists of the whole set against the dense
    reference over the class's rows alone.  `classes`: static_rows = Ns, the static rows' dead channels return 0."""
    from mobgs_amd import rendering
    cs, dev = R.case(case), hip_device
    name, knobs = arm
    classes = [c for c in (1, 2) if (mask >> c) & 1]
    refs = _layer_refs(cs, classes)
    static_rows = cs.Ns if case == "classes" else 0
    if static_rows and 1 in classes:
        refs[1] = tuple({**r, "v_colors": r["v_colors"].clone()} for r in refs[1][:2]) + refs[1][2:]
        for r in refs[1][:2]:
            r["v_colors"][:cs.Ns, 6:9] = 0.0
    cots = {c: [v.to(dev) for v in R.cotangents(cs, 10, ("all", "static", "dynamic")[c])] for c in classes}
    fwd, bwd, heavy, heavy_len = _expected(10, knobs)
    for cull in _culling():
        t = _dev_inputs(cs, dev, 9, True)
        bg = t.pop("backgrounds").detach()   # (the node returns no background gradient)
        with _tuned(knobs) as log:
            radii, tl = _lists(cs, dev, t, cull)
            outs = rendering._RasterizeClasses.apply(t["means2d"], t["conics"], t["colors"], t["opacities"], t["extra"],
                                                     bg, radii, tl, cs.W, cs.H, cs.Ns, mask, None, static_rows)
            torch.autograd.backward([outs[2 * (c - 1) + i] for c in classes for i in (0, 1)],
                                    [cots[c][i].reshape(outs[2 * (c - 1) + i].shape) for c in classes for i in (0, 1)])
            torch.cuda.synchronize()
            log = list(log)
        _check_arms(log, cs, 10, True, fwd, bwd, heavy, heavy_len, _lens(tl.tile_offsets[:-1], tl.n_isects))
        assert len([e for e in log if e["dir"] == "fwd"]) == len(classes)
        what = f"{case} classes mask{mask} {name} cull{int(cull)}"
        for c in (1, 2):
            if c not in classes:
                assert outs[2 * (c - 1)].numel() == 0
                continue
            tag = f"{what} class{c}"
            _compare(tag, {"render": outs[2 * (c - 1)], "alpha": outs[2 * (c - 1) + 1]}, refs[c])
            _background_is_exact(tag, outs[2 * (c - 1)], bg, R.no_contributor(case, _class_rows(cs)[c]))
        full = {c: refs[c] + (R.stored_alpha_shift(case, 9, True, _class_rows(cs)[c], tag=("all", "static", "dynamic")[c],
                                                   stored=outs[2 * (c - 1) + 1]),) for c in classes}
        got = _grads(t)
        sums = ({}, {}, {}, {}, {})   # float64, fp32, ulp bound, moment term, stored-alpha shift
        for key, g in got.items():
            for d, v in zip(sums, _sum_refs(full, classes, key, g.detach().cpu())):
                d[key] = v
        _compare(what, got, sums[:4], bwd, sums[4])


@pytest.mark.parametrize("use_bg", (False, True), ids=("alpha", "over_bg"))
@pytest.mark.parametrize("sel", (1, 2))
@pytest.mark.parametrize("arm", ARMS_CLASS, ids=[a[0] for a in ARMS_CLASS])
@pytest.mark.parametrize("case", CLASS_CASES)
def test_class_alpha_matches_float64(hip_device, case, arm, sel, use_bg):
    """_RasterizeClassAlpha (the class-filtered 1-channel build): coverage of one class, as alpha or as the ones-colour
    render over a background [C,1]."""
    from mobgs_amd import rendering
    cs, dev = R.case(case), hip_device
    name, knobs = arm
    rows = _class_rows(cs)[sel]
    refs = _flat(R.reference(case, 1, False, rows=rows, use_bg=use_bg, ones=True, tag=f"cover{sel}",
                             only="render" if use_bg else "alpha"))
    v_r, v_a = (v.to(dev) for v in R.cotangents(cs, 1, f"cover{sel}"))
    _, bwd, heavy, heavy_len = _expected(1, knobs)
    for cull in _culling():
        t = _dev_inputs(cs, dev, 0, False, use_bg, D=1)
        with _tuned(knobs) as log:
            radii, tl = _lists(cs, dev, t, cull)
            out = rendering._RasterizeClassAlpha.apply(t["means2d"], t["conics"], t["opacities"], radii, tl, cs.W, cs.H,
                                                       cs.Ns, sel, t["backgrounds"].detach() if use_bg else None)
            out.backward((v_r if use_bg else v_a).reshape(out.shape))
            torch.cuda.synchronize()
            log = list(log)
        _check_arms(log, cs, 1, True, "quadrant", bwd, heavy, heavy_len, _lens(tl.tile_offsets[:-1], tl.n_isects))
        what = f"{case} class_alpha{sel} {'bg' if use_bg else 'alpha'} {name} cull{int(cull)}"
        got = {"render" if use_bg else "alpha": out}
        got.update({k: v for k, v in _grads(t).items() if k != "v_backgrounds"})
        shift = R.stored_alpha_shift(case, 1, False, rows, use_bg, True, f"cover{sel}", "render" if use_bg else "alpha",
                                     stored=None if use_bg else out)   # (over a background the alpha image is not an output)
        _compare(what, got, refs, bwd, shift)
        if use_bg:
            _background_is_exact(what, out.reshape(cs.C, cs.H, cs.W, 1), t["backgrounds"], R.no_contributor(case, rows))
