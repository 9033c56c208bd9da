"""GPU parity of the operator API (B2) against the CPU oracle (oracle/gsplat_torch.py).

Tolerances: radii / tile lists exact; means2d, depths, conics rel 1e-5 where radii>0;
pixels max-abs <= 2e-5 (x channel scale); gradients rel 1e-3 / abs 1e-6 of the gradient scale.
"""
import math

import pytest
import torch

from mobgs_amd.synth import SynthCamera, splat_inputs

pytestmark = pytest.mark.gpu


def _scene(n, w, h, seed=0, channels=9):
    cam = SynthCamera().scaled(w, h)
    return splat_inputs(n, cam, seed, channels), cam


def _to(d, dev):
    return {k: v.to(dev) for k, v in d.items()}


def _close(a, b, rtol, atol, what, flip_frac=0.0, flip_atol=0.0):
    """|a-b| <= atol + rtol*|b| everywhere, except that a fraction `flip_frac` of the elements may differ by up
    to `flip_atol`: a splat whose alpha sits within an ulp of the 1/255 cut (or whose transmittance sits at the
    1e-4 stop) can fall on the other side when exp() differs in the last bit -- the same happens between two
    GPUs running upstream gsplat -- and moves that one pixel by at most alpha*T <= 1/255."""
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = err > tol
    nbad = int(bad.sum())
    msg = f"{what}: {nbad}/{bad.numel()} off, max err {err.max():.3e} (ref max {b.abs().max():.3e})"
    from helpers import observe
    observe(what, nbad, bad.numel(), float(err.max()) if err.numel() else 0.0, flip_frac, flip_atol,
            float(b.abs().max()) if b.numel() else 0.0)
    assert nbad <= flip_frac * bad.numel(), msg
    if nbad:
        assert float(err.max()) <= flip_atol, msg


def _psnr(img, target):
    mse = ((img.double() - target.double()) ** 2).mean()
    return float(20 * torch.log10(1.0 / torch.sqrt(mse)))


@pytest.mark.parametrize("n,w,h,seed", [(2000, 160, 128, 0), (500, 96, 64, 1), (3000, 200, 90, 2)])
def test_projection_forward(hip_device, n, w, h, seed):
    from mobgs_amd.rendering import fully_fused_projection
    from oracle import gsplat_torch as G
    s, _ = _scene(n, w, h, seed)
    # a non-trivial camera
    vm = s["viewmats"].clone()
    ang = 0.05
    vm[0, :3, :3] = torch.tensor([[math.cos(ang), 0, math.sin(ang)], [0, 1, 0], [-math.sin(ang), 0, math.cos(ang)]])
    vm[0, :3, 3] = torch.tensor([0.05, -0.02, 0.1])
    s["viewmats"] = vm
    ref = G.fully_fused_projection(s["means"], None, s["quats"], s["scales"], s["viewmats"], s["Ks"], w, h)
    d = _to(s, hip_device)
    out = fully_fused_projection(d["means"], None, d["quats"], d["scales"], d["viewmats"], d["Ks"], w, h)
    assert torch.equal(out[0].cpu(), ref[0]), "radii differ"
    vis = ref[0] > 0
    assert vis.sum() > 0.5 * n
    _close(out[1].cpu()[vis], ref[1][vis], 1e-5, 1e-4, "means2d")
    _close(out[2].cpu()[vis], ref[2][vis], 1e-6, 1e-6, "depths")
    _close(out[3].cpu()[vis], ref[3][vis], 2e-4, 1e-7, "conics")


@pytest.mark.parametrize("mode,channels,use_bg", [("RGB+ED", 9, True), ("RGB", 1, True), ("RGB", 2, False),
                                                  ("RGB", 3, True), ("ED", 3, False), ("RGB+D", 5, True)])
def test_rasterization_forward(hip_device, mode, channels, use_bg):
    from mobgs_amd.rendering import rasterization
    from oracle import gsplat_torch as G
    n, w, h = 2500, 168, 120  # 168 = 10.5 tiles, 120 = 7.5 tiles: ragged right/bottom edges
    s, _ = _scene(n, w, h, 3, channels)
    bg = torch.rand(1, channels, generator=torch.Generator().manual_seed(5)) if use_bg else None
    ref_img, ref_a, ref_meta = G.rasterization(s["means"], s["quats"], s["scales"], s["opacities"], s["colors"],
                                               s["viewmats"], s["Ks"], w, h, packed=False, backgrounds=bg,
                                               render_mode=mode)
    d = _to(s, hip_device)
    from mobgs_amd import rendering
    rendering.set_tile_culling(False)  # exactly upstream's lists
    try:
        img, a, meta = rasterization(d["means"], d["quats"], d["scales"], d["opacities"], d["colors"], d["viewmats"],
                                     d["Ks"], w, h, packed=False,
                                     backgrounds=None if bg is None else bg.to(hip_device), render_mode=mode)
    finally:
        rendering.set_tile_culling(True)
    assert img.shape == ref_img.shape and a.shape == ref_a.shape
    assert torch.equal(meta["radii"].cpu(), ref_meta["radii"])
    assert torch.equal(meta["tiles_per_gauss"].cpu(), ref_meta["tiles_per_gauss"])
    assert torch.equal(meta["flatten_ids"].cpu(), ref_meta["flatten_ids"]), "per-tile depth order differs"
    assert torch.equal(meta["isect_offsets"].cpu(), ref_meta["isect_offsets"])
    assert torch.equal(meta["isect_ids"].cpu(), ref_meta["isect_ids"])
    scale = max(1.0, float(ref_img.abs().max()))
    # discrete decisions (the 1/255 skip, the 1e-4 stop) are bounded by the DERIVED one-blend-step bound of
    # helpers.close_image_with_blend_flips -- w (|c| + |pixel|) per colour channel, w spread / alpha for an expected
    # depth -- for 2e-4 of the elements (observed: none; was a flat 1/255 of the range for 1e-3 of them)
    from helpers import close_image_with_blend_flips
    _close(a, ref_a, 0, 2e-5, "alphas", flip_frac=2e-4, flip_atol=2.0 * 1.001 / 255)
    vis = ref_meta["depths"][ref_meta["radii"] > 0]
    spread = float(vis.max() - vis.min()) if vis.numel() else 0.0
    n_col = {"RGB": channels, "RGB+D": channels, "RGB+ED": channels, "D": 0, "ED": 0}[mode]
    col_max = max(float(s["colors"].abs().max()), float(vis.max()) if (mode in ("D", "RGB+D") and vis.numel()) else 0.0)
    if mode in ("D", "RGB+D"):   # accumulated (not normalised) depth: a colour-like channel whose "colour" is the depth
        n_col = ref_img.shape[-1]
    close_image_with_blend_flips(img, ref_img, ref_a, col_max, spread, 2e-5 * scale, f"image[{mode}]", flip_frac=2e-4,
                                 n_colour_channels=n_col, alphas_img=a)
    # the north-star criterion: PSNR against a common target agrees to 1e-4 dB
    target = (ref_img + 0.05 * torch.randn(ref_img.shape, generator=torch.Generator().manual_seed(9))) / scale
    assert abs(_psnr(img.cpu() / scale, target) - _psnr(ref_img / scale, target)) <= 1e-4


@pytest.mark.parametrize("mode,channels,use_bg", [("RGB+ED", 9, True), ("RGB", 1, True), ("RGB", 2, False)])
def test_rasterization_backward(hip_device, mode, channels, use_bg):
    from mobgs_amd.rendering import rasterization
    from oracle import gsplat_torch as G
    n, w, h = 1500, 120, 88
    s, _ = _scene(n, w, h, 4, channels)
    gen = torch.Generator().manual_seed(104)
    bg = torch.rand(1, channels, generator=gen) if use_bg else None
    names = ["means", "quats", "scales", "opacities", "colors", "viewmats"]

    def run(fn, dev):
        t = {k: v.to(dev).clone().requires_grad_(k in names) for k, v in s.items()}
        b = None if bg is None else bg.to(dev)
        img, a, meta = fn(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], t["viewmats"], t["Ks"],
                          w, h, packed=False, backgrounds=b, render_mode=mode)
        meta["means2d"].retain_grad()
        g = torch.Generator().manual_seed(7)
        v_img = torch.randn(img.shape, generator=g).to(dev)
        v_a = torch.randn(a.shape, generator=g).to(dev)
        ((img * v_img).sum() + (a * v_a).sum()).backward()
        grads = {k: t[k].grad.detach().cpu() for k in names}
        grads["means2d"] = meta["means2d"].grad.detach().cpu()
        return grads

    ref = run(G.rasterization, torch.device("cpu"))
    out = run(rasterization, hip_device)
    # (1) against autograd over the independent torch formulation: fp32 reformulation noise is ~1e-4 of the
    #     largest gradient (the C restatement of upstream's backward shows the same distance, see
    #     tests/test_oracle_cpu.py)
    for k in ref:
        scale = float(ref[k].abs().max())
        _close(out[k], ref[k], 1e-3, 5e-4 * scale + 1e-6, f"grad[{k}] vs torch oracle")
    # (2) against the C restatement of upstream's backward kernels (same recurrences): summation order and the fp32
    #     rounding of alpha differ (the kernels evaluate opacity * exp(-sigma) as exp2 of ONE polynomial, common.h
    #     write_splat_record).  The camera gradient is a sum over every splat with heavy cancellation:
    #     scripts/exp_form_accuracy.py (profiles/r04/exp_form_accuracy.txt) measures this very scene against the exact
    #     float64 gradients -- HIP 1.2e-4 of the maximum, the C restatement 1.9e-4, their mutual distance 6.8e-5 -- so
    #     the allowance between the two fp32 evaluations is 1e-4 of the maximum there, 2e-5 elsewhere
    from oracle import gsplat_cpu as Cc
    g = torch.Generator().manual_seed(7)
    C = s["viewmats"].shape[0]
    X = channels + (1 if mode in ("RGB+D", "RGB+ED") else 0)
    v_img = torch.randn((C, h, w, X), generator=g)
    v_a = torch.randn((C, h, w, 1), generator=g)
    r = Cc.rasterization_fwd_bwd(*(s[k].numpy() for k in ["means", "quats", "scales", "opacities", "colors",
                                                          "viewmats", "Ks"]), w, h,
                                 backgrounds=None if bg is None else bg.numpy(), render_mode=mode,
                                 v_render=v_img.numpy(), v_alphas=v_a[..., 0].numpy())
    for k, ck in [("means", "v_means"), ("quats", "v_quats"), ("scales", "v_scales"), ("opacities", "v_opacities"),
                  ("colors", "v_colors"), ("viewmats", "v_viewmats"), ("means2d", "v_means2d")]:
        refc = torch.from_numpy(r[ck])
        scale = float(refc.abs().max())
        _close(out[k], refc, 2e-4, (1e-4 if k == "viewmats" else 2e-5) * scale + 1e-7, f"grad[{k}] vs C oracle",
               flip_frac=2e-3, flip_atol=5e-4 * scale)


@pytest.mark.parametrize("mode,channels", [("RGB+ED", 9), ("RGB", 2)])
def test_tile_culling_is_bit_exact(hip_device, mode, channels):
    """Reach culling drops only (tile, splat) pairs the compositor skips at every pixel: images are bit-identical
    to the un-culled run, gradients consist of the same non-zero terms (equal up to fp32 summation order), the
    culled lists are ordered sub-sequences of upstream's."""
    from mobgs_amd import rendering
    from mobgs_amd.rendering import rasterization
    n, w, h = 6000, 200, 152
    s, _ = _scene(n, w, h, 11, channels)
    names = ["means", "quats", "scales", "opacities", "colors", "viewmats"]
    gen = torch.Generator().manual_seed(3)
    res = {}
    for cull in (False, True):
        rendering.set_tile_culling(cull)
        try:
            t = {k: v.to(hip_device).clone().requires_grad_(k in names) for k, v in s.items()}
            img, a, meta = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"],
                                         t["viewmats"], t["Ks"], w, h, packed=False, render_mode=mode)
            g = torch.Generator().manual_seed(7)
            v_img = torch.randn(img.shape, generator=g).to(hip_device)
            ((img * v_img).sum() + a.sum()).backward()
            res[cull] = (img.detach().cpu(), a.detach().cpu(), {k: t[k].grad.cpu() for k in names},
                         meta["flatten_ids"].cpu(), meta["isect_offsets"].cpu().reshape(-1))
        finally:
            rendering.set_tile_culling(True)
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    for k in names:  # same terms; the per-splat slot sum associates them differently once the zero slots are gone
        g = res[False][2][k]
        # (1e-5 of the largest entry: on a grid this small every tile is composited quadrant-per-wave, and the four
        # quadrant records of an entry are summed per splat in slot order, which culling changes)
        _close(res[True][2][k], g, 1e-5, 1e-5 * float(g.abs().max()), f"grad[{k}] under culling")
    n_full, n_cull = res[False][3].numel(), res[True][3].numel()
    assert n_cull < 0.8 * n_full, (n_cull, n_full)
    # per tile: the culled list is a sub-sequence (same order) of the full list
    of, oc = res[False][4].tolist() + [n_full], res[True][4].tolist() + [n_cull]
    for tile in range(0, len(of) - 1, 7):
        full = res[False][3][of[tile]:of[tile + 1]].tolist()
        sub = res[True][3][oc[tile]:oc[tile + 1]].tolist()
        it = iter(full)
        assert all(x in it for x in sub), f"tile {tile}: not a sub-sequence"


@pytest.mark.parametrize("mode,channels,tile_cull,size", [("RGB+ED", 9, True, (232, 168)), ("RGB", 3, True, (232, 168)),
                                                           ("RGB+ED", 9, False, (232, 168)),
                                                           ("RGB+ED", 9, True, (1101, 613)), ("D", 0, True, (333, 250))])
def test_block_walk_equals_quadrant_kernel(hip_device, mode, channels, tile_cull, size):
    """Round 3: the plain forward passes run the block-walk compositor (sixteen independent 4x4-pixel workers per wave,
    each walking only the entries that can reach its block, MobgsTuning.block_walk = 1).  A worker skips an entry only
    when a conservative bound says no pixel centre of its block can pass the alpha test, so every pixel blends exactly
    the same entries in the same order through the same instructions: images, alphas, last ids -- and therefore all
    gradients, which the backward pass derives from them and from the per-entry quadrant masks the forward leaves
    behind -- must be bit-identical to the quadrant kernel's (block_walk = 0).  The small grids run with heavy_tile_len
    = 0 (one wave per tile, as on large images; by default every tile of such a grid goes to a whole workgroup, the
    path both kernels share), 1101x613 is a large ragged image with the default schedule."""
    from mobgs_amd import rendering
    from mobgs_amd.rendering import rasterization
    w, h = size
    n = 8000 if w < 1000 else 60000
    s, _ = _scene(n, w, h, 23, max(channels, 1))
    g0 = torch.Generator().manual_seed(6)
    s["scales"] = s["scales"] * torch.exp(torch.randn(s["scales"].shape, generator=g0) * 0.9)  # needles and blobs
    names = ["means", "quats", "scales", "opacities", "colors", "viewmats"]
    res = {}
    rendering.set_tile_culling(tile_cull)
    try:
        for bw in (1, 0):
            rendering.tuning.block_walk = bw
            rendering.tuning.heavy_tile_len = 0 if w < 1000 else -1   # small grids: one wave per tile all the same
            t = {k: v.to(hip_device).clone().requires_grad_(k in names) for k, v in s.items()}
            img, a, meta = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"],
                                         t["viewmats"], t["Ks"], w, h, packed=False, render_mode=mode)
            g = torch.Generator().manual_seed(7)
            v_img = torch.randn(img.shape, generator=g).to(hip_device)
            ((img * v_img).sum() + (a * a).sum()).backward()
            res[bw] = (img.detach().cpu(), a.detach().cpu(),
                       {k: t[k].grad.cpu() for k in names if t[k].grad is not None})
    finally:
        rendering.tuning.block_walk = -1
        rendering.tuning.heavy_tile_len = -1
        rendering.set_tile_culling(True)
    assert torch.equal(res[1][0], res[0][0]), "image differs"
    assert torch.equal(res[1][1], res[0][1]), "alpha differs"
    for k in res[0][2]:
        assert torch.equal(res[1][2][k], res[0][2][k]), f"grad[{k}] differs"


@pytest.mark.parametrize("size", [(232, 168), (1101, 613)])
def test_backward_block_walk_matches_quadrant_kernel(hip_device, size):
    """The experimental backward block walk (MobgsTuning.bwd_block_walk = 1: sixteen 4x4-pixel workers per wave, partial
    records combined in LDS under an integer claim) blends exactly the pairs the quadrant kernel blends; only the order
    in which a (tile, splat) record's terms are summed differs.  Gradients therefore agree to fp32 summation noise --
    bounded here by 2e-4 of each tensor's largest entry plus 1e-4 relative (the quaternion gradient amplifies the
    record's rounding through the projection backward: 7.5e-5 of the maximum observed) -- and repeat bit for bit run to run."""
    from mobgs_amd import rendering
    from mobgs_amd.rendering import rasterization
    w, h = size
    n = 8000 if w < 1000 else 60000
    s, _ = _scene(n, w, h, 29, 9)
    names = ["means", "quats", "scales", "opacities", "colors", "viewmats"]
    res = {}
    try:
        for tag, bw in (("quad", 0), ("blocks", 1), ("blocks2", 1)):
            rendering.tuning.bwd_block_walk = bw
            rendering.tuning.heavy_tile_len = 0 if w < 1000 else -1
            t = {k: v.to(hip_device).clone().requires_grad_(k in names) for k, v in s.items()}
            img, a, meta = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"],
                                         t["viewmats"], t["Ks"], w, h, packed=False, render_mode="RGB+ED")
            g = torch.Generator().manual_seed(7)
            v_img = torch.randn(img.shape, generator=g).to(hip_device)
            ((img * v_img).sum() + (a * a).sum()).backward()
            res[tag] = {k: t[k].grad.cpu() for k in names}
    finally:
        rendering.tuning.bwd_block_walk = -1
        rendering.tuning.heavy_tile_len = -1
    for k in names:
        assert torch.equal(res["blocks"][k], res["blocks2"][k]), f"grad[{k}] not reproducible"
        ref = res["quad"][k].double()
        err = (res["blocks"][k].double() - ref).abs()
        tol = 2e-4 * float(ref.abs().max()) + 1e-4 * ref.abs()
        assert bool((err <= tol).all()), f"grad[{k}]: max err {float(err.max()):.3e} vs max {float(ref.abs().max()):.3e}"


@pytest.mark.parametrize("mode,channels,tile_cull", [("RGB+ED", 9, True), ("RGB", 3, True), ("RGB+ED", 9, False)])
def test_quadrant_reach_masks_change_nothing(hip_device, mode, channels, tile_cull):
    """Inside the compositors every list entry carries a 4-bit mask of the 8x8 quadrants its splat can reach; the
    other quadrants are not evaluated.  That only removes work that is predicated off at every pixel, so with the
    masks switched off (MobgsTuning.quadrant_culling = 0: everything is evaluated) images, alphas AND gradients must
    be bit-identical -- skipped terms are exact zeros added to the same sums in the same order.  Small, thin and
    rotated splats stress the conservative margin of the reach test; with tile culling off the lists also hold
    entries that reach no quadrant at all."""
    from mobgs_amd import _lib, rendering
    from mobgs_amd.rendering import rasterization
    lib = _lib.load()
    n, w, h = 8000, 232, 168
    s, _ = _scene(n, w, h, 21, channels)
    g0 = torch.Generator().manual_seed(5)
    s["scales"] = s["scales"] * torch.exp(torch.randn(s["scales"].shape, generator=g0) * 0.9)  # needles and blobs
    names = ["means", "quats", "scales", "opacities", "colors", "viewmats"]
    res = {}
    rendering.set_tile_culling(tile_cull)
    try:
        for masks in (1, 0):
            rendering.tuning.quadrant_culling = masks
            t = {k: v.to(hip_device).clone().requires_grad_(k in names) for k, v in s.items()}
            img, a, meta = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"],
                                         t["viewmats"], t["Ks"], w, h, packed=False, render_mode=mode)
            g = torch.Generator().manual_seed(7)
            v_img = torch.randn(img.shape, generator=g).to(hip_device)
            ((img * v_img).sum() + (a * a).sum()).backward()
            res[masks] = (img.detach().cpu(), a.detach().cpu(), {k: t[k].grad.cpu() for k in names})
    finally:
        rendering.tuning.quadrant_culling = -1
        rendering.set_tile_culling(True)
    assert torch.equal(res[1][0], res[0][0]), "image differs"
    assert torch.equal(res[1][1], res[0][1]), "alpha differs"
    for k in names:
        assert torch.equal(res[1][2][k], res[0][2][k]), f"grad[{k}] differs"


def test_counts_reach_the_host_without_an_event(hip_device):
    """Speculative binning: the last binning kernel stores {I_box, I, longest list} and then a sequence number into
    the caller's pinned, device-mapped slot; the host polls that word.  No event is recorded (no marker packet
    between the binning kernels and the compositing launch) and the counts are the synchronous path's."""
    from mobgs_amd import rendering
    n, w, h = 5000, 176, 144
    s, _ = _scene(n, w, h, 13, 3)
    d = _to(s, hip_device)
    assert rendering.SPECULATIVE_BINNING
    sp = rendering.SharedProjection(d["means"], d["quats"], d["scales"], d["opacities"], d["viewmats"], d["Ks"], w, h)
    pend = sp.tl._pending
    assert pend is not None and pend.event is None and pend.seq > 0
    n_spec = sp.tl.n_isects  # resolves by polling
    assert not sp.tl.pending
    tl = rendering.build_tile_lists(sp.means2d.detach(), sp.radii, sp.depths.detach(), sp.conics.detach(),
                                    d["opacities"], sp.tiles_per_gauss, w, h)
    assert n_spec == tl.n_isects and n_spec > 0
    assert torch.equal(sp.tl.tile_offsets.cpu(), tl.tile_offsets.cpu())


def test_tile_schedule_is_a_permutation_and_changes_nothing(hip_device):
    """TileLists.tile_order: every tile exactly once, list lengths non-increasing up to the width of one length
    class; images and gradients are bit-identical with the schedule on or off (it only reorders workgroups)."""
    import sys
    from mobgs_amd import _lib, rendering
    n, w, h = 6000, 200, 152
    s, _ = _scene(n, w, h, 21, 9)
    names = ["means", "quats", "scales", "opacities", "colors", "viewmats"]
    res = {}
    old_heavy = rendering.tuning.heavy_tile_len
    rendering.tuning.heavy_tile_len = 0  # a pure permutation: no workgroup-per-tile splitting (its own test below)
    for sched in (False, True):
        rendering.TILE_SCHEDULE = sched
        try:
            t = {k: v.to(hip_device).clone().requires_grad_(k in names) for k, v in s.items()}
            sp = rendering.SharedProjection(t["means"], t["quats"], t["scales"], t["opacities"], t["viewmats"],
                                            t["Ks"], w, h)
            img, a = sp.composite(t["colors"])
            g = torch.Generator().manual_seed(7)
            v_img = torch.randn(img.shape, generator=g).to(hip_device)
            ((img * v_img).sum() + a.sum()).backward()
            res[sched] = (img.detach().cpu(), a.detach().cpu(),
                          {k: t[k].grad.cpu() for k in names if t[k].grad is not None})
            if sched:
                off = sp.tl.tile_offsets.cpu()
                lens = (off[1:] - off[:-1])
                slots = sp.tl.tile_order.cpu().long()
                assert slots.numel() == _lib.load().mobgs_tile_order_len(lens.numel()) >= lens.numel() + 4
                used = slots[slots >= 0]
                heavy = (used & (1 << 30)) != 0
                assert not bool(heavy.any())
                order = used
                assert sorted(order.tolist()) == list(range(lens.numel()))
                assert bool((slots[:lens.numel()] >= 0).all()) and bool((slots[lens.numel():] < 0).all())
                ol = lens[order]
                width_of_class = int(lens.max()) // 1023 + 1
                assert bool((ol[1:] <= ol[:-1] + width_of_class).all())
                assert int(ol[0]) >= int(lens.max()) - width_of_class
            else:
                assert sp.tl.tile_order is None
        finally:
            rendering.TILE_SCHEDULE = True
            if sched or sys.exc_info()[0] is not None:
                rendering.tuning.heavy_tile_len = old_heavy
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    for k in res[False][2]:
        assert torch.equal(res[True][2][k], res[False][2][k]), k


@pytest.mark.parametrize("n,w,h,scale,quant", [(3000, 48, 32, 8.0, 4), (12000, 64, 48, 3.0, 4),
                                               (12000, 64, 48, 3.0, 2048), (40000, 64, 48, 3.0, 4),
                                               (70000, 64, 48, 3.0, 2048), (150000, 96, 64, 2.5, 65536)])
def test_long_tile_lists_sort_exactly(hip_device, n, w, h, scale, quant):
    """Few tiles, many big splats: per-tile lists of several hundred to > 4096 entries exercise the multi-chunk
    LDS network, the radix sort of the 1024-thread variant -- with short runs of equal depth (quant 2048: tie fix-up
    by flat id) and with runs of hundreds (quant 4: falls back to the network on the full keys) -- and, from the
    fourth case on, lists beyond the LDS sort (> 16384 entries; round 3: radix-sorted 16384-entry chunks + merge-path
    passes, 3 to 10 chunks per list here, with and without long runs of equal depth); order must be upstream's."""
    from mobgs_amd import rendering
    from mobgs_amd.rendering import rasterization
    from oracle import gsplat_cpu as Cc
    s, _ = _scene(n, w, h, 5, 3)
    s["scales"] = s["scales"] * scale
    g = torch.Generator().manual_seed(1)
    s["means"][:, 2] = torch.round(s["means"][:, 2] * quant) / quant + 1.0  # exact depth ties -> index tie-break
    d = _to(s, hip_device)
    rendering.set_tile_culling(False)
    try:
        img, a, meta = rasterization(d["means"], d["quats"], d["scales"], d["opacities"], d["colors"], d["viewmats"],
                                     d["Ks"], w, h, packed=False)
    finally:
        rendering.set_tile_culling(True)
    # expected lists = upstream's binning + stable sort (C oracle) applied to the GPU's OWN projection outputs, so a
    # last-ulp radius difference between the two projections cannot masquerade as an ordering error
    tpg, ids, flat, eoffs = Cc.isect(meta["means2d"].cpu().numpy(), meta["radii"].cpu().numpy(),
                                     meta["depths"].cpu().numpy(), w, h)
    offs = meta["isect_offsets"].cpu().reshape(-1).tolist() + [meta["flatten_ids"].numel()]
    longest = max(b - a_ for a_, b in zip(offs[:-1], offs[1:]))
    assert longest > 500, longest
    assert torch.equal(meta["tiles_per_gauss"].cpu(), torch.from_numpy(tpg))
    assert torch.equal(meta["isect_offsets"].cpu().reshape(-1), torch.from_numpy(eoffs).reshape(-1))
    assert torch.equal(meta["flatten_ids"].cpu(), torch.from_numpy(flat)), f"order differs (longest {longest})"
    assert torch.equal(meta["isect_ids"].cpu(), torch.from_numpy(ids))


@pytest.mark.parametrize("n,w,h,scale,quant,arm", [(12000, 64, 48, 3.0, 2048, 2048), (40000, 64, 48, 3.0, 4, 12288)])
def test_long_tile_lists_sort_exactly_on_a_speculative_second_frame(hip_device, n, w, h, scale, quant, arm):
    """The speculative emit + sort (counts still on the device) with a hint beyond the one-launch sort: the second frame of
    a workload whose first frame had lists > 2048 entries takes the long-list launch, and with lists > 3/4 x 16384 the
    chunk + merge passes sized from the ARENA (the count is not known on the host).  12 tiles; the lists must be the
    synchronous path's, entry for entry."""
    from mobgs_amd import rendering
    from mobgs_amd.rendering import rasterization
    s, _ = _scene(n, w, h, 5, 3)
    s["scales"] = s["scales"] * scale
    s["means"][:, 2] = torch.round(s["means"][:, 2] * quant) / quant + 1.0  # exact depth ties -> index tie-break
    d = _to(s, hip_device)
    key = rendering._workload_key(hip_device, 1, n, w, h)
    res = {}
    rendering.set_tile_culling(False)
    try:
        for spec in (True, False):
            rendering.SPECULATIVE_BINNING = spec
            rendering.forget_hints()
            for frame in range(2 if spec else 1):
                if frame:  # what the first frame left selects the arm of the second
                    assert rendering.hint_record(key).longest > arm, rendering.hint_record(key).longest
                before = (rendering.list_rebuilds[0], rendering.fused_calls[0])
                _, _, meta = rasterization(d["means"], d["quats"], d["scales"], d["opacities"], d["colors"], d["viewmats"],
                                           d["Ks"], w, h, packed=False)
                if frame:  # ... whose lists are the speculative two-pass call's own: no synchronous rebuild, no segments
                    assert (rendering.list_rebuilds[0], rendering.fused_calls[0]) == before
            res[spec] = {k: meta[k].cpu() for k in ("isect_offsets", "flatten_ids", "isect_ids")}
    finally:
        rendering.SPECULATIVE_BINNING = True
        rendering.set_tile_culling(True)
    offs = res[False]["isect_offsets"].reshape(-1).tolist() + [res[False]["flatten_ids"].numel()]
    assert max(b - a_ for a_, b in zip(offs[:-1], offs[1:])) > arm
    for k in res[False]:
        assert torch.equal(res[True][k], res[False][k]), k


def test_two_cameras_forward_backward(hip_device):
    """C = 2 cameras in one call (gsplat's batched-camera form): lists, images and all gradients incl. both viewmats."""
    from mobgs_amd import rendering
    from mobgs_amd.rendering import rasterization
    from oracle import gsplat_torch as G
    n, w, h = 1800, 104, 72
    s, _ = _scene(n, w, h, 6, 3)
    vm = torch.eye(4)[None].repeat(2, 1, 1)
    ang = 0.06
    vm[1, :3, :3] = torch.tensor([[math.cos(ang), 0, math.sin(ang)], [0, 1, 0], [-math.sin(ang), 0, math.cos(ang)]])
    vm[1, :3, 3] = torch.tensor([0.1, 0.03, 0.2])
    s["viewmats"] = vm
    s["Ks"] = s["Ks"].repeat(2, 1, 1)
    bg = torch.rand(2, 3, generator=torch.Generator().manual_seed(2))
    names = ["means", "quats", "scales", "opacities", "colors", "viewmats"]

    def run(fn, dev):
        t = {k: v.to(dev).clone().requires_grad_(k in names) for k, v in s.items()}
        img, a, meta = fn(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], t["viewmats"], t["Ks"],
                          w, h, packed=False, backgrounds=bg.to(dev), render_mode="RGB+ED")
        g = torch.Generator().manual_seed(7)
        v_img = torch.randn(img.shape, generator=g).to(dev)
        v_a = torch.randn(a.shape, generator=g).to(dev)
        ((img * v_img).sum() + (a * v_a).sum()).backward()
        return img.detach().cpu(), a.detach().cpu(), meta, {k: t[k].grad.cpu() for k in names}

    ref = run(G.rasterization, torch.device("cpu"))
    rendering.set_tile_culling(False)
    try:
        out = run(rasterization, hip_device)
    finally:
        rendering.set_tile_culling(True)
    assert out[0].shape == (2, h, w, 4)
    for key in ("radii", "tiles_per_gauss", "flatten_ids", "isect_offsets", "isect_ids"):
        assert torch.equal(out[2][key].cpu(), ref[2][key]), key
    scale = float(ref[0].abs().max())
    # one blend step: 2 w (|c| + |pixel|), w <= 1/255 (was a flat scale / 50); observed: no flipped element
    step = 2.0 * (1.001 / 255.0) * 2.0 * scale
    close_ = lambda a, b, what, tol: _close(a, b, 0, tol, what, flip_frac=5e-4, flip_atol=step)  # noqa: E731
    close_(out[0], ref[0], "image", 3e-5 * scale)
    close_(out[1], ref[1], "alpha", 3e-5)
    for k in names:
        sc = float(ref[3][k].abs().max())
        _close(out[3][k], ref[3][k], 1e-3, 5e-4 * sc + 1e-6, f"grad[{k}]")
    assert float(out[3]["viewmats"][1].abs().max()) > 0 and float(out[3]["viewmats"][0].abs().max()) > 0


def test_speculative_arena_overflow_is_transparent(hip_device):
    """First frame of a dense scene: the speculative binning arena (sized by guess) is too small, the kernels enqueued
    behind it see empty lists, resolve() rebuilds the lists synchronously and the compositing launch is re-issued.
    Outputs and gradients equal the synchronous path bit for bit."""
    from mobgs_amd import rendering
    n, w, h = 2000, 256, 192
    s, _ = _scene(n, w, h, 31, 9)
    s["scales"] = s["scales"] * 12.0  # every splat covers dozens of tiles: I_box >> 16 N + 1024
    names = ["means", "quats", "scales", "opacities", "colors", "viewmats"]
    res = {}
    for spec in (True, False):
        rendering.SPECULATIVE_BINNING = spec
        rendering.forget_hints()
        try:
            t = {k: v.to(hip_device).clone().requires_grad_(k in names) for k, v in s.items()}
            sp = rendering.SharedProjection(t["means"], t["quats"], t["scales"], t["opacities"], t["viewmats"],
                                            t["Ks"], w, h)
            if spec:
                assert sp.tl.pending
            img, a = sp.composite(t["colors"])
            assert not sp.tl.pending
            if spec:
                assert sp.tl.n_box > 16 * n + 1024, sp.tl.n_box  # the guess WAS too small
            g = torch.Generator().manual_seed(7)
            v_img = torch.randn(img.shape, generator=g).to(hip_device)
            ((img * v_img).sum() + a.sum()).backward()
            res[spec] = (img.detach().cpu(), a.detach().cpu(), sp.tl.flatten_ids.cpu(),
                         {k: t[k].grad.cpu() for k in names if t[k].grad is not None})
            # second frame: the arena has grown, no rebuild
            if spec:
                sp2 = rendering.SharedProjection(t["means"], t["quats"], t["scales"], t["opacities"], t["viewmats"],
                                                 t["Ks"], w, h)
                img2, _ = sp2.composite(t["colors"])
                assert torch.equal(img2.detach().cpu(), res[spec][0])
        finally:
            rendering.SPECULATIVE_BINNING = True
    assert float(res[True][1].max()) > 0.5  # something was actually rendered
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    assert torch.equal(res[True][2], res[False][2])
    for k in res[False][3]:
        assert torch.equal(res[True][3][k], res[False][3][k]), k


def _clustered_scene(n, w, h, seed, frac=0.4, region=0.12):
    s, cam = _scene(n, w, h, seed, 9)
    g = torch.Generator().manual_seed(seed + 1)
    k = int(frac * n)
    m = s["means"].clone()
    z = m[:k, 2]
    m[:k, 0] = (torch.rand(k, generator=g) - 0.5) * region * z * cam.width / cam.focal
    m[:k, 1] = (torch.rand(k, generator=g) - 0.5) * region * z * cam.height / cam.focal
    s["means"] = m
    return s


def test_heavy_tiles_are_split_over_a_workgroup(hip_device):
    """Tiles with long lists are composited by 4 waves (one 8x8 quadrant each).  Images are bit-identical to the
    one-wave-per-tile path, gradients equal up to the summation order of the four quadrant records; the schedule
    marks exactly the longest tiles, in all 4 slots of a workgroup."""
    from mobgs_amd import _lib, rendering
    lib = _lib.load()
    n, w, h = 8000, 208, 160
    s = _clustered_scene(n, w, h, 41)
    names = ["means", "quats", "scales", "opacities", "colors", "viewmats"]
    res = {}
    old = rendering.tuning.heavy_tile_len
    try:
        thr = 48
        for mode in ("light", "heavy", "raster"):
            rendering.tuning.heavy_tile_len = thr if mode == "heavy" else 0
            rendering.TILE_SCHEDULE = mode != "raster"
            t = {k: v.to(hip_device).clone().requires_grad_(k in names) for k, v in s.items()}
            sp = rendering.SharedProjection(t["means"], t["quats"], t["scales"], t["opacities"], t["viewmats"],
                                            t["Ks"], w, h)
            img, a = sp.composite(t["colors"])
            g = torch.Generator().manual_seed(7)
            v_img = torch.randn(img.shape, generator=g).to(hip_device)
            ((img * v_img).sum() + a.sum()).backward()
            res[mode] = (img.detach().cpu(), a.detach().cpu(), {k: t[k].grad.cpu() for k in names if t[k].grad is not None})
            if mode == "light":  # threshold for the heavy run: about the longest eighth of this scene's lists
                off = sp.tl.tile_offsets.cpu()
                lens = (off[1:] - off[:-1])
                thr = max(48, int(lens.sort().values[-max(lens.numel() // 8, 1)]))
            if mode == "heavy":
                off = sp.tl.tile_offsets.cpu()
                lens = (off[1:] - off[:-1])
                slots = sp.tl.tile_order.cpu().long()
                used = slots[slots >= 0]
                hv = (used & (1 << 30)) != 0
                n_heavy = int(hv.sum()) // 4
                nt = lens.numel()  # a grid this small may go heavy entirely (include/mobgs_hip.h)
                assert 0 < n_heavy <= (nt if nt <= 1024 else nt // 8), n_heavy
                assert 0 < int((~hv).sum()), "the scene must keep some light tiles for the checks below"
                head = slots[:4 * n_heavy].reshape(n_heavy, 4)
                assert bool((head == head[:, :1]).all()) and bool(((head & (1 << 30)) != 0).all())
                heavy_tiles = (head[:, 0] & ~(1 << 30))
                light_tiles = used[~hv]
                assert sorted(heavy_tiles.tolist() + light_tiles.tolist()) == list(range(lens.numel()))
                assert int(lens[heavy_tiles].min()) >= int(lens[light_tiles].max()) - (int(lens.max()) // 1023 + 1)
                assert int(lens[heavy_tiles].min()) >= thr - (int(lens.max()) // 1023 + 1)
    finally:
        rendering.tuning.heavy_tile_len = old
        rendering.TILE_SCHEDULE = True
    for other in ("light", "raster"):
        assert torch.equal(res["heavy"][0], res[other][0]) and torch.equal(res["heavy"][1], res[other][1]), other
        for k in res[other][2]:
            ref = res[other][2][k]
            # same terms, summed per quadrant first: fp32 re-association (amplified by cancellation in the
            # projection backward for a few quaternion / scale components)
            _close(res["heavy"][2][k], ref, 1e-4, 1e-5 * float(ref.abs().max()), f"grad[{k}] heavy vs {other}")


def test_zero_cotangent_pixels_are_skipped_exactly(hip_device):
    """Pixels whose cotangents are exactly zero are dropped from the backward walk: gradients equal those of the
    same cotangent image with a tiny non-zero value there, up to that value's contribution; an all-zero cotangent
    gives exactly zero gradients."""
    from mobgs_amd import rendering
    n, w, h = 4000, 160, 112
    s, _ = _scene(n, w, h, 51, 9)
    names = ["means", "quats", "scales", "opacities", "colors"]

    def grads(v_img, v_a):
        t = {k: v.to(hip_device).clone().requires_grad_(k in names) for k, v in s.items()}
        sp = rendering.SharedProjection(t["means"], t["quats"], t["scales"], t["opacities"], t["viewmats"], t["Ks"],
                                        w, h)
        img, a = sp.composite(t["colors"])
        torch.autograd.backward([img, a], [v_img.to(hip_device), v_a.to(hip_device)])
        return {k: t[k].grad.cpu() for k in names}

    g = torch.Generator().manual_seed(3)
    v_img = torch.randn(1, h, w, 10, generator=g)
    v_a = torch.randn(1, h, w, 1, generator=g)
    mask = torch.zeros(1, h, w, 1)
    mask[:, 20:70, 30:120] = 1.0  # loss restricted to a window
    ref = grads(v_img * mask + 1e-30 * (1 - mask), v_a * mask)   # nowhere exactly zero: nothing is skipped
    got = grads(v_img * mask, v_a * mask)
    for k in names:
        # (the skipped pixels shorten the walk, which moves the batch boundaries: the matrix-pipe backward then groups the
        # same terms differently -- observed 2e-6 of the maximum; the quadrant kernel adds them in the same order)
        _close(got[k], ref[k], 1e-5, 1e-5 * float(ref[k].abs().max()) + 1e-12, f"grad[{k}] with masked cotangents")
    zero = grads(torch.zeros_like(v_img), torch.zeros_like(v_a))
    for k in names:
        assert float(zero[k].abs().max()) == 0.0, k


def test_small_grids_go_heavy_by_default(hip_device):
    """A grid with fewer tiles than the chip has wave slots (512x288, the reference's training resolution: 576 tiles)
    is scheduled workgroup-per-tile by default -- every non-empty tile of a grid of <= 1024 tiles; images are
    bit-identical to the one-wave-per-tile schedule, gradients equal up to the summation order of the quadrants."""
    from mobgs_amd import rendering
    n, w, h = 20000, 512, 288
    s, _ = _scene(n, w, h, 33, 9)
    names = ["means", "quats", "scales", "opacities", "colors", "viewmats"]
    res = {}
    old = rendering.tuning.heavy_tile_len
    try:
        for mode, knob in (("default", -1), ("light", 0)):
            rendering.tuning.heavy_tile_len = knob
            t = {k: v.to(hip_device).clone().requires_grad_(k in names) for k, v in s.items()}
            sp = rendering.SharedProjection(t["means"], t["quats"], t["scales"], t["opacities"], t["viewmats"],
                                            t["Ks"], w, h)
            img, a = sp.composite(t["colors"])
            g = torch.Generator().manual_seed(7)
            ((img * torch.randn(img.shape, generator=g).to(hip_device)).sum() + a.sum()).backward()
            res[mode] = (img.detach().cpu(), a.detach().cpu(), {k: t[k].grad.cpu() for k in names})
            slots = sp.tl.tile_order.cpu().long()
            used = slots[slots >= 0]
            n_heavy = int(((used & (1 << 30)) != 0).sum()) // 4
            off = sp.tl.tile_offsets.cpu()
            lens = off[1:] - off[:-1]
            if mode == "default":
                assert lens.numel() == 32 * 18 and n_heavy == int((lens > 0).sum()) > 500, (n_heavy, lens.numel())
            else:
                assert n_heavy == 0
    finally:
        rendering.tuning.heavy_tile_len = old
    assert torch.equal(res["default"][0], res["light"][0]) and torch.equal(res["default"][1], res["light"][1])
    for k, ref in res["light"][2].items():
        tol = 1e-4 * float(ref.abs().max()) + 1e-9  # fp32 sums of the same terms in another order
        assert float((res["default"][2][k] - ref).abs().max()) <= tol, k


@pytest.mark.parametrize("channels", [9, 2])
def test_zero_cotangents_give_exact_zero_gradients(hip_device, channels):
    """A compositing pass whose cotangents are all exactly zero (a loss term with weight 0) writes no gradient record;
    the per-splat reduction then reads no slot (any_record flag, include/mobgs_hip.h) and every gradient is an exact
    zero -- while a single non-zero cotangent pixel brings back the ordinary result."""
    from mobgs_amd.rendering import rasterization
    n, w, h = 5000, 200, 152
    s, _ = _scene(n, w, h, 17, channels)
    names = ["means", "quats", "scales", "opacities", "colors"]
    res = {}
    for mode in ("zero", "one_pixel"):
        t = {k: v.to(hip_device).clone().requires_grad_(k in names) for k, v in s.items()}
        img, a, _ = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], t["viewmats"],
                                  t["Ks"], w, h, packed=False, render_mode="RGB")
        v = torch.zeros_like(img)
        if mode == "one_pixel":
            v[0, h // 2, w // 2, 0] = 1.0
        torch.autograd.backward([img, a], [v, torch.zeros_like(a)])
        res[mode] = {k: t[k].grad.cpu() for k in names}
    for k, g in res["zero"].items():
        assert float(g.abs().max()) == 0.0, k
    assert float(res["one_pixel"]["colors"].abs().max()) > 0.0
    assert float(res["one_pixel"]["means"].abs().max()) > 0.0
