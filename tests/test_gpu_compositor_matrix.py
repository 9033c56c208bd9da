"""Oracle parity for every compositor build the dispatcher can select.

The compositors are a matrix: one build per total channel count D in rendering._SUPPORTED (other counts are zero-padded
up to the next build), and per build the arms mobgs_raster_path() picks from MobgsTuning and the grid size -- forward
quadrant / block-walk kernel, heavy-tile schedule none / all / mixed, backward quadrant / mfma / mfma_team / block-walk --
plus the class-filtered builds (D = 10 and D = 1) behind SharedProjection.composite_layers() / class_alpha().

Every row below states the kernels it must take (asserted from rendering.path_log) and is compared with the C oracle
(oracle/gsplat_cpu.c, computed once per scene / channel count / mode and cached): image, alphas, projection outputs and
all input gradients, within the bounds of test_gpu_operator_parity.py.  The class passes are compared with the oracle run
on the class's rows alone.  test_every_reachable_build_has_an_oracle_row fails when a build or an arm becomes reachable
that no row covers.

MOBGS_TEST_REPORT=1 (with -s) prints every comparison's observed error next to its allowance (tests/helpers.observe).
"""
import contextlib
import itertools
import math
import zlib

import numpy as np
import pytest
import torch

from helpers import close_image_with_blend_flips, observe
from mobgs_amd.synth import SynthCamera, splat_inputs

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------------
# scenes: grids on both sides of SCHED_SMALL_GRID = 1024 tiles, where the arm defaults change
# ---------------------------------------------------------------------------------------------------------------------
SCENES = {
    # 13 x 9 = 117 tiles (small-grid defaults), a third of the splats pulled into a window: list lengths ~30 .. ~400
    "S": dict(n=3000, w=200, h=136, seed=1, scale=0.4, cluster=(0.3, 0.3)),
    # 33 x 32 = 1056 tiles, ragged (520 = 32.5 tiles, 504 = 31.5 tiles), uniform: no list near 1024 entries
    "Bu": dict(n=12000, w=520, h=504, seed=2, scale=0.4),
    # the same grid, half the splats in a small window: some (< 10 %) tiles above 1024 entries
    "Bc": dict(n=16000, w=520, h=504, seed=3, scale=0.5, cluster=(0.5, 0.06)),
    # two cameras of 25 x 24 = 600 tiles: each below the threshold, the batch (1200) above it
    "C2": dict(n=8000, w=392, h=376, seed=6, scale=0.4, cams=2),
    # narrower than one tile
    "N": dict(n=1500, w=12, h=136, seed=4, scale=0.4),
}
CLUSTERED = ("S", "Bc")
HEAVY_SMALL = 96   # the "small" heavy_tile_len: between the bulk and the clustered tiles of S and Bc
NAMES = ["means", "quats", "scales", "opacities", "colors", "viewmats"]

_scene_cache = {}


def _scene(name, channels):
    """CPU inputs of a scene with `channels` colour channels (C2: per-camera colours [C,N,D] and opacities [C,N])."""
    key = (name, channels)
    if key in _scene_cache:
        return _scene_cache[key]
    sp = SCENES[name]
    cam = SynthCamera().scaled(sp["w"], sp["h"])
    s = splat_inputs(sp["n"], cam, sp["seed"], max(channels, 1))
    s["scales"] = s["scales"] * sp["scale"]
    if "cluster" in sp:   # scripts/heavy_tail.py's recipe
        frac, region = sp["cluster"]
        g = torch.Generator().manual_seed(sp["seed"] + 1)
        k = int(frac * sp["n"])
        m = s["means"].clone()
        z = m[:k, 2]
        m[:k, 0] = (torch.rand(k, generator=g) - 0.5) * region * z * cam.width / cam.focal
        m[:k, 1] = (torch.rand(k, generator=g) - 0.5) * region * z * cam.height / cam.focal
        s["means"] = m
    if sp.get("cams", 1) == 2:
        g = torch.Generator().manual_seed(sp["seed"] + 2)
        ang = 0.06
        vm = torch.eye(4)[None].repeat(2, 1, 1)
        vm[1, :3, :3] = torch.tensor([[math.cos(ang), 0, math.sin(ang)], [0, 1, 0], [-math.sin(ang), 0, math.cos(ang)]])
        vm[1, :3, 3] = torch.tensor([0.1, 0.03, 0.2])
        s["viewmats"] = vm
        s["Ks"] = s["Ks"].repeat(2, 1, 1)
        s["colors"] = torch.stack([s["colors"], torch.randn(s["colors"].shape, generator=g)])
        s["opacities"] = torch.stack([s["opacities"], 0.05 + 0.9 * torch.rand(s["opacities"].shape, generator=g)])
    _scene_cache[key] = s
    return s


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _total(channels, mode):
    return channels + (1 if mode == "RGB+ED" else 0)


# ---------------------------------------------------------------------------------------------------------------------
# the arm table: (scene, colour channels, render_mode, knobs) -> the (fwd_kernel, bwd_kernel, heavy mode) it must take
# knobs: "bw0" block_walk = 0, "bb1" bwd_block_walk = 1, "m<k>" bwd_mfma = k, "h<k>" heavy_tile_len = k; unnamed = default
# heavy mode: "none" (heavy_tile_len 0), "all" (1: every non-empty tile), "mixed" (lists >= heavy_tile_len)
# ---------------------------------------------------------------------------------------------------------------------
_KNOB = {"bw": "block_walk", "bb": "bwd_block_walk", "m": "bwd_mfma", "h": "heavy_tile_len"}
_HS = f"h{HEAVY_SMALL}"

FWD_BLOCKS = {"": "blocks", "bw0": "quadrant"}         # D = 9, 10, 12: the block-walk forward exists
FWD_QUAD = {"": "quadrant"}
# small grids: bwd_mfma defaults to 1; bwd_block_walk (D = 9, 10 only) takes precedence over it
BWD_SMALL_WALK = {"": "mfma", "m0": "quadrant", "m2": "mfma_team", "bb1": "block_walk"}   # D = 9, 10
BWD_SMALL_MFMA = {"": "mfma", "m0": "quadrant", "m2": "mfma_team", "bb1": "quadrant"}    # D = 1, 3, 4
BWD_SMALL_QUAD = {"": "quadrant", "m2": "quadrant", "bb1": "quadrant"}                   # D = 2, 12, 16, 26
HEAVY_SMALL_GRID = {"": "all", "h0": "none", _HS: "mixed"}


def _product(scene, channels, mode, fwd, bwd, heavy):
    return [(scene, channels, mode, " ".join(k for k in (kf, kb, kh) if k), ef, eb, eh)
            for (kf, ef), (kb, eb), (kh, eh) in itertools.product(fwd.items(), bwd.items(), heavy.items())]


ROWS = (
    # --- S (117 tiles): every arm combination of every build
    _product("S", 1, "RGB", FWD_QUAD, BWD_SMALL_MFMA, HEAVY_SMALL_GRID)
    + _product("S", 2, "RGB", FWD_QUAD, BWD_SMALL_QUAD, HEAVY_SMALL_GRID)
    + _product("S", 3, "RGB", FWD_QUAD, BWD_SMALL_MFMA, HEAVY_SMALL_GRID)
    + _product("S", 4, "RGB", FWD_QUAD, BWD_SMALL_MFMA, HEAVY_SMALL_GRID)
    + _product("S", 9, "RGB", FWD_BLOCKS, BWD_SMALL_WALK, HEAVY_SMALL_GRID)
    + _product("S", 9, "RGB+ED", FWD_BLOCKS, BWD_SMALL_WALK, HEAVY_SMALL_GRID)   # D = 10
    + _product("S", 12, "RGB", FWD_BLOCKS, BWD_SMALL_QUAD, HEAVY_SMALL_GRID)
    + _product("S", 16, "RGB", FWD_QUAD, BWD_SMALL_QUAD, HEAVY_SMALL_GRID)
    + _product("S", 26, "RGB", FWD_QUAD, BWD_SMALL_QUAD, HEAVY_SMALL_GRID)
    + [
        # every build as channels = D - 1 with the expected-depth channel
        ("S", 1, "RGB+ED", "", "quadrant", "quadrant", "all"),
        ("S", 2, "RGB+ED", "", "quadrant", "mfma", "all"),
        ("S", 3, "RGB+ED", "", "quadrant", "mfma", "all"),
        ("S", 8, "RGB+ED", "", "blocks", "mfma", "all"),
        ("S", 10, "RGB", "", "blocks", "mfma", "all"),
        ("S", 11, "RGB+ED", "", "blocks", "quadrant", "all"),
        ("S", 15, "RGB+ED", "", "quadrant", "quadrant", "all"),
        ("S", 25, "RGB+ED", "", "quadrant", "quadrant", "all"),
        # padded totals 5, 7, 11, 13, 20, 25 (-> builds 9, 9, 12, 16, 26, 26)
        ("S", 4, "RGB+ED", "", "blocks", "mfma", "all"),
        ("S", 6, "RGB+ED", "m2", "blocks", "mfma_team", "all"),
        ("S", 10, "RGB+ED", "", "blocks", "quadrant", "all"),
        ("S", 12, "RGB+ED", "h0", "quadrant", "quadrant", "none"),
        ("S", 19, "RGB+ED", "", "quadrant", "quadrant", "all"),
        ("S", 24, "RGB+ED", _HS, "quadrant", "quadrant", "mixed"),
        ("Bu", 4, "RGB+ED", "", "blocks", "quadrant", "mixed"),
        ("Bc", 24, "RGB+ED", "", "quadrant", "quadrant", "mixed"),
        # --- B (1056 tiles): defaults there are quadrant backward + lists >= 1024 heavy
        ("Bu", 9, "RGB+ED", "", "blocks", "quadrant", "mixed"),
        ("Bu", 1, "RGB", "h0", "quadrant", "quadrant", "none"),
        ("Bu", 2, "RGB", "h0", "quadrant", "quadrant", "none"),
        ("Bu", 3, "RGB", "h0", "quadrant", "quadrant", "none"),
        ("Bu", 4, "RGB", "h0", "quadrant", "quadrant", "none"),
        ("Bu", 9, "RGB", "h0", "blocks", "quadrant", "none"),
        ("Bu", 9, "RGB+ED", "h0", "blocks", "quadrant", "none"),
        ("Bu", 12, "RGB", "h0", "blocks", "quadrant", "none"),
        ("Bu", 16, "RGB", "h0", "quadrant", "quadrant", "none"),
        ("Bu", 26, "RGB", "h0", "quadrant", "quadrant", "none"),
        ("Bu", 9, "RGB", "bw0", "quadrant", "quadrant", "mixed"),
        ("Bu", 9, "RGB+ED", "bw0", "quadrant", "quadrant", "mixed"),
        ("Bu", 12, "RGB", "bw0", "quadrant", "quadrant", "mixed"),
        ("Bc", 1, "RGB", "", "quadrant", "quadrant", "mixed"),
        ("Bc", 2, "RGB", "", "quadrant", "quadrant", "mixed"),
        ("Bc", 3, "RGB", "", "quadrant", "quadrant", "mixed"),
        ("Bc", 4, "RGB", "", "quadrant", "quadrant", "mixed"),
        ("Bc", 9, "RGB", "", "blocks", "quadrant", "mixed"),
        ("Bc", 9, "RGB+ED", "", "blocks", "quadrant", "mixed"),
        ("Bc", 12, "RGB", "", "blocks", "quadrant", "mixed"),
        ("Bc", 16, "RGB", "", "quadrant", "quadrant", "mixed"),
        ("Bc", 26, "RGB", "", "quadrant", "quadrant", "mixed"),
        ("Bc", 3, "RGB", _HS, "quadrant", "quadrant", "mixed"),
        ("Bc", 9, "RGB+ED", _HS, "blocks", "quadrant", "mixed"),
        ("Bc", 16, "RGB", _HS, "quadrant", "quadrant", "mixed"),
        ("Bc", 1, "RGB", "m1", "quadrant", "mfma", "mixed"),
        ("Bc", 1, "RGB", "m2", "quadrant", "mfma_team", "mixed"),
        ("Bc", 3, "RGB", "m1", "quadrant", "mfma", "mixed"),
        ("Bc", 3, "RGB", "m2", "quadrant", "mfma_team", "mixed"),
        ("Bc", 4, "RGB", "m1", "quadrant", "mfma", "mixed"),
        ("Bc", 4, "RGB", "m2", "quadrant", "mfma_team", "mixed"),
        ("Bc", 9, "RGB", "m1", "blocks", "mfma", "mixed"),
        ("Bc", 9, "RGB", "m2", "blocks", "mfma_team", "mixed"),
        ("Bc", 9, "RGB+ED", "m1", "blocks", "mfma", "mixed"),
        ("Bc", 9, "RGB+ED", "m2", "blocks", "mfma_team", "mixed"),
        ("Bc", 9, "RGB", "bb1", "blocks", "block_walk", "mixed"),
        ("Bc", 9, "RGB+ED", "bb1", "blocks", "block_walk", "mixed"),
        # --- two cameras (1200 tiles in the batch): default and the benchmark's selection
        ("C2", 9, "RGB+ED", "", "blocks", "quadrant", "mixed"),
        ("C2", 9, "RGB+ED", "h0 m0", "blocks", "quadrant", "none"),
        ("C2", 3, "RGB", "", "quadrant", "quadrant", "mixed"),
        ("C2", 3, "RGB", "h0 m0", "quadrant", "quadrant", "none"),
        ("C2", 1, "RGB", "m2", "quadrant", "mfma_team", "mixed"),
        # --- an image narrower than a tile
        ("N", 9, "RGB+ED", "", "blocks", "mfma", "all"),
        ("N", 3, "RGB", "h0 m0", "quadrant", "quadrant", "none"),
    ]
)

# class passes: (scene, knobs, Ns) -> (fwd of the 10-channel pass, bwd of both class builds, heavy mode); the 1-channel
# coverage pass always takes the quadrant forward.  Ns "odd": about 0.45 N, not a multiple of 64; 0 / "N": one class empty
CLASS_ROWS = (
    [("S", " ".join(k for k in (kb, km, kh) if k), "odd", fb, bm, hm)
     for (kb, fb), (km, bm), (kh, hm) in itertools.product(
         {"": "blocks", "bw0": "quadrant"}.items(), {"m0": "quadrant", "": "mfma", "m2": "mfma_team"}.items(),
         HEAVY_SMALL_GRID.items())]
    + [("S", "", 0, "blocks", "mfma", "all"), ("S", "h0 m0", 0, "blocks", "quadrant", "none"),
       ("S", "", "N", "blocks", "mfma", "all"), ("S", "h0 m0", "N", "blocks", "quadrant", "none"),
       ("S", "bb1", "odd", "blocks", "mfma", "all")]   # bwd_block_walk does not apply to class passes
    + [(sc, " ".join(k for k in (km, kh) if k), "odd", "blocks", bm, hm)
       for sc in ("Bc", "C2")
       for (km, bm), (kh, hm) in itertools.product({"m0": "quadrant", "m1": "mfma", "m2": "mfma_team"}.items(),
                                                   {"": "mixed", "h0": "none"}.items())]
)


def _row_id(r):
    return f"{r[0]}-{r[1]}{'ed' if r[2] == 'RGB+ED' else ''}-{r[3].replace(' ', '_') or 'default'}"


def _class_id(r):
    return f"{r[0]}-Ns{r[2]}-{r[1].replace(' ', '_') or 'default'}"


@contextlib.contextmanager
def _tuned(knobs):
    """rendering.tuning with `knobs` applied and a fresh path_log; both restored afterwards."""
    from mobgs_amd import rendering
    t = rendering.tuning
    saved = {f: getattr(t, f) for f in _KNOB.values()}
    saved_log = rendering.path_log
    try:
        for k in knobs.split():
            name = k.rstrip("-0123456789")
            setattr(t, _KNOB[name], int(k[len(name):]))
        rendering.path_log = []
        yield rendering.path_log
    finally:
        for f, v in saved.items():
            setattr(t, f, v)
        rendering.path_log = saved_log


def _heavy_mode(heavy_len):
    return "none" if heavy_len == 0 else "all" if heavy_len == 1 else "mixed"


def _check_path(log, D, class_filter, fwd, bwd, heavy, lens, scene, directions=("fwd", "bwd")):
    """The logged passes of D channels took the expected kernels, and the schedule marked the tiles heavy_len says."""
    es = [e for e in log if e["D"] == D and e["class_filter"] == class_filter]
    assert sorted({e["dir"] for e in es}) == sorted(directions), es
    n_tiles = lens.numel()
    cap = n_tiles if n_tiles <= 1024 else n_tiles // 8
    width = int(lens.max()) // 1023 + 1   # the schedule sorts by length classes of this width
    for e in es:
        assert e["n_tiles"] == n_tiles, e
        got = (e["fwd_kernel"], e["bwd_kernel"], _heavy_mode(e["heavy_len"]))
        if e["dir"] == "fwd":
            assert got[0] == fwd and got[2] == heavy, (got, (fwd, bwd, heavy))
        else:
            assert got[1] == bwd and got[2] == heavy, (got, (fwd, bwd, heavy))
        n_heavy, thr = e["heavy_tiles"], e["heavy_len"]
        if heavy == "none":
            assert n_heavy == 0, e
        elif heavy == "all":
            assert n_heavy == int((lens > 0).sum()), e
        else:
            lo = min(int((lens >= thr + width).sum()), cap)
            hi = min(int((lens >= max(thr - width, 1)).sum()), cap)
            assert lo <= n_heavy <= hi, (e, lo, hi)
            if scene in CLUSTERED:   # a mixed row on a clustered scene really mixes
                assert 0 < n_heavy < int((lens > 0).sum()), e


def _lens(tl_offsets, total):
    off = tl_offsets.reshape(-1).cpu().long()
    return torch.diff(torch.cat([off, torch.tensor([int(total)])]))


def _close(a, b, rtol, atol, what, flip_frac=0.0, flip_atol=0.0):
    """test_gpu_operator_parity._close: |a-b| <= atol + rtol |b| except for a fraction flip_frac of the elements, which may
    be off by up to flip_atol (an alpha on the 1/255 cut or a transmittance at the 1e-4 stop)."""
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    nbad = int(bad.sum())
    emax = float(err.max()) if err.numel() else 0.0
    bmax = float(b.abs().max()) if b.numel() else 0.0
    msg = f"{what}: {nbad}/{bad.numel()} off, max err {emax:.3e} (ref max {bmax:.3e})"
    observe(what, nbad, bad.numel(), emax, flip_frac, flip_atol, bmax)
    assert nbad <= flip_frac * bad.numel(), msg
    if nbad:
        assert emax <= flip_atol, msg


def _close_grad(out, ref, what, camera=False):
    """test_rasterization_backward's bounds "vs C oracle" (1e-4 of the maximum for a camera-matrix gradient)."""
    scale = float(torch.as_tensor(ref).abs().max()) if torch.as_tensor(ref).numel() else 0.0
    _close(out, ref, 2e-4, (1e-4 if camera else 2e-5) * scale + 1e-7, what, flip_frac=2e-3, flip_atol=5e-4 * scale)


def _close_pixels(img, a, ref_img, ref_a, colors_max, spread, n_col, what):
    """test_rasterization_forward's bounds: alphas 2e-5, pixels 2e-5 of the range, 2e-4 of the elements within one blend
    step (helpers.close_image_with_blend_flips)."""
    img = img.detach().cpu().reshape(ref_img.shape)
    a = a.detach().cpu().reshape(ref_a.shape)
    _close(a, ref_a, 0, 2e-5, f"{what} alphas", flip_frac=2e-4, flip_atol=2.0 * 1.001 / 255)
    scale = max(1.0, float(ref_img.abs().max()))
    close_image_with_blend_flips(img, ref_img, ref_a, colors_max, spread, 2e-5 * scale, f"{what} image", flip_frac=2e-4,
                                 n_colour_channels=n_col, alphas_img=a)


# ---------------------------------------------------------------------------------------------------------------------
# references (C oracle), cached per (scene, channels, mode, background)
# ---------------------------------------------------------------------------------------------------------------------
_REF = {}


def _background(scene, channels, C):
    return torch.rand(C, channels, generator=_gen("bg", scene, channels))


def _cotangents(key, C, h, w, X):
    g = _gen("cot", *key)
    return torch.randn(C, h, w, X, generator=g), torch.randn(C, h, w, 1, generator=g)


def _reference(scene, channels, mode, use_bg):
    key = (scene, channels, mode, use_bg)
    if key not in _REF:
        from oracle import gsplat_cpu as Cc
        s = _scene(scene, channels)
        C, sp = s["viewmats"].shape[0], SCENES[scene]
        bg = _background(scene, channels, C) if use_bg else None
        v_img, v_a = _cotangents(key, C, sp["h"], sp["w"], _total(channels, mode))
        r = Cc.rasterization_fwd_bwd(*(s[k].numpy() for k in ["means", "quats", "scales", "opacities", "colors",
                                                              "viewmats", "Ks"]), sp["w"], sp["h"],
                                     backgrounds=None if bg is None else bg.numpy(), render_mode=mode,
                                     v_render=v_img.numpy(), v_alphas=v_a[..., 0].numpy())
        _REF[key] = ({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in r.items() if v is not None}, bg, v_img, v_a)
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------------------
# 1. plain passes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,channels,mode,knobs,fwd,bwd,heavy", ROWS, ids=[_row_id(r) for r in ROWS])
def test_plain_pass_matches_oracle(hip_device, scene, channels, mode, knobs, fwd, bwd, heavy):
    from mobgs_amd import rendering
    from mobgs_amd.rendering import rasterization
    s = _scene(scene, channels)
    sp = SCENES[scene]
    w, h = sp["w"], sp["h"]
    use_bg = mode == "RGB+ED" or channels % 2 == 1
    ref, bg, v_img, v_a = _reference(scene, channels, mode, use_bg)
    t = {k: v.to(hip_device).clone().requires_grad_(k in NAMES) for k, v in s.items()}
    with _tuned(knobs) as log:
        img, a, meta = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], t["viewmats"],
                                     t["Ks"], w, h, packed=False, render_mode=mode,
                                     backgrounds=None if bg is None else bg.to(hip_device))
        meta["means2d"].retain_grad()
        ((img * v_img.to(hip_device)).sum() + (a * v_a.to(hip_device)).sum()).backward()
        torch.cuda.synchronize()
        log = list(log)
    D = rendering._pad_channels(_total(channels, mode))
    lens = _lens(meta["isect_offsets"], meta["flatten_ids"].numel())
    _check_path(log, D, False, fwd, bwd, heavy, lens, scene)
    # projection
    assert torch.equal(meta["radii"].cpu(), ref["radii"]), "radii differ"
    vis = ref["radii"] > 0
    _close(meta["means2d"].detach().cpu()[vis], ref["means2d"][vis], 1e-5, 1e-4, "means2d")
    _close(meta["depths"].detach().cpu()[vis], ref["depths"][vis], 1e-6, 1e-6, "depths")
    _close(meta["conics"].detach().cpu()[vis], ref["conics"][vis], 2e-4, 1e-7, "conics")
    # pixels
    dv = ref["depths"][vis]
    spread = float(dv.max() - dv.min())
    _close_pixels(img, a, ref["render"], ref["alphas"].unsqueeze(-1), float(s["colors"].abs().max()), spread, channels,
                  f"[{_row_id((scene, channels, mode, knobs))}]")
    # gradients
    for k in NAMES + ["means2d"]:
        got = meta["means2d"].grad if k == "means2d" else t[k].grad
        _close_grad(got, ref["v_" + k], f"grad[{k}]", camera=k == "viewmats")


def test_more_channels_than_the_widest_build_are_refused(hip_device):
    """27 or more total channels have no build: NotImplementedError before any compositing launch."""
    from mobgs_amd.rendering import rasterization
    s = _scene("S", 27)
    d = {k: v.to(hip_device) for k, v in s.items()}
    sp = SCENES["S"]
    for cols, mode in ((d["colors"], "RGB"), (d["colors"][:, :26], "RGB+ED"), (torch.cat([d["colors"]] * 2, -1), "RGB")):
        with pytest.raises(NotImplementedError):
            rasterization(d["means"], d["quats"], d["scales"], d["opacities"], cols, d["viewmats"], d["Ks"], sp["w"],
                          sp["h"], packed=False, render_mode=mode)
    torch.cuda.synchronize()


def test_scene_premises(hip_device):
    """The grids and list lengths the rows rely on: S small, B / C2 above the threshold (C2 per camera below it), N
    narrower than a tile; the clustered scenes have lists on both sides of HEAVY_SMALL and Bc some, but fewer than 10 %,
    tiles above 1024 entries (so its default schedule really is mixed)."""
    from mobgs_amd.rendering import rasterization
    tiles = {"S": (13, 9), "Bu": (33, 32), "Bc": (33, 32), "C2": (25, 24), "N": (1, 9)}
    for name, sp in SCENES.items():
        s = _scene(name, 3)
        d = {k: v.to(hip_device) for k, v in s.items()}
        with torch.no_grad():
            _, _, meta = rasterization(d["means"], d["quats"], d["scales"], d["opacities"], d["colors"], d["viewmats"],
                                       d["Ks"], sp["w"], sp["h"], packed=False)
        C = sp.get("cams", 1)
        assert tuple(meta["isect_offsets"].shape) == (C, tiles[name][1], tiles[name][0]), name
        lens = _lens(meta["isect_offsets"], meta["flatten_ids"].numel())
        if name in CLUSTERED:
            assert int((lens < HEAVY_SMALL).sum()) > 0 and int((lens >= HEAVY_SMALL).sum()) > 0, (name, lens.min(), lens.max())
        if name == "Bc":
            long_ = int((lens > 1024).sum())
            assert 0 < long_ < 0.1 * lens.numel(), long_
        if name == "C2":
            assert lens.numel() > 1024 and lens.numel() // 2 <= 1024


# ---------------------------------------------------------------------------------------------------------------------
# 2. class-restricted and layered passes
# ---------------------------------------------------------------------------------------------------------------------
def _class_scene(scene):
    """The scene with 9 colours shared by all cameras (what composite_layers / class_alpha composite)."""
    s = dict(_scene(scene, 9))
    if s["colors"].dim() == 3:
        s["colors"], s["opacities"] = s["colors"][0], s["opacities"][0]
    return s


def _subset_reference(scene, rows, kind, use_bg):
    """C oracle on splat rows `rows` (a slice) alone: kind "rgbd" = the 9 colours + accumulated depth ("RGB+D"), "alpha" =
    a ones colour (the coverage pass; over the background [C,1] when use_bg).  An empty subset renders the background."""
    key = ("sub", scene, rows.start, rows.stop, kind, use_bg)
    if key in _REF:
        return _REF[key]
    from oracle import gsplat_cpu as Cc
    s = _class_scene(scene)
    sp = SCENES[scene]
    C, h, w = s["viewmats"].shape[0], sp["h"], sp["w"]
    X = 10 if kind == "rgbd" else 1
    bg = _background(scene, X - 1 if kind == "rgbd" else 1, C) if use_bg else None
    v_img, v_a = _cotangents(key, C, h, w, X)
    if kind == "alpha":   # class_alpha has one output: the render over a background, else the alphas
        if use_bg:
            v_a = torch.zeros_like(v_a)
        else:
            v_img = torch.zeros_like(v_img)
    n = len(range(s["means"].shape[0])[rows])
    if n == 0:
        render = torch.zeros(C, h, w, X)
        if bg is not None:
            render[..., :bg.shape[-1]] = bg[:, None, None, :]
        ref = {"render": render, "alphas": torch.zeros(C, h, w), "v_viewmats": torch.zeros(C, 4, 4)}
        for k, shp in (("means", 3), ("quats", 4), ("scales", 3), ("colors", 9)):
            ref["v_" + k] = torch.zeros(0, shp)
        ref["v_opacities"] = torch.zeros(0)
    else:
        cols = s["colors"][rows] if kind == "rgbd" else torch.ones(n, 1)
        r = Cc.rasterization_fwd_bwd(s["means"][rows].numpy(), s["quats"][rows].numpy(), s["scales"][rows].numpy(),
                                     s["opacities"][rows].numpy(), cols.numpy(), s["viewmats"].numpy(), s["Ks"].numpy(),
                                     w, h, backgrounds=None if bg is None else bg.numpy(),
                                     render_mode="RGB+D" if kind == "rgbd" else "RGB",
                                     v_render=v_img.numpy(), v_alphas=v_a[..., 0].numpy())
        ref = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in r.items() if v is not None}
    _REF[key] = (ref, bg, v_img, v_a)
    return _REF[key]


def _merged(parts, k, N):
    """Per-splat gradient over all N rows from per-subset references [(rows, ref), ...] (rows outside: 0), summed."""
    out = None
    for rows, ref in parts:
        if k == "viewmats":
            g = ref["v_viewmats"].clone()
        else:
            first = ref["v_" + k]
            g = torch.zeros((N,) + tuple(first.shape[1:]), dtype=first.dtype)
            g[rows] = first
        out = g if out is None else out + g
    return out


def _ns(scene, which):
    N = SCENES[scene]["n"]
    if which == "odd":
        ns = int(0.45 * N) | 1
        assert ns % 64 != 0
        return ns
    return N if which == "N" else int(which)


@pytest.mark.parametrize("scene,knobs,ns_kind,fwd,bwd,heavy", CLASS_ROWS, ids=[_class_id(r) for r in CLASS_ROWS])
def test_class_passes_match_oracle_on_each_class(hip_device, scene, knobs, ns_kind, fwd, bwd, heavy):
    """SharedProjection.composite_layers (static + dynamic: the FILTER builds of D = 10; want_all: raster_layers.hip) and
    class_alpha (D = 1, with and without a background) over the whole set's lists equal the C oracle run on the class's
    rows alone -- images, alphas and every input gradient."""
    from mobgs_amd.rendering import SharedProjection
    s = _class_scene(scene)
    sp = SCENES[scene]
    N, w, h = sp["n"], sp["w"], sp["h"]
    C = s["viewmats"].shape[0]
    Ns = _ns(scene, ns_kind)
    st, dy, al = slice(0, Ns), slice(Ns, N), slice(0, N)
    names = ["means", "quats", "scales", "opacities", "colors", "viewmats"]
    vis = _reference_vis(scene)
    cmax = max(float(s["colors"].abs().max()), float(vis.max()))
    spread = float(vis.max() - vis.min())

    def run(body):
        t = {k: v.to(hip_device).clone().requires_grad_(k in names) for k, v in s.items()}
        with _tuned(knobs) as log:
            proj = SharedProjection(t["means"], t["quats"], t["scales"], t["opacities"], t["viewmats"], t["Ks"], w, h)
            loss = body(proj, t)
            loss.backward()
            torch.cuda.synchronize()
            lens = _lens(proj.tl.tile_offsets[:-1], proj.tl.n_isects)
            return {k: t[k].grad.cpu() if t[k].grad is not None else torch.zeros_like(s[k]) for k in names}, list(log), lens

    def loss_of(outs, refs):
        return sum((o * v.to(hip_device).reshape(o.shape)).sum() for o, v in zip(outs, refs))

    def check_grads(got, parts, what):
        for k in names:
            _close_grad(got[k], _merged(parts, k, N), f"{what} grad[{k}]", camera=k == "viewmats")

    # (a) static + dynamic class passes (D = 10, FILTER = true)
    r_s = _subset_reference(scene, st, "rgbd", True)
    r_d = _subset_reference(scene, dy, "rgbd", True)
    bg9 = r_s[1].to(hip_device)
    held = {}

    def classes(proj, t):
        rs, als = proj.composite_layers(t["colors"], Ns, backgrounds=bg9)
        held["out"] = (rs[1], als[1], rs[2], als[2])
        return loss_of([rs[1], als[1], rs[2], als[2]], [r_s[2], r_s[3], r_d[2], r_d[3]])

    got, log, lens = run(classes)
    _check_path(log, 10, True, fwd, bwd, heavy, lens, scene)
    for (img, a), (ref, *_), tag in ((held["out"][:2], r_s, "static"), (held["out"][2:], r_d, "dynamic")):
        _close_pixels(img, a, ref["render"], ref["alphas"].unsqueeze(-1), cmax, spread, 10, f"class {tag}")
    check_grads(got, [(st, r_s[0]), (dy, r_d[0])], "classes")

    # (b) the layered walk: all + static + dynamic in one pass (raster_layers.hip); the gradient of each layer on its own
    #     (one backward pass per layer), each against its own reference
    layer_refs = ((al, _subset_reference(scene, al, "rgbd", True)), (st, _subset_reference(scene, st, "rgbd", True)),
                  (dy, _subset_reference(scene, dy, "rgbd", True)))
    for li, (rows, ref) in enumerate(layer_refs):
        def layers(proj, t):
            rs, als = proj.composite_layers(t["colors"], Ns, backgrounds=bg9, want_all=True)
            held["out"] = list(zip(rs, als))
            return loss_of([rs[li], als[li]], [ref[2], ref[3]])

        got, _, _ = run(layers)
        tag = ("all", "static", "dynamic")[li]
        img, a = held["out"][li]
        _close_pixels(img, a, ref[0]["render"], ref[0]["alphas"].unsqueeze(-1), cmax, spread, 10, f"layers {tag}")
        check_grads(got, [(rows, ref[0])], f"layers {tag}")

    # (c) coverage of each class (D = 1, FILTER = true): static over a background, dynamic without
    for sel, rows, use_bg in ((1, st, True), (2, dy, False)):
        r_c = _subset_reference(scene, rows, "alpha", use_bg)

        def cover(proj, t):
            out = proj.class_alpha(Ns, sel, None if r_c[1] is None else r_c[1].to(hip_device))
            held["out"] = out
            return loss_of([out], [r_c[2] if use_bg else r_c[3]])

        got, log, lens = run(cover)
        _check_path(log, 1, True, "quadrant", bwd, heavy, lens, scene)
        ref = r_c[0]
        if use_bg:
            close_image_with_blend_flips(held["out"].detach().cpu().reshape(ref["render"].shape), ref["render"],
                                         ref["alphas"].unsqueeze(-1), 1.0, 0.0, 2e-5, f"coverage {sel} over bg",
                                         flip_frac=2e-4)
        else:
            _close(held["out"].detach().cpu().reshape(ref["alphas"].shape), ref["alphas"], 0, 2e-5,
                   f"coverage {sel}", flip_frac=2e-4, flip_atol=2.0 * 1.001 / 255)
        for k in ("means", "quats", "scales", "opacities", "viewmats"):
            _close_grad(got[k], _merged([(rows, ref)], k, N), f"coverage {sel} grad[{k}]", camera=k == "viewmats")


_vis_cache = {}


def _reference_vis(scene):
    """Depths of the splats the oracle projects visibly (the depth channel's range)."""
    if scene not in _vis_cache:
        from oracle import gsplat_cpu as Cc
        s = _scene(scene, 9)
        sp = SCENES[scene]
        radii, _, depths, _ = Cc.project_fwd(s["means"].numpy(), s["quats"].numpy(), s["scales"].numpy(),
                                              s["viewmats"].numpy(), s["Ks"].numpy(), sp["w"], sp["h"])
        _vis_cache[scene] = torch.from_numpy(depths[radii > 0])
    return _vis_cache[scene]


def test_layers_of_other_widths_are_refused(hip_device):
    """composite_layers is built for 9 colours + depth: other widths raise NotImplementedError (class or layered path
    alike), they are never composited with the wrong record stride."""
    from mobgs_amd.rendering import SharedProjection
    s = _scene("S", 9)
    sp = SCENES["S"]
    d = {k: v.to(hip_device) for k, v in s.items()}
    proj = SharedProjection(d["means"], d["quats"], d["scales"], d["opacities"], d["viewmats"], d["Ks"], sp["w"], sp["h"])
    Ns = _ns("S", "odd")
    for width in (3, 8, 10, 12):
        cols = torch.randn(sp["n"], width, device=hip_device)
        for want_all in (False, True):
            with pytest.raises(NotImplementedError):
                proj.composite_layers(cols, Ns, want_all=want_all)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 3. coverage guard
# ---------------------------------------------------------------------------------------------------------------------
def _reachable():
    """Every (D, class_filter, fwd_kernel, bwd_kernel, heavy mode) mobgs_raster_path() selects for the builds, the tuning
    values the table uses and grids on both sides of the threshold."""
    from mobgs_amd import _lib, rendering
    lib = _lib.load()
    out = set()
    for D, cf in [(d, 0) for d in rendering._SUPPORTED] + [(1, 1), (10, 1)]:
        for bw, bb, m, hv, nt in itertools.product((-1, 0, 1), (-1, 0, 1), (-1, 0, 1, 2), (-1, 0, HEAVY_SMALL),
                                                   (117, 1056)):
            t = _lib.MobgsTuning(heavy_tile_len=hv, block_walk=bw, bwd_block_walk=bb, bwd_mfma=m)
            bits = int(lib.mobgs_raster_path(D, cf, nt, t.ref()))
            out.add((D, cf, "blocks" if bits & 4 else "quadrant", rendering._BWD_NAMES[bits & 3], _heavy_mode(bits >> 8)))
    return out


def _covered():
    from mobgs_amd import rendering
    rows = {(rendering._pad_channels(_total(ch, mode)), 0, f, b, hm) for _, ch, mode, _, f, b, hm in ROWS}
    for _, _, _, f, b, hm in CLASS_ROWS:
        rows.add((10, 1, f, b, hm))
        rows.add((1, 1, "quadrant", b, hm))
    return rows


def test_every_reachable_build_has_an_oracle_row():
    reach, covered = _reachable(), _covered()
    missing = sorted(reach - covered)
    assert not missing, f"{len(missing)} reachable compositor builds / arms without an oracle row: {missing}"
    stale = sorted(covered - reach)
    assert not stale, f"rows expecting selections mobgs_raster_path never makes: {stale}"
