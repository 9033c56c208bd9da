"""Deterministic cases for the Farneback kernels (csrc/tof.hip, include/mobgs_hip.h K25): level shapes and contents for the
stage tests, kink-safe seeds for the end-to-end tests, the strata of every stage output, the per-element bounds and the
comparator of tests/test_gpu_tof_kernels.py.  numpy and tests/tof_restatement.py only: nothing of the package under test is
imported here; tests/test_tof_cases_cpu.py checks from the references alone that every case reaches the edge it is named
after, that the fp32 twin of the restatement stays inside the bounds, and that the comparator rejects planted errors.

Stage cases.  A level image of one of LEVEL_HW's shapes holding one of CONTENTS, two frames (the second is the first moved by
(1.3, -0.7) level pixels).  48x48, 49x65 and 32x33 are the COARSEST level of a 48x48, 98x130 and 256x264 image (3, 3 and 19
taps), so the pyramid kernel runs on them too; 7x13 and 2x2 are the content itself (of a finer texture, `SMALL`) and go through
the stage entry points only.  Each stage is fed the restatement's own float64 input rounded to fp32.

Bounds (nothing here comes from a run of the code under test).  Element i of a stage output may be off
by  k * C[stage] * 2^-23 * T_i,  T_i its sum of absolute terms in float64:
  * pyramid, polyexp, upsample (linear): the stage on |taps| and |input|; for the expansion the closed form the normal
    equations have (`polyexp_closed_form`), r_xx: |ig03| sum g g |x| + |ig33| sum k^2 g g |x|;
  * update: tof_restatement.update_terms, first-order propagation of the same sums through the products; for the fp32 twin
    it includes the rounding of the sample position x + u, which plain fp32 (and OpenCV) incurs; the kernel splits u
    exactly and is compared without that term (`T_exact`);
  * solve: |result| (its rounding to fp32) + 2^-24 sum_j |d result / d q_j| Q_j, Q_j the box mean of |M_j|: the box means
    q_j are float64 sums of 225 + 30 terms on both sides, off by at most 2^6 2^-53 Q_j each (`solve_terms`).
C[stage] >= 1 is the smallest factor with which the fp32 twin of the restatement (the same numpy statements in float32)
stays within k <= 1 on every case and stratum, measured by tests/test_tof_cases_cpu.py and recorded below; the kernels are
allowed k = K = 3, their summation order differing from numpy's.  T_i carries the floor 16 x 2^-126 for gradual underflow
(the squares of the 1e-14 coefficients a flat region has): T_i = 0 asks for the float64 value to within 48 c of the smallest
denormal, and the exact zeros are asserted bit for bit beside the comparator.  No share of the elements is left out and no
pixel is excused."""
import functools
from types import SimpleNamespace

import numpy as np

import tof_restatement as TR

K = 3
EPS = 2.0 ** -23
FLOOR = 16 * 2.0 ** -126   # gradual underflow: each of a stage's fp32 operations may also be off by 2^-149 = 2^-23 2^-126
TILE = 16
STAGES = ("pyramid", "polyexp", "upsample", "update", "solve")
# measured: tests/test_tof_cases_cpu.py::test_fp32_twin_stays_within_the_bounds (docs/MEASUREMENT_LOG.md)
C = {"pyramid": 1.9, "polyexp": 5.1, "upsample": 3.9, "update": 1.4, "solve": 1.0}
# band width of a stage's border stratum in level pixels (the pyramid's is its Gaussian radius, `pyramid_band`)
BAND = {"polyexp": TR.POLY_N, "upsample": 1, "update": len(TR.BORDER), "solve": TR.WINSIZE // 2}
CONTENTS = ("smooth", "low_contrast", "saturated", "const_half")
LEVEL_HW = {"48x48": (48, 48), "49x65": (49, 65), "32x33": (32, 33), "7x13": (7, 13), "2x2": (2, 2)}
IMAGE_HW = {"48x48": (48, 48), "49x65": (98, 130), "32x33": (256, 264), "7x13": None, "2x2": None}
SHAPES = tuple(LEVEL_HW)
STRATA = ("band", "corners", "seams", "tail", "const", "const_edge", "interior")
SHIFT = (1.3, -0.7)
# 7x13 and 2x2: TR.texture (periods of 8 to 64 px) barely varies over so few pixels, so their content is the texture of a level
# STRIDE times as large, every STRIDE-th pixel (periods of 1.3 to 11 level pixels); (stride, seed) chosen on the CPU so that
# every content is what it is named (tests/test_tof_cases_cpu.py::test_contents_are_what_they_are_named)
SMALL = {"7x13": (6, 3), "2x2": (6, 54)}

# name -> (H, W, frames, seed) of TR.moving_frames.  OLD_END_TO_END are the cases of tests/test_gpu_tof.py (seed = H): none
# of them keeps the margin that tests/test_tof_cases_cpu.py::test_kink_margins asks for (docs/MEASUREMENT_LOG.md), so each
# has a twin here with a seed searched on the CPU, next to the three new shapes (the four-level shapes with one pair: the
# margin is a minimum over every border pixel of every update, and a second pair halves the share of seeds that keep it).
# A comparison of tOF scores a case's flows against their negatives, so that every flow in it is one of a vetted trace.
OLD_END_TO_END = {"75x50 (old)": (50, 75, 3, 50), "136x72 (old)": (72, 136, 3, 72), "262x259 (old)": (259, 262, 3, 259)}
END_TO_END = {
    "48x48": (48, 48, 3, 83),
    "64x64": (64, 64, 3, 42),
    "256x256": (256, 256, 2, 3099),
    "75x50": (50, 75, 3, 137),
    "136x72": (72, 136, 3, 112),
    "262x259": (259, 262, 2, 1235),
}
MARGIN_RATIO = 100.0   # kink margin / the fp32 twin's own flow error, as tests/flow_cases.py


# ---- contents ------------------------------------------------------------------------------------------------------------
def content(kind, H, W, seed, shift=(0.0, 0.0), stride=1):
    """[H,W] float64 holding 8-bit values, all derived from TR.texture(H, W, seed, shift), or from every `stride`-th pixel of
    the texture `stride` times as large (the shift stays in pixels of the result)."""
    base = TR.texture(H * stride, W * stride, seed, (shift[0] * stride, shift[1] * stride))[::stride, ::stride]
    if kind == "smooth":
        return base
    if kind == "low_contrast":        # amplitude 2 grey levels around 128: the 8-bit steps dominate
        return np.rint(128.0 + (base - 127.5) * 0.02)
    if kind == "saturated":           # gain 4 around mid-grey: about a third of the pixels end at 0 or 255
        return (128.0 + (base - 128.0) * 4.0).clip(0, 255)
    if kind == "const_half":          # the left half is flat; the right half moves
        out = base.copy()
        out[:, :W // 2] = 128.0
        return out
    raise KeyError(kind)


def saturated_share(img):
    return float(((img == 0) | (img == 255)).mean())


# ---- sums of absolute terms ------------------------------------------------------------------------------------------------
def polyexp_closed_form(img, absolute=False):
    """[h,w] -> [5,h,w]: the solution the normal equations of TR.poly_exp have for the separable even weight g(x) g(y) --
    r_x = ig11 <x g g, p>, r_xx = ig03 <g g, p> + ig33 <x^2 g g, p>, r_xy = ig55 <xy g g, p> -- or, `absolute`, the same with
    every term in absolute value."""
    n = TR.POLY_N
    t = np.arange(-n, n + 1, dtype=np.float64)
    g = np.exp(-t * t / (2.0 * TR.POLY_SIGMA * TR.POLY_SIGMA))
    g /= g.sum()
    m2, m4 = (g * t * t).sum(), (g * t ** 4).sum()
    ig11, ig33, ig03, ig55 = 1.0 / m2, 1.0 / (m4 - m2 * m2), -m2 / (m4 - m2 * m2), 1.0 / (m2 * m2)
    p = np.asarray(img, np.float64)
    g1, g2 = g * t, g * t * t
    if absolute:
        p, g1, ig03 = np.abs(p), np.abs(g1), abs(ig03)

    def sep(ty, tx):
        return TR.correlate_axis(TR.correlate_axis(p, tx, 1, "edge"), ty, 0, "edge")

    s00 = sep(g, g)
    return np.stack([ig11 * sep(g, g1), ig11 * sep(g1, g), ig03 * s00 + ig33 * sep(g, g2), ig03 * s00 + ig33 * sep(g2, g),
                     ig55 * sep(g1, g1)])


def solve_terms(M):
    """M [5,h,w] (fp32 values) -> T [h,w,2] of TR.blur_solve (module docstring)."""
    box = np.full(TR.WINSIZE, 1.0 / TR.WINSIZE)

    def mean(m):
        return TR.correlate_axis(TR.correlate_axis(m, box, 1, "edge"), box, 0, "edge")

    M = np.asarray(M, np.float64)
    q0, q1, q2, q3, q4 = (mean(m) for m in M)
    Q0, Q1, Q2, Q3, Q4 = (mean(np.abs(m)) for m in M)
    det = q0 * q2 - q1 * q1 + 1e-3
    ru, rv = (q2 * q3 - q1 * q4) / det, (q0 * q4 - q1 * q3) / det
    du = (np.abs(ru * q2) * Q0 + np.abs(2 * ru * q1 - q4) * Q1 + np.abs(q3 - ru * q0) * Q2 + np.abs(q2) * Q3
          + np.abs(q1) * Q4) / np.abs(det)
    dv = (np.abs(q4 - rv * q2) * Q0 + np.abs(2 * rv * q1 - q3) * Q1 + np.abs(rv * q0) * Q2 + np.abs(q1) * Q3
          + np.abs(q0) * Q4) / np.abs(det)
    return np.stack([np.abs(ru) + 2.0 ** -24 * du, np.abs(rv) + 2.0 ** -24 * dv], -1)


# ---- stage cases -----------------------------------------------------------------------------------------------------------
def pyramid_band(level, W):
    """The Gaussian radius (and the resize's one more tap) in level pixels."""
    return int(np.ceil((level[2] // 2 + 1) * level[0] / W))


def own_flow(h, w, seed):
    """[1,h,w,2] fp32: a smooth flow of the level's own size, some samples leaving the image."""
    return TR.smooth_flow(h, w, seed=seed, amplitude=max(0.1 * min(h, w), 1.5))[None]


def coarse_flow(h, w, seed):
    """[1,sh,sw,2] fp32 of the size the next coarser level would have: upsampled and doubled it is a flow of about 2 px."""
    sh, sw = max(int(np.rint(h * 0.5)), 1), max(int(np.rint(w * 0.5)), 1)
    return TR.smooth_flow(sh, sw, seed=seed + 1, amplitude=1.0)[None]


def planes(a):
    """A flow [..., h, w, 2] with its pixel plane last."""
    return np.moveaxis(a, -1, -3)


@functools.lru_cache(maxsize=None)
def stage_case(shape, kind):
    """-> namespace(shape, kind, h, w, image (H, W) or None, level, grey [2,H,W] or None, edge (const_half: the first level
    column that is not flat), stage {name: namespace(inp (fp32), ref (float64), twin (the fp32 restatement), T, band,
    reach; update also T_exact, without the position term)}).  Computed once and shared: leave it unchanged."""
    h, w = LEVEL_HW[shape]
    seed = 11 + SHAPES.index(shape)
    f32 = np.float32
    c = SimpleNamespace(shape=shape, kind=kind, h=h, w=w, image=IMAGE_HW[shape], level=None, grey=None, edge=None, stage={})

    def put(name, inp, ref, twin, T, band, reach):
        c.stage[name] = SimpleNamespace(inp=inp, ref=ref, twin=np.asarray(twin, np.float64), T=T, band=band, reach=reach)

    if c.image:
        H, W = c.image
        s = W / w
        c.grey = np.stack([content(kind, H, W, seed), content(kind, H, W, seed, (SHIFT[0] * s, SHIFT[1] * s))])
        c.level = TR.levels(H, W)[0]
        assert c.level[:2] == (w, h), (c.level, shape)
        img = np.stack([TR.pyramid_level(g, c.level) for g in c.grey])
        put("pyramid", c.grey.astype(f32), img, np.stack([TR.pyramid_level(g, c.level, f32) for g in c.grey]),
            np.abs(img), pyramid_band(c.level, W), 0)        # taps and grey values are not negative: T = |value|
    else:
        stride, seed = SMALL[shape]
        img = np.stack([content(kind, h, w, seed, stride=stride), content(kind, h, w, seed, SHIFT, stride)])
    img32 = img.astype(f32)
    if kind == "const_half":
        flat = np.all(img32 == f32(128.0), axis=(0, 1))
        c.edge = int(np.argmin(flat)) if not flat.all() else w
    R = np.stack([TR.poly_exp(a.astype(np.float64)) for a in img32])
    put("polyexp", img32, R, np.stack([TR.poly_exp(a, f32) for a in img32]),
        np.stack([polyexp_closed_form(a, absolute=True) for a in img32]), BAND["polyexp"], TR.POLY_N)
    R32 = R.astype(f32)
    R64 = R32.astype(np.float64)
    coarse = coarse_flow(h, w, 11 + SHAPES.index(shape))
    up = np.stack([TR.resize_bilinear(f.astype(np.float64), h, w) * 2.0 for f in coarse])
    put("upsample", coarse, up, np.stack([TR.resize_bilinear(f, h, w, f32) * f32(2.0) for f in coarse]),
        np.stack([TR.resize_bilinear(np.abs(f).astype(np.float64), h, w) * 2.0 for f in coarse]), BAND["upsample"], None)
    flow = own_flow(h, w, 11 + SHAPES.index(shape))
    M = TR.update_matrices(R64[0], R64[1], flow[0])[None]
    far = TR.POLY_N + int(np.ceil(np.abs(flow).max())) + 1
    put("update", (R32, flow), M, TR.update_matrices(R32[0], R32[1], flow[0], f32)[None],
        TR.update_terms(R64[0], R64[1], flow[0])[None], BAND["update"], far)
    c.stage["update"].T_exact = TR.update_terms(R64[0], R64[1], flow[0], position=False)[None]
    M32 = M.astype(f32)
    put("solve", (M32, R32), TR.blur_solve(M32[0].astype(np.float64))[None], TR.blur_solve(M32[0], f32)[None],
        solve_terms(M32[0])[None], BAND["solve"], far + TR.WINSIZE // 2)
    return c


def stage_cases(stage=None):
    """Every (shape, content); the pyramid only where the level is one of an image."""
    return [(s, k) for s in SHAPES for k in CONTENTS if stage != "pyramid" or IMAGE_HW[s]]


# ---- strata ----------------------------------------------------------------------------------------------------------------
def strata(h, w, band, edge=None, reach=None):
    """{stratum: bool [h,w]}.  band: within `band` pixels of a side; corners: of two sides; seams: the rows and columns on
    either side of a tile boundary (15 / 16, 31 / 32, ...); tail: the partial tile of either axis; const (const_half only,
    `reach` given): columns whose windows stay inside the flat half; const_edge: columns within `reach` of its end;
    interior: none of these.  The tags overlap; every pixel carries at least one."""
    y, x = np.mgrid[0:h, 0:w]
    bx, by = (x < band) | (x >= w - band), (y < band) | (y >= h - band)

    def seam(i, n):
        return ((i % TILE == TILE - 1) & (i < n - 1)) | ((i % TILE == 0) & (i > 0))

    out = {"band": bx | by, "corners": bx & by, "seams": seam(x, w) | seam(y, h),
           "tail": (x >= (w // TILE) * TILE) | (y >= (h // TILE) * TILE)}
    if edge is not None and reach is not None:
        out["const"] = x + reach < edge
        out["const_edge"] = (x + reach >= edge) & (x - reach <= edge)
    rest = np.ones((h, w), bool)
    for m in out.values():
        rest &= ~m
    out["interior"] = rest
    return out


def case_strata(c, stage):
    st = c.stage[stage]
    return strata(c.h, c.w, st.band, c.edge, st.reach)


def exact_zero_regions(c, flow):
    """const_half: {stage: bool [h,w]} where the KERNELS' outputs are exactly 0.  The expansion kernel fits a 16x16 tile from
    one 26x26 patch, relative to one value of that patch: where the whole patch is flat every entry is exactly 0, so the
    fact holds per tile, for the leading tiles whose patch ends left of `edge`.  From exactly zero coefficients the update
    matrices of `flow` [h,w,2] are exactly 0 wherever the sampled taps stay inside those tiles, and the solved flow wherever
    the box window does."""
    tiles = (c.edge - (TILE + TR.POLY_N)) // TILE + 1 if c.edge >= TILE + TR.POLY_N else 0
    x = np.mgrid[0:c.h, 0:c.w][1]
    sample = int(np.ceil(np.abs(flow).max())) + 1
    return {"polyexp": x < tiles * TILE, "update": x + sample < tiles * TILE,
            "solve": x + sample + TR.WINSIZE // 2 < tiles * TILE}


# ---- the comparator --------------------------------------------------------------------------------------------------------
def needed_k(got, ref, T, c, mask=None):
    """The largest |got - ref| / (c 2^-23 (T + FLOOR)) over the pixels `mask` of arrays [..., h, w]: 0 where got equals ref,
    nan for a nan; None over no pixel."""
    got, ref, T = (np.asarray(a, np.float64) for a in (got, ref, T))
    assert got.shape == ref.shape == T.shape, (got.shape, ref.shape, T.shape)
    if mask is not None:
        got, ref, T = got[..., mask], ref[..., mask], T[..., mask]
    if got.size == 0:
        return None
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(err == 0, 0.0, err / (c * EPS * (T + FLOOR)))
    return float("nan") if np.isnan(k).any() else float(k.max())


def rel_to_max(got, ref):
    """The rule of tests/test_gpu_tof.py: the largest error relative to the array's largest magnitude."""
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


def compare(c, stage, got, what, limit=K, sink=None, ref=None, T=None):
    """One stage output against float64 under the module's rule, stratum by stratum.  Every comparison prints a RATIO line;
    failures are gathered and raised once.  `sink`, a list, collects (stage, shape, content, stratum, k).  Flows are given
    as [P,h,w,2].  `ref`, `T`: the float64 result and its terms for another input than the case's own (the update matrices
    of the flow a kernel upsampled)."""
    st = c.stage[stage]
    factor = C[stage]
    flow = stage in ("upsample", "solve")
    g, ref, T = (planes(a) if flow else a for a in (np.asarray(got, np.float64), st.ref if ref is None else ref,
                                                    st.T if T is None else T))
    assert g.shape == ref.shape, f"{what}: shape {g.shape} != {ref.shape}"
    failures, out = [], []
    for name, mask in case_strata(c, stage).items():
        k = needed_k(g, ref, T, factor, mask)
        if k is None:
            continue
        print(f"[tof] RATIO {what} {stage} {c.shape} {c.kind} [{name}]: k = {k:.3f} (allowed {limit}, c = {factor:g}, "
              f"{int(mask.sum())} px)")
        out.append((stage, c.shape, c.kind, name, k))
        if not k <= limit:
            failures.append(f"{what} {stage} {c.shape} {c.kind} [{name}]: k = {k:.3f} > {limit}")
    if sink is not None:
        sink.extend(out)
    assert not failures, "\n".join(failures)
    return out


# ---- end to end ------------------------------------------------------------------------------------------------------------
def kink_distance(flow):
    """Smallest distance (px) of a sample position x + u, y + v from x = 0, x = w - 1, y = 0, y = h - 1, where the in-bounds
    test 0 <= floor(.) < size - 1 jumps."""
    h, w = flow.shape[:2]
    fx, fy = TR.sample_positions(np.asarray(flow, np.float64))
    return float(min(np.abs(fx).min(), np.abs(fx - (w - 1)).min(), np.abs(fy).min(), np.abs(fy - (h - 1)).min()))


@functools.lru_cache(maxsize=None)
def frames(name):
    """(rgb [F,3,H,W] fp32, grey [F,H,W] float64) of an end-to-end case."""
    H, W, F, seed = {**OLD_END_TO_END, **END_TO_END}[name]
    rgb = TR.moving_frames(F, H, W, seed)
    return rgb, TR.grey(rgb)


@functools.lru_cache(maxsize=None)
def flow_trace(name, dtype=np.float64):
    """-> (flows [F-1,H,W,2], updates: per pair the flows its update steps sample with, the zero flow of the coarsest level
    left out).  Computed once and shared: leave it unchanged."""
    grey = frames(name)[1]
    flows, updates = [], []
    for p in range(len(grey) - 1):
        ups = []
        flows.append(TR.farneback(grey[p], grey[p + 1], dtype, ups))
        updates.append(ups)
    return np.stack(flows), updates


def kink_margin(name):
    """(smallest kink distance over every update of every level and pair of the float64 trace, the fp32 twin's largest
    distance from float64 over the same flows and the final ones), both in px."""
    f64, u64 = flow_trace(name)
    f32, u32 = flow_trace(name, np.float32)
    margin = min(kink_distance(f) for ups in u64 for f in ups)
    err = max([float(np.abs(f32.astype(np.float64) - f64).max())]
              + [float(np.abs(a.astype(np.float64) - b).max()) for x, y in zip(u32, u64) for a, b in zip(x, y)])
    return margin, err
