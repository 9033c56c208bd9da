"""Constructed screen-space cases for the compositors (mobgs_amd/csrc/raster.hip, raster_bwd_mfma.hip, raster_layers.hip),
their dense float64 / fp32 references and the comparator of tests/test_gpu_raster_kernels.py.  Torch and numpy on the CPU
only: nothing of the package under test is imported here; tests/test_raster_cases_cpu.py shows from the reference alone
that every case reaches the edge it is named after.

Inputs are given directly in screen space: means2d [C,N,2], conics [C,N,3], colours, opacities, depths, integer radii
[C,N] and backgrounds -- no projection.  The reference (dense_eval) is upstream compositing restated WITHOUT tile lists: per
pixel it walks all splats of the camera by increasing depth with sigma, alpha = min(0.999, op exp(-sigma)) and the tests
sigma >= 0, alpha >= 1/255, T <= 1e-4 of oracle/gsplat_torch.py::rasterize_to_pixels; gradients come from autograd.  That
is legitimate because the radii are inputs: every case but `boxcut` sets radius = ceil(3.4 x the larger standard
deviation), beyond sqrt(2 ln 255) = 3.33 deviations, so every pair with alpha >= 1/255 lies inside the splat's tile
rectangle (isect_cases.tile_rects) and the result depends on neither the lists nor tile culling.  `boxcut` uses 3 deviations
at opacity 0.9 (alpha at the box edge about 0.01): there the reference restricts each splat to its tile rectangle.

Near-kink filter (as deform_cases._keep_first / splat_cases.proj_near_kink).  Candidates are drawn in excess, per group of
a case; the float64 walk looks at the chosen ones and a splat is BAD when at any pixel where it is still evaluated (inside
its tile rectangle and not behind the pixel's stop) 255 raw or raw / 0.999 lies within relative M_A of 1, or the
inclusive transmittance T (1 - alpha) of a passing pair lies within relative M_T of 1e-4.  Bad candidates are banned, the
first wanted number of every group is chosen again (dropping changes T behind the splat) and so on until no chosen pair is
near a kink; fp32 and float64 then take the same branch at every pair and no comparison needs a flip allowance.  A case
that bans more than 10 % of its candidates raises.  tests/test_raster_cases_cpu.py checks that each margin is at least
16 x the fp32 reference's own relative error of the quantity it guards.

Depths are distinct fp32 values, conics positive definite: ties and list order belong to tests/isect_cases.py."""
import functools
import math
import zlib
from types import SimpleNamespace

import numpy as np
import torch

import isect_cases
from deform_cases import close_to_f64, needed_k  # noqa: F401  (the comparator: imported, not copied)

TILE = 16
# (the clamp is the fp32 constant 0.999f of upstream and of the kernels: 1 - 0.999f differs from 1 - 0.999 by 1.3e-5 of itself)
ALPHA_MIN, ALPHA_MAX, T_STOP = 1.0 / 255.0, float(np.float32(0.999)), 1e-4
M_A, M_T = 1e-4, 2e-4      # relative distance every evaluated pair keeps from the alpha kinks / the stop
# `centre` blends alpha = 0.9985: T = 1 - alpha = 1.5e-3 carries 2^-24 / 1.5e-3 = 4e-5 of relative error in ANY fp32
# evaluation, and the fp32 reference measures 1.3e-5 -- 16 x that is above 2e-4, so this case keeps twice the distance
M_T_OF = {"centre": 4e-4}
RAW_FLOOR = 1e-3           # pairs with raw below this are a factor 3.9 under the lowest kink (1/255): see margins()
MARGIN_FACTOR = 16         # ... each at least this many times the fp32 reference's own error
MAX_DROP = 0.10
K_RADIUS, K_BOXCUT = 3.4, 3.0
MAX_CH = 26
DEPTH_STEP = 1.0 / 4096.0  # depths lo + k / 4096 with lo <= 8: exact and distinct in fp32

CASES = ("len0_1", "seam63", "seam64", "seam65", "seam128", "seam129", "stop_mid", "quadrant", "span", "centre", "narrow",
         "two_cams", "boxcut", "heavy", "classes")
SEAM_TILE = {"seam63": (0, 0), "seam64": (2, 0), "seam65": (1, 1), "seam128": (0, 2), "seam129": (2, 2)}
HEAVY_TILE, HEAVY_LEN, HEAVY_REST_MAX = (1, 1), 300, 40
CLASS_NS = 64


# ---- drawing candidates ------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _draw(g, n, box, sig, op, depth0, rho=0.6, k_radius=K_RADIUS):
    """n candidates (float64): means uniform in box (x0, y0, x1, y1), standard deviations uniform in sig, correlation in
    +-rho, opacities uniform in op, depths depth0 + (a permutation of 0 .. n-1) / 4096."""
    u = torch.rand(n, 6, generator=g, dtype=torch.float64)
    x0, y0, x1, y1 = box
    mean = torch.stack([x0 + (x1 - x0) * u[:, 0], y0 + (y1 - y0) * u[:, 1]], 1)
    sx, sy = sig[0] + (sig[1] - sig[0]) * u[:, 2], sig[0] + (sig[1] - sig[0]) * u[:, 3]
    r = rho * (2.0 * u[:, 4] - 1.0)
    depth = depth0 + torch.randperm(n, generator=g).double() * DEPTH_STEP
    return _splats(mean, sx, sy, r, op[0] + (op[1] - op[0]) * u[:, 5], depth, k_radius)


def _splats(mean, sx, sy, rho, op, depth, k_radius=K_RADIUS):
    """Conic = the inverse of the covariance [[sx^2, rho sx sy], [rho sx sy, sy^2]]; radius = ceil(k x the larger standard
    deviation) (the root of the covariance's larger eigenvalue)."""
    mean, sx, sy, rho, op, depth = (torch.as_tensor(v, dtype=torch.float64) for v in (mean, sx, sy, rho, op, depth))
    one = 1.0 - rho * rho
    conic = torch.stack([1.0 / (sx * sx * one), -rho / (sx * sy * one), 1.0 / (sy * sy * one)], 1)
    mid, dif = 0.5 * (sx * sx + sy * sy), 0.5 * (sx * sx - sy * sy)
    smax = torch.sqrt(mid + torch.sqrt(dif * dif + (rho * sx * sy) ** 2))
    return dict(mean=mean, conic=conic, op=op, depth=depth, radius=torch.ceil(k_radius * smax).long())


def _take(part, keep):
    return {k: v[keep] for k, v in part.items()}


def _rect_of(part, W, H):
    """isect_cases.tile_rects of the candidates (means and radii rounded to what the device gets)."""
    return isect_cases.tile_rects(part["mean"].float().numpy(), part["radius"].numpy(), -(-W // TILE), -(-H // TILE))


def _avoiding(part, tiles, W, H):
    """The candidates whose tile rectangle touches none of `tiles` [(tx, ty)] (construction, not the near-kink filter)."""
    x0, y0, x1, y1 = _rect_of(part, W, H)
    hit = np.zeros(len(x0), bool)
    for tx, ty in tiles:
        hit |= (x0 <= tx) & (tx < x1) & (y0 <= ty) & (ty < y1)
    return _take(part, torch.from_numpy(~hit))


def _tile_box(tx, ty, W, H, margin):
    """The part of tile (tx, ty) inside the image, shrunk by `margin` (a pair of numbers: per axis) on every side."""
    mx, my = margin if isinstance(margin, tuple) else (margin, margin)
    x1, y1 = min(16 * tx + 16, W), min(16 * ty + 16, H)
    bx, by = min(mx, 0.5 * (x1 - 16 * tx) - 0.25), min(my, 0.5 * (y1 - 16 * ty) - 0.25)
    return 16 * tx + bx, 16 * ty + by, x1 - bx, y1 - by


def _fillers(g, per_tile, tiles, avoid, W, H, depth0, op=(0.05, 0.6)):
    """per_tile short-list splats in each of `tiles` (one group per tile), none touching a tile of `avoid`; a tile in which
    too few candidates manage that gets none."""
    parts = []
    for i, (tx, ty) in enumerate(tiles):
        p = _avoiding(_draw(g, 10 * per_tile + 20, _tile_box(tx, ty, W, H, 3.0), (0.6, 0.9), op, depth0 + 0.05 * i,
                            rho=0.3), avoid, W, H)
        if len(p["op"]) < per_tile + 2:
            continue  # (a 4-pixel-high tile below an avoided one: every splat centred in it reaches up)
        parts.append(_take(p, slice(0, per_tile + 2)))
    return parts, [per_tile] * len(parts)


# ---- the dense walk ----------------------------------------------------------------------------------------------------
def _pixels(W, H, dtype):
    py, px = torch.meshgrid(torch.arange(H, dtype=dtype) + 0.5, torch.arange(W, dtype=dtype) + 0.5, indexing="ij")
    return px.reshape(-1), py.reshape(-1)


def _pairs(m, con, op, px, py):
    """sigma, raw = op exp(-sigma) and alpha of every (pixel, splat) pair, [P, n]: oracle/gsplat_torch.py's statements."""
    dx = m[None, :, 0] - px[:, None]
    dy = m[None, :, 1] - py[:, None]
    sigma = 0.5 * (con[None, :, 0] * dx * dx + con[None, :, 2] * dy * dy) + con[None, :, 1] * dx * dy
    raw = op[None, :] * torch.exp(-sigma)
    return sigma, raw, torch.clamp(raw, max=ALPHA_MAX)


def _decide(sigma, alpha, inside):
    """-> valid, T_incl (over the valid pairs), done (pairs behind the pixel's stop, the stopping pair included), contrib."""
    valid = (sigma >= 0) & (alpha >= ALPHA_MIN)
    if inside is not None:
        valid = valid & inside
    a_eff = torch.where(valid, alpha, torch.zeros_like(alpha))
    T_incl = torch.cumprod(1 - a_eff, dim=1)
    stop = valid & (T_incl <= T_STOP)
    done = torch.cummax(stop.to(torch.int8), dim=1).values.bool() if stop.shape[1] else stop
    return valid, T_incl, done, valid & ~done


def _in_rect(means, radii, W, H):
    """[P, n] bool: the pixel lies in a tile of the splat's tile rectangle (isect_cases.tile_rects; fp32 as the device)."""
    x0, y0, x1, y1 = (torch.from_numpy(v) for v in isect_cases.tile_rects(
        means.float().numpy(), radii.numpy(), -(-W // TILE), -(-H // TILE)))
    py, px = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    tx, ty = (px.reshape(-1) // TILE)[:, None], (py.reshape(-1) // TILE)[:, None]
    return (x0[None] <= tx) & (tx < x1[None]) & (y0[None] <= ty) & (ty < y1[None])


def _order(depths, radii, rows):
    """Rows (of `rows`, all) with radius > 0 by increasing fp32 depth."""
    idx = torch.arange(radii.shape[0]) if rows is None else torch.arange(radii.shape[0])[rows]
    idx = idx[radii[idx] > 0]
    return idx[torch.argsort(depths[idx].float(), stable=True)]


def walk(arr, W, H, dtype, boxcut=False, rows=None):
    """The forward decisions per camera, no gradients: list of namespaces(idx [n] rows by depth, sigma, raw, valid, T_incl,
    contrib, evaluated, inside -- all [P, n]).  evaluated: inside the tile rectangle and not after the pixel's stop (the
    stopping pair itself is evaluated)."""
    px, py = _pixels(W, H, dtype)
    out = []
    with torch.no_grad():
        for c in range(arr["means2d"].shape[0]):
            idx = _order(arr["depths"][c], arr["radii"][c], rows)
            op = arr["opacities"][c] if arr["opacities"].dim() == 2 else arr["opacities"]
            sigma, raw, alpha = _pairs(arr["means2d"][c, idx].to(dtype), arr["conics"][c, idx].to(dtype), op[idx].to(dtype),
                                       px, py)
            inside = _in_rect(arr["means2d"][c, idx], arr["radii"][c, idx], W, H)
            valid, T_incl, done, contrib = _decide(sigma, alpha, inside if boxcut else None)
            before = torch.cat([torch.zeros_like(done[:, :1]), done[:, :-1]], dim=1)
            out.append(SimpleNamespace(idx=idx, sigma=sigma, raw=raw, valid=valid, T_incl=T_incl, contrib=contrib,
                                       evaluated=inside & ~before, inside=inside))
    return out


def near_kink(arr, W, H, boxcut=False, m_t=M_T):
    """-> bool [N]: the splat has an evaluated pair near a kink in some camera (float64)."""
    bad = torch.zeros(arr["radii"].shape[1], dtype=torch.bool)
    for w in walk(arr, W, H, torch.float64, boxcut):
        pair = ((255.0 * w.raw - 1.0).abs() < M_A) | ((w.raw / ALPHA_MAX - 1.0).abs() < M_A)
        pair |= w.valid & ((w.T_incl / T_STOP - 1.0).abs() < m_t)
        bad[w.idx[(pair & w.evaluated).any(dim=0)]] = True
    return bad


# ---- cases -------------------------------------------------------------------------------------------------------------
def _stack(parts):
    """Parts (one camera: dict of [M, ..]; or a list per camera) -> candidate arrays [C, M, ..] float64 + group ids [M]."""
    per_cam = parts if isinstance(parts[0], list) else [parts]
    cams = [{k: torch.cat([p[k] for p in cam]) for k in cam[0]} for cam in per_cam]
    group = torch.cat([torch.full((len(p["op"]),), i) for i, p in enumerate(per_cam[0])])
    return {k: torch.stack([cam[k] for cam in cams]) for k in cams[0]}, group


def _arrays(cand, keep, shared_op):
    """The device's inputs (fp32 / int32 CPU tensors) of the candidates `keep`."""
    arr = dict(means2d=cand["mean"][:, keep].float(), conics=cand["conic"][:, keep].float(),
               opacities=cand["op"][:, keep].float(), depths=cand["depth"][:, keep].float(),
               radii=cand["radius"][:, keep].int())
    if shared_op:
        arr["opacities"] = arr["opacities"][0]
    return arr


def _select(name, cand, group, want, W, H, boxcut=False, shared_op=True, post=None):
    """The first want[g] candidates of every group g that are not banned, banning near-kink ones until none is chosen.
    post(arr): a last edit of the chosen arrays (depth ranks), checked again.  -> arrays, share of candidates banned."""
    M = group.numel()
    banned = torch.zeros(M, dtype=torch.bool)
    for _ in range(32):
        keep = []
        for gi, n in enumerate(want):
            free = torch.nonzero((group == gi) & ~banned).reshape(-1)
            if free.numel() < n:
                raise ValueError(f"raster case {name}: group {gi} has {free.numel()} usable candidates for {n} rows")
            keep.append(free[:n])
        keep = torch.cat(keep)
        arr = _arrays(cand, keep, shared_op)
        if post is not None:
            post(arr)
        bad = near_kink(arr, W, H, boxcut, M_T_OF.get(name, M_T))
        if not bad.any():
            dropped = float(banned.double().mean())
            if dropped > MAX_DROP:
                raise ValueError(f"raster case {name}: the near-kink filter drops {dropped:.1%} of the candidates "
                                 f"(cap {MAX_DROP:.0%})")
            return arr, dropped, M
        banned[keep[bad]] = True
    raise ValueError(f"raster case {name}: the near-kink filter did not settle")


def _surplus(n):
    return n + max(2, math.ceil(0.08 * n))


def _all_tiles(W, H):
    return [(tx, ty) for ty in range(-(-H // TILE)) for tx in range(-(-W // TILE))]


def _build(name):
    g = _gen("raster case", name)
    W, H, C = 40, 36, 1
    extra = {}
    boxcut, shared_op, post = False, True, None
    if name == "len0_1":
        keep_out = [(0, 0), (1, 0)]
        one = _avoiding(_draw(g, 12, _tile_box(1, 0, W, H, 6.2), (1.0, 1.7), (0.3, 0.8), 1.0), [(0, 0)], W, H)
        parts, want = _fillers(g, 4, [t for t in _all_tiles(W, H) if t not in keep_out], keep_out, W, H, 2.0)
        parts, want = [_take(one, slice(0, 3))] + parts, [1] + want
        extra = dict(empty_tile=(0, 0), single_tile=(1, 0))
    elif name in SEAM_TILE:
        n, t = int(name[4:]), SEAM_TILE[name]
        target = _draw(g, _surplus(n), _tile_box(*t, W, H, 0.8), (1.2, 2.2), (0.02, 0.05), 1.0)
        parts, want = _fillers(g, 4, [u for u in _all_tiles(W, H) if u != t], [t], W, H, 2.0)
        parts, want = [target] + parts, [n] + want
        extra = dict(target=t, length=n)
    elif name == "stop_mid":
        # front: opaque splats over quadrant 0 of tile (0, 0), then a crowd over the whole tile, then walls that end every
        # pixel of the image, then a tail nothing evaluates
        front = _draw(g, _surplus(20), (2.5, 2.5, 5.5, 5.5), (4.0, 5.0), (0.85, 0.99), 1.0, rho=0.2)
        crowd = _draw(g, _surplus(90), (0.5, 0.5, 15.5, 15.5), (1.5, 4.0), (0.5, 0.99), 2.0)
        walls = _draw(g, _surplus(12), (18.0, 16.0, 22.0, 20.0), (38.0, 42.0), (0.97, 0.99), 3.0, rho=0.2)
        tail = _draw(g, _surplus(30), (0.5, 0.5, 15.5, 15.5), (1.5, 4.0), (0.5, 0.99), 4.0)
        parts, want = [front, crowd, walls, tail], [20, 90, 12, 30]
        extra = dict(target=(0, 0), groups=want)
    elif name == "quadrant":
        parts, want = [], []
        for tx, ty in _all_tiles(W, H):
            for q in range(4):
                cx, cy = 16 * tx + 8 * (q & 1) + 4.0, 16 * ty + 8 * (q >> 1) + 4.0
                if cx + 4 > W or cy + 4 > H:
                    continue  # the quadrant lies (partly) outside the image
                parts.append(_draw(g, 4, (cx - 0.5, cy - 0.5, cx + 0.5, cy + 0.5), (0.7, 1.0), (0.3, 0.9),
                                   1.0 + 0.01 * len(parts), rho=0.3))
                want.append(2)
        extra = dict(small=2 * len(parts))
        parts.append(_draw(g, 3, (15.7, 15.7, 16.3, 16.3), (2.0, 3.0), (0.3, 0.9), 3.0))
        want.append(1)
    elif name == "span":
        everything = _draw(g, 3, (19.0, 17.0, 21.0, 19.0), (12.0, 14.0), (0.2, 0.5), 1.0, rho=0.2)
        top = _draw(g, 4, (23.0, 3.0, 25.0, 3.6), (3.0, 3.3), (0.2, 0.7), 1.2, rho=0.1)     # radius 11 / 12: 3 x 1 tiles
        left = _draw(g, 4, (0.6, 18.5, 0.9, 19.0), (4.0, 4.15), (0.2, 0.7), 1.4, rho=0.1)   # radius 14 / 15: 1 x 3 tiles
        long_x = _splats(torch.tensor([[20.0, 8.3], [19.0, 24.6], [21.0, 34.2]]), [8.0, 7.0, 8.0], [1.0, 1.2, 0.9],
                         [0.0, 0.1, -0.1], [0.6, 0.5, 0.7], [1.6, 1.6 + DEPTH_STEP, 1.6 + 2 * DEPTH_STEP])
        long_y = _splats(torch.tensor([[8.3, 18.0], [24.4, 17.0], [36.2, 19.0]]), [1.0, 1.2, 0.9], [8.0, 7.0, 8.0],
                         [0.0, -0.1, 0.1], [0.6, 0.5, 0.7], [1.7, 1.7 + DEPTH_STEP, 1.7 + 2 * DEPTH_STEP])
        crowd = _draw(g, _surplus(20), (0.5, 0.5, W - 0.5, H - 0.5), (1.0, 5.0), (0.1, 0.8), 2.0)
        unseen = _draw(g, 1, (10.0, 10.0, 30.0, 30.0), (2.0, 3.0), (0.5, 0.6), 3.0)
        unseen["radius"][:] = 0
        parts, want = [everything, top, left, long_x, long_y, crowd, unseen], [1, 2, 2, 3, 3, 20, 1]
        extra = dict(unseen_row=31)
    elif name == "centre":
        k = 14
        cells = torch.randperm(W * H, generator=g)[:k]
        mean = torch.stack([(cells % W).double() + 0.5, (cells // W).double() + 0.5], 1)
        u = torch.rand(k, 3, generator=g, dtype=torch.float64)
        op = torch.where(torch.arange(k) % 2 == 0, torch.tensor(0.9985, dtype=torch.float64),
                         torch.tensor(0.9995, dtype=torch.float64))
        parts = [_splats(mean, 1.5 + 1.5 * u[:, 0], 1.5 + 1.5 * u[:, 1], 0.5 * (2 * u[:, 2] - 1), op,
                         1.0 + torch.randperm(k, generator=g).double() * DEPTH_STEP)]
        want = [12]
    elif name == "narrow":
        W, H = 12, 40
        parts, want = [_draw(g, _surplus(40), (0.5, 0.5, W - 0.5, H - 0.5), (1.0, 4.0), (0.05, 0.9), 1.0)], [40]
    elif name == "two_cams":
        C, shared_op = 2, False
        n = _surplus(60)
        parts = [[_draw(g, n, (0.5, 0.5, W - 0.5, H - 0.5), (1.0, 5.0), (0.05, 0.9), 1.0 + c)] for c in range(C)]
        want = [60]
    elif name == "boxcut":
        boxcut = True
        p = _draw(g, 120, (0.5, 0.5, W - 0.5, H - 0.5), (1.5, 3.0), (0.9, 0.9), 1.0, rho=0.1, k_radius=K_BOXCUT)
        edges = torch.stack([p["mean"][:, a] + s * p["radius"] for a in (0, 1) for s in (-1.0, 1.0)], 1) / TILE
        ok = ((edges - edges.round()).abs() >= 1e-3).all(dim=1)  # tx +- tr, ty +- tr stay away from an integer
        p = _take(p, ok)
        # planted: 3 sigma = 8.97 -> radius 9 and a box edge 0.2 +- 0.05 pixels before a tile seam, so the first pixel column /
        # row past the seam lies 3.23 deviations out (alpha 0.0049 >= 1/255) and OUTSIDE the tile rectangle
        at = torch.tensor([[x, y] for x in (6.8, 22.8, 25.2) for y in (6.8, 22.8, 25.2)] * 2, dtype=torch.float64)
        at = at + 0.1 * torch.rand(18, 2, generator=g, dtype=torch.float64) - 0.05
        planted = _splats(at, [2.99] * 18, [2.99] * 18, [0.0] * 18, [0.9] * 18,
                          0.5 + torch.randperm(18, generator=g).double() * DEPTH_STEP, K_BOXCUT)
        parts, want = [planted, _take(p, slice(0, _surplus(30)))], [9, 30]
    elif name == "heavy":
        t = HEAVY_TILE
        target = _draw(g, _surplus(HEAVY_LEN), _tile_box(*t, W, H, 6.2), (1.0, 1.5), (0.01, 0.25), 1.0, rho=0.2)
        assert len(_avoiding(target, [u for u in _all_tiles(W, H) if u != t], W, H)["op"]) == len(target["op"])
        parts, want = _fillers(g, 16, [u for u in _all_tiles(W, H) if u != t], [t], W, H, 2.0)
        parts, want = [target] + parts, [HEAVY_LEN] + want
        extra = dict(target=t)
    elif name == "classes":
        # rows: static [only tile B x 32 | elsewhere x 32], dynamic [only tile A x 32 | tiles A and B x 32 | elsewhere x 2];
        # A = (0, 0): 64 dynamic entries, B = (1, 0): 32 static and 32 dynamic entries, alternating by depth
        A, B = (0, 0), (1, 0)
        thin, low = (1.2, 1.45), (0.03, 0.08)   # radius 5 / 6
        s_b = _avoiding(_draw(g, 60, (21.2, 5.2, 26.8, 10.8), thin, low, 1.0, rho=0.2), [A, (2, 0), (1, 1)], W, H)
        d_a = _avoiding(_draw(g, 60, (5.2, 5.2, 10.8, 10.8), thin, low, 1.0, rho=0.2), [B, (0, 1)], W, H)
        d_ab = _draw(g, 40, (15.0, 5.2, 17.0, 10.8), thin, low, 1.0, rho=0.2)
        row1 = (0.5, 21.5, W - 0.5, 30.5)
        s_rest = _avoiding(_draw(g, 80, row1, (1.0, 1.5), (0.05, 0.6), 3.0), [A, B, (2, 0)], W, H)
        d_rest = _avoiding(_draw(g, 12, row1, (1.0, 1.5), (0.05, 0.6), 4.0), [A, B, (2, 0)], W, H)
        parts = [_take(s_b, slice(0, 36)), _take(s_rest, slice(0, 36)), _take(d_a, slice(0, 36)), d_ab,
                 _take(d_rest, slice(0, 4))]
        want = [32, 32, 32, 32, 2]
        assert sum(want) == 130 and want[0] + want[1] == CLASS_NS

        def post(arr):   # tile B alternates: static k at rank 2 k, shared dynamic k at rank 2 k + 1; tile A's own first
            d = arr["depths"][0]
            d[0:32] = 2.0 + 2 * torch.arange(32) * DEPTH_STEP
            d[96:128] = 2.0 + (2 * torch.arange(32) + 1) * DEPTH_STEP
            d[64:96] = 1.0 + torch.arange(32) * DEPTH_STEP
        extra = dict(tile_a=A, tile_b=B, Ns=CLASS_NS)
    else:
        raise KeyError(name)
    cand, group = _stack(parts)
    arr, dropped, M = _select(name, cand, group, want, W, H, boxcut, shared_op, post)
    N = arr["radii"].shape[1]
    colors = torch.randn(*((C, N) if C > 1 else (N,)), MAX_CH, generator=g)
    Ns = extra.get("Ns", (N // 2) | 1)
    if name == "classes":
        colors[:Ns, 6:11] = 0.0  # the static rows' dead channels (csrc/raster_shared.h dead_channels: D = 10 and D = 12)
    return SimpleNamespace(name=name, W=W, H=H, C=C, N=N, Ns=Ns, boxcut=boxcut, dropped=dropped, candidates=M,
                           colors=colors, backgrounds=torch.rand(C, MAX_CH, generator=g), edge=extra, **arr)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> namespace(name, W, H, C, N, Ns, boxcut, means2d [C,N,2], conics [C,N,3], opacities [N] | [C,N], depths [C,N], radii
    [C,N] int32, colors [N,26] | [C,N,26], backgrounds [C,26], dropped, candidates, edge): fp32 CPU tensors, unchanged by
    every user."""
    return _build(name)


def arrays_of(cs):
    return dict(means2d=cs.means2d, conics=cs.conics, opacities=cs.opacities, depths=cs.depths, radii=cs.radii)


def isect_case(cs):
    """The case in tests/isect_cases.py's format (for its numpy restatement of the tile lists)."""
    return dict(name=cs.name, means2d=cs.means2d.numpy(), radii=cs.radii.numpy(), depths=cs.depths.numpy(),
                conics=cs.conics.numpy(), opacities=cs.opacities.numpy(), W=cs.W, H=cs.H, C=cs.C, edge={})


def tiles_per_gauss(cs):
    """[C,N] int32 from isect_cases.tile_rects (csrc/common.h tile_rect restated)."""
    tw, th = -(-cs.W // TILE), -(-cs.H // TILE)
    x0, y0, x1, y1 = isect_cases.tile_rects(cs.means2d.reshape(-1, 2).numpy(), cs.radii.reshape(-1).numpy(), tw, th)
    tpg = np.where(cs.radii.reshape(-1).numpy() > 0, (x1 - x0) * (y1 - y0), 0)
    return torch.from_numpy(tpg.astype(np.int32)).reshape(cs.C, cs.N)


# ---- references --------------------------------------------------------------------------------------------------------
def layout_of(D, depth_channel=None):
    """(colour channels, depth as the `extra` channel) of a pass of D total channels: D = 10 is the training build, 9
    features + depth; every other count is colours alone unless depth_channel says otherwise."""
    extra = (D == 10) if depth_channel is None else depth_channel
    return D - (1 if extra else 0), extra


def cotangents(cs, D, tag=""):
    """(v_render [C,H,W,D], v_alpha [C,H,W,1]) of a seeded generator.  tag "one clamped pixel" (case `centre`): zero but at
    the centre pixel of clamped_front_row()."""
    g = _gen("cot", cs.name, D, tag)
    v_r, v_a = torch.randn(cs.C, cs.H, cs.W, D, generator=g), torch.randn(cs.C, cs.H, cs.W, 1, generator=g)
    if tag == "one clamped pixel":
        x, y = (int(v) for v in cs.means2d[0, clamped_front_row(cs)])
        keep = torch.zeros(cs.C, cs.H, cs.W, 1)
        keep[0, y, x] = 1.0
        v_r, v_a = v_r * keep, v_a * keep
    return v_r, v_a


def clamped_front_row(cs):
    """The row with opacity > 0.999 that is first in depth at its own centre pixel (T = 1 there: it blends, clamped)."""
    w = walk(arrays_of(cs), cs.W, cs.H, torch.float64, cs.boxcut)[0]
    for j, row in enumerate(w.idx.tolist()):
        p = int(cs.means2d[0, row, 1]) * cs.W + int(cs.means2d[0, row, 0])
        if float(cs.opacities[row]) > ALPHA_MAX and not w.valid[p, :j].any():
            return row
    raise ValueError("no clamped splat is first at its centre")


def dense_eval(cs, dtype, ch, has_extra, rows=None, use_bg=True, ones=False, cot=None, only=None, moment_mass=False):
    """The dense reference in `dtype` over the splat rows `rows` (a slice; all): render [C,H,W,D], alpha [C,H,W,1] and, with
    cot = (v_render, v_alpha), the gradients of <render, v_render> + <alpha, v_alpha> by autograd, each of its input's full
    shape (rows outside `rows`: exactly 0).  ones: a ones colour [N,1] (the coverage pass).  only = "alpha" / "render": the
    other output's cotangent is zero.  moment_mass: also "moment_mass" [C,N,3], see moment_term()."""
    def leaf(t):
        return t.to(dtype).clone().requires_grad_(True)
    m, con, op = leaf(cs.means2d), leaf(cs.conics), leaf(cs.opacities)
    cols = None if ones else leaf(cs.colors[..., :ch])
    extra = leaf(cs.depths) if has_extra else None
    D = (1 if ones else ch) + (1 if has_extra else 0)
    bg = leaf(cs.backgrounds[:, :D]) if use_bg else None
    px, py = _pixels(cs.W, cs.H, dtype)
    P = px.numel()
    renders, alphas, sigmas = [], [], []
    for c in range(cs.C):
        idx = _order(cs.depths[c], cs.radii[c], rows)
        n = idx.numel()
        opc = op[c] if op.dim() == 2 else op
        sigma, _, alpha = _pairs(m[c, idx], con[c, idx], opc[idx], px, py)
        if moment_mass:
            sigma.retain_grad()
            sigmas.append((idx, sigma))
        inside = _in_rect(cs.means2d[c, idx], cs.radii[c, idx], cs.W, cs.H) if cs.boxcut else None
        contrib = _decide(sigma.detach(), alpha.detach(), inside)[3]
        a_inc = torch.where(contrib, alpha, torch.zeros_like(alpha))
        T_incl = torch.cumprod(1 - a_inc, dim=1)
        T_excl = torch.cat([torch.ones_like(T_incl[:, :1]), T_incl[:, :-1]], dim=1)
        if ones:
            feat = torch.ones(n, 1, dtype=dtype)
        else:
            feat = (cols[c] if cols.dim() == 3 else cols)[idx]
        if has_extra:
            feat = torch.cat([feat, extra[c, idx, None]], dim=1)
        pc = (a_inc * T_excl) @ feat
        T_fin = T_incl[:, -1] if n else torch.ones(P, dtype=dtype)
        if bg is not None:
            pc = pc + T_fin[:, None] * bg[c][None, :]
        renders.append(pc.reshape(cs.H, cs.W, D))
        alphas.append((1 - T_fin).reshape(cs.H, cs.W, 1))
    render, alpha = torch.stack(renders), torch.stack(alphas)
    out = {"render": render.detach(), "alpha": alpha.detach()}
    if cot is not None:
        v_r, v_a = _cot_for(cot, only)
        torch.autograd.backward([render, alpha], [v_r.to(dtype), v_a.to(dtype)])

        def grad(t):
            return t.grad if t.grad is not None else torch.zeros_like(t)
        out.update(v_means2d=grad(m), v_conics=grad(con), v_opacities=grad(op))
        if cols is not None:
            out["v_colors"] = grad(cols)
        if extra is not None:
            out["v_extra"] = grad(extra)
        if bg is not None:
            out["v_backgrounds"] = grad(bg)
        if moment_mass:
            # sum over pixels of |v_sigma| (|m| + |c|)^2-type products, m = splat centre and c = pixel centre relative to
            # the centre of the pixel's tile: the size of the terms the moment conversion of raster_bwd_mfma.hip cancels
            tcx, tcy = torch.floor(px / TILE) * TILE + TILE / 2, torch.floor(py / TILE) * TILE + TILE / 2
            mass = torch.zeros(cs.C, cs.N, 5, dtype=dtype)
            for c, (idx, sigma) in enumerate(sigmas):
                vs = sigma.grad.abs() if sigma.grad is not None else torch.zeros_like(sigma)
                ax = (m.detach()[c, idx, 0][None, :] - tcx[:, None]).abs() + (px - tcx).abs()[:, None]
                ay = (m.detach()[c, idx, 1][None, :] - tcy[:, None]).abs() + (py - tcy).abs()[:, None]
                ca, cb, cc = (con.detach()[c, idx, i].abs()[None, :] for i in range(3))
                mass[c, idx] = torch.stack([0.5 * (vs * ax * ax).sum(0), (vs * ax * ay).sum(0), 0.5 * (vs * ay * ay).sum(0),
                                            (vs * (ca * ax + cb * ay)).sum(0), (vs * (cb * ax + cc * ay)).sum(0)], 1)
            out["moment_mass"] = mass
    return out


def moment_term(mass):
    """The additive term of the matrix-pipe backward arms (csrc/raster_bwd_mfma.hip) -> (conics [C,N,3], means2d [C,N,2]).
    Those kernels sum vs {1, cx, cy, cx^2, cx cy, cy^2} over the pixels of a tile (c = pixel centre relative to the tile
    centre) and convert with the splat centre m relative to the tile centre: sum vs dx^2 = m_x (m_x S0 - 2 Sx) + Sxx, ...
    Every intermediate is at most  mass = sum |vs| (|m| + |c|)^2  (the conic's components; for the position gradient
    sum |vs| (|ca| (|m_x| + |c_x|) + |cb| (|m_y| + |c_y|))), and a product passes the 16 chained v_mfma_f32_16x16x4
    accumulations of a quadrant (counted as one rounding of the accumulator per instruction), 4 quadrant adds and 6
    operations of the conversion: 26 roundings of at most 2^-24 mass each (the sum over a splat's tiles is the quadrant
    kernel's too).  First order.  Counting the four products inside an instruction separately would give 74; the largest
    residual measured on an MI355X is 7 x 2^-24 mass."""
    b = MOMENT_OPS * 2.0 ** -24 * mass
    return b[..., :3], b[..., 3:]


def stored_alpha_shift(name, ch, has_extra, rows=None, use_bg=True, ones=False, tag="", only=None, stored=None):
    """The signed first-order effect, on every gradient, of the backward kernels starting their walk from the STORED alpha:
    they read the pixel's final transmittance back as T' = 1 - alpha32 (upstream's way), and half an ulp of alpha (3e-8
    next to 1) is 3e-4 of a transmittance that stopped just above 1e-4.  Every gradient share of a pixel is linear in the
    pixel's cotangents AND proportional to the transmittance the walk starts from, so the effect of T' = T (1 + eps) is
    the float64 gradient of the same loss with the cotangents eps x v: name -> float64 tensor.
    stored: the alpha image the forward kernel wrote ([C,H,W,1] or [C,H,W] fp32; compared with float64 on its own) --
    exactly what the backward pass reads; None (the image is not an output): the float64 alpha rounded to fp32."""
    cs = case(name)
    D = (1 if ones else ch) + (1 if has_extra else 0)
    sl = None if rows is None else slice(*rows)
    alpha64 = reference(name, ch, has_extra, rows, use_bg, ones, tag, only)[0]["alpha"]
    a32 = alpha64.float() if stored is None else stored.detach().cpu().float().reshape(alpha64.shape)
    eps = (1.0 - a32.double()) / (1.0 - alpha64) - 1.0
    v_r, v_a = _cot_for(cotangents(cs, D, tag), only)
    out = dense_eval(cs, torch.float64, ch, has_extra, sl, use_bg, ones, (v_r.double() * eps, v_a.double() * eps))
    return {k: v for k, v in out.items() if k.startswith("v_")}


def _cot_for(cot, only):
    v_r, v_a = cot
    return (torch.zeros_like(v_r) if only == "alpha" else v_r), (torch.zeros_like(v_a) if only == "render" else v_a)


LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
ULP_OP = 2.0 ** -23        # v_exp_f32 and v_rcp_f32: 1 ulp
MOMENT_OPS = 26            # roundings on the way of one product into a converted moment: see moment_term()


@torch.no_grad()
def kernel_form_eval(cs, dtype, ch, has_extra, rows=None, use_bg=True, ones=False, cot=None, only=None, moments=False,
                     ulp_bound=False):
    """The same operation in the NUMBER FORMS the compositors state for themselves, evaluated in `dtype` on the CPU -- the
    second fp32 reference (float64: equals dense_eval, which tests/test_raster_cases_cpu.py checks):
      * alpha from the record's exponent form (csrc/common.h record_exponent_form, csrc/raster_shared.h eval_splat): raw =
        exp2(L + A dx^2 + C dy^2 + B dx dy), A = -log2(e) a / 2, B = -log2(e) b, C = -log2(e) c / 2, L = log2(opacity).  The
        exponent is a sum of magnitude |L| + sigma log2(e), so raw carries ulp(|L| + ..) ln 2 of relative error where
        opacity x exp(-sigma) carries ulp(sigma): several times more at a low opacity;
      * the backward walk of upstream's rasterize_to_pixels_bwd, which the kernels follow: the pixel's final transmittance
        is recovered from the STORED alpha, T = 1 - fl(1 - T), and the walk goes back to front with T <- T / (1 - alpha)
        and the running sum of what lies behind.  Half an ulp of alpha (3e-8 next to 1) is 3e-4 of a transmittance that
        stopped just above 1e-4, and every gradient share of that pixel scales with it;
      * position gradients from the raw sums  sum v_sigma dx,  sum v_sigma dy  times the conic (csrc/raster.hip stage 2);
      * moments = True, the matrix-pipe backward (csrc/raster_bwd_mfma.hip): per tile the MOMENTS sum vs {1, cx, cy, cx^2,
        cx cy, cy^2} of the pixel centres c relative to the tile centre (|c| <= 7.5), converted with the splat centre m
        relative to the tile centre -- sum vs dx^2 = m_x (m_x S0 - 2 Sx) + Sxx and so on.  Terms of size (|m| + |c|)^2 sum
        |vs| cancel down to d^2: for a splat a few pixels wide the conic gradient carries some 25 x the rounding error of
        the direct sum.
    The decisions (which pair blends) are the float64 walk's: no pair is near a kink.
    ulp_bound (float64, with cot): also "ulp_bound", name -> per gradient element the first-order bound of what the one
    ulp (U = 2^-23) of v_exp_f32 and v_rcp_f32 can do.  alpha (1 + U) makes
    1 - alpha wrong by eta = U alpha / (1 - alpha), and every transmittance behind that pair scales with it: the
    transmittance in front of pair i is off by E_i = sum_{k in front} eta_k + U x (pairs the backward walk has divided by),
    the final one by E_fin = sum eta_k.  With  v_alpha_i = T_i dot_i + ra_i (tvab - sum_{m behind} fac_m dot_m):
      |d v_alpha_i| <= |T_i dot_i| E_i + ra_i (|tvab| E_fin + sum_m |fac_m dot_m| (U + E_m)) + ra_i |tvab - behind_i| (eta_i + U),
      |d v_sigma_i| <= raw_i |d v_alpha_i| + U |v_sigma_i|,  colour shares fac_i (U + E_i) |v|, background T_fin E_fin |v|,
    summed over the pixels with the absolute geometric factor of each gradient."""
    t = dtype
    U = ULP_OP
    D = (1 if ones else ch) + (1 if has_extra else 0)
    px, py = _pixels(cs.W, cs.H, t)
    P = px.numel()
    out = dict(render=torch.zeros(cs.C, cs.H, cs.W, D, dtype=t), alpha=torch.zeros(cs.C, cs.H, cs.W, 1, dtype=t))
    if cot is not None:
        v_r, v_a = (v.to(t) for v in _cot_for(cot, only))
        out.update(v_means2d=torch.zeros(cs.C, cs.N, 2, dtype=t), v_conics=torch.zeros(cs.C, cs.N, 3, dtype=t),
                   v_opacities=torch.zeros(cs.opacities.shape, dtype=t))
        if not ones:
            out["v_colors"] = torch.zeros(cs.colors[..., :ch].shape, dtype=t)
        if has_extra:
            out["v_extra"] = torch.zeros(cs.C, cs.N, dtype=t)
        if use_bg:
            out["v_backgrounds"] = torch.zeros(cs.C, D, dtype=t)
    walks = walk(arrays_of(cs), cs.W, cs.H, torch.float64, cs.boxcut, rows)
    tw, th = -(-cs.W // TILE), -(-cs.H // TILE)
    tcx, tcy = torch.floor(px / TILE) * TILE + TILE / 2, torch.floor(py / TILE) * TILE + TILE / 2   # the pixel's tile centre
    tile_of = (torch.floor(py / TILE) * tw + torch.floor(px / TILE)).long()
    tile_cx = (torch.arange(tw * th) % tw).to(t) * TILE + TILE / 2
    tile_cy = (torch.arange(tw * th) // tw).to(t) * TILE + TILE / 2
    cx, cy = px - tcx, py - tcy
    for c, w in enumerate(walks):
        idx, contrib = w.idx, w.contrib
        n = idx.numel()
        con, m = cs.conics[c, idx].to(t), cs.means2d[c, idx].to(t)
        op = (cs.opacities[c] if cs.opacities.dim() == 2 else cs.opacities)[idx].to(t)
        A, B, Cc, L = (-0.5 * LOG2E) * con[:, 0], -LOG2E * con[:, 1], (-0.5 * LOG2E) * con[:, 2], torch.log2(op)
        if ones:
            feat = torch.ones(n, 1, dtype=t)
        else:
            feat = (cs.colors[c] if cs.colors.dim() == 3 else cs.colors)[idx, :ch].to(t)
        if has_extra:
            feat = torch.cat([feat, cs.depths[c, idx, None].to(t)], dim=1)
        bg = cs.backgrounds[c, :D].to(t) if use_bg else None
        dx, dy = m[None, :, 0] - px[:, None], m[None, :, 1] - py[:, None]
        s = (B * dx) * dy + ((Cc * dy) * dy + ((A * dx) * dx + L))
        raw = torch.exp2(s)
        alpha = torch.clamp(raw, max=ALPHA_MAX)
        T = torch.ones(P, dtype=t)
        acc = torch.zeros(P, D, dtype=t)
        eta = torch.where(contrib, U * alpha / (1 - alpha), torch.zeros_like(alpha))
        e_front = torch.cumsum(eta, dim=1) - eta               # sum of eta over the pairs in front
        e_fin = eta.sum(dim=1)
        for j in range(n):
            on = contrib[:, j]
            wgt = torch.where(on, alpha[:, j] * T, torch.zeros_like(T))
            acc += wgt[:, None] * feat[j][None, :]
            T = torch.where(on, T * (1 - alpha[:, j]), T)
        alpha_out = 1 - T
        out["render"][c] = (acc + T[:, None] * bg[None, :] if use_bg else acc).reshape(cs.H, cs.W, D)
        out["alpha"][c] = alpha_out.reshape(cs.H, cs.W, 1)
        if cot is None:
            continue
        vr, va = v_r[c].reshape(P, D), v_a[c].reshape(P)
        T_fin = 1 - alpha_out                                  # what the backward kernels read back
        T = T_fin.clone()
        behind = torch.zeros(P, D, dtype=t)
        v_bg_dot = (vr * bg[None, :]).sum(1) if use_bg else None
        tvab = T_fin * (va - v_bg_dot) if use_bg else T_fin * va
        divided = torch.zeros(P, dtype=t)                      # pairs the walk has divided by so far
        beh_err = torch.zeros(P, dtype=t)
        if ulp_bound:
            ub = out.setdefault("ulp_bound", {k: torch.zeros_like(v) for k, v in out.items() if k.startswith("v_")})
        for j in reversed(range(n)):
            on = contrib[:, j]
            if not on.any():
                continue
            a = alpha[:, j]
            ra = 1 / (1 - a)
            T = torch.where(on, T * ra, T)                     # transmittance in front of splat j
            fac = torch.where(on, a * T, torch.zeros_like(T))
            v_feat = (fac[:, None] * vr).sum(0)
            v_alpha = ((feat[j][None, :] * T[:, None] - behind * ra[:, None]) * vr).sum(1) + T_fin * ra * va
            if use_bg:
                v_alpha = v_alpha - T_fin * ra * v_bg_dot
            behind = behind + feat[j][None, :] * fac[:, None]
            live = on & (raw[:, j] < ALPHA_MAX)
            v_sigma = torch.where(live, -raw[:, j] * v_alpha, torch.zeros_like(T))
            if ulp_bound:
                divided = divided + on.to(t)
                e_T = e_front[:, j] + U * divided
                dot = (feat[j][None, :] * vr).sum(1)
                q = v_alpha - T * dot                          # ra (tvab - behind . v)
                d_va = (T * dot).abs() * e_T + ra * (tvab.abs() * e_fin + beh_err) + q.abs() * (eta[:, j] + U)
                d_vs = torch.where(live, raw[:, j] * d_va + U * v_sigma.abs(), torch.zeros_like(T))
                beh_err = beh_err + (fac * dot).abs() * (U + e_T)
                i_, (ca_, cb_, cc_) = int(idx[j]), con[j]
                ub["v_means2d"][c, i_] = torch.stack([(d_vs * (ca_ * dx[:, j] + cb_ * dy[:, j]).abs()).sum(),
                                                      (d_vs * (cb_ * dx[:, j] + cc_ * dy[:, j]).abs()).sum()])
                ub["v_conics"][c, i_] = torch.stack([0.5 * (d_vs * dx[:, j] ** 2).sum(), (d_vs * (dx[:, j] * dy[:, j]).abs()).sum(),
                                                     0.5 * (d_vs * dy[:, j] ** 2).sum()])
                col_b = ((fac * (U + e_T))[:, None] * vr.abs()).sum(0)
                if ub["v_opacities"].dim() == 2:
                    ub["v_opacities"][c, i_] = (d_vs / op[j]).sum()
                else:
                    ub["v_opacities"][i_] += (d_vs / op[j]).sum()
                if "v_colors" in ub:
                    if ub["v_colors"].dim() == 3:
                        ub["v_colors"][c, i_] = col_b[:ch]
                    else:
                        ub["v_colors"][i_] += col_b[:ch]
                if has_extra:
                    ub["v_extra"][c, i_] = col_b[D - 1]
            v_op = torch.where(live, (raw[:, j] / op[j]) * v_alpha, torch.zeros_like(T)).sum()
            dxj, dyj = dx[:, j], dy[:, j]
            if moments:
                S = torch.zeros(tw * th, 6, dtype=t).index_add_(0, tile_of, torch.stack(
                    [v_sigma, v_sigma * cx, v_sigma * cy, v_sigma * cx * cx, v_sigma * cx * cy, v_sigma * cy * cy], 1))
                mx, my = m[j, 0] - tile_cx, m[j, 1] - tile_cy
                sx, sy = (mx * S[:, 0] - S[:, 1]).sum(), (my * S[:, 0] - S[:, 2]).sum()
                sxx = (mx * (mx * S[:, 0] - 2 * S[:, 1]) + S[:, 3]).sum()
                sxy = (mx * my * S[:, 0] - mx * S[:, 2] - my * S[:, 1] + S[:, 4]).sum()
                syy = (my * (my * S[:, 0] - 2 * S[:, 2]) + S[:, 5]).sum()
            else:
                sx, sy = (v_sigma * dxj).sum(), (v_sigma * dyj).sum()
                sxx, sxy, syy = (v_sigma * dxj * dxj).sum(), (v_sigma * dxj * dyj).sum(), (v_sigma * dyj * dyj).sum()
            i = int(idx[j])
            ca, cb, cc = con[j]
            out["v_means2d"][c, i] = torch.stack([ca * sx + cb * sy, cb * sx + cc * sy])
            out["v_conics"][c, i] = torch.stack([0.5 * sxx, sxy, 0.5 * syy])
            if out["v_opacities"].dim() == 2:
                out["v_opacities"][c, i] = v_op
            else:
                out["v_opacities"][i] += v_op
            if "v_colors" in out:
                if out["v_colors"].dim() == 3:
                    out["v_colors"][c, i] = v_feat[:ch]
                else:
                    out["v_colors"][i] += v_feat[:ch]
            if has_extra:
                out["v_extra"][c, i] = v_feat[D - 1]
        if use_bg:
            out["v_backgrounds"][c] = (vr * T_fin[:, None]).sum(0)
            if ulp_bound:
                ub["v_backgrounds"][c] = (vr.abs() * (T_fin * e_fin)[:, None]).sum(0)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, ch, has_extra, rows=None, use_bg=True, ones=False, tag="", only=None):
    """(float64, fp32) dense references of a case with the cotangents cotangents(case, D, tag), and the additive terms of
    tests/test_gpu_raster_kernels.py: "ulp_bound" (name -> tensor) and "moment_mass" [C,N,5].  Computed once and shared:
    leave them unchanged.  rows: None or (start, stop)."""
    cs = case(name)
    D = (1 if ones else ch) + (1 if has_extra else 0)
    cot = cotangents(cs, D, tag)
    sl = None if rows is None else slice(*rows)
    ref64 = dense_eval(cs, torch.float64, ch, has_extra, sl, use_bg, ones, cot, only, moment_mass=True)
    ref32 = dense_eval(cs, torch.float32, ch, has_extra, sl, use_bg, ones, cot, only)
    ulp = kernel_form_eval(cs, torch.float64, ch, has_extra, sl, use_bg, ones, cot, only, ulp_bound=True)["ulp_bound"]
    terms = {"moment_mass": ref64.pop("moment_mass"), "ulp_bound": ulp}
    return ref64, ref32, terms


def close_with_terms(got, ref64, ref32, shift, bound, k, what):
    """deform_cases.close_to_f64 with the dense fp32 reference as the yardstick, after the derived terms of a gradient:
    the signed stored-alpha `shift` is taken off `got`, and the difference to float64 is shrunk, element by element, by the
    additive `bound`; both count as 0 wherever the float64 reference is exactly 0, so the zero rule is untouched.  Prints
    the k needed without and with the terms and returns the latter."""
    g = got.detach().cpu().double().reshape(ref64.shape)
    plain = needed_k(g, ref64, ref32)[3]
    bound = torch.where(ref64 == 0, torch.zeros_like(bound), bound)
    d = torch.where(ref64 == 0, g, g - shift - ref64)
    print(f"TERMS {what}: dense-only k {plain:.3f}; largest additive term {float(bound.max()) if bound.numel() else 0.0:.3e}")
    return close_to_f64(ref64 + torch.sign(d) * (d.abs() - bound).clamp(min=0), ref64, ref32, k, what)


def summed(refs, key):
    """The gradient `key` of a loss that adds several passes: the sum of their references (float64)."""
    return sum(r[key].double() for r in refs)


def no_contributor(name, rows=None):
    """[C,H,W] bool: no splat (of `rows`) contributes to the pixel (float64 walk)."""
    cs = case(name)
    sl = None if rows is None else slice(*rows)
    return torch.stack([~w.contrib.any(dim=1).reshape(cs.H, cs.W)
                        for w in walk(arrays_of(cs), cs.W, cs.H, torch.float64, cs.boxcut, sl)])


def margins(name):
    """-> (largest relative |ref32 - ref64| of raw, of the inclusive T) over the evaluated pairs of a case.  raw: over the
    pairs with raw >= RAW_FLOOR -- inside a tile rectangle sigma reaches 100 and more, where exp(-sigma) is a denormal fp32
    number with a relative error of order 1, but such a pair is hundreds of e-folds under 1/255 and no rounding moves it
    across; a pair within a factor 3.9 of the lowest kink is measured.  T: over the evaluated pairs that pass."""
    cs = case(name)
    a = arrays_of(cs)
    e_raw = e_T = 0.0
    for w64, w32 in zip(walk(a, cs.W, cs.H, torch.float64, cs.boxcut), walk(a, cs.W, cs.H, torch.float32, cs.boxcut)):
        sel = w64.evaluated & (w64.raw >= RAW_FLOOR)
        if sel.any():
            e_raw = max(e_raw, float(((w32.raw.double() - w64.raw).abs() / w64.raw)[sel].max()))
        sel = w64.evaluated & w64.valid
        if sel.any():
            e_T = max(e_T, float(((w32.T_incl.double() - w64.T_incl).abs() / w64.T_incl)[sel].max()))
    return e_raw, e_T
