"""Constructed tile-list cases for the binning kernels (mobgs_amd/csrc/isect.hip): every case places a list length, a run
of equal depths, a chunk boundary or an owner span ON a value at which the kernels change behaviour, a plain numpy
restatement of upstream binning gives the expected outputs, and one driver calls the C entry points with guard words
around every output buffer.

tests/test_isect_cases_cpu.py proves (without a GPU) that each case reaches the edge it names and that the restatement
equals the C oracle; tests/test_gpu_isect_kernels.py runs the cases on the device.  All outputs are integers: every
comparison is exact."""
import math

import numpy as np

TILE = 16

# The values the cases aim at, restated ONCE.  They are the constants of mobgs_amd/csrc/isect_launch.h (pinned there by
# the static_asserts on sort_plan / short_sort_epl) and of isect.hip; whoever retunes the header updates the cases.
EPL8_MAX = 512          # short_sort_epl: <= 512 -> 8 keys per lane
EPL16_MAX = 1024        # <= 1024 -> 16 keys per lane, beyond: 32
SHORT_SORT_LDS_KEYS = 2048   # sort_plan().split from 2049; also mobgs_fused_max_seg_stride()
HUGE_FROM = 12288       # sort_plan().huge from 12289 (3/4 of LONG_SORT_LDS_KEYS)
LONG_SORT_LDS_KEYS = 16384   # RADIX_CAP: the LDS radix sort; merge passes step at 16384 << p
RADIX_MAX_RUN = 48      # longest run of equal depth bits the radix fix-up orders itself
OWNER_LDS = 4096        # bin_kernel: owner span cached in LDS up to this many splats
KEEP_CHUNK = 2048       # intersections per keep_scan chunk = per bin_kernel workgroup = per scan workgroup
SCAN_LOOKBACK = 64      # predecessors one look-back step inspects
DENSE_MAX_TILES = 8192  # = ORDER_LDS_TILES
TC_COPIES = 8
THRESHOLDS = dict(EPL8_MAX=512, EPL16_MAX=1024, SHORT_SORT_LDS_KEYS=2048, HUGE_FROM=12288, LONG_SORT_LDS_KEYS=16384,
                  RADIX_MAX_RUN=48, OWNER_LDS=4096)

ONE = 0x3F800000  # bits of 1.0f


# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------
def tile_rects(means2d, radii, tile_w, tile_h):
    """csrc/common.h tile_rect in float32, per splat: -> x0, y0, x1, y1 (int64 arrays)."""
    f = np.float32
    inv = f(1.0) / f(TILE)
    tr = radii.astype(f) * inv
    tx, ty = means2d[:, 0].astype(f) * inv, means2d[:, 1].astype(f) * inv

    def clamp(v, hi):
        return np.minimum(np.maximum(v, f(0)), f(hi)).astype(np.int64)
    return (clamp(np.floor(tx - tr), tile_w), clamp(np.floor(ty - tr), tile_h),
            clamp(np.ceil(tx + tr), tile_w), clamp(np.ceil(ty + tr), tile_h))


def tile_bits_of(tiles_per_cam):
    return int(math.floor(math.log2(tiles_per_cam))) + 1


def min_sigma64(mx, my, a, b, c, x0, x1, y0, y1):
    """float64 minimum of sigma = (a dx^2 + c dy^2) / 2 + b dx dy over the rectangle [x0, x1] x [y0, y1] (arrays): 0 with
    the mean inside, else attained on one of the four edges (convex quadratic)."""
    mx, my, a, b, c, x0, x1, y0, y1 = (np.asarray(v, np.float64) for v in (mx, my, a, b, c, x0, x1, y0, y1))
    inside = (mx >= x0) & (mx <= x1) & (my >= y0) & (my <= y1)

    def sig(dx, dy):
        return 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy
    best = np.full(np.broadcast(mx, x0).shape, np.inf)
    with np.errstate(all="ignore"):
        for px in (x0, x1):
            dx = mx - px
            py = np.clip(my + (b / c) * dx, y0, y1)
            best = np.minimum(best, sig(dx, my - py))
        for py in (y0, y1):
            dy = my - py
            px = np.clip(mx + (b / a) * dy, x0, x1)
            best = np.minimum(best, sig(mx - px, dy))
    return np.where(inside, 0.0, best)


def tau_of(op):
    """ln(255 op) with the product taken in float32 as the kernels take it; -inf where the splat is never listed
    (!(op * 255 >= 1), NaN included)."""
    p = np.asarray(op, np.float32) * np.float32(255.0)
    with np.errstate(all="ignore"):
        return np.where(p >= np.float32(1.0), np.log(p.astype(np.float64)), -np.inf)


def reference(case, cull=0, capacity=None, order=None):
    """Upstream binning restated: -> dict with tiles_per_gauss, cum_tiles [n+1], tile_offsets [nt+1], flatten_ids,
    isect_ids (int64 view of the u64 keys), stats (I_box, I_listed, longest), slots [min(I_box, capacity) + 1] (compact
    index of every box intersection j, j = I_box included), plus the per-box-intersection arrays owner / tile / keep and,
    with cull, sigma / tau for the margin check.  order: the enumeration order of the fused path (a permutation)."""
    C, W, H = case["C"], case["W"], case["H"]
    means2d = case["means2d"].reshape(-1, 2)
    radii = case["radii"].reshape(-1).astype(np.int64)
    dbits = np.ascontiguousarray(case["depths"], np.float32).reshape(-1).view(np.uint32).astype(np.uint64)
    n = radii.shape[0]
    N = n // C
    tile_w, tile_h = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    tpc = tile_w * tile_h
    nt = C * tpc
    x0, y0, x1, y1 = tile_rects(means2d, radii, tile_w, tile_h)
    tpg = np.where(radii > 0, (x1 - x0) * (y1 - y0), 0)
    o = np.arange(n) if order is None else np.asarray(order, np.int64)
    cum_enum = np.concatenate([[0], np.cumsum(tpg[o])])
    cum = np.empty(n + 1, np.int64)
    cum[o] = cum_enum[:-1]
    cum[n] = cum_enum[-1]
    I_box = int(cum[n])
    I = I_box if capacity is None else min(I_box, int(capacity))
    owner = o[np.repeat(np.arange(n), tpg[o])][:I]
    q = np.arange(I) - cum[owner]
    w = (x1 - x0)[owner]
    row = q // np.maximum(w, 1)
    tx, ty = x0[owner] + (q - row * w), y0[owner] + row
    cam = owner // N
    tile_in_cam = ty * tile_w + tx
    tile = cam * tpc + tile_in_cam
    keep = np.ones(I, bool)
    out = {}
    if cull:
        con = case["conics"].reshape(-1, 3).astype(np.float64)
        op = np.asarray(case["opacities"], np.float32)
        op = op.reshape(-1)[owner if op.size == n else owner % N]
        tau = tau_of(op)
        a, b, c = con[owner, 0], con[owner, 1], con[owner, 2]
        px0, py0 = tx * TILE + 0.5, ty * TILE + 0.5
        px1, py1 = np.minimum(tx * TILE + 15.5, W - 0.5), np.minimum(ty * TILE + 15.5, H - 0.5)
        sigma = min_sigma64(means2d[owner, 0], means2d[owner, 1], a, b, c, px0, px1, py0, py1)
        degenerate = ~((a > 0) & (c > 0))
        keep = np.isfinite(tau) & (degenerate | (sigma <= tau))
        out.update(sigma=sigma, tau=tau, degenerate=degenerate)
    bits = tile_bits_of(tpc)
    key = (((cam.astype(np.uint64) << np.uint64(bits)) | tile_in_cam.astype(np.uint64)) << np.uint64(32)) | dbits[owner]
    kk, kf = key[keep], owner[keep]
    perm = np.lexsort((kf, kk))
    lens = np.bincount(tile[keep], minlength=nt)
    out.update(tiles_per_gauss=tpg.astype(np.int32), cum_tiles=cum.astype(np.int32),
               tile_offsets=np.concatenate([[0], np.cumsum(lens)]).astype(np.int32),
               flatten_ids=kf[perm].astype(np.int32), isect_ids=kk[perm].view(np.int64),
               stats=(I_box, int(keep.sum()), int(lens.max()) if nt else 0),
               slots=np.concatenate([[0], np.cumsum(keep)]).astype(np.int64),
               owner=owner, tile=tile, keep=keep, lens=lens, nt=nt, tile_bits=bits, tile_w=tile_w, tile_h=tile_h)
    return out


def runs_of(sorted_keys):
    """[(position, length)] of the runs (length >= 2) of equal values in a sorted array."""
    if len(sorted_keys) == 0:
        return []
    cut = np.flatnonzero(np.diff(sorted_keys) != 0) + 1
    starts = np.concatenate([[0], cut])
    lens = np.diff(np.concatenate([starts, [len(sorted_keys)]]))
    return [(int(s), int(l)) for s, l in zip(starts, lens) if l >= 2]


def chunk_owner_span(ref, chunk):
    """Splats in the owner range bin_kernel's workgroup `chunk` searches: from the owner of the chunk's first intersection
    to the owner of the NEXT chunk's first intersection (the last chunk: of its own last intersection)."""
    owner = ref["owner"]
    start, nxt = chunk * KEEP_CHUNK, (chunk + 1) * KEEP_CHUNK
    hi = owner[nxt] if nxt < len(owner) else owner[-1]
    return int(hi - owner[start] + 1)


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def distinct_ints(rng, hi, n):
    """n distinct integers of [0, hi) in random order (without the hi-sized permutation rng.choice would build)."""
    u = np.empty(0, np.int64)
    while len(u) < n:
        u = np.unique(np.concatenate([u, rng.integers(0, hi, size=n + n // 2 + 16)]))
    return rng.permutation(u)[:n]


def distinct_depth_bits(n, rng):
    """n distinct float32 bit patterns in [1, 2): bytes 0-2 vary, byte 3 is constant (one radix pass is a no-op)."""
    return (ONE + distinct_ints(rng, 1 << 23, n)).astype(np.uint32)


def _case(name, means, radii, bits, W, H, C=1, conics=None, opacities=None, **edge):
    n = len(radii)
    assert n % C == 0
    N = n // C
    bits = np.asarray(bits, np.uint32)
    assert ((bits >= 0x00800000) & (bits < 0x7F800000)).all(), "depths: positive, normal, finite"
    if conics is None:
        conics = np.tile(np.float32([1e-4, 0.0, 1e-4]), (n, 1))
    if opacities is None:
        opacities = np.full(N, 0.9, np.float32)
    return dict(name=name, means2d=np.asarray(means, np.float32).reshape(C, N, 2),
                radii=np.asarray(radii, np.int32).reshape(C, N), depths=bits.view(np.float32).reshape(C, N),
                conics=np.asarray(conics, np.float32).reshape(C, N, 3), opacities=np.asarray(opacities, np.float32),
                W=W, H=H, C=C, edge=edge)


def pile(n, grid, bits=None, seed=0, name=None):
    """n splats over the same tile (grid 1: a 16x16 image, mean at the tile centre) or the same 2x2 tiles (grid 2: mean at
    the shared corner); radius 4: floor and ceil sit a quarter tile from the seam.  Every list has exactly n entries."""
    rng = np.random.default_rng(1000 * grid + n + seed)
    if bits is None:
        bits = distinct_depth_bits(n, rng)
    c = 8.0 if grid == 1 else 16.0
    return _case(name or f"pile{n}_g{grid}", np.full((n, 2), c), np.full(n, 4), bits, 16 * grid, 16 * grid,
                 longest=n, lists=grid * grid)


PILE_N = (1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 12288, 12289, 16383, 16384, 16385, 32768,
          32769, 65537)
HINT_TRUTHS = (300, 513, 1025, 2049, 3000, 16385, 40000)
HINTS = (0, 512, 513, 1025, 2049, 12289, 40000)


def pile_cases():
    out = [pile(n, g) for n in PILE_N for g in (1, 2)]
    for n in (2049, 16385):
        srt = np.sort(distinct_depth_bits(n, np.random.default_rng(n)))
        out.append(pile(n, 1, srt, name=f"pile{n}_sorted"))
        out.append(pile(n, 1, srt[::-1].copy(), name=f"pile{n}_reversed"))
    return out


def mixed_case():
    """One 4x2-tile grid with lists of 0, 1, 513, 1025, 2049 and 16385 entries (and two more short ones): the long-list
    compaction and both sort launches side by side."""
    lens = [0, 1, 513, 1025, 2049, 16385, 0, 7]
    rng = np.random.default_rng(7)
    tiles = rng.permutation(np.repeat(np.arange(8), lens))
    means = np.stack([(tiles % 4) * 16 + 8.0, (tiles // 4) * 16 + 8.0], 1)
    return _case("mixed", means, np.full(len(tiles), 4), distinct_depth_bits(len(tiles), rng), 64, 32,
                 lens=lens, longest=16385)


def tie_case(n, runs, name=None):
    """A 1-tile pile of n splats whose sorted depth list holds the given runs [(position, length)] of equal bits and no
    other tie.  Input (splat) order is random."""
    rng = np.random.default_rng(n + 31 * len(runs) + sum(p for p, _ in runs))
    srt = np.sort(distinct_depth_bits(n, rng))
    for p, length in runs:
        srt[p:p + length] = srt[p]
    ids = rng.permutation(n)  # ids[i] = the splat that takes sorted position i
    bits = np.empty(n, np.uint32)
    bits[ids] = srt
    return pile(n, 1, bits, name=name or f"ties{n}_" + "_".join(f"{p}x{l}" for p, l in runs[:2]))


def descending_tie_case(n, chunks, per_chunk, pos):
    """A 2x2-tile pile of n splats with ONE run of equal depth bits whose members reach the sort in an order of FALLING
    flat ids -- by construction, not by timing.  Splat g owns box intersections 4 g .. 4 g + 3, so it is binned by
    workgroup (chunk) g >> 9, which ranks through counter copy (g >> 9) & 7; tile_scan_kernel lays a tile's segment out
    copy by copy (tile_base), so whatever the atomics do, an entry ranked through a lower copy precedes one ranked through
    a higher copy in the sort's input.  `chunks` names one chunk per copy 0, 1, ... with FALLING chunk numbers (24, 17,
    10, 3: copies 0, 1, 2, 3); the run takes per_chunk splats from each (a number, or one per chunk).  Members of copy 0 (the highest ids) therefore
    come first in the input and members of the last copy (the lowest ids) last; the stable radix passes keep that order,
    and only the fix-up (or the fallback network) can put the run into ascending id order."""
    assert all(c & 7 == k for k, c in enumerate(chunks)) and list(chunks) == sorted(chunks, reverse=True)
    assert n >= 512 * (max(chunks) + 1)
    rng = np.random.default_rng(n + pos)
    per = [per_chunk] * len(chunks) if np.isscalar(per_chunk) else list(per_chunk)
    members = np.concatenate([512 * c + rng.choice(512, k, replace=False) for c, k in zip(chunks, per)])
    length = len(members)
    rest = rng.permutation(np.setdiff1d(np.arange(n), members))
    ids = np.concatenate([rest[:pos], rng.permutation(members), rest[pos:]])  # ids[i]: the splat at sorted position i
    srt = np.sort(distinct_depth_bits(n, rng))
    srt[pos:pos + length] = srt[pos]
    bits = np.empty(n, np.uint32)
    bits[ids] = srt
    c = pile(n, 2, bits, name=f"ties{n}_g2_{pos}x{length}_desc")
    c["edge"].update(runs=[(pos, length)], desc_chunks=tuple(chunks))
    return c


def tie_cases():
    out = []
    for n in (3000, 16384):
        for length in (2, 47, 48, 49):
            for pos in (0, n - length, 1024 - length // 2):
                c = tie_case(n, [(pos, length)])
                c["edge"].update(runs=[(pos, length)])
                out.append(c)
        full = [(p, 48) for p in range(0, n - 47, 48)]
        c = tie_case(n, full, name=f"ties{n}_all48")
        c["edge"].update(runs=full)
        out.append(c)
        c = tie_case(n, [(1000, 48), (n - 47, 47)])
        c["edge"].update(runs=[(1000, 48), (n - 47, 47)])
        out.append(c)
    # falling ids along the run: 5000 splats (chunk 8 wraps to copy 0 and precedes chunk 1) and 12800 (four copies); both
    # lists are longer than 2048 and at most 16384 entries: radix_sort_long; runs of 48 (fix-up) and 49 (fallback)
    out.append(descending_tie_case(5000, (8, 1), 24, 1000))
    out.append(descending_tie_case(12800, (24, 17, 10, 3), 12, 1000))
    out.append(descending_tie_case(12800, (24, 17, 10, 3), 12, 12800 - 48))
    out.append(descending_tie_case(5000, (8, 1), (25, 24), 0))
    return out


def byte_cases():
    n, rng = 3000, np.random.default_rng(5)
    i = rng.permutation(n)
    pats = {
        "byte0": ONE | (i % 256),                                     # 256 values: runs of 11 / 12
        "byte3": ((1 + i % 126) << 24),                               # 126 values: runs of 23 / 24
        "bytes12": 0x3F000000 | (distinct_ints(rng, 1 << 16, n) << 8),
        "bytes0123": 0x00800000 + distinct_ints(rng, 0x7E800000, n),
        "equal": np.full(n, ONE + 12345),                             # one run of 3000: the network fallback
    }
    out = []
    for k, b in pats.items():
        c = pile(n, 1, np.asarray(b, np.uint32), name=f"bits_{k}")
        c["edge"].update(pattern=k)
        out.append(c)
    return out


def _one_tile_splats(n_total, visible_at, rng, W=64, H=64):
    """n_total splats, those at `visible_at` cover one random tile each (radius 4 at the tile centre), the others are
    invisible (radius 0)."""
    tw, th = W // TILE, H // TILE
    t = rng.integers(0, tw * th, n_total)
    means = np.stack([(t % tw) * 16 + 8.0, (t // tw) * 16 + 8.0], 1)
    radii = np.zeros(n_total, np.int64)
    radii[visible_at] = 4
    return means, radii


def seam_cases():
    out = []
    for ibox in (2047, 2048, 2049, 4096, 6144):
        rng = np.random.default_rng(ibox)
        means, radii = _one_tile_splats(ibox, np.arange(ibox), rng)
        out.append(_case(f"ibox{ibox}", means, radii, distinct_depth_bits(ibox, rng), 64, 64, ibox=ibox))
    # owner span of chunk 0: visible splat 0 is splat 0, visible splat 2048 (the next chunk's first owner) is splat span - 1
    for span in (4095, 4096, 4097, 20000):
        rng = np.random.default_rng(span)
        n_vis, tail_invisible = 2600, 37
        mid = np.sort(rng.choice(np.arange(1, span - 1), 2047, replace=False))
        vis = np.concatenate([[0], mid, [span - 1], span + 2 * np.arange(n_vis - 2049)])
        n_total = int(vis[-1]) + 1 + tail_invisible
        means, radii = _one_tile_splats(n_total, vis, rng)
        out.append(_case(f"span{span}", means, radii, distinct_depth_bits(n_total, rng), 64, 64, span=span,
                         trailing=tail_invisible))
    rng = np.random.default_rng(140)
    vis = np.sort(rng.choice(139000, 300, replace=False))
    means, radii = _one_tile_splats(140000, vis, rng)
    out.append(_case("scan69", means, radii, distinct_depth_bits(140000, rng), 64, 64, scan_chunks=69, ibox=300))
    return out


def wide_cases():
    out = []
    rng = np.random.default_rng(9)
    # 64 x 48 tiles: the middle splat covers all 3072
    means = [[24.0, 24.0], [512.0, 384.0], [1000.0, 744.0]]
    out.append(_case("wide3072", means, [20, 2004, 4], distinct_depth_bits(3, rng), 1024, 768, wide=3072, wide_id=1))
    # 257 x 130 tiles (> DENSE_MAX_TILES = ORDER_LDS_TILES): box widths 7, 3, 1 before and after the full-grid splat
    small = [([40 * 16 + 8.0, 50 * 16 + 8.0], 52), ([100 * 16 + 8.0, 20 * 16 + 8.0], 20), ([200 * 16 + 8.0, 99 * 16 + 8.0], 4)]
    means = [m for m, _ in small] + [[2056.0, 1040.0]] + [[m[0] + 320.0, m[1] + 160.0] for m, _ in small]
    radii = [r for _, r in small] + [6004] + [r for _, r in small]
    out.append(_case("wide33410", means, radii, distinct_depth_bits(7, rng), 257 * 16, 130 * 16, wide=33410, wide_id=3,
                     widths=[7, 3, 1, 257, 7, 3, 1]))
    return out


def camera_cases():
    """C = 3 on a 4x4-tile grid (dense build: 48 tiles); camera c piles its visible splats on tile 5 c + 1."""
    out = []
    for name, counts, edge in (("cams_inside1", (2048, 3000, 700), dict(boundary_inside_cam=1, boundary=4096)),
                               ("cams_straddle01", (1000, 500, 300), dict(straddle=(0, 1), chunk=0)),
                               ("cams_long", (3000, 3000, 10), dict(straddle=(0, 1), chunk=1))):
        rng = np.random.default_rng(sum(counts))
        N = 3100
        means, radii = [], []
        for c, k in enumerate(counts):
            t = 5 * c + 1
            means.append(np.tile([(t % 4) * 16 + 8.0, (t // 4) * 16 + 8.0], (N, 1)))
            r = np.zeros(N, np.int64)
            r[np.sort(rng.choice(N, k, replace=False))] = 4
            radii.append(r)
        out.append(_case(name, np.concatenate(means), np.concatenate(radii), distinct_depth_bits(3 * N, rng), 64, 64, C=3,
                         counts=counts, **edge))
    return out


OP_EXACT = np.float32(1.0) / np.float32(255.0)
assert OP_EXACT * np.float32(255.0) >= np.float32(1.0)
OP_BELOW = np.nextafter(OP_EXACT, np.float32(0))
while OP_BELOW * np.float32(255.0) >= np.float32(1.0):
    OP_BELOW = np.nextafter(OP_BELOW, np.float32(0))


def cull_case():
    """8x8 tiles, every splat at the centre of an interior tile.  Radius 20: a 3x3 box whose edge tiles are 8.5 px and
    whose corner tiles are 8.5 sqrt(2) px away.  Isotropic conic a: 0.01 keeps all nine (sigma <= 0.73 against ln(127.5) =
    4.85), 0.5 keeps the centre only (sigma >= 18).  Kinds, cycled through the mixed blocks:
      0 op 0.5 a 0.01 (9 kept)   1 op 0.5 a 0.5 (1 kept)   2 op 0 (none)   3 op NaN (none)   4 op just below 1/255 (none)
      5 op 1/255, radius 4 (its one tile kept)   6 op 1/255 a 0.5 (centre kept)   7 op 0.5, a = -1 (degenerate: all 9)
      8 op 0.5, a = 0 (degenerate: all 9)
    Splat order: 300 mixed (2436 intersections: kept and dropped inside chunk 0 and across position 2048), 460 of kind 2
    (4140 intersections, 2436 .. 6575: chunk 2 = 4096 .. 6143 keeps nothing), 100 mixed."""
    rng = np.random.default_rng(11)
    kinds = np.concatenate([np.arange(300) % 9, np.full(460, 2), np.arange(100) % 9])
    n = len(kinds)
    op = np.select([kinds == 2, kinds == 3, kinds == 4, (kinds == 5) | (kinds == 6)],
                   [0.0, np.nan, OP_BELOW, OP_EXACT], 0.5).astype(np.float32)
    a = np.select([kinds == 0, kinds == 7, kinds == 8], [0.01, -1.0, 0.0], 0.5)
    conics = np.stack([a, np.zeros(n), np.where(kinds == 7, 0.5, a)], 1)
    t = rng.integers(0, 36, n)
    means = np.stack([(1 + t % 6) * 16 + 8.0, (1 + t // 6) * 16 + 8.0], 1)
    radii = np.where(kinds == 5, 4, 20)
    return _case("cull", means, radii, distinct_depth_bits(n, rng), 128, 128, conics=conics, opacities=op, kinds=kinds,
                 empty_chunk=2)


def direct_cases():
    """Every two-pass case (cull = 0; the culling case also runs with cull = 1), by name."""
    cases = pile_cases() + [pile(n, 1) for n in HINT_TRUTHS if n not in PILE_N] + [mixed_case()] + tie_cases() + \
        byte_cases() + seam_cases() + wide_cases() + camera_cases() + [cull_case()]
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names), "case names must be unique"
    return {c["name"]: c for c in cases}


_CASES, _REFS = None, {}


def cases():
    global _CASES
    if _CASES is None:
        _CASES = direct_cases()
    return _CASES


def case_names():
    return list(cases())


def ref_of(name, cull=0):
    """The reference of a case, computed once and shared (callers must not modify it)."""
    k = (name, cull)
    if k not in _REFS:
        _REFS[k] = reference(cases()[name], cull)
    return _REFS[k]


# ---- fused path: 3-D piles under an identity camera -------------------------------------------------------------------
FUSED_N = (511, 512, 513, 1023, 1024, 1025, 2047, 2048)
FUSED_GRIDS = (1, 4, 6)   # tiles per side: 1 chunk = 1 counter copy; 4x4 (>= 8 chunks from 1023 splats on); 6x6 (>= 8
#                           chunks, so all 8 copies, at every N: 36 * 511 / 2048 = 8.98)


def fused_pile(n, grid, runs=()):
    """n splats at the optical axis, distinct z in [1, 2) except the given runs [(position in depth order, length)] of
    equal z; identity camera, focal length = the image size, scale 2: the 3-sigma radius exceeds 6 image sizes, every
    splat covers every tile.  -> dict of float32 arrays (means, quats, scales, opacities, viewmats, Ks) + W, H."""
    rng = np.random.default_rng(77 * grid + n)
    z = np.sort(distinct_depth_bits(n, rng))
    for p, length in runs:
        z[p:p + length] = z[p]
    z = z[rng.permutation(n)].view(np.float32)
    S = 16 * grid
    means = np.stack([np.zeros(n, np.float32), np.zeros(n, np.float32), z], 1)
    K = np.float32([[S, 0, S / 2], [0, S, S / 2], [0, 0, 1]])
    return dict(means=means, quats=np.tile(np.float32([1, 0, 0, 0]), (n, 1)), scales=np.full((n, 3), 2.0, np.float32),
                opacities=np.full(n, 0.9, np.float32), viewmats=np.eye(4, dtype=np.float32)[None], Ks=K[None], W=S, H=S)


# ---------------------------------------------------------------------------------------------------------------------
# driver (GPU)
# ---------------------------------------------------------------------------------------------------------------------
GUARD = 64
_GUARD_BYTE, _POISON_BYTE = 0x5C, 0x6B


class _Guarded:
    """`count` elements of `dtype` on the device between two rows of GUARD guard elements; the payload starts out as
    poison, so an element the kernels never wrote cannot pass for a result."""

    def __init__(self, count, dtype, dev):
        import torch
        self.size = torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full(((count + 2 * GUARD) * self.size,), _POISON_BYTE, dtype=torch.uint8, device=dev)
        self.raw[:GUARD * self.size] = _GUARD_BYTE
        self.raw[(GUARD + count) * self.size:] = _GUARD_BYTE
        self.t = self.raw[GUARD * self.size:(GUARD + count) * self.size].view(dtype)

    def intact(self):
        g = GUARD * self.size
        return bool((self.raw[:g] == _GUARD_BYTE).all()) and bool((self.raw[-g:] == _GUARD_BYTE).all())


def slots_from_keep_scan(keep_scan, upto):
    """include/mobgs_hip.h: compact index of box intersection j, for j = 0 .. upto."""
    ks = np.asarray(keep_scan).astype(np.int64)
    j = np.arange(upto + 1)
    return ks[(j >> 11) * 2049] + ks[(j >> 11) * 2049 + 1 + (j & 2047)]


def run_two_pass(case, ref, dev, cull=0, capacity=None, hint=None, capacity_listed=None):
    """mobgs_isect_offsets + mobgs_isect_emit_sort (hint None), or mobgs_isect_offsets(capacity_listed > 0) +
    mobgs_isect_emit_sort_speculative (hint = max_tile_len_hint), straight through the C ABI with an explicit arena
    `capacity` (default: I_box) and guard words around every output.  -> dict of numpy outputs + guards_ok.
    capacity < I_box: only the offsets call runs (the header: "call again with capacity >= I_box")."""
    import torch
    from mobgs_amd import _lib
    lib = _lib.load(build_if_missing=False)
    ptr, check = _lib.ptr, _lib.check
    C, W, H = case["C"], case["W"], case["H"]
    N = case["radii"].shape[1]
    tile_w, tile_h = ref["tile_w"], ref["tile_h"]
    nt = ref["nt"]
    I_box, I_listed, longest = ref["stats"]
    cap = max(1, I_box if capacity is None else capacity)
    T = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev).contiguous()  # noqa: E731
    means2d, radii = T(case["means2d"], torch.float32), T(case["radii"], torch.int32)
    depths, conics = T(case["depths"], torch.float32), T(case["conics"], torch.float32)
    opac, tpg = T(case["opacities"], torch.float32), T(ref["tiles_per_gauss"], torch.int32)
    i32, i64 = torch.int32, torch.int64
    bufs = dict(cum_tiles=_Guarded(C * N + 1, i32, dev), keep_scan=_Guarded(lib.mobgs_keep_scan_len(cap), i32, dev),
                tile_offsets=_Guarded(nt + 1, i32, dev), tile_order=_Guarded(lib.mobgs_tile_order_len(nt), i32, dev),
                stats=_Guarded(3, i64, dev), scratch=_Guarded(lib.mobgs_isect_scratch_bytes(C * N, nt, cap), torch.uint8, dev))
    speculative = hint is not None
    cl = 0
    if speculative:
        cl = max(1, I_listed) if capacity_listed is None else capacity_listed
    b = {k: v.t for k, v in bufs.items()}
    check(lib.mobgs_isect_offsets(C, N, tile_w, tile_h, W, H, int(cull), cap, ptr(tpg), ptr(means2d), ptr(radii),
                                  ptr(conics), ptr(opac), 1 if opac.dim() == 2 else 0, ptr(b["cum_tiles"]),
                                  ptr(b["keep_scan"]), ptr(b["tile_offsets"]), ptr(b["tile_order"]), cl, ptr(b["stats"]),
                                  ptr(b["scratch"]), None, _lib.stream()), "mobgs_isect_offsets")
    stats = tuple(int(v) for v in b["stats"].tolist())
    n_out = cl if speculative else stats[1]
    lists = dict(sort_keys=_Guarded(max(n_out, 1), i64, dev), flatten_ids=_Guarded(max(n_out, 1), i32, dev),
                 isect_ids=_Guarded(max(n_out, 1), i64, dev))
    bufs.update(lists)
    if speculative:
        check(lib.mobgs_isect_emit_sort_speculative(C, N, tile_w, tile_h, cap, cl, int(hint), ptr(depths),
                                                    ptr(b["cum_tiles"]), ptr(b["tile_offsets"]), ptr(b["stats"]),
                                                    ptr(b["scratch"]), ptr(lists["sort_keys"].t),
                                                    ptr(lists["flatten_ids"].t), ptr(lists["isect_ids"].t),
                                                    _lib.stream()), "mobgs_isect_emit_sort_speculative")
    elif stats[0] <= cap and stats[1] > 0:
        check(lib.mobgs_isect_emit_sort(C, N, tile_w, tile_h, cap, stats[1], stats[2], ptr(depths), ptr(b["cum_tiles"]),
                                        ptr(b["tile_offsets"]), ptr(b["scratch"]), ptr(lists["sort_keys"].t),
                                        ptr(lists["flatten_ids"].t), ptr(lists["isect_ids"].t), _lib.stream()),
              "mobgs_isect_emit_sort")
    torch.cuda.synchronize()
    out = {k: bufs[k].t.cpu().numpy() for k in ("cum_tiles", "keep_scan", "tile_offsets", "tile_order", "flatten_ids",
                                               "isect_ids")}
    out["stats"] = stats
    out["slots"] = slots_from_keep_scan(out["keep_scan"], min(stats[0], cap))
    out["guards_ok"] = all(v.intact() for v in bufs.values())
    out["broken_guards"] = [k for k, v in bufs.items() if not v.intact()]
    return out
