"""Deterministic, kink-free cases for the flow-warp loss kernels (csrc/flowloss.hip through
mobgs_amd.loss_utils.flow_warp_loss), their float64 and fp32 references from oracle/render_torch.flow_warp_loss, the strata
of every output tensor and the comparator of tests/test_gpu_flow_kernels.py.  Torch on the CPU and the oracle only: nothing of
the package under test is imported here; tests/test_flow_cases_cpu.py checks from the references alone that every case is
kink-free, reaches the edge it is named after, and that the comparator rejects planted errors.

Kinks.  The block has three: floor(ix) and the border clamp of the sample positions, and sgn((warp - target) mask) of the two
L1 terms.  fp32 and float64 must take the same branch everywhere, so that no comparison needs a flip allowance:
  * coordinates: the float64 sample positions ix, iy (the reference's arithmetic: c / (size - 1), 2 n - 1,
    ((g + 1) size - 1) / 2, on the fp32 coordinate) keep their fractional part MARGIN_X away from 0 and 1 and themselves
    MARGIN_X away from the clamp thresholds 0 and size - 1; an offending coordinate is moved by NUDGE pixels, not dropped
    (the bands of the clamp_* cases lie at least one pixel outside the image);
  * differences: where the float64 |warp - target| of some channel is below MARGIN_D the mask of that pixel is set to
    exactly 0 -- latent_alpha[b,k] for the first term, d_alpha[b] (over all k) for the second.  Such holes are part of the
    test: a zero mask issues no atomic and gives exact zeros.
Margins: at least 100 x the largest distance of the fp32 reference's own ix / difference from float64 over the case table
(tests/test_flow_cases_cpu.py::test_margins_are_100_times_the_fp32_references_own_error measures both).

Builds.  `expected_rows` restates the dispatch rule of mobgs_flow_warp_loss_bwd; the GPU test pairs it with the library's
mobgs_flow_warp_loss_bwd_rows.

Comparators (k = 3; nothing here comes from a run of the code under test):
  * the six gradients, per tensor and per stratum: loss_cases.close_map = deform_cases.close_to_f64 -- max |got - ref64| <=
    3 max |ref32 - ref64| + 2^-23 max |ref64|, exact zeros where float64 has exact zeros;
  * term allowance for the two scatter targets (g_ori, g_latent) only, after the precedent of loss_cases: an element of them
    is the fp32 sum of n terms -- every tap that lands on the cell, plus the direct terms -- added one at a time in an order
    that is not fixed.  Each addition rounds a running sum that is at most T, the sum of the terms in absolute value, by at
    most 2^-24 of it (uniformly: standard deviation <= 2^-24 T / sqrt 3); the running sum grows to T over the n steps, so
    the n roundings add up to a random walk of standard deviation <= 2^-24 T sqrt(n) / 3.  Three of them,
    2^-24 sqrt(n) T (`term_magnitude`: n and T per cell in float64, from the inputs alone), maximised over the stratum, is
    added to the bound.  Four taps and a direct term give 1.1 x 2^-23 T, the floor of loss_cases; the cells of pile_up,
    where 3800 samples land, get 31 x 2^-23 T.  A RATIO line shows the k of the plain rule unless it says `with extra`;
  * the loss: loss_cases.close_scalar.
No flip allowance, and no share of elements is left out."""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from deform_cases import needed_k
from loss_cases import K, close_map, close_scalar, gather
from oracle import render_torch as RT

# measured over the case table (tests/test_flow_cases_cpu.py): the fp32 reference's own ix is at most 4.2e-5 px from float64
# (tall8_a and white_noise_8, H = 500; positions within one pixel of the image: farther out the clamp decides), its own
# difference warp - target at most 2.9e-5 (the same two cases: the position error times the image's slope)
MARGIN_X = 5e-3   # pixels: >= 100 x 4.2e-5
MARGIN_D = 3.2e-3  # image units: >= 100 x 2.9e-5
NUDGE = 0.0137    # pixels: more than 2 MARGIN_X, less than the distance to the next kink
COTANGENTS = (1.0, 0.37, -2.5)
NAMES = ("ori", "latent", "e2m", "m2e", "la", "da")
SCATTER = ("ori", "latent")      # atomic sums; the other four gradients and the loss are plain stores
PLAIN = ("e2m", "m2e", "la", "da")
STRATA = ("strip_last", "strip_first", "col63_64", "clamped", "zero_mask", "interior")
EDGE_STRATA = ("strip_last", "strip_first", "col63_64")
TX, TALL_WORKGROUPS = 64, 1024   # csrc/flowloss.hip FL_TX and the threshold of the 8-row build

# name -> (B, K, H, W, kind)
_CASES = {
    "min_2x2": (1, 1, 2, 2, "smooth"),
    "row_pair_2x70": (1, 2, 2, 70, "smooth"),
    "col_pair_70x2": (1, 2, 70, 2, "smooth"),
    "w64": (1, 2, 9, 64, "smooth"),
    "w65": (1, 2, 9, 65, "smooth"),
    "w129": (2, 2, 19, 129, "smooth"),
    "rows_tail4": (1, 3, 37, 70, "smooth"),
    "tall8_a": (32, 2, 500, 70, "smooth"),
    "tall8_b": (256, 1, 33, 65, "smooth"),
    "below_tall": (255, 1, 33, 65, "smooth"),
    "white_noise_4": (2, 3, 37, 70, "white_noise"),
    "white_noise_8": (32, 1, 500, 70, "white_noise"),
    "pile_up": (1, 2, 37, 70, "pile_up"),
    "shift": (1, 2, 37, 70, "shift"),
    "clamp_left": (1, 1, 19, 70, "clamp"),
    "clamp_right": (1, 1, 19, 70, "clamp"),
    "clamp_top": (1, 1, 19, 70, "clamp"),
    "clamp_bottom": (1, 1, 19, 70, "clamp"),
    "clamp_corner": (1, 1, 19, 70, "clamp"),
    "holes": (2, 2, 37, 70, "holes"),
    "smooth_a": (2, 3, 37, 70, "smooth"),
    "smooth_b": (1, 9, 67, 129, "smooth"),
}
CASES = tuple(_CASES)
# cases whose first draw left an edge stratum of a few dozen entries short of the sensitivity that
# tests/test_flow_cases_cpu.py::test_sensitivity asks for (one near-zero entry among 74): drawn again, inputs changed
RESEED = {"clamp_left": 1}
CLAMP_SIDES = {"clamp_left": {"left"}, "clamp_right": {"right"}, "clamp_top": {"top"}, "clamp_bottom": {"bottom"},
               "clamp_corner": {"right", "top"}}
BAND = 6              # width of the clamped band of the clamp_* cases, pixels
PILE = ((23.37, 11.62), (40.3, 20.71))    # the two constant coordinates of pile_up (exp2mid, mid2exp)
SHIFT = ((0.37, 0.61), (0.73, 0.21))      # the sub-pixel translations of shift, in sample positions


def expected_rows(B, H, W, combine):
    """The dispatch rule of mobgs_flow_warp_loss_bwd, restated: rows of a wave's strip in the build it launches."""
    tall = ((W + TX - 1) // TX) * ((H + 31) // 32) * B >= TALL_WORKGROUPS
    return 8 if (combine and tall) else 4


# ---- the reference's arithmetic ----------------------------------------------------------------------------------------
def sample_pos(c, size):
    """Pixel coordinate -> unclamped sample position in c's dtype, statement by statement: train.py's normalisation and
    grid_sampler_unnormalize with align_corners = False."""
    n = c / (size - 1)
    g = 2.0 * n - 1.0
    return ((g + 1.0) * size - 1.0) / 2.0


def positions(coord, H, W, dtype=torch.float64):
    """[B,K,H,W,2] pixel coordinates -> (ix, iy) unclamped, in `dtype`."""
    c = coord.to(dtype)
    return sample_pos(c[..., 0], W), sample_pos(c[..., 1], H)


def taps(coord, H, W):
    """float64 taps of a coordinate map -> namespace(x0, y0 (north-west tap, long), left / right / top / bottom (clamped at
    that side), clamped (on either axis), east / south (the tap x0 + 1 / y0 + 1 lies inside the image))."""
    ix, iy = positions(coord, H, W)
    left, right, top, bottom = ix <= 0, ix >= W - 1, iy <= 0, iy >= H - 1
    x0 = ix.clamp(0, W - 1).floor().long()
    y0 = iy.clamp(0, H - 1).floor().long()
    return SimpleNamespace(ix=ix, iy=iy, x0=x0, y0=y0, left=left, right=right, top=top, bottom=bottom,
                           clamped=left | right | top | bottom, east=x0 + 1 < W, south=y0 + 1 < H)


def near_kink(coord, H, W, margin=None):
    """bool [B,K,H,W,2]: the float64 sample position is within the margin of an integer or of a clamp threshold."""
    margin = MARGIN_X if margin is None else margin
    out = []
    for i, size in ((0, W), (1, H)):
        p = sample_pos(coord[..., i].double(), size)
        fr = p - p.floor()
        out.append((fr < margin) | (fr > 1 - margin) | (p.abs() < margin) | ((p - (size - 1)).abs() < margin))
    return torch.stack(out, dim=-1)


def _settle(coord, H, W):
    """Nudges the coordinates that are near a kink; -> (coordinates, share that was nudged)."""
    moved = torch.zeros_like(coord, dtype=torch.bool)
    for _ in range(8):
        bad = near_kink(coord, H, W)
        if not bad.any():
            return coord.contiguous(), float(moved.double().mean())
        moved |= bad
        coord = torch.where(bad, coord + NUDGE, coord)
    raise ValueError("coordinates do not settle away from the kinks")


def warps(inp, dtype):
    """The two warped images [B,K,3,H,W] in `dtype`, by the reference's statements."""
    ori, latent = inp["ori"].to(dtype), inp["latent"].to(dtype)
    B, Kx, _, H, W = latent.shape

    def norm(coord):
        c = coord.to(dtype)
        return (2.0 * torch.stack([c[..., 0] / (W - 1), c[..., 1] / (H - 1)], dim=-1) - 1.0).flatten(0, 1)

    ori_k = ori.unsqueeze(1).expand(-1, Kx, -1, -1, -1).flatten(0, 1)
    kw = dict(mode="bilinear", padding_mode="border", align_corners=False)
    return (F.grid_sample(ori_k, norm(inp["e2m"]), **kw).reshape(B, Kx, -1, H, W),
            F.grid_sample(latent.flatten(0, 1), norm(inp["m2e"]), **kw).reshape(B, Kx, -1, H, W))


def differences(inp, dtype):
    """(warp_1 - latent, warp_2 - ori) [B,K,3,H,W] in `dtype`."""
    w1, w2 = warps(inp, dtype)
    return w1 - inp["latent"].to(dtype), w2 - inp["ori"].to(dtype).unsqueeze(1)


# ---- the case builder --------------------------------------------------------------------------------------------------
def _pixels(H, W):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    return torch.stack([xs, ys], dim=-1)


def _smooth(B, Kx, H, W, g, flow=2.5, far=0.02):
    """A smooth flow (what get_flow renders) + 0.3 px of noise per pixel + a few far-away samples that the border clamps."""
    low = torch.randn(B, Kx, max(H // 8, 2), max(W // 8, 2), 2, generator=g) * flow
    smooth = F.interpolate(low.flatten(0, 1).permute(0, 3, 1, 2), size=(H, W), mode="bilinear",
                           align_corners=True).permute(0, 2, 3, 1).reshape(B, Kx, H, W, 2)
    c = _pixels(H, W) + smooth + 0.3 * torch.randn(B, Kx, H, W, 2, generator=g)
    out = torch.rand(B, Kx, H, W, generator=g) < far
    c[out] += 3.0 * max(H, W) * torch.randn(int(out.sum()), 2, generator=g)
    return c


def _coords(name, kind, which, B, Kx, H, W, g):
    size = torch.tensor([W, H], dtype=torch.float32)
    if kind == "white_noise":  # uniform over the image and 2 px around it: no two neighbours sample neighbouring cells
        return torch.rand(B, Kx, H, W, 2, generator=g) * (size + 3.0) - 2.0
    if kind == "pile_up":
        return torch.tensor(PILE[which]).expand(B, Kx, H, W, 2).clone()
    if kind == "shift":        # ix = x + sx, iy = y + sy: the cell of lane l + 1 is the right neighbour, of row y + 1 the one below
        return (_pixels(H, W) + 0.5 + torch.tensor(SHIFT[which])) * ((size - 1.0) / size) + torch.zeros(B, Kx, H, W, 2)
    if kind != "clamp":
        return _smooth(B, Kx, H, W, g)
    c = _smooth(B, Kx, H, W, g, flow=1.0, far=0.0)
    c = torch.minimum(torch.maximum(c, torch.ones(2)), size - 2.0)  # the base stays inside: no other side is clamped
    pix = _pixels(H, W)
    below = -(1.5 + 3.0 * torch.rand(B, Kx, H, W, 2, generator=g))           # sample position <= -1
    above = size + 0.5 + 3.0 * torch.rand(B, Kx, H, W, 2, generator=g)       # sample position >= size
    sides = CLAMP_SIDES[name]
    band = torch.ones(H, W, dtype=torch.bool)
    if "left" in sides:
        band &= pix[..., 0] < BAND
    if "right" in sides:
        band &= pix[..., 0] >= W - BAND
    if "top" in sides:
        band &= pix[..., 1] < BAND
    if "bottom" in sides:
        band &= pix[..., 1] >= H - BAND
    for side, axis, value in (("left", 0, below), ("right", 0, above), ("top", 1, below), ("bottom", 1, above)):
        if side in sides:
            c[..., axis] = torch.where(band, value[..., axis], c[..., axis])
    return c


def _mask(shape, H, W, g, zero_frac=0.2):
    """Values from [0.25, 1], exactly zero over blocks of about 6 x 6 pixels (a fifth of them), like a dynamic-object alpha."""
    m = 0.25 + 0.75 * torch.rand(*shape, generator=g)
    blocks = torch.rand(*shape[:-2], max(H // 6, 1), max(W // 6, 1), generator=g) < zero_frac
    z = F.interpolate(blocks.float().reshape(-1, 1, *blocks.shape[-2:]), size=(H, W)).reshape(shape)
    return m * (1 - z)


def _hole_mask(shape, H, W, g):
    """Zero over whole 8 x 8 blocks aligned to 8 (three in ten), block (0, 0) always: it holds the strip end between rows 3
    and 4 of the 4-row builds."""
    m = 0.25 + 0.75 * torch.rand(*shape, generator=g)
    blocks = torch.rand(*shape[:-2], (H + 7) // 8, (W + 7) // 8, generator=g) < 0.3
    blocks[..., 0, 0] = True
    z = blocks.repeat_interleave(8, dim=-2).repeat_interleave(8, dim=-1)[..., :H, :W]
    return m * (~z)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> namespace(name, B, K, H, W, kind, v (the cotangent), inputs {ori [B,3,H,W], latent [B,K,3,H,W], e2m / m2e
    [B,K,H,W,2], la [B,K,1,H,W], da [B,1,H,W]} fp32 CPU tensors, nudged (share of coordinates), zeroed (share of mask
    entries set to 0 for a near-zero difference))."""
    B, Kx, H, W, kind = _CASES[name]
    index = CASES.index(name)
    g = torch.Generator().manual_seed(7000 + index + 100 * RESEED.get(name, 0))
    inp = {"ori": torch.rand(B, 3, H, W, generator=g), "latent": torch.rand(B, Kx, 3, H, W, generator=g)}
    nudged = []
    for which, key in enumerate(("e2m", "m2e")):
        inp[key], share = _settle(_coords(name, kind, which, B, Kx, H, W, g), H, W)
        nudged.append(share)
    make = _hole_mask if kind == "holes" else _mask
    la, da = make((B, Kx, 1, H, W), H, W, g), make((B, 1, H, W), H, W, g)
    if kind == "holes":
        da[B - 1] = 0.0  # one batch entry without a second term: nothing is scattered into its latent gradient
    d1, d2 = differences(inp, torch.float64)
    near1 = (d1.abs() < MARGIN_D).any(dim=2, keepdim=True)           # [B,K,1,H,W]
    near2 = (d2.abs() < MARGIN_D).any(dim=2).any(dim=1, keepdim=True)  # [B,1,H,W]
    zeroed = (float(((la != 0) & near1).double().mean()), float(((da != 0) & near2).double().mean()))
    inp["la"] = torch.where(near1, torch.zeros(()), la).contiguous()
    inp["da"] = torch.where(near2, torch.zeros(()), da).contiguous()
    if not (inp["la"].any() and inp["da"].any()):
        raise ValueError(f"flow case {name}: a mask is zero everywhere")
    return SimpleNamespace(name=name, B=B, K=Kx, H=H, W=W, kind=kind, v=COTANGENTS[index % len(COTANGENTS)], inputs=inp,
                           nudged=max(nudged), zeroed=max(zeroed))


def evaluate(c, dtype, v=None):
    """-> {loss, ori, latent, e2m, m2e, la, da}: the value and the six gradients (cotangent v, the case's own by default) of
    oracle/render_torch.flow_warp_loss in `dtype` on the CPU."""
    t = {k: x.to(dtype, copy=True).requires_grad_(True) for k, x in c.inputs.items()}
    loss = RT.flow_warp_loss(*(t[k] for k in NAMES))
    loss.backward(torch.tensor(c.v if v is None else v, dtype=dtype))
    out = {k: t[k].grad for k in NAMES}
    out["loss"] = loss.detach()
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """(float64, fp32) references of a case, computed once and shared: leave them unchanged."""
    c = case(name)
    return evaluate(c, torch.float64), evaluate(c, torch.float32)


# ---- strata ------------------------------------------------------------------------------------------------------------
def planes(key, t):
    """An output tensor with its pixel plane last: the coordinate gradients [B,K,H,W,2] -> [B,K,2,H,W]."""
    return t.permute(0, 1, 4, 2, 3) if key in ("e2m", "m2e") else t


def _landing(tp, sel, H, W):
    """[B,K,H,W]: how many taps of the selected source pixels land on each cell."""
    B, Kx = sel.shape[:2]
    hit = torch.zeros(B * Kx, H * W, dtype=torch.float64)
    plane = torch.arange(B * Kx).reshape(B, Kx, 1, 1).expand(B, Kx, H, W)
    for dy, dx, inside in ((0, 0, sel), (0, 1, sel & tp.east), (1, 0, sel & tp.south), (1, 1, sel & tp.east & tp.south)):
        hit.index_put_((plane[inside], ((tp.y0 + dy) * W + tp.x0 + dx)[inside]), torch.ones((), dtype=torch.float64),
                       accumulate=True)
    return hit.reshape(B, Kx, H, W)


def _touched(tp, sel, H, W):
    """bool [B,K,H,W]: the cells that a tap of a selected source pixel lands on."""
    return _landing(tp, sel, H, W) > 0


@functools.lru_cache(maxsize=None)
def strata(name, rows):
    """-> {tensor: {stratum: bool mask that broadcasts against planes(tensor)}} for the build with `rows` rows per strip.
    A pixel is tagged by its place in the walk of the build -- strip_last (the last live row of a strip: its carried row
    leaves through flush()), strip_first (the first row of the next strip), col63_64 (lane 63, whose right-hand column no
    lane takes, and lane 0 of the next strip) --, and by its inputs: clamped (a coordinate gradient whose sample is clamped
    on an axis; a scatter target that a clamped sample lands on), zero_mask (the mask that scales this entry's own term is
    exactly 0), interior (none of these).  The tags overlap; every entry carries at least one."""
    c = case(name)
    B, Kx, H, W, inp = c.B, c.K, c.H, c.W, c.inputs
    y = torch.arange(H).reshape(H, 1).expand(H, W)
    x = torch.arange(W).reshape(1, W).expand(H, W)
    walk = {"strip_last": (y % rows == rows - 1) | (y == H - 1), "strip_first": (y % rows == 0) & (y > 0),
            "col63_64": (x % TX == TX - 1) | ((x % TX == 0) & (x > 0))}
    t1, t2 = taps(inp["e2m"], H, W), taps(inp["m2e"], H, W)
    la0, da0 = inp["la"] == 0, inp["da"] == 0                       # [B,K,1,H,W], [B,1,H,W]
    on1, on2 = ~la0[:, :, 0], (~da0).expand(B, Kx, H, W)           # sources that scatter: [B,K,H,W]
    clamped = {"e2m": t1.clamped.unsqueeze(2), "la": t1.clamped.unsqueeze(2), "m2e": t2.clamped.unsqueeze(2),
               "da": t2.clamped.any(dim=1, keepdim=True),
               "ori": _touched(t1, on1 & t1.clamped, H, W).any(dim=1, keepdim=True),
               "latent": _touched(t2, on2 & t2.clamped, H, W).unsqueeze(2)}
    zero = {"e2m": la0, "la": la0, "m2e": da0.unsqueeze(1), "da": da0, "ori": da0, "latent": la0}
    out = {}
    for key in NAMES:
        shape = planes(key, inp[key]).shape
        full = shape[:-3] + (1, H, W)
        tags = {s: m.expand(full) for s, m in walk.items()}
        tags["clamped"], tags["zero_mask"] = clamped[key].expand(full), zero[key].expand(full)
        rest = torch.ones(full, dtype=torch.bool)
        for m in tags.values():
            rest = rest & ~m
        tags["interior"] = rest
        out[key] = tags
    return out


@functools.lru_cache(maxsize=None)
def term_magnitude(name):
    """float64 {ori [B,1,H,W], latent [B,K,1,H,W]} -> (T, n) per cell of the two scatter targets (the same for the three
    channels).  T: the element with every term in absolute value -- |v| / S of the other term's mask, spread by the bilinear
    weights of every sample that lands on the cell, plus the direct terms (|sgn| = 1 wherever a mask is not 0: the
    differences there are at least MARGIN_D).  n: the number of those terms."""
    c = case(name)
    inp = {k: t.double() for k, t in c.inputs.items()}
    B, Kx, H, W = c.B, c.K, c.H, c.W
    S1, S2 = 3.0 * inp["la"].sum() + 1e-8, 3.0 * Kx * inp["da"].sum() + 1e-8
    one = {"ori": torch.ones(B, 1, H, W, dtype=torch.float64, requires_grad=True),
           "latent": torch.ones(B, Kx, 1, H, W, dtype=torch.float64, requires_grad=True),
           "e2m": inp["e2m"], "m2e": inp["m2e"]}
    w1, w2 = warps(one, torch.float64)  # linear in the images: the gradient of a weighted sum is the scatter of the weights
    ((w1 * inp["la"]).sum() / S1 + (w2 * inp["da"].unsqueeze(1)).sum() / S2).backward()
    v = abs(c.v)
    la_on, da_on = c.inputs["la"] != 0, c.inputs["da"] != 0
    n1 = _landing(taps(c.inputs["e2m"], H, W), la_on[:, :, 0], H, W).sum(dim=1, keepdim=True)         # [B,1,H,W]
    n2 = _landing(taps(c.inputs["m2e"], H, W), da_on.expand(B, Kx, H, W), H, W).unsqueeze(2)         # [B,K,1,H,W]
    return {"ori": (v * (one["ori"].grad + Kx * inp["da"] / S2), n1 + Kx * da_on),
            "latent": (v * (one["latent"].grad + inp["la"] / S1), n2 + la_on)}


def term_extra(name, key, ref64, mask):
    """max 2^-24 sqrt(n) T over the entries `mask` of a scatter target (module docstring); 0 for the other tensors."""
    if key not in SCATTER:
        return 0.0
    T, n = term_magnitude(name)[key]
    return 2.0 ** -24 * float((n.sqrt() * T).expand(ref64.shape)[mask].max())


def bound(name, key, rows, stratum, refs=None):
    """3 x the fp32 reference's gap + 2^-23 max |ref64| + the term allowance of one stratum of one tensor; None if empty."""
    ref64, ref32 = refs or reference(name)
    r64, r32 = planes(key, ref64[key]), planes(key, ref32[key]).double()
    m = strata(name, rows)[key][stratum].expand(r64.shape)
    if not m.any():
        return None
    return K * float((r32[m] - r64[m]).abs().max()) + 2.0 ** -23 * float(r64[m].abs().max()) + term_extra(name, key, r64, m)


# ---- the comparator ----------------------------------------------------------------------------------------------------
def compare(name, rows, got, what, keys=NAMES, loss=True, refs=None, sink=None):
    """The rule of the module docstring on the loss and on the gradients `keys` of one run: every gradient per stratum of
    the build with `rows` rows.  Every comparison prints its RATIO line; the failures are gathered and raised once.  `sink`,
    a list, collects (family, stratum, what, k needed, k of the plain rule without the term allowance)."""
    ref64, ref32 = refs or reference(name)
    tags = strata(name, rows)
    needs, failures = [], []
    if loss:
        k = gather(failures, close_scalar, got["loss"], ref64["loss"], ref32["loss"], f"{what} loss")
        needs.append(("loss", "-", f"{what} loss", k, k))
    for key in keys:
        g = got[key].detach().cpu()
        assert tuple(g.shape) == tuple(ref64[key].shape), f"{what} g_{key}: shape {tuple(g.shape)} != {tuple(ref64[key].shape)}"
        g, r64, r32 = planes(key, g), planes(key, ref64[key]), planes(key, ref32[key])
        for s in STRATA:
            m = tags[key][s].expand(r64.shape)
            if not m.any():
                continue
            tag = f"{what} g_{key} [{s}]"
            family = "scatter" if key in SCATTER else ("coordinate" if key in ("e2m", "m2e") else "mask")
            needs.append((family, s, tag, gather(failures, close_map, g[m], r64[m], r32[m], K, tag,
                                                 term_extra(name, key, r64, m)), needed_k(g[m], r64[m], r32[m])[3]))
    if sink is not None:
        sink.extend(needs)
    assert not failures, "\n".join(failures)
    return needs
