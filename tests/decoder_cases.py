"""Deterministic cases for the Sandwich colour decoder (csrc/decoder.hip, csrc/decoder_shared.h and the decode arms of
csrc/raster.hip), a plain torch restatement of the operation differentiated by autograd, and the comparison of
tests/test_gpu_decoder_kernels.py.  Torch on the CPU only: nothing of the package under test is imported here;
tests/test_decoder_cases_cpu.py shows from the restatement alone that every case reaches the edge it is built for.

The operation, per pixel p = py * W + px of an image [H, W, CF] (channels-last, CF >= 9, + accumulated depth in channel 9):
    rays    either column p of a map [6, P] (origin | unit direction), or from (intr = fx, fy, cx, cy; c2w = [R | t]):
            loc = ((px + .5 - cx) / fx, (py + .5 - cy) / fy),  d = R [loc, 1],  dir = d / |d|,  origin = t
    colour  rgb = sigmoid(albedo + W2 relu(W1 [spec | timefeat | origin | dir])),  albedo | spec | timefeat = channels 0..8
    depth   depth = channel 9 / max(alpha, 1e-10)
`evaluate` states it once; it is run in float64 (ref64) and in fp32 (ref32) from the same statements.

Kink safety, from float64 alone: every case has min |s_j| >= 2^-10 over all pixels and all six hidden pre-activations
s = W1 x, so fp32 and float64 take the same ReLU branch everywhere and every tensor is compared in full.
  * Synthetic cases (w1 = 0.5 randn, unit-normal features, unit directions): the six spec / time features of an offending
    pixel are redrawn, in at most 8 rounds, and no case redraws more than 2 % of its pixels.  The albedo of a pixel with
    |albedo + y| > 6 is moved so that the sum is 6: no sigmoid is saturated (|albedo + y| stays below 8).
  * Render-derived cases, whose features come out of the compositor and cannot be redrawn, exclude no pixel: the camera
    origin t is constant per image and serves as a bias.  `bias_weights` solves W1[:, 6:9] . t = sign x (+3, -3, +3, -3,
    +3, -3) with the other columns 0.25 randn; the two signs show every unit once active and once inactive.
Alphas are exactly 0 at designated pixels ("holes": nothing was composited there, channel 9 is 0 too) and at least 0.05
elsewhere.  At a hole with a depth cotangent g the image cotangent of channel 9 is g / 1e-10: channel 9 is therefore
compared as tensors of its own, holes and the rest apart, so that 1e10 g does not become the scale of anything else."""
import functools
import math
import zlib
from types import SimpleNamespace

import torch

from deform_cases import close_to_f64, needed_k  # noqa: F401  (the comparator of the deformation tests, unchanged)

MARGIN = 2.0 ** -10
Z_MAX = 8.0
MAX_REDRAW = 0.02
ROUNDS = 8
ALPHA_MIN = 0.05
BIG_P = 4096 * 256 + 65      # the forward kernel's grid-stride loop starts above 4096 workgroups x 256 pixels
# H, W per pixel count: around the 64-lane wave, the 256-thread workgroup and decoder_grid's 768 pixels per workgroup
SHAPES = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13), 256: (16, 16), 257: (1, 257), 767: (13, 59), 768: (24, 32),
          769: (1, 769), 1537: (29, 53), BIG_P: (3, 349547)}
SINGLE_P = (1, 63, 64, 65, 256, 257, 767, 768, 769, 1537)
DEPTH_FORMS = ((True, 10, True), (True, 10, False), (False, 9, False), (True, 12, True))   # has_depth, CF, depth cotangent
RAY_FORMS = ("map", "pin34", "pin44")
COT_SCALES = (1.0, -2.5, 0.5)   # per image of a batch: a partial row credited to the wrong image shows
T_BIAS = (3.0, -2.0, 4.0)       # camera origin of the render-derived cases
FAMILIES = ("outputs", "cots", "weights", "pose")
# k per family: twice the worst any tensor needed on an MI355X, rounded up (tests/test_gpu_decoder_kernels.py has the table)
K = {"outputs": 2, "cots": 4, "weights": 5, "pose": 8}


# ---- the restatement ---------------------------------------------------------------------------------------------------
def pinhole_rays(intr, c2w, H, W):
    """intr [4], c2w [3|4, 4] -> [6, P]: origin | unit direction through every pixel centre, in the inputs' precision."""
    dt = c2w.dtype
    p = torch.arange(H * W)
    py = torch.div(p, W, rounding_mode="floor")
    px = p - py * W
    lx = (px.to(dt) + 0.5 - intr[2]) / intr[0]
    ly = (py.to(dt) + 0.5 - intr[3]) / intr[1]
    R, t = c2w[:3, :3], c2w[:3, 3]
    d = R[:, 0:1] * lx + R[:, 1:2] * ly + R[:, 2:3]
    return torch.cat([t[:, None].expand(3, H * W), d / d.pow(2).sum(0).sqrt()], dim=0)


def decode_statements(feat, alphas, rays6, w1, w2, has_depth, relu=torch.relu):
    """feat [P, CF], alphas [P] | None, rays6 [6, P] -> rgb [3, P], depth [P] | None, s [6, P], z [3, P]."""
    x = torch.cat([feat[:, 3:9].t(), rays6], dim=0)
    s = w1 @ x
    z = feat[:, 0:3].t() + w2 @ relu(s)
    depth = feat[:, 9] / alphas.clamp(min=1e-10) if has_depth else None
    return torch.sigmoid(z), depth, s, z


def _image_rays(case, c, dtype, c2w_leaf=None, map_leaf=None, rays_fn=None):
    rays_fn = rays_fn or pinhole_rays
    if case.ray == "map":
        m = case.rays.to(dtype) if map_leaf is None else map_leaf
        return m[c if m.shape[0] == case.C else 0]
    intr = case.intr[c if case.intr.shape[0] == case.C else 0].to(dtype)
    c2w = case.c2w[c if case.c2w.shape[0] == case.C else 0].to(dtype) if c2w_leaf is None else c2w_leaf
    return rays_fn(intr, c2w, case.H, case.W)


def pre_activations(case):
    """float64: s [C, 6, P] and z = albedo + y [C, 3, P]."""
    s, z = [], []
    for c in range(case.C):
        _, _, sc, zc = decode_statements(case.feat[c].double(), None, _image_rays(case, c, torch.float64),
                                         case.w1.double(), case.w2.double(), False)
        s.append(sc)
        z.append(zc)
    return torch.stack(s), torch.stack(z)


def evaluate(case, dtype, cot_scale=1.0, forward_only=False, relu=torch.relu, rays_fn=None):
    """The statements in `dtype`, differentiated by autograd with the case's cotangents times `cot_scale` -> dict:
    rgb [C,3,P], depth [C,P] (has_depth), v_feat [C,P,CF], v_alphas [C,P] (has_depth; zeros without a depth cotangent),
    v_rays [C,6,P] (a map per image), g_w1 [6,12], g_w2 [3,6] (sums over all images), g_c2w [C,3|4,4] (pinhole rays: one
    leaf per image, also where the images share a pose).  `relu`, `rays_fn`: tests/test_decoder_cases_cpu.py puts a wrong
    statement in their place to show that the comparison notices."""
    C = case.C
    grad = not forward_only
    feat = case.feat.to(dtype, copy=True).requires_grad_(grad)
    alphas = case.alphas.to(dtype, copy=True).requires_grad_(grad) if case.has_depth else None
    w1, w2 = (t.to(dtype, copy=True).requires_grad_(grad) for t in (case.w1, case.w2))
    map_leaf, poses = None, [None] * C
    if case.ray == "map":
        map_leaf = case.rays.to(dtype, copy=True).requires_grad_(grad)
    else:
        poses = [case.c2w[c if case.c2w.shape[0] == C else 0].to(dtype, copy=True).requires_grad_(grad) for c in range(C)]
    rgb, depth = [], []
    with torch.set_grad_enabled(grad):
        for c in range(C):
            r, d, _, _ = decode_statements(feat[c], alphas[c] if case.has_depth else None,
                                           _image_rays(case, c, dtype, poses[c], map_leaf, rays_fn), w1, w2, case.has_depth,
                                           relu)
            rgb.append(r)
            depth.append(d)
        out = {"rgb": torch.stack(rgb)}
        if case.has_depth:
            out["depth"] = torch.stack(depth)
    if forward_only:
        return out
    loss = (out["rgb"] * (cot_scale * case.v_rgb.to(dtype))).sum()
    if case.v_depth is not None:
        loss = loss + (out["depth"] * (cot_scale * case.v_depth.to(dtype))).sum()
    loss.backward()
    out = {k: v.detach() for k, v in out.items()}
    out.update(v_feat=feat.grad, g_w1=w1.grad, g_w2=w2.grad)
    if case.has_depth:
        out["v_alphas"] = alphas.grad if alphas.grad is not None else torch.zeros_like(alphas)
    if case.ray == "map":
        if case.rays.shape[0] == C:
            out["v_rays"] = map_leaf.grad
    else:
        out["g_c2w"] = torch.stack([p.grad for p in poses])
    return out


# ---- comparison --------------------------------------------------------------------------------------------------------
def parts(case, out):
    """The tensors of `out` as they are compared: name -> (family, tensor).  Channel 9 of the image cotangent apart from
    the other channels, and its holes apart from the rest (module docstring)."""
    fam = {"rgb": "outputs", "depth": "outputs", "v_alphas": "cots", "v_rays": "cots", "g_w1": "weights", "g_w2": "weights",
           "g_c2w": "pose"}
    res = {k: (fam[k], out[k]) for k in fam if k in out}
    if "v_feat" in out:
        vf = out["v_feat"]
        if case.has_depth:
            res["v_feat[not 9]"] = ("cots", torch.cat([vf[..., :9], vf[..., 10:]], dim=-1))
            hole = case.hole.to(vf.device)
            res["v_feat[9]"] = ("cots", vf[..., 9][~hole])
            res["v_feat[9] holes"] = ("cots", vf[..., 9][hole])
        else:
            res["v_feat"] = ("cots", vf)
    return res


def compare(case, got, ref64, ref32, K, tag, expect):
    """close_to_f64 on every tensor of `got` (shaped as `evaluate` shapes them); `expect`: the names that must be there.
    -> {name: (family, k needed)}."""
    missing = [k for k in expect if k not in got or got[k] is None]
    assert not missing, f"{tag}: no {missing}"
    g, r64, r32 = parts(case, got), parts(case, ref64), parts(case, ref32)
    needs = {}
    for name, (family, t) in g.items():
        needs[name] = (family, close_to_f64(t, r64[name][1], r32[name][1], K[family], f"{tag} [{family}] {name}"))
    return needs


# ---- synthetic cases ---------------------------------------------------------------------------------------------------
def pose(k, rows, t):
    """fp32 [rows, 4] camera-to-world matrix number k: a rotation by 0.3 + 0.2 k about (1 + k, 2, 3), origin t; the
    fourth row of the 4 x 4 form is (0, 0, 0, 1)."""
    axis = torch.tensor([1.0 + k, 2.0, 3.0], dtype=torch.float64)
    axis = axis / axis.norm()
    a = 0.3 + 0.2 * k
    Kx = torch.tensor([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]], dtype=torch.float64)
    R = torch.eye(3, dtype=torch.float64) + math.sin(a) * Kx + (1.0 - math.cos(a)) * (Kx @ Kx)
    m = torch.eye(4, dtype=torch.float64)
    m[:3, :3], m[:3, 3] = R, torch.tensor(t, dtype=torch.float64)
    return m[:rows].float().contiguous()


def make_kink_safe(case, g):
    """Redraws the spec / time features of offending pixels (module docstring), then moves the albedo of a pixel whose
    |albedo + y| exceeds 6 so that it is 6 (the albedo enters no pre-activation); sets case.margin, case.z_max and
    case.redrawn (the share of pixels redrawn at least once)."""
    ever = torch.zeros(case.C, case.P, dtype=torch.bool)
    for rnd in range(ROUNDS + 1):
        s, z = pre_activations(case)
        bad = s.abs().amin(dim=1) < MARGIN
        if not bad.any():
            break
        if rnd == ROUNDS:
            raise ValueError(f"{case.name}: {int(bad.sum())} pixels still near a kink after {ROUNDS} rounds")
        ever |= bad
        case.feat[..., 3:9][bad] = torch.randn(int(bad.sum()), 6, generator=g)
    case.feat[..., 0:3] += (z.clamp(-6.0, 6.0) - z).transpose(1, 2).float()
    s, z = pre_activations(case)
    case.margin, case.z_max = float(s.abs().min()), float(z.abs().max())
    case.redrawn = float(ever.double().mean())
    return case


@functools.lru_cache(maxsize=None)
def synth_case(P, ray, has_depth=True, CF=10, depth_cot=True, C=1, share=""):
    """fp32 CPU tensors, flat over the pixels: feat [C,P,CF], alphas [C,P] | None, hole [C,P] bool, w1 [6,12], w2 [3,6],
    v_rgb [C,3,P], v_depth [C,P] | None and, ray == "map": rays [C | 1, 6, P]; "pin34" / "pin44": intr [C | 1, 4], c2w
    [C | 1, 3 | 4, 4].  `share`: which of "intr", "c2w", "map" the images of a batch share.  Leave them unchanged.
    A draw that redraws more than 2 % of its pixels (two pixels of 64 are 3 %) is discarded whole and drawn again from the
    next seed, `case.draws` times in all, at most 4."""
    for draw in range(4):
        case = _draw_synth_case(draw, P, ray, has_depth, CF, depth_cot, C, share)
        if case.redrawn <= MAX_REDRAW:
            case.draws = draw + 1
            return case
    raise ValueError(f"{case.name}: {case.redrawn:.2%} of the pixels redrawn (cap {MAX_REDRAW:.0%}) in 4 draws")


def _draw_synth_case(draw, P, ray, has_depth, CF, depth_cot, C, share):
    key = (draw, P, ray, has_depth, CF, depth_cot, C, share)
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    H, W = SHAPES[P]
    feat = torch.randn(C, P, CF, generator=g)
    feat[..., 0:3] = 4.0 * torch.rand(C, P, 3, generator=g) - 2.0
    hole = torch.zeros(C, P, dtype=torch.bool)
    alphas = None
    if has_depth:
        alphas = ALPHA_MIN + (1.0 - ALPHA_MIN) * torch.rand(C, P, generator=g)
        if P >= 63:
            hole[:, 0] = hole[:, P - 1] = True
            hole[:, 5::97] = True
        alphas[hole] = 0.0
        feat[..., 9] = alphas * (0.5 + 5.0 * torch.rand(C, P, generator=g))
    w1, w2 = 0.5 * torch.randn(6, 12, generator=g), 0.5 * torch.randn(3, 6, generator=g)
    fx = max(50.0, W / 4.0)
    intr = torch.tensor([[fx * (1.0 + 0.1 * c), 0.96 * fx * (1.0 - 0.05 * c), W / 2.0 + 0.3 + c, H / 2.0 + 6.8 - 0.5 * c]
                         for c in range(C)])
    c2w = torch.stack([pose(c, 4 if ray == "pin44" else 3, (0.2 + 0.1 * c, -0.3, 0.1 - 0.2 * c)) for c in range(C)])
    rays = None
    if ray == "map":
        rays = torch.stack([pinhole_rays(intr[c].double(), c2w[c].double(), H, W)
                            for c in range(1 if "map" in share else C)]).float()
        intr = c2w = None
    else:
        intr = intr[:1 if "intr" in share else C].contiguous()
        c2w = c2w[:1 if "c2w" in share else C].contiguous()
    scale = torch.tensor(COT_SCALES[:C])
    v_rgb = torch.randn(C, 3, P, generator=g) * scale[:, None, None]
    v_depth = torch.randn(C, P, generator=g) * scale[:, None] if (has_depth and depth_cot) else None
    case = SimpleNamespace(name=f"P{P} {ray} depth{int(has_depth)} CF{CF} cot{int(depth_cot)} C{C} {share}".strip(), P=P, H=H,
                           W=W, C=C, CF=CF, has_depth=has_depth, ray=ray, feat=feat, alphas=alphas, hole=hole, w1=w1, w2=w2,
                           rays=rays, intr=intr, c2w=c2w, v_rgb=v_rgb, v_depth=v_depth)
    return make_kink_safe(case, g)


@functools.lru_cache(maxsize=None)
def synth_reference(P, ray, has_depth=True, CF=10, depth_cot=True, C=1, share="", cot_scale=1.0, forward_only=False):
    """(float64, fp32) references of a synthetic case, computed once and shared: leave them unchanged."""
    case = synth_case(P, ray, has_depth, CF, depth_cot, C, share)
    return (evaluate(case, torch.float64, cot_scale, forward_only), evaluate(case, torch.float32, cot_scale, forward_only))


def summed_pose(ref):
    """A reference whose per-image pose gradients are summed: what a pose shared by the images of a batch receives."""
    return dict(ref, g_c2w=ref["g_c2w"].sum(dim=0, keepdim=True))


# ---- render-derived cases ----------------------------------------------------------------------------------------------
def bias_weights(sign, seed=0, t=T_BIAS):
    """-> w1 [6,12], w2 [3,6] (fp32): W1[:, 6:9] . t = sign x (+3, -3, +3, -3, +3, -3) -- the smallest change to a 0.25 randn
    draw that makes it so --, the other columns of W1 0.25 randn, W2 0.5 randn."""
    g = torch.Generator().manual_seed(4000 + seed)
    w1 = 0.25 * torch.randn(6, 12, generator=g, dtype=torch.float64)
    w2 = 0.5 * torch.randn(3, 6, generator=g, dtype=torch.float64)
    t = torch.tensor(t, dtype=torch.float64)
    target = sign * torch.tensor([3.0, -3.0, 3.0, -3.0, 3.0, -3.0], dtype=torch.float64)
    w1[:, 6:9] += ((target - w1[:, 6:9] @ t) / (t @ t))[:, None] * t
    return w1.float(), w2.float()


def rendered_case(name, img, alphas, intr, c2w, w1, w2, seed):
    """A case on a composited image: img [C,H,W,10] and alphas [C,H,W] or [C,H,W,1] (fp32, as the compositor returned them),
    intr [C | 1, 4], c2w [C | 1, 3 | 4, 4].  Cotangents on rgb and depth only; the depth cotangent is 0 where alpha < 0.05
    ("holes": no splat, or a sliver of one -- g / alpha there would become the scale of channel 9's comparison).  No pixel is
    excluded or redrawn: margin and z_max are what the image gives, for the caller to assert."""
    C, H, W, CF = img.shape
    P = H * W
    g = torch.Generator().manual_seed(5000 + seed)
    alphas = alphas.reshape(C, P).clone()
    hole = alphas < ALPHA_MIN
    scale = torch.tensor(COT_SCALES[:C])
    v_rgb = torch.randn(C, 3, P, generator=g) * scale[:, None, None]
    v_depth = torch.randn(C, P, generator=g) * scale[:, None] * (~hole)
    case = SimpleNamespace(name=name, P=P, H=H, W=W, C=C, CF=CF, has_depth=True, ray="pin44" if c2w.shape[-2] == 4 else "pin34",
                           feat=img.reshape(C, P, CF).clone(), alphas=alphas, hole=hole, w1=w1.clone(), w2=w2.clone(), rays=None,
                           intr=intr.reshape(-1, 4).clone(), c2w=c2w.reshape(-1, c2w.shape[-2], 4).clone(), v_rgb=v_rgb,
                           v_depth=v_depth, redrawn=0.0)
    s, z = pre_activations(case)
    case.margin, case.z_max = float(s.abs().min()), float(z.abs().max())
    case.signs = torch.sign(s).amin(dim=(0, 2)), torch.sign(s).amax(dim=(0, 2))   # per unit: equal = one branch everywhere
    return case


# ---- launch geometry, restated for tests/test_decoder_cases_cpu.py -------------------------------------------------------
BATCH = (3, 769)   # images, pixels per image of the batched cases
# name -> width, height, static + dynamic splats, cameras
FUSED_GRIDS = {"tiny": (37, 21, 200, 100, 1), "small": (250, 170, 4000, 2000, 1), "large": (728, 712, 4000, 2000, 1),
               "cams": (250, 170, 4000, 2000, 3)}


def bwd_rows(P):
    """Partial rows (workgroups) of the stand-alone backward per image: decoder_grid of csrc/decoder.hip."""
    return min(4096, max(1, -(-P // 768)))


def tiles(W, H):
    """16 x 16 tiles across and down: the fused backward leaves one partial row per (camera, tile)."""
    return -(-W // 16), -(-H // 16)
