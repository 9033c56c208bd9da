"""A camera with the reference's read-side interface and nothing else, and the float64 truth of the gradients that reach
its ray map (tests/test_gpu_reference_cameras.py on the device, tests/test_reference_cameras_cpu.py without one).

`RefCamera` carries exactly the attributes mobgs_amd/camera.py's docstring lists -- world_view_transform, K, time, max_time,
image_width, image_height, cam_ray [1,6,H,W], get_pixels() -- so gaussian_renderer._rays_of() hands the decoder its MAP and
_rays_of_many() returns None: the arm the reference's own scene.cameras.Camera takes.

Truth for the map's gradient is oracle/render_torch.render on the CPU in float64 on the same camera cast to double.  Two
fp32 evaluations cannot be compared with it at a pixel whose float64 walk sits at a discrete decision, so such pixels are
left out; which ones is decided by the two oracles alone (no device result enters):

  * blend decisions, per (pixel, splat) pair the float64 walk evaluates (tests/raster_cases.py's statements): 255 raw or
    raw / 0.999 within MARGIN_MULT = 8 x B_a of 1, or the inclusive transmittance of a passing pair within 8 x B_t of the
    1e-4 stop.  B_a and B_t are first-order bounds PER PAIR of an fp32 evaluation's relative error, built from the fp32
    oracle's own projection error of that splat and the roundings of the walk (_decisions); the fp32 oracle is checked
    to stay inside them on every pair (tests/test_reference_cameras_cpu.py).  A flat margin from the oracle's worst pair --
    an ill-conditioned conic, 1e-5 off -- would leave out 3 - 5 % of the pixels;
  * ReLU kinks of the decoder: a hidden unit j with |y_j| < KINK_MULT x tau_f x sum_c |W1[j, c]| over the six feature
    columns c, where tau_f -- the feature tolerance -- is DESIGN.md 3a's rule applied to the composited features: 3 x the
    fp32 oracle's distance from float64 on the pixels that pass the first filter, at least 8 x 2^-24 of the largest
    feature.  KINK_MULT = 4.  (The rays enter both oracles and the kernel as the same fp32 numbers: no term for them.)

A train-mode render decodes three images (all, static, dynamic) whose ray gradients add into the one map: a pixel is left
out when any of the three walks or decodes flags it.  CAP_ORACLE (0.5 %) bounds the share on the oracles alone."""
import functools

import numpy as np
import torch

import raster_cases as RC
from mobgs_amd.camera import PinholeCamera

CAMERA_ATTRIBUTES = ("world_view_transform", "K", "time", "max_time", "image_width", "image_height", "cam_ray", "get_pixels")
PINHOLE_ONLY = ("ray_c2w", "ray_intrinsics", "_w2c")

SIZES = ((80, 64), (50, 37))   # 50 x 37: ragged tiles both ways, a pixel stride of the map that is no multiple of 16
MODES = ("lean", "train")
MARGIN_MULT = 2
# seeds of gaussian_cloud for the static / the dynamic set: the first of six pairs tried -- (0, 1), (2, 3) .. (10, 11) --
# with which all four cases leave out less than CAP_ORACLE (0.11 .. 0.43 %; the others reach 0.59 .. 1.03 % in one case)
SCENE_SEEDS = (10, 11)
KINK_MULT = 4
CAP_EXCLUDED, CAP_ORACLE = 0.01, 0.005
FLOOR = 8.0 * 2.0 ** -24


class RefCamera:
    def __init__(self, image_width, image_height, K, world_view_transform, time, max_time, cam_ray):
        self.image_width = int(image_width)
        self.image_height = int(image_height)
        self.K = K
        self.world_view_transform = world_view_transform
        self.time = float(time)
        self.max_time = max_time
        self.cam_ray = cam_ray

    def get_pixels(self, image_size_x, image_size_y, use_center=None):
        xx, yy = np.meshgrid(np.arange(image_size_x, dtype=np.float32), np.arange(image_size_y, dtype=np.float32))
        return np.stack([xx, yy], axis=-1) + (0.5 if use_center else 0)


def ref_camera(pin, pose_leaf=False, ray_leaf=False):
    """-> (RefCamera with the values of the PinholeCamera `pin`, the leaf or None).
    pose_leaf: the map is built by PinholeCamera.build_cam_ray_c2w from a c2w [3,4] leaf that requires grad -- a non-leaf
    with a graph, as the maps of the reference's warped cameras are; the leaf is returned, the camera does not hold it.
    ray_leaf: the map itself is a leaf that requires grad (and is what is returned)."""
    assert not (pose_leaf and ray_leaf)
    W, H = pin.image_width, pin.image_height
    leaf = None
    if pose_leaf:
        leaf = torch.inverse(pin._w2c)[:3, :].detach().clone().requires_grad_(True)
        ray = PinholeCamera.build_cam_ray_c2w(W, H, pin.K, leaf)
    else:
        ray = PinholeCamera.build_cam_ray(W, H, pin.K, pin._w2c)   # the reference's formula
        if ray_leaf:
            leaf = ray = ray.detach().clone().requires_grad_(True)
    return RefCamera(W, H, pin.K, pin.world_view_transform, pin.time, pin.max_time, ray), leaf


def cast_camera(cam, dtype, device="cpu", ray_requires_grad=False):
    """The same camera with its tensors cast (the map: the SAME numbers, detached; optionally a leaf)."""
    ray = cam.cam_ray.detach().to(device=device, dtype=dtype).clone().requires_grad_(ray_requires_grad)
    return RefCamera(cam.image_width, cam.image_height, cam.K.detach().to(device=device, dtype=dtype),
                     cam.world_view_transform.detach().to(device=device, dtype=dtype), cam.time, cam.max_time, ray)


def ray_map_from_c2w(width, height, K, c2w):
    """PinholeCamera.build_cam_ray_c2w statement by statement in c2w's dtype (that function draws its pixel grid in fp32)."""
    dt = c2w.dtype
    ys, xs = torch.meshgrid(torch.arange(height, dtype=dt), torch.arange(width, dtype=dt), indexing="ij")
    K = K.to(dt)
    x = (xs + 0.5 - K[0, 2]) / K[0, 0]
    y = (ys + 0.5 - K[1, 2]) / K[1, 1]
    local = torch.stack([x, y, torch.ones_like(x)], dim=-1)
    dirs = local @ c2w[:3, :3].transpose(0, 1)
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    ray = torch.cat([c2w[:3, 3].expand_as(dirs), dirs], dim=-1)
    return ray.permute(2, 0, 1).unsqueeze(0).contiguous()


# ---- the scene of tests/test_gpu_tto.py ---------------------------------------------------------------------------------
def scene(device, W, H, dtype=torch.float32):
    """gaussian_cloud(1500) + gaussian_cloud(700), Sandwich(9, 3) seeded 0 -> (SynthCamera, stat, dyn), all leaves."""
    from mobgs_amd.gaussian_model import GaussianParams
    from mobgs_amd.helper_model import Sandwich
    from mobgs_amd.synth import SynthCamera, dynamic_extras, gaussian_cloud
    scam = SynthCamera().scaled(W, H)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        dec = Sandwich(9, 3)
    dec = dec.to(device=device, dtype=dtype)
    stat_p, dyn_p = gaussian_cloud(1500, scam, SCENE_SEEDS[0]), gaussian_cloud(700, scam, SCENE_SEEDS[1])
    dyn_x = dynamic_extras(dyn_p["xyz"], SCENE_SEEDS[0])

    def cast(d):
        return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in d.items()}

    stat = GaussianParams(cast(stat_p), None, dec, device, requires_grad=True, attr_dtype=dtype)
    dyn = GaussianParams(cast(dyn_p), cast(dyn_x), dec, device, requires_grad=True, attr_dtype=dtype)
    return scam, stat, dyn


def pose(k=0):
    """World-to-camera matrix k: a rotation about an oblique axis and a shift, both growing with k."""
    a = 0.06 + 0.05 * k
    axis = torch.tensor([0.3, 1.0, -0.2 + 0.3 * k], dtype=torch.float64)
    axis = axis / axis.norm()
    kx = torch.tensor([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]], dtype=torch.float64)
    rot = torch.eye(3, dtype=torch.float64) + np.sin(a) * kx + (1.0 - np.cos(a)) * (kx @ kx)
    m = torch.eye(4, dtype=torch.float64)
    m[:3, :3] = rot
    m[:3, 3] = torch.tensor([0.05 - 0.04 * k, 0.03 * k - 0.02, 0.1 + 0.02 * k], dtype=torch.float64)
    return m.float()


def pinhole(scam, W, H, device, k=0):
    return PinholeCamera(W, H, scam.K, pose(k), scam.time, scam.max_time, device=device)


def cotangents(W, H, seed=7):
    g = torch.Generator().manual_seed(seed)
    return {"render": torch.randn(3, H, W, generator=g), "depth": torch.randn(1, H, W, generator=g),
            "s_render": torch.randn(3, H, W, generator=g), "d_render": torch.randn(3, H, W, generator=g)}


def loss_of(out, cot, train):
    """Lean: the decoded image and the depth; train mode: the static-only and dynamic-only decodes as well."""
    c = {k: v.to(device=out["render"].device, dtype=out["render"].dtype) for k, v in cot.items()}
    loss = (out["render"] * c["render"]).sum() + (out["depth"].reshape(c["depth"].shape) * c["depth"]).sum()
    if train:
        loss = loss + (out["s_render"] * c["s_render"]).sum() + (out["d_render"] * c["d_render"]).sum()
    return loss


def tolerance(gap, ref):
    """3 x the fp32 oracle's own distance from float64, not less than 8 x 2^-24 of the largest entry."""
    return max(3.0 * float(gap), FLOOR * float(torch.as_tensor(ref).abs().max()))


# ---- the two oracles ------------------------------------------------------------------------------------------------------
_META = ("radii", "means2d", "depths", "conics", "opacities")


def _oracle_run(W, H, train, dtype):
    """oracle/render_torch.render of the case in `dtype` -> (d loss / d map [H*W,6], d loss / d c2w [3,4], the feature
    images and projections of its 9-feature passes, w1, the map)."""
    from oracle import gsplat_torch as G
    from oracle import render_torch as R
    scam, stat, dyn = scene("cpu", W, H, dtype)
    pin = pinhole(scam, W, H, "cpu")
    cam32, c2w32 = ref_camera(pin, pose_leaf=True)
    cam = cast_camera(cam32, dtype, ray_requires_grad=True)
    seen = []

    def rasterization(**kw):
        img, alphas, meta = G.rasterization(**kw)
        if kw["render_mode"] == "RGB+ED" and kw["colors"].shape[-1] == 9:
            seen.append((img.detach()[0, ..., :9].reshape(H * W, 9), {k: meta[k].detach() for k in _META}))
        return img, alphas, meta

    out = R.render(cam, stat, dyn, torch.zeros(9, dtype=dtype), get_static=train, get_dynamic=train,
                   rasterization=rasterization)
    loss_of(out, cotangents(W, H), train).backward()
    v_map = cam.cam_ray.grad
    # the pose behind the map: the chain rule through the map's construction, in this dtype, at the same c2w
    c2w = c2w32.detach().to(dtype).requires_grad_(True)
    build = ray_map_from_c2w if dtype == torch.float64 else PinholeCamera.build_cam_ray_c2w
    g_c2w, = torch.autograd.grad(build(W, H, pin.K.to(dtype), c2w), c2w, grad_outputs=v_map)
    w1 = dyn.rgbdecoder.mlp1.weight.detach().reshape(6, 12)
    return (v_map[0].permute(1, 2, 0).reshape(H * W, 6).detach(), g_c2w.detach(), seen, w1,
            cam.cam_ray.detach()[0].permute(1, 2, 0).reshape(H * W, 6))


U = 2.0 ** -24


def _decisions(m64, m32, W, H, chunk=1024):
    """The float64 walk over one pass's own lists -> (bool [H*W]: the pixel evaluates a pair that sits at a decision, the
    fp32 oracle's largest observed error / bound of raw and of T over the pairs: both must stay <= 1).

    Per (pixel, splat) pair, B_a bounds the relative error of an fp32 raw = op exp(-sigma) to first order: the fp32 oracle's
    own projection error of that splat (conic entries dc, centre dm, opacity) carried through sigma's statement,
    |d sigma| <= dc . (dx^2/2, |dx dy|, dy^2/2) + (|a dx| + |b dy|) dm_x + (|c dy| + |b dx|) dm_y, plus 8 u S for the
    roundings of the evaluation itself (S: the sum of sigma's terms in magnitude) and 4 u for exp and the product.  B_t, the same for the
    inclusive transmittance: sum over the passing pairs so far of alpha B_a / (1 - alpha), plus 2 u each.  A pair sits at a
    decision when 255 raw or raw / 0.999 is within MARGIN_MULT x B_a of 1, or a passing pair's T / 1e-4 within MARGIN_MULT
    x B_t of 1."""
    idx = RC._order(m64["depths"][0], m64["radii"][0], None)
    idx = idx[m32["radii"][0][idx] > 0]
    flagged = torch.zeros(H * W, dtype=torch.bool)
    if idx.numel() == 0:
        return flagged, 0.0, 0.0
    px, py = RC._pixels(W, H, torch.float64)
    inside = RC._in_rect(m64["means2d"][0, idx], m64["radii"][0, idx], W, H)
    m, con, op = (m64[k][0, idx] for k in ("means2d", "conics", "opacities"))
    m32_, con32, op32 = (m32[k][0, idx] for k in ("means2d", "conics", "opacities"))
    dm, dc, dop = (m32_.double() - m).abs(), (con32.double() - con).abs(), ((op32.double() - op) / op).abs()
    worst_a = worst_t = 0.0
    for s in range(0, H * W, chunk):
        e = min(H * W, s + chunk)
        sigma, raw, alpha = RC._pairs(m, con, op, px[s:e], py[s:e])
        valid, T_incl, done, _ = RC._decide(sigma, alpha, inside[s:e])
        before = torch.cat([torch.zeros_like(done[:, :1]), done[:, :-1]], dim=1)
        ev = inside[s:e] & ~before
        vt = ev & valid
        dx, dy = (m[None, :, 0] - px[s:e, None]).abs(), (m[None, :, 1] - py[s:e, None]).abs()
        a, b, c = con[None, :, 0], con[None, :, 1].abs(), con[None, :, 2]
        S = 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy
        B_a = 0.5 * (dc[None, :, 0] * dx * dx + dc[None, :, 2] * dy * dy) + dc[None, :, 1] * dx * dy \
            + (a * dx + b * dy) * dm[None, :, 0] + (c * dy + b * dx) * dm[None, :, 1] + dop[None, :] + 8 * U * S + 4 * U
        # (a clamped alpha is the constant 0.999 on both sides: no error of its own)
        B_t = torch.cumsum(torch.where(vt & (raw < RC.ALPHA_MAX), alpha * B_a / (1 - alpha), torch.zeros_like(B_a))
                           + torch.where(vt, 2 * U, 0.0), dim=1)
        # the fp32 oracle's own pairs (its projection, its arithmetic) against the bounds
        _, raw32, alpha32 = RC._pairs(m32_, con32, op32, px[s:e].float(), py[s:e].float())
        T32 = torch.cumprod(1 - torch.where(valid, alpha32, torch.zeros_like(alpha32)), dim=1)
        big = ev & (raw >= RC.RAW_FLOOR)
        if bool(big.any()):
            worst_a = max(worst_a, float((((raw32.double() - raw) / raw).abs() / B_a)[big].max()))
        if bool(vt.any()):
            worst_t = max(worst_t, float((((T32.double() - T_incl) / T_incl).abs() / B_t)[vt].max()))
        near = torch.minimum((255.0 * raw - 1.0).abs(), (raw / RC.ALPHA_MAX - 1.0).abs())
        flagged[s:e] = (ev & (near < MARGIN_MULT * B_a)).any(dim=1) | \
            (vt & ((T_incl / RC.T_STOP - 1.0).abs() < MARGIN_MULT * B_t)).any(dim=1)
    return flagged, worst_a, worst_t


@functools.lru_cache(maxsize=None)
def oracle_case(size, mode):
    """Both oracles on case (size, mode), once per process -> dict: the float64 and fp32 gradients of the map [H*W,6] and of
    c2w [3,4], `keep` [H*W] (the pixels compared), the share left out, and the allowed distances `tol_map`, `tol_c2w` with the
    fp32 oracle's own `gap_map`, `gap_c2w` they come from."""
    W, H = size
    train = mode == "train"
    v64, g64, seen64, w1, rays = _oracle_run(W, H, train, torch.float64)
    v32, g32, seen32, _, _ = _oracle_run(W, H, train, torch.float32)
    assert len(seen64) == len(seen32) == (3 if train else 1)
    out = torch.zeros(H * W, dtype=torch.bool)
    res = {"worst_a": 0.0, "worst_t": 0.0, "tau_f": 0.0}
    flagged = []
    for (f64, m64), (f32, m32) in zip(seen64, seen32):
        decision, worst_a, worst_t = _decisions(m64, m32, W, H)
        tau_f = tolerance((f32.double() - f64).abs()[~decision].max(), f64)
        y = torch.cat([f64[:, 3:9], rays], dim=1) @ w1.t()                       # [P,6] pre-activations
        kink = (y.abs() < KINK_MULT * tau_f * w1[:, :6].abs().sum(1)[None, :]).any(dim=1)
        flagged.append((int(decision.sum()), int(kink.sum())))
        out |= decision | kink
        res["worst_a"], res["worst_t"] = max(res["worst_a"], worst_a), max(res["worst_t"], worst_t)
        res["tau_f"] = max(res["tau_f"], tau_f)
    keep = ~out
    gap_map = float((v32.double() - v64)[keep].abs().max())
    gap_c2w = float((g32.double() - g64).abs().max())
    res.update(size=size, mode=mode, keep=keep, excluded=float(out.float().mean()), flagged=flagged,
               map64=v64, map32=v32, c2w64=g64, c2w32=g32, gap_map=gap_map, gap_c2w=gap_c2w,
               tol_map=tolerance(gap_map, v64[keep]), tol_c2w=tolerance(gap_c2w, g64))
    return res


NINE = [(k - 4) / 4.0 for k in range(9)]   # train.py:570-573: exposure_max_delta (k - half) / half, 0.0 among them


def flow_weights(W, H, seed=5):
    """Per exposure the cotangents of get_flow()'s four maps (exp2mid, mid2exp, latent image, latent coverage)."""
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(*s, generator=g) for s in ((1, H, W, 2), (1, H, W, 2), (3, H, W), (1, H, W))] for _ in NINE]


@functools.lru_cache(maxsize=None)
def oracle_flow_pose_case(size):
    """The c2w gradient of a loss over the nine get_flow() calls of a view, in float64 and in fp32.  Of get_flow()'s four maps
    only the latent image reads the rays, and it is the lean render at that exposure offset (same splats, same features, same
    background, same decoder): nine oracle/render_torch.render calls per dtype instead of nine get_flow restatements with
    their four rasterizations each.  -> dict(c2w64, c2w32, gap, tol)."""
    from oracle import render_torch as R
    W, H = size
    ws = flow_weights(W, H)
    g = {}
    for dtype in (torch.float64, torch.float32):
        scam, stat, dyn = scene("cpu", W, H, dtype)
        pin = pinhole(scam, W, H, "cpu")
        c2w = torch.inverse(pin._w2c)[:3, :].to(dtype).requires_grad_(True)
        build = ray_map_from_c2w if dtype == torch.float64 else PinholeCamera.build_cam_ray_c2w
        # (the fp32 map's numbers on both sides, a leaf; the pose behind it by the chain rule as in _oracle_run)
        ray32 = PinholeCamera.build_cam_ray_c2w(W, H, pin.K, c2w.detach().float())
        cam = RefCamera(W, H, pin.K.to(dtype), pin.world_view_transform.to(dtype), pin.time, pin.max_time,
                        ray32.to(dtype).requires_grad_(True))
        loss = sum((R.render(cam, stat, dyn, torch.zeros(9, dtype=dtype), delta_exposure=d)["render"] * w[2].to(dtype)).sum()
                   for d, w in zip(NINE, ws))
        loss.backward()
        g[dtype], = torch.autograd.grad(build(W, H, pin.K.to(dtype), c2w), c2w, grad_outputs=cam.cam_ray.grad)
    gap = float((g[torch.float32].double() - g[torch.float64]).abs().max())
    return dict(c2w64=g[torch.float64], c2w32=g[torch.float32], gap=gap, tol=tolerance(gap, g[torch.float64]))


def report(tag, case, observed_map=None, observed_c2w=None):
    """One line per case: what is observed next to what the fp32 oracle does and what is allowed."""
    o = lambda v: "-" if v is None else f"{v:.3e}"   # noqa: E731
    print(f"[refcam] {tag} {case['size'][0]}x{case['size'][1]} {case['mode']}: left out {case['excluded']:.2%} "
          f"(decision, kink pixels per decode {case['flagged']}; fp32 oracle / pair bound: raw {case['worst_a']:.2f}, "
          f"T {case['worst_t']:.2f}; tau_f {case['tau_f']:.1e}); map gradient: observed {o(observed_map)}, fp32 oracle "
          f"{case['gap_map']:.3e}, allowed "
          f"{case['tol_map']:.3e} (largest {float(case['map64'].abs().max()):.3e}); c2w gradient: observed "
          f"{o(observed_c2w)}, fp32 oracle {case['gap_c2w']:.3e}, allowed {case['tol_c2w']:.3e} "
          f"(largest {float(case['c2w64'].abs().max()):.3e})")
