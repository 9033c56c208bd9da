"""The report sheets in numpy float64: every panel kind of mobgs_report_compose and flow_vis.flow_to_color, restated from
the reference's statements (utils/scene_utils.py:94-104, :130-163, :177-188, :196-212) and, for the colour wheel, from
memory of the flow_vis package (UNPINNED, README).  Not a copy of either.

Every function returns the float64 value x BEFORE the 8-bit conversion; to_bytes(x) = floor(clip(x, 0, 1) * 255) is the
reference's (np.clip(x, 0, 1) * 255).astype('uint8'), and level(x) = 255 * clip(x, 0, 1) is the number whose distance to
an integer decides whether an fp32 evaluation may land one level off (tests/report_cases.py).
"""
import numpy as np

SEGMENTS = (("RY", 15), ("YG", 6), ("GC", 4), ("CB", 11), ("BM", 13), ("MR", 6))
NCOLS = 55


def wheel():
    """[55, 3] integers 0 .. 255.  Segment s runs from one primary / secondary colour to the next: RY red -> yellow (green
    rises), YG (red falls), GC (blue rises), CB (green falls), BM (red rises), MR (blue falls).  Rising: floor(255 i / L);
    falling: 255 - floor(255 i / L); the third channel keeps what the previous segment left it at."""
    rising = {"RY": 1, "GC": 2, "BM": 0}
    falling = {"YG": 0, "CB": 1, "MR": 2}
    full = {"RY": 0, "YG": 1, "GC": 1, "CB": 2, "BM": 2, "MR": 0}
    w = np.zeros((NCOLS, 3), dtype=np.int64)
    k = 0
    for name, L in SEGMENTS:
        for i in range(L):
            w[k, full[name]] = 255
            if name in rising:
                w[k, rising[name]] = (255 * i) // L
            else:
                w[k, falling[name]] = 255 - (255 * i) // L
            k += 1
    assert k == NCOLS
    return w


def level(x):
    return 255.0 * np.clip(np.asarray(x, dtype=np.float64), 0.0, 1.0)


def to_bytes(x):
    return np.floor(level(x)).astype(np.uint8)


def hwc(a):
    """[C,H,W] -> float64 [H,W,C]"""
    return np.asarray(a, dtype=np.float64).transpose(1, 2, 0)


def rgb(a):
    return hwc(a)


def grey(a):
    return np.repeat(hwc(np.asarray(a).reshape(1, *np.asarray(a).shape[-2:])), 3, axis=2)


def grey_div_max(a):
    """x / max(x); where the maximum is 0 the panel is 0 (the reference divides by zero there)."""
    g = grey(a)
    m = g.max()
    return np.zeros_like(g) if m == 0 else g / m


def error(image, gt):
    e = (hwc(image) - hwc(gt)) ** 2
    return (e - e.min()) / max(e.max() - e.min(), 1e-8)


def signed3(a):
    return (hwc(a) + 1.0) / 2.0


def view_dirs(H, W, cam):
    """cam = (focal, cx, cy, skew, offset): ((px - cx - y skew) / focal, y = (py - cy) / focal, 1), one focal length."""
    focal, cx, cy, skew, offset = (float(c) for c in cam)
    py, px = np.meshgrid(np.arange(H, dtype=np.float64) + offset, np.arange(W, dtype=np.float64) + offset, indexing="ij")
    y = (py - cy) / focal
    x = (px - cx - y * skew) / focal
    return np.stack([x, y, np.ones_like(x)], axis=0)


def normals_fd(depth, cam):
    """The sheet's own normals: z = depth + 1e-6, camera-frame points dirs * z, forward differences along u and v with the
    last column / row replicated, cross product (dv x du as the reference writes it), unit length with eps 1e-12,
    (n + 1) / 2."""
    z = np.asarray(depth, dtype=np.float64).reshape(np.asarray(depth).shape[-2:]) + 1e-6
    H, W = z.shape
    if H < 2 or W < 2:
        raise ValueError("normals_fd needs H >= 2 and W >= 2")
    p = view_dirs(H, W, cam) * z[None]
    du = p[:, :, 1:] - p[:, :, :-1]
    du = np.concatenate([du, du[:, :, -1:]], axis=2)
    dv = p[:, 1:, :] - p[:, :-1, :]
    dv = np.concatenate([dv, dv[:, -1:, :]], axis=1)
    n = np.stack([dv[1] * du[2] - du[1] * dv[2], dv[2] * du[0] - du[2] * dv[0], dv[0] * du[1] - du[0] * dv[1]], axis=0)
    n = n / np.maximum(np.sqrt((n ** 2).sum(0, keepdims=True)), 1e-12)
    return (n.transpose(1, 2, 0) + 1.0) / 2.0


def flow_uv_to_colors(u, v):
    """Normalised u, v -> float64 colour [H,W,3] in 0 .. 1 (the byte is floor(255 col)).  With the `* 0.75` arm for a
    radius above 1, which flow_to_color's normalisation makes unreachable."""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    w = wheel().astype(np.float64)
    rad = np.sqrt(u * u + v * v)
    a = np.arctan2(-v, -u) / np.pi
    fk = (a + 1.0) / 2.0 * (NCOLS - 1)
    k0 = np.floor(fk).astype(np.int64)
    k1 = np.where(k0 + 1 == NCOLS, 0, k0 + 1)
    f = fk - k0
    out = np.empty(u.shape + (3,), dtype=np.float64)
    for c in range(3):
        # (1 - f) c0 + f c1, written so that it is exact where both entries agree: on a channel that the two entries
        # hold at 255 the package (float64 wheel, float32 f) returns exactly 1, and so must this
        col = w[k0, c] / 255.0 + f * (w[k1, c] / 255.0 - w[k0, c] / 255.0)
        out[..., c] = np.where(rad <= 1.0, 1.0 - rad * (1.0 - col), col * 0.75)
    return out


def flow(flow_uv, clip_flow=None):
    """flow_to_color(flow, clip_flow, convert_to_bgr=False) before the truncation: float64 [H,W,3]."""
    f = np.asarray(flow_uv, dtype=np.float64)
    if clip_flow is not None:
        f = np.clip(f, 0.0, clip_flow)
    u, v = f[..., 0], f[..., 1]
    rad_max = np.sqrt(u * u + v * v).max()
    return flow_uv_to_colors(u / (rad_max + 1e-5), v / (rad_max + 1e-5))


def flow_to_color(flow_uv, clip_flow=None, convert_to_bgr=False):
    img = to_bytes(flow(flow_uv, clip_flow))
    return img[..., ::-1] if convert_to_bgr else img


def panel(kind, a, b=None, cam=None, clip=None):
    if kind == "RGB":
        return rgb(a)
    if kind == "GREY":
        return grey(a)
    if kind == "GREY_DIV_MAX":
        return grey_div_max(a)
    if kind == "ERROR":
        return error(a, b)
    if kind == "SIGNED3":
        return signed3(a)
    if kind == "NORMALS_FD":
        return normals_fd(a, cam)
    if kind == "FLOW":
        return flow(a, clip)
    raise ValueError(kind)


def sheet(panels, cam=None):
    """panels: (kind, a[, b[, clip]]) -> float64 [H, P W, 3], the panels side by side."""
    return np.concatenate([panel(p[0], p[1], p[2] if len(p) > 2 else None, cam, p[3] if len(p) > 3 else None)
                           for p in panels], axis=1)


def image_panels(case, r):
    """The image sheet of a view (scene_utils.py:200-210).  case: "test" | "train" | "train_blur"; r: the render outputs
    and targets by name."""
    if case == "test":
        return [("RGB", r["gt"]), ("RGB", r["render"]), ("ERROR", r["render"], r["gt"]), ("GREY", r["d_alpha"]),
                ("RGB", r["d_render"]), ("RGB", r["s_render"])]
    if case == "train":
        return [("RGB", r["gt"]), ("RGB", r["render"]), ("GREY", r["d_alpha"]), ("RGB", r["d_render"]),
                ("RGB", r["s_render"])]
    if case == "train_blur":
        return [("RGB", r["gt"]), ("RGB", r["blurry"]), ("RGB", r["render"]), ("GREY", r["d_alpha"])]
    raise ValueError(case)


def decomp_panels(case, r):
    if case == "test":
        return [("NORMALS_FD", r["depth"]), ("GREY_DIV_MAX", r["depth"])]
    return [("SIGNED3", r["gt_normal"]), ("NORMALS_FD", r["depth"]), ("GREY_DIV_MAX", r["gt_depth"]),
            ("GREY_DIV_MAX", r["depth"])]
