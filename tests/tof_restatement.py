"""The temporal optical-flow metric in numpy float64, written for reading: one function per stage of csrc/tof.hip
(include/mobgs_hip.h K25), each taking the stage's own input.  It restates cv2.calcOpticalFlowFarneback(prev, next, None,
0.5, 3, 15, 3, 5, 1.2, 0) from memory of OpenCV's optflowgf.cpp -- OpenCV could not be run where this was written (README,
"UNPINNED") -- and the reference's metrics.py:14-47, :100-110.  x = column; flow[..., 0] = u along x, prev to next.

Nothing here is fitted to the kernels: tests/test_tof_cpu.py checks it against facts that need no OpenCV (an exact
quadratic, an analytically translated texture), tests/test_gpu_tof.py checks the kernels against it."""
import numpy as np

PYR_SCALE, LEVELS, WINSIZE, ITERATIONS, POLY_N, POLY_SIGMA = 0.5, 3, 15, 3, 5, 1.2
MIN_SIZE = 32
BORDER = (0.14, 0.14, 0.4472, 0.4472, 0.4472)


# ---- 8-bit grey --------------------------------------------------------------------------------------------------------

def quantize8(x):
    """eval.py:162 and metrics.py:100: the written PNG read back, floor(clip(x) * 255) / 255, every step in fp32."""
    x = np.clip(np.asarray(x, np.float32), np.float32(0), np.float32(1))
    return np.floor(x * np.float32(255)) / np.float32(255)


def to_uint8(x):
    """metrics.py:109-110, (img * 255.0).astype(np.uint8) on a float32 image: the product is rounded to fp32, then truncated
    (saturated here; the reference's images are in [0, 1])."""
    t = np.trunc(np.asarray(x, np.float32) * np.float32(255.0))
    return np.clip(t, 0, 255).astype(np.uint8)


def round_trip_table():
    """k -> what the reference's grey conversion sees for the 8-bit value k of a PNG: np.float32(k) / 255 * 255.0, truncated."""
    return to_uint8(np.arange(256, dtype=np.float32) / np.float32(255))


def rgb_to_grey(rgb8):
    """OpenCV's 8-bit COLOR_RGB2GRAY: [...,3,H,W] uint8 -> [...,H,W] uint8, fixed point with 14 fractional bits."""
    c = rgb8.astype(np.int64)
    return ((4899 * c[..., 0, :, :] + 9617 * c[..., 1, :, :] + 1868 * c[..., 2, :, :] + 8192) >> 14).astype(np.uint8)


def grey(rgb, clamp=False, quantize=False):
    """[...,3,H,W] float32 -> [...,H,W] float64 holding 8-bit values."""
    x = np.asarray(rgb, np.float32)
    if clamp:
        x = np.clip(x, np.float32(0), np.float32(1))
    if quantize:
        x = quantize8(x)
    return rgb_to_grey(to_uint8(x)).astype(np.float64)


# ---- crop_8x8 ------------------------------------------------------------------------------------------------------------

def crop_window(H, W):
    """metrics.py:32-47 -> (y, x, h, w)."""
    h, w = (H // 32) * 32, (W // 32) * 32
    while h > H - 16:
        h -= 32
    while w > W - 16:
        w -= 32
    return (H - h) // 2, (W - w) // 2, h, w


def crop_8x8(a):
    y, x, h, w = crop_window(a.shape[0], a.shape[1])
    return a[y:y + h, x:x + w]


# ---- pyramid -------------------------------------------------------------------------------------------------------------

def levels(H, W):
    """[(width, height, taps, sigma)], coarsest first.  np.rint rounds half to even, as cvRound does."""
    scale, k = 1.0, 0
    while k < LEVELS:
        scale *= PYR_SCALE
        if W * scale < MIN_SIZE or H * scale < MIN_SIZE:
            break
        k += 1
    out = []
    for kk in range(k, -1, -1):
        s = PYR_SCALE ** kk
        sigma = (1.0 / s - 1.0) * 0.5
        taps = max(int(np.rint(sigma * 5)) | 1, 3)
        out.append((int(np.rint(W * s)), int(np.rint(H * s)), taps, sigma))
    return out


def gaussian_taps(taps, sigma):
    """cv::getGaussianKernel: a fixed table for sigma <= 0 and 3 taps, else exp(-t^2 / (2 sigma^2)) normalised to sum 1."""
    if sigma <= 0:
        assert taps == 3
        return np.array([0.25, 0.5, 0.25])
    t = np.arange(taps) - taps // 2
    g = np.exp(-t * t / (2.0 * sigma * sigma))
    return g / g.sum()


def correlate_axis(a, taps, axis, mode, dtype=np.float64):
    """sum_k taps[k] a[i + k - r] along `axis`, the border filled by np.pad's `mode` ('reflect' = OpenCV's reflect-101,
    'edge' = replicate).  Image, taps and the running sum are held in `dtype`."""
    a, taps = np.asarray(a, dtype), np.asarray(taps, dtype)
    r = len(taps) // 2
    pad = [(0, 0)] * a.ndim
    pad[axis] = (r, r)
    p = np.pad(a, pad, mode=mode)
    n = a.shape[axis]
    out = np.zeros_like(a, dtype=dtype)
    for k, t in enumerate(taps):
        out += t * np.take(p, np.arange(k, k + n), axis=axis)
    return out


def resize_taps(dst, src):
    """OpenCV's INTER_LINEAR: index and weight of the left tap of every destination index."""
    s = (np.arange(dst) + 0.5) * (src / dst) - 0.5
    i0 = np.floor(s).astype(np.int64)
    f = s - i0
    f[i0 < 0], i0[i0 < 0] = 0.0, 0
    f[i0 >= src - 1], i0[i0 >= src - 1] = 0.0, src - 1
    return i0, f


def resize_bilinear(a, h, w, dtype=np.float64):
    """[H,W,...] -> [h,w,...].  The weights are formed in float64 and rounded to `dtype`, which holds everything else."""
    a = np.asarray(a, dtype)
    y0, fy = resize_taps(h, a.shape[0])
    x0, fx = resize_taps(w, a.shape[1])
    fy, fx = fy.astype(dtype), fx.astype(dtype)
    y1, x1 = np.minimum(y0 + 1, a.shape[0] - 1), np.minimum(x0 + 1, a.shape[1] - 1)
    shape = (-1,) + (1,) * (a.ndim - 2)
    rows = a[y0] * (1 - fy).reshape((-1, 1) + shape[1:]) + a[y1] * fy.reshape((-1, 1) + shape[1:])
    return rows[:, x0] * (1 - fx).reshape((1,) + shape) + rows[:, x1] * fx.reshape((1,) + shape)


def pyramid_level(grey_full, level, dtype=np.float64):
    """The full-size grey image blurred (reflect-101) and resized to the level's size; the taps are rounded to `dtype`."""
    w, h, taps, sigma = level
    g = gaussian_taps(taps, sigma)
    blurred = correlate_axis(correlate_axis(np.asarray(grey_full, dtype), g, 1, "reflect", dtype), g, 0, "reflect", dtype)
    return resize_bilinear(blurred, h, w, dtype)


# ---- polynomial expansion ------------------------------------------------------------------------------------------------

def poly_exp(img, dtype=np.float64):
    """[h,w] -> [5,h,w] = (r_x, r_y, r_xx, r_yy, r_xy): per pixel the weighted least-squares fit of c + r_x x + r_y y + r_xx x^2
    + r_yy y^2 + r_xy xy over the 11x11 window, weight g(x) g(y), replicate border.  Solved as the 6x6 normal equations, as
    the definition reads; OpenCV (and the kernel) use the closed form those equations have for a separable even weight.
    The tables (basis, weight, Gram matrix) are formed in float64 and rounded to `dtype`, which holds the sums and the solve."""
    n = POLY_N
    t = np.arange(-n, n + 1, dtype=np.float64)
    g = np.exp(-t * t / (2.0 * POLY_SIGMA * POLY_SIGMA))
    g /= g.sum()
    X, Y = np.meshgrid(t, t)                                        # X varies along columns
    basis = np.stack([np.ones_like(X), X, Y, X * X, Y * Y, X * Y])  # [6,11,11]
    wgt = np.outer(g, g)
    gram = np.einsum("ayx,byx,yx->ab", basis, basis, wgt).astype(dtype)
    basis, wgt = basis.astype(dtype), wgt.astype(dtype)
    h, w = img.shape
    p = np.pad(np.asarray(img, dtype), n, mode="edge")
    rhs = np.zeros((6, h, w), dtype)
    for dy in range(2 * n + 1):
        for dx in range(2 * n + 1):
            rhs += (basis[:, dy, dx] * wgt[dy, dx])[:, None, None] * p[dy:dy + h, dx:dx + w]
    coef = np.linalg.solve(gram, rhs.reshape(6, -1)).reshape(6, h, w)
    return coef[1:]


# ---- update matrices -----------------------------------------------------------------------------------------------------

def border_factor(h, w):
    def side(n):
        s = np.ones(n)
        for d, t in enumerate(BORDER[:n]):       # (a side shorter than the band: both ends scale the same pixel)
            s[d] *= t
            s[n - 1 - d] *= t
        return s
    return np.outer(side(h), side(w))


def sample_positions(flow, dtype=np.float64):
    h, w = flow.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    return xs.astype(dtype) + flow[..., 0].astype(dtype), ys.astype(dtype) + flow[..., 1].astype(dtype)


def update_matrices(R0, R1, flow, dtype=np.float64):
    """R0, R1 [5,h,w], flow [h,w,2] -> M [5,h,w] = (G11, G12, G22, h1, h2), every statement in `dtype`."""
    h, w = flow.shape[:2]
    R0, R1 = np.asarray(R0, dtype), np.asarray(R1, dtype)
    u, v = flow[..., 0].astype(dtype), flow[..., 1].astype(dtype)
    fx, fy = sample_positions(flow, dtype)
    x1, y1 = np.floor(fx), np.floor(fy)
    inb = (x1 >= 0) & (x1 < w - 1) & (y1 >= 0) & (y1 < h - 1)
    xi, yi = np.where(inb, x1, 0).astype(np.int64), np.where(inb, y1, 0).astype(np.int64)
    ax, ay = fx - x1, fy - y1
    S = ((1 - ax) * (1 - ay) * R1[:, yi, xi] + ax * (1 - ay) * R1[:, yi, xi + 1]
         + (1 - ax) * ay * R1[:, yi + 1, xi] + ax * ay * R1[:, yi + 1, xi + 1])
    a_xx = np.where(inb, (R0[2] + S[2]) / 2, R0[2])
    a_yy = np.where(inb, (R0[3] + S[3]) / 2, R0[3])
    a_xy = np.where(inb, (R0[4] + S[4]) / 4, R0[4] / 2)
    b_x = np.where(inb, (R0[0] - S[0]) / 2, R0[0] / 2)
    b_y = np.where(inb, (R0[1] - S[1]) / 2, R0[1] / 2)
    b_x = b_x + a_xx * u + a_xy * v
    b_y = b_y + a_xy * u + a_yy * v
    s = border_factor(h, w).astype(dtype)
    a_xx, a_yy, a_xy, b_x, b_y = a_xx * s, a_yy * s, a_xy * s, b_x * s, b_y * s
    return np.stack([a_xx ** 2 + a_xy ** 2, (a_xx + a_yy) * a_xy, a_yy ** 2 + a_xy ** 2,
                     a_xx * b_x + a_xy * b_y, a_xy * b_x + a_yy * b_y])


def update_terms(R0, R1, flow, position=True):
    """The magnitude T [5,h,w] that a rounding error of update_matrices is measured against (tests/tof_cases.py: element i
    may be off by c 2^-23 T_i), by first-order propagation in float64.  Every intermediate x gets E_x >= |x|, its sum of
    absolute terms: an fp32 evaluation is off by a few 2^-24 E_x.
      S = sum wgt R1                       E_S = sum wgt |R1| + (|x + u| |dS/dx| + |y + v| |dS/dy|) / 2
                                           (the bilinear weights are not negative; fp32 rounds the position x + u itself by
                                           up to 2^-24 |x + u| before it takes the fraction, as OpenCV does: the kernel,
                                           which splits u exactly, does not, but the twin of this file does:
                                           `position` = False leaves the term out, for the kernel's comparison)
      a = (R0 + S) / 2 (or / 4; R0, R0 / 2 out of bounds)   E_a = (|R0| + E_S) / 2 (...)
      b = (R0 - S) / 2 + a_xx u + a_xy v   E_b = (|R0| + E_S) / 2 + E_axx |u| + E_axy |v|
      all five scaled by the border factor, E with them
      G11 = a_xx^2 + a_xy^2                T = 2 (|a_xx| E_axx + |a_xy| E_axy)
      G12 = (a_xx + a_yy) a_xy             T = (E_axx + E_ayy) |a_xy| + (|a_xx| + |a_yy|) E_axy
      h1  = a_xx b_x + a_xy b_y            T = E_axx |b_x| + |a_xx| E_bx + E_axy |b_y| + |a_xy| E_by
    and G22, h2 by symmetry: d(xy) = x dy + y dx with |dx| <= E_x, and the product's own rounding is below any of these."""
    h, w = flow.shape[:2]
    R0, R1 = np.asarray(R0, np.float64), np.asarray(R1, np.float64)
    A0, A1 = np.abs(R0), np.abs(R1)
    u, v = flow[..., 0].astype(np.float64), flow[..., 1].astype(np.float64)
    fx, fy = sample_positions(flow)
    x1, y1 = np.floor(fx), np.floor(fy)
    inb = (x1 >= 0) & (x1 < w - 1) & (y1 >= 0) & (y1 < h - 1)
    xi, yi = np.where(inb, x1, 0).astype(np.int64), np.where(inb, y1, 0).astype(np.int64)
    ax, ay = fx - x1, fy - y1

    def sample(Q):
        return np.where(inb, (1 - ax) * (1 - ay) * Q[:, yi, xi] + ax * (1 - ay) * Q[:, yi, xi + 1]
                        + (1 - ax) * ay * Q[:, yi + 1, xi] + ax * ay * Q[:, yi + 1, xi + 1], 0.0)

    S, ES = sample(R1), sample(A1)
    dx = (1 - ay) * (R1[:, yi, xi + 1] - R1[:, yi, xi]) + ay * (R1[:, yi + 1, xi + 1] - R1[:, yi + 1, xi])
    dy = (1 - ax) * (R1[:, yi + 1, xi] - R1[:, yi, xi]) + ax * (R1[:, yi + 1, xi + 1] - R1[:, yi, xi + 1])
    if position:
        ES = ES + np.where(inb, (np.abs(fx) * np.abs(dx) + np.abs(fy) * np.abs(dy)) / 2, 0.0)
    half = np.where(inb, 0.5, 1.0)
    a_xx, E_xx = (R0[2] + S[2]) * half, (A0[2] + ES[2]) * half
    a_yy, E_yy = (R0[3] + S[3]) * half, (A0[3] + ES[3]) * half
    a_xy, E_xy = (R0[4] + S[4]) * half / 2, (A0[4] + ES[4]) * half / 2
    b_x = (R0[0] - S[0]) / 2 + a_xx * u + a_xy * v
    b_y = (R0[1] - S[1]) / 2 + a_xy * u + a_yy * v
    E_bx = (A0[0] + ES[0]) / 2 + E_xx * np.abs(u) + E_xy * np.abs(v)
    E_by = (A0[1] + ES[1]) / 2 + E_xy * np.abs(u) + E_yy * np.abs(v)
    s = border_factor(h, w)
    a_xx, a_yy, a_xy, b_x, b_y = (np.abs(t * s) for t in (a_xx, a_yy, a_xy, b_x, b_y))
    E_xx, E_yy, E_xy, E_bx, E_by = (t * s for t in (E_xx, E_yy, E_xy, E_bx, E_by))
    return np.stack([2 * (a_xx * E_xx + a_xy * E_xy), (E_xx + E_yy) * a_xy + (a_xx + a_yy) * E_xy,
                     2 * (a_yy * E_yy + a_xy * E_xy), E_xx * b_x + a_xx * E_bx + E_xy * b_y + a_xy * E_by,
                     E_xy * b_x + a_xy * E_bx + E_yy * b_y + a_yy * E_by])


def near_bounds_test(flow, eps=1e-3):
    """Pixels whose sample position lies within eps of x = 0, x = w - 1, y = 0 or y = h - 1, where the in-bounds test jumps."""
    h, w = flow.shape[:2]
    fx, fy = sample_positions(flow)
    return (np.abs(fx) < eps) | (np.abs(fx - (w - 1)) < eps) | (np.abs(fy) < eps) | (np.abs(fy - (h - 1)) < eps)


# ---- box mean and solve ----------------------------------------------------------------------------------------------------

def blur_solve(M, dtype=np.float64):
    """M [5,h,w] -> flow [h,w,2].  The sums and the solve are float64 whatever `dtype` (OpenCV's and the kernel's are too):
    only the result is rounded to it."""
    box = np.full(WINSIZE, 1.0 / WINSIZE)
    G11, G12, G22, h1, h2 = (correlate_axis(correlate_axis(m, box, 1, "edge"), box, 0, "edge") for m in M)
    det = G11 * G22 - G12 * G12 + 1e-3
    return np.stack([(G22 * h1 - G12 * h2) / det, (G11 * h2 - G12 * h1) / det], -1).astype(dtype)


# ---- the whole ---------------------------------------------------------------------------------------------------------

def farneback(prev_grey, next_grey, dtype=np.float64, updates=None):
    """Two [H,W] grey images (8-bit values) -> flow [H,W,2] in `dtype`.  `updates`, a list, collects every flow an update
    step samples with, in order, except each pair's zero flow of the coarsest level."""
    H, W = prev_grey.shape
    flow = None
    for level in levels(H, W):
        w, h = level[:2]
        R0 = poly_exp(pyramid_level(prev_grey, level, dtype), dtype)
        R1 = poly_exp(pyramid_level(next_grey, level, dtype), dtype)
        if flow is None:
            flow = np.zeros((h, w, 2), dtype)
        else:
            flow = resize_bilinear(flow, h, w, dtype) * dtype(1.0 / PYR_SCALE)
            if updates is not None:
                updates.append(flow)
        M = update_matrices(R0, R1, flow, dtype)
        for i in range(ITERATIONS):
            flow = blur_solve(M, dtype)
            if i < ITERATIONS - 1:
                if updates is not None:
                    updates.append(flow)
                M = update_matrices(R0, R1, flow, dtype)
    return flow


def flows(frames_grey):
    """[F,H,W] -> [F-1,H,W,2]."""
    return np.stack([farneback(frames_grey[i], frames_grey[i + 1]) for i in range(len(frames_grey) - 1)])


def score(flow_a, flow_b, mask=None):
    """metrics.py:18-29 for one pair: [H,W,2] flows, mask [H,W] or None."""
    d = crop_8x8(np.asarray(flow_a, np.float64)) - crop_8x8(np.asarray(flow_b, np.float64))
    n = np.sqrt((d * d).sum(-1))
    if mask is None:
        return n.mean()
    m = crop_8x8(np.asarray(mask, np.float64))
    return (n * m).sum() / m.sum()


def get_tOF(pre_gt_grey, gt_grey, pre_output_grey, output_grey, mask=None):
    return score(farneback(pre_gt_grey, gt_grey), farneback(pre_output_grey, output_grey), mask)


# ---- test images -----------------------------------------------------------------------------------------------------------

def texture(H, W, seed, shift=(0.0, 0.0), n=12):
    """A band-limited texture, 8-bit: n sinusoids with periods of 8 to 64 px, evaluated at (x - shift_x, y - shift_y): the
    content moves by +shift, exactly."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    xs, ys = xs - shift[0], ys - shift[1]
    img = np.zeros((H, W))
    for _ in range(n):
        period = np.exp(rng.uniform(np.log(8.0), np.log(64.0)))
        theta, phase = rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
        k = 2 * np.pi / period
        img += np.sin(k * (np.cos(theta) * xs + np.sin(theta) * ys) + phase)
    return np.rint(127.5 + 100.0 * img / np.sqrt(n / 2) / 3.0).clip(0, 255)


def moving_frames(F, H, W, seed, amplitude=4.0):
    """[F,3,H,W] float32 in [0, 1]: a smooth colour texture under a smooth, spatially varying motion of at most `amplitude` px
    per frame, sampled analytically."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    waves = [(np.exp(rng.uniform(np.log(8.0), np.log(48.0))), rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi, 3))
             for _ in range(10)]
    a, b = rng.uniform(0, 2 * np.pi, 2)
    out = np.zeros((F, 3, H, W), np.float32)
    for f in range(F):
        dx = amplitude * f * 0.7 * np.sin(2 * np.pi * ys / (1.7 * H) + a)
        dy = amplitude * f * 0.7 * np.cos(2 * np.pi * xs / (1.3 * W) + b)
        for c in range(3):
            img = np.zeros((H, W))
            for period, theta, phase in waves:
                k = 2 * np.pi / period
                img += np.sin(k * (np.cos(theta) * (xs - dx) + np.sin(theta) * (ys - dy)) + phase[c])
            out[f, c] = (0.5 + 0.4 * img / np.sqrt(len(waves) / 2) / 3.0).astype(np.float32)
    return out


def smooth_flow(h, w, seed, amplitude):
    """[h,w,2] float32: a smooth random flow; with amplitude ~ the border distance some samples leave the image."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((h, w, 2))
    for c in range(2):
        for _ in range(4):
            kx, ky = rng.uniform(-3, 3, 2) * 2 * np.pi
            out[..., c] += np.sin(kx * xs / w + ky * ys / h + rng.uniform(0, 2 * np.pi))
    return (amplitude * out / 2.0).astype(np.float32)


def update_test_flows(h, w, pairs=2):
    """The flows tests/test_gpu_tof.py feeds the update matrices: about a tenth of the samples leave the image."""
    return np.stack([smooth_flow(h, w, seed=10 * h + p, amplitude=0.1 * min(h, w)) for p in range(pairs)])


def out_of_bounds_share(flow):
    h, w = flow.shape[:2]
    fx, fy = sample_positions(flow)
    inb = (np.floor(fx) >= 0) & (np.floor(fx) < w - 1) & (np.floor(fy) >= 0) & (np.floor(fy) < h - 1)
    return 1.0 - inb.mean()
