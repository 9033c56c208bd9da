"""The evaluation metrics (include/mobgs_hip.h K22) restated with numpy and scipy on the CPU, for the tests to compare
against: /root/reference/metrics.py:54-79, :123-125 (what scikit-image's peak_signal_noise_ratio and structural_similarity
compute there), dycheck_metrics.py:42-200 and the L1 / PSNR of train.py:903-919, in our own words, parameterised by dtype.

    image_metrics(pred, gt, mask, data_range=..., clamp=..., quantize=..., arms=..., dtype=...)   -> {name: [B] array}

The same code is evaluated in either dtype.  dtype=np.float32 stands for "the reference as it can be run here": every
element-wise statement and every window is evaluated in fp32 (scipy.ndimage.uniform_filter and scipy.signal.convolve2d keep
the dtype they are given); a REDUCTION to one number is accumulated in float64 and rounded to fp32 once, so that its value
does not depend on how a numpy build orders a sum.  dtype=np.float64 is the truth the GPU tests measure against: inputs
widened exactly.  The clamp and the 8-bit quantisation are fp32 operations in both (they produce the fp32 inputs).

Also here: the fixture's cases (CASES, make_case: seeded PCG64 streams, nothing stored but a checksum probe), the mask
strata, and the tolerance rule of the GPU tests (regterms_restatement.allowed over the fixture's largest reference gap)."""
from __future__ import annotations

import math

import numpy as np
from scipy.ndimage import uniform_filter
from scipy.signal import convolve2d

from regterms_restatement import FLOOR, FLOOR_DB, allowed, rel_gap  # noqa: F401  (the rule of DESIGN 3a)

METRICS = ("l1", "mse", "psnr", "psnr_masked", "ssim_box", "ssim_box_masked", "ssim_gauss")
DB = ("psnr", "psnr_masked")
SIZES = ((7, 7), (11, 11), (12, 27), (37, 53), (64, 80), (97, 131))      # (H, W)
STRATA = ("absent", "ones", "random60", "empty", "single", "hole", "stripes")
EXTRAS = ("identical", "flat", "clamp", "quantize")
EXTRA_SIZE = (37, 53)
NOISE = 0.05


def _total(x, dtype):
    return dtype(np.sum(x, dtype=np.float64))


def quantize8(x):
    """eval.py:162 then metrics.py:99-100: the 8-bit image and back, in fp32."""
    x = np.asarray(x, dtype=np.float32)
    return np.float32((np.clip(x, 0, 1) * 255).astype("uint8")) / 255


def gauss_taps(dtype):
    """dycheck_metrics.py:146-151 (filter_size 11, sigma 1.5)."""
    hw = 11 // 2
    shift = (2 * hw - 11 + 1) / 2
    f_i = ((np.arange(11).astype(dtype) - dtype(hw) + dtype(shift)) / dtype(1.5)) ** 2
    filt = np.exp(dtype(-0.5) * f_i)
    return (filt / filt.sum(dtype=dtype)).astype(dtype)


def _partial_conv(z, m, f):
    """dycheck_metrics.py:154-166: one 1-D pass, renormalised by (taps / mask count), and the mask it leaves."""
    z_ = convolve2d(z * m, f, mode="valid")
    m_ = convolve2d(m, np.ones_like(f), mode="valid")
    assert z_.dtype == z.dtype and m_.dtype == z.dtype
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(m_ != 0, z_ * np.ones_like(f).sum() / m_, 0).astype(z.dtype)
    return out, (m_ != 0).astype(z.dtype)


def gauss_filter(z, m, dtype):
    """filt_fn of dycheck_metrics.py:168-174: along x with the mask, then along y with the mask the first pass leaves."""
    filt = gauss_taps(dtype)
    return _partial_conv(*_partial_conv(z, m, filt[None, :]), filt[:, None])[0]


def ssim_gauss_map(a, b, m, max_val, dtype):
    """dycheck_metrics.py:176-197 for one channel: a, b, m [H,W] -> [H-10, W-10]."""
    mu0, mu1 = gauss_filter(a, m, dtype), gauss_filter(b, m, dtype)
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    s00 = gauss_filter(a ** 2, m, dtype) - mu00
    s11 = gauss_filter(b ** 2, m, dtype) - mu11
    s01 = gauss_filter(a * b, m, dtype) - mu01
    s00, s11 = np.maximum(dtype(0), s00), np.maximum(dtype(0), s11)
    s01 = np.sign(s01) * np.minimum(np.sqrt(s00 * s11), np.abs(s01))
    c1, c2 = dtype((0.01 * max_val) ** 2), dtype((0.03 * max_val) ** 2)
    out = ((2 * mu01 + c1) * (2 * s01 + c2)) / ((mu00 + mu11 + c1) * (s00 + s11 + c2))
    assert out.dtype == dtype
    return out


def ssim_box_map(a, b, data_range, dtype):
    """skimage.metrics.structural_similarity (gaussian_weights=False, use_sample_covariance=True, K1 = 0.01, K2 = 0.03,
    win_size = 7) for one channel, uncropped: a, b [H,W] -> [H,W]."""
    cov_norm = dtype(49.0 / 48.0)
    ux, uy = uniform_filter(a, size=7), uniform_filter(b, size=7)           # mode='reflect' is scipy's default
    uxx, uyy, uxy = uniform_filter(a * a, size=7), uniform_filter(b * b, size=7), uniform_filter(a * b, size=7)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    c1, c2 = dtype((0.01 * data_range) ** 2), dtype((0.03 * data_range) ** 2)
    out = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
    assert out.dtype == dtype
    return out


def prepare(pred, gt, clamp, quantize):
    """The fp32 images the metrics are taken of (train.py:903-907, eval.py:160-162)."""
    pred, gt = np.asarray(pred, dtype=np.float32), np.asarray(gt, dtype=np.float32)
    if clamp:
        pred, gt = np.clip(pred, np.float32(0), np.float32(1)), np.clip(gt, np.float32(0), np.float32(1))
    if quantize:
        pred = quantize8(pred)
    return pred, gt


def image_metrics(pred, gt, mask=None, *, data_range, clamp=False, quantize=False, arms=("box", "gauss"),
                  dtype=np.float64):
    """pred, gt [B,3,H,W], mask [B,H,W] in {0, 1} or None -> {metric: [B] array of dtype}; NaN for an arm not asked for."""
    pred, gt = prepare(pred, gt, clamp, quantize)
    B, C, H, W = pred.shape
    out = {k: np.full(B, np.nan, dtype=dtype) for k in METRICS}
    for i in range(B):
        a, b = pred[i].astype(dtype), gt[i].astype(dtype)
        m = np.ones((H, W), dtype=dtype) if mask is None else np.asarray(mask[i]).astype(dtype)
        n, big_m = dtype(C * H * W), dtype(C) * _total(m, dtype)            # the mask broadcast over the channels
        d = a - b
        out["l1"][i] = _total(np.abs(d), dtype) / n
        mse = _total(d ** 2, dtype) / n
        out["mse"][i] = mse
        with np.errstate(divide="ignore"):
            out["psnr"][i] = dtype(20) * np.log10(dtype(1) / np.sqrt(mse))
            masked_mean = _total(d ** 2 * m[None], dtype) / max(big_m, dtype(1e-6))
            out["psnr_masked"][i] = dtype(-10.0) / np.log(dtype(10.0)) * np.log(masked_mean)
        if "box" in arms:
            maps = [ssim_box_map(a[c], b[c], data_range, dtype) for c in range(C)]
            per_channel = [_total(s[3:H - 3, 3:W - 3], dtype) / dtype((H - 6) * (W - 6)) for s in maps]
            out["ssim_box"][i] = _total(np.array(per_channel, dtype=dtype), dtype) / dtype(C)
            out["ssim_box_masked"][i] = _total(np.stack(maps) * m[None], dtype) / (big_m + dtype(1e-8))
        if "gauss" in arms:
            maps = [ssim_gauss_map(a[c], b[c], m, data_range, dtype) for c in range(C)]
            out["ssim_gauss"][i] = _total(np.stack(maps), dtype) / dtype(C * (H - 10) * (W - 10))
    return out


# ---- the same two maps by a direct double loop over windows (the index conventions of the scipy route, spelled out) ----

def ssim_box_map_bruteforce(a, b, data_range):
    H, W = a.shape
    refl = lambda i, n: -i - 1 if i < 0 else (2 * n - 1 - i if i >= n else i)    # noqa: E731  (d c b a | a b c d | d c b a)
    out = np.empty((H, W))
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    for y in range(H):
        for x in range(W):
            ys = [refl(y + k, H) for k in range(-3, 4)]
            xs = [refl(x + k, W) for k in range(-3, 4)]
            p, q = a[np.ix_(ys, xs)], b[np.ix_(ys, xs)]
            ux, uy = p.mean(), q.mean()
            vx, vy = 49 / 48 * ((p * p).mean() - ux * ux), 49 / 48 * ((q * q).mean() - uy * uy)
            vxy = 49 / 48 * ((p * q).mean() - ux * uy)
            out[y, x] = (2 * ux * uy + c1) * (2 * vxy + c2) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return out


def ssim_gauss_map_bruteforce(a, b, m, max_val):
    H, W = a.shape
    w = gauss_taps(np.float64)

    def filt(z):
        hz, hm = np.zeros((H, W - 10)), np.zeros((H, W - 10))
        for y in range(H):
            for x in range(W - 10):
                cnt = m[y, x:x + 11].sum()
                if cnt != 0:
                    hz[y, x], hm[y, x] = (w * (z[y, x:x + 11] * m[y, x:x + 11])).sum() * 11 / cnt, 1.0
        out = np.zeros((H - 10, W - 10))
        for y in range(H - 10):
            for x in range(W - 10):
                cnt = hm[y:y + 11, x].sum()
                if cnt != 0:
                    out[y, x] = (w * (hz[y:y + 11, x] * hm[y:y + 11, x])).sum() * 11 / cnt
        return out

    mu0, mu1 = filt(a), filt(b)
    s00 = np.maximum(0.0, filt(a * a) - mu0 * mu0)
    s11 = np.maximum(0.0, filt(b * b) - mu1 * mu1)
    s01 = filt(a * b) - mu0 * mu1
    s01 = np.sign(s01) * np.minimum(np.sqrt(s00 * s11), np.abs(s01))
    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    return (2 * mu0 * mu1 + c1) * (2 * s01 + c2) / ((mu0 * mu0 + mu1 * mu1 + c1) * (s00 + s11 + c2))


# ---- the fixture's cases ---------------------------------------------------------------------------------------------

def _cases():
    out = []
    for H, W in SIZES:
        for B in (1, 3):
            for stratum in STRATA:
                out.append((H, W, B, stratum))
    H, W = EXTRA_SIZE
    return tuple(out) + tuple((H, W, 1, e) for e in EXTRAS)


CASES = _cases()                     # (H, W, B, mask stratum or extra)


def case_name(i):
    H, W, B, what = CASES[i]
    return f"{H}x{W}-B{B}-{what}"


def make_mask(stratum, B, H, W, rng):
    """[B,H,W] fp32 in {0, 1}, or None."""
    if stratum == "absent":
        return None
    m = np.ones((B, H, W), dtype=np.float32)
    if stratum == "random60":
        m = (rng.random((B, H, W)) < 0.6).astype(np.float32)
    elif stratum == "empty":
        m[:] = 0
    elif stratum == "single":
        m[:] = 0
        m[:, H // 2, W // 3] = 1
    elif stratum == "hole":                      # 5 wide: narrower than either window
        y, x = max(0, H // 2 - 2), max(0, W // 2 - 2)
        m[:, y:y + 5, x:x + 5] = 0
    elif stratum == "stripes":                   # bands of 12 columns: whole 11-tap window rows, and whole windows, are empty
        m[:, :, (np.arange(W) // 12) % 2 == 0] = 0
    elif stratum != "ones":
        raise ValueError(stratum)
    return m


def make_case(i):
    """-> dict(pred, gt [B,3,H,W] fp32, mask [B,H,W] fp32 or None, data_range, clamp, quantize, arms)."""
    H, W, B, what = CASES[i]
    rng = np.random.Generator(np.random.PCG64(1000 + i))
    gt = uniform_filter(rng.random((B, 3, H, W)), size=(1, 1, 5, 5)) * 1.6 - 0.3        # smoothed, mostly inside [0, 1]
    gt = np.clip(gt, 0, 1).astype(np.float32)
    pred = (gt + NOISE * rng.standard_normal((B, 3, H, W))).astype(np.float32)
    c = dict(mask=None, data_range=1.0 if B == 1 else 2.0, clamp=False, quantize=False,
             arms=("box", "gauss") if min(H, W) >= 11 else ("box",))
    if what in STRATA:
        c["mask"] = make_mask(what, B, H, W, rng)
    elif what == "identical":
        pred = gt.copy()
    elif what == "flat":
        gt = np.full_like(gt, 0.5)
        pred = gt.copy()
    elif what == "clamp":
        gt = (gt * 2 - 0.5).astype(np.float32)
        pred = (pred * 2 - 0.5).astype(np.float32)
        c["clamp"] = True
        c["mask"] = make_mask("random60", B, H, W, rng)
    elif what == "quantize":
        gt = quantize8(gt)
        pred = (pred * 2 - 0.5).astype(np.float32)
        c["quantize"] = True
    c.update(pred=pred, gt=gt)
    return c


def probe(c):
    """A checksum of a case's inputs: what the fixture stores instead of the images."""
    m = c["mask"]
    flat = c["pred"].reshape(-1).astype(np.float64)[::7]
    return np.array([c["pred"].sum(dtype=np.float64), c["gt"].sum(dtype=np.float64), float(flat @ np.arange(flat.size)),
                     -1.0 if m is None else float(m.sum(dtype=np.float64))])


def evaluate(c, dtype):
    """[B, 7]: the METRICS of every image of case c."""
    r = image_metrics(c["pred"], c["gt"], c["mask"], data_range=c["data_range"], clamp=c["clamp"], quantize=c["quantize"],
                      arms=c["arms"], dtype=dtype)
    return np.stack([r[k] for k in METRICS], axis=1)


def gap(name, got, truth):
    """Distance of a value from the truth: in dB for a PSNR, relative otherwise; 0 where both are the same infinity or
    both NaN (an arm that was not evaluated)."""
    got, truth = float(got), float(truth)
    if (math.isnan(got) and math.isnan(truth)) or got == truth:
        return 0.0
    if math.isinf(got) or math.isinf(truth) or math.isnan(got) or math.isnan(truth):
        return math.inf
    return abs(got - truth) if name in DB else rel_gap(got, truth)


def reference_gaps(fx):
    """Per metric, the LARGEST distance of the fixture's fp32 values from its float64 values over all cases and images: the
    fp32 window's error on E[x^2] - mu^2 is systematic (1e-5 on smooth images), and where a case happens to land closer
    that is luck, not a bound."""
    out = {}
    for j, name in enumerate(METRICS):
        out[name] = max(gap(name, a, b) for a, b in zip(fx["f32"][:, j], fx["f64"][:, j]))
    return out


def tolerance(name, ref_gaps):
    return allowed(ref_gaps[name], FLOOR_DB if name in DB else FLOOR)
