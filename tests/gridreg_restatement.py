"""The grid regularisers in numpy: a restatement of the reference's scene/regulation.py:13-28 (compute_plane_tv,
compute_plane_smoothness) and scene/gaussian_model.py:1373-1415 (_plane_regulation, _time_regulation, _l1_regulation,
compute_regulation) from their statements.  Not a copy.

A difference is formed in fp32, exactly as the reference's slice statements round it: the first difference (a - b), then
the difference of two first differences; 1 - t likewise.  Everything after that -- squares, sums, divisions, the
gradient's combination -- is float64.  The gradients are closed forms, not autograd:

    smoothness  L = inv sum_k sd[k]^2,  sd[k] = (t[k+2] - t[k+1]) - (t[k+1] - t[k]),  inv = 1 / (B C (h - 2) w)
                dL/dt[j] = 2 inv (sd[j-2] - 2 sd[j-1] + sd[j])          (sd = 0 outside 0 .. h - 3)
    tv          L = 2 (inv_h sum dh^2 + inv_w sum dw^2)
                dL/dt[j, i] = 4 inv_h (dh[j-1] - dh[j]) + 4 inv_w (dw[i-1] - dw[i])     (0 outside)
    l1          L = inv sum |1 - t|,  dL/dt = -inv sign(1 - t),  sign(0) = 0 (torch.abs)

Every *_grad function also returns `mag`, the sum of the absolute values of the terms of the combination: what a
rounding of the result is measured against (tests/test_gpu_gridreg.py).
"""
import numpy as np

SPATIAL, TIME = (0, 1, 3), (2, 4, 5)


def _f32(t):
    t = np.asarray(t)
    assert t.dtype == np.float32 and t.ndim == 4, (t.dtype, t.shape)
    return t


def second_differences(t):
    """[B, C, h - 2, w] fp32."""
    t = _f32(t)
    fd = t[:, :, 1:, :] - t[:, :, :-1, :]
    return fd[:, :, 1:, :] - fd[:, :, :-1, :]


def smoothness(t):
    sd = second_differences(t).astype(np.float64)
    return float((sd * sd).sum() / sd.size)


def _pad_h(x, before, after):
    return np.pad(x, ((0, 0), (0, 0), (before, after), (0, 0)))


def smoothness_grad(t, scale=1.0):
    """scale = the cotangent (times the weight).  -> (grad float64 [B,C,h,w], mag)."""
    sd = second_differences(t).astype(np.float64)
    c = 2.0 * scale / sd.size
    a, b, d = _pad_h(sd, 2, 0), _pad_h(sd, 1, 1), _pad_h(sd, 0, 2)      # sd[j-2], sd[j-1], sd[j]
    return c * ((a - 2.0 * b) + d), abs(c) * (np.abs(a) + 2.0 * np.abs(b) + np.abs(d))


def tv(t):
    t = _f32(t)
    B, C, h, w = t.shape
    dh = (t[:, :, 1:, :] - t[:, :, :-1, :]).astype(np.float64)
    dw = (t[:, :, :, 1:] - t[:, :, :, :-1]).astype(np.float64)
    return float(2.0 * ((dh * dh).sum() / (B * C * (h - 1) * w + 1e-6) + (dw * dw).sum() / (B * C * h * (w - 1) + 1e-6)))


def tv_grad(t, scale=1.0):
    t = _f32(t)
    B, C, h, w = t.shape
    dh = (t[:, :, 1:, :] - t[:, :, :-1, :]).astype(np.float64)
    dw = (t[:, :, :, 1:] - t[:, :, :, :-1]).astype(np.float64)
    ch = 4.0 * scale / (B * C * (h - 1) * w + 1e-6)
    cw = 4.0 * scale / (B * C * h * (w - 1) + 1e-6)
    hp, hn = _pad_h(dh, 1, 0), _pad_h(dh, 0, 1)                           # dh[j-1], dh[j]
    wp = np.pad(dw, ((0, 0), (0, 0), (0, 0), (1, 0)))
    wn = np.pad(dw, ((0, 0), (0, 0), (0, 0), (0, 1)))
    g = ch * (hp - hn) + cw * (wp - wn)
    return g, abs(ch) * (np.abs(hp) + np.abs(hn)) + abs(cw) * (np.abs(wp) + np.abs(wn))


def l1(t):
    d = (np.float32(1) - _f32(t)).astype(np.float64)
    return float(np.abs(d).sum() / d.size)


def l1_grad(t, scale=1.0):
    d = np.float32(1) - _f32(t)
    g = -(scale / d.size) * np.sign(d).astype(np.float64)
    return g, np.abs(g)


def _contributing(grids):
    return [level for level in grids if len(level) != 3]


def terms(grids):
    """(plane, time, l1) as float64."""
    plane = sum(smoothness(level[i]) for level in _contributing(grids) for i in SPATIAL)
    time = sum(smoothness(level[i]) for level in _contributing(grids) for i in TIME)
    ell = sum(l1(level[i]) for level in _contributing(grids) for i in TIME)
    return float(plane), float(time), float(ell)


def weighted(values, weights):
    """compute_regulation from the three terms as the reference's fp32 statement forms it: the terms and the weights
    are fp32 values, every product and sum rounded to fp32, left to right.  weights = (plane_tv, time_smoothness, l1)."""
    v = [np.float32(x) for x in values]
    w = [np.float32(x) for x in weights]
    return np.float32(np.float32(np.float32(w[0] * v[0]) + np.float32(w[1] * v[1])) + np.float32(w[2] * v[2]))


def regulation_grads(grids, scales):
    """scales = (cotangent x weight) of (plane, time, l1), float64.  -> per level a list of (grad, mag), or None for a plane
    of a level that does not contribute."""
    out = []
    for level in grids:
        if len(level) == 3:
            out.append([None] * 3)
            continue
        row = []
        for i, p in enumerate(level):
            if i in SPATIAL:
                row.append(smoothness_grad(p, scales[0]))
            else:
                gs, ms = smoothness_grad(p, scales[1])
                gl, ml = l1_grad(p, scales[2])
                row.append((gs + gl, ms + ml))
        out.append(row)
    return out
