"""The cases of tests/test_gpu_report.py, checked without a GPU: the cap on bytes inside a band holds for every case on the
restatement alone, the bands are small, the row lengths take every residue modulo 4, no flow sits at the wrap -- and a
numpy float32 evaluation of the same statements (a stand-in for the kernel's arithmetic, not the kernel) obeys the rule."""
import numpy as np
import pytest

import report_cases as RC
import report_restatement as R

CASES = RC.compose_cases()
F = np.float32


def emulate32(kind, a, b=None, cam=None, clip=None):
    """The panel in numpy float32, one rounding per written operation -> uint8 [H,W,3]."""
    def q(x):
        return np.floor(np.clip(x, F(0), F(1)) * F(255)).astype(np.uint8)

    if kind == "RGB":
        return q(a.transpose(1, 2, 0))
    if kind == "GREY":
        return q(np.repeat(a.transpose(1, 2, 0), 3, axis=2))
    if kind == "GREY_DIV_MAX":
        g = np.repeat(a.transpose(1, 2, 0), 3, axis=2)
        return q(g / g.max()) if g.max() != 0 else q(np.zeros_like(g))
    if kind == "ERROR":
        e = (a.transpose(1, 2, 0) - b.transpose(1, 2, 0)) ** 2
        return q((e - e.min()) / max(e.max() - e.min(), F(1e-8)))
    if kind == "SIGNED3":
        return q((a.transpose(1, 2, 0) + F(1)) / F(2))
    if kind == "NORMALS_FD":
        focal, cx, cy, skew, offset = (F(c) for c in cam)
        z = a.reshape(a.shape[-2:]) + F(1e-6)
        H, W = z.shape
        py, px = np.meshgrid(np.arange(H, dtype=F) + offset, np.arange(W, dtype=F) + offset, indexing="ij")
        y = (py - cy) / focal
        x = (px - cx - y * skew) / focal
        p = np.stack([x * z, y * z, z])
        du = p[:, :, 1:] - p[:, :, :-1]
        du = np.concatenate([du, du[:, :, -1:]], axis=2)
        dv = p[:, 1:, :] - p[:, :-1, :]
        dv = np.concatenate([dv, dv[:, -1:, :]], axis=1)
        n = np.stack([dv[1] * du[2] - du[1] * dv[2], dv[2] * du[0] - du[2] * dv[0], dv[0] * du[1] - du[0] * dv[1]])
        length = np.maximum(np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), F(1e-12))
        assert n.dtype == F
        return q(((n / length + F(1)) / F(2)).transpose(1, 2, 0))
    if kind == "FLOW":
        f = a if clip is None else np.clip(a, F(0), F(clip))
        u, v = f[..., 0], f[..., 1]
        den = np.sqrt(u * u + v * v).max() + F(1e-5)
        u, v = u / den, v / den
        rad = np.sqrt(u * u + v * v)
        fk = (np.arctan2(-v, -u) / F(np.pi) + F(1)) / F(2) * F(54)
        k0 = np.floor(fk).astype(np.int64)
        k1 = np.where(k0 + 1 == 55, 0, k0 + 1)
        w = fk - k0.astype(F)
        wheel = R.wheel().astype(F)
        col = wheel[k0] / F(255) + w[..., None] * (wheel[k1] / F(255) - wheel[k0] / F(255))
        out = F(1) - rad[..., None] * (F(1) - col)
        assert out.dtype == F
        return np.floor(F(255) * out).astype(np.uint8)
    raise ValueError(kind)


def test_row_lengths_take_every_residue():
    assert {(3 * P * W) % 4 for _, W, P in RC.SIZES} == {0, 1, 2, 3}
    assert set(RC.SIZES) >= {(2, 2, 1), (3, 5, 6), (13, 17, 5), (48, 80, 4), (270, 300, 2)}
    assert max(P for _, _, P in RC.SIZES) <= 16 and any(H * W * P > 4 * 256 for H, W, P in RC.SIZES)   # > 1 workgroup


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_case_meets_the_cap_and_float32_obeys_the_rule(case):
    name, H, W, panels = case
    cam = RC.camera(H, W)
    assert all(F(c) == c for c in cam)                    # the intrinsics are exact in fp32
    L, b = RC.expected(panels, H, W)
    assert L.shape == b.shape == (H, len(panels) * W, 3)
    assert b.max() < 0.5, f"{name}: a band of {b.max():.2e} levels admits more than two levels"
    got = []
    for k, p in enumerate(panels):
        sl = slice(k * W, (k + 1) * W)
        frac = RC.in_band(L[:, sl], b[:, sl]).mean()
        assert frac <= RC.CAP, f"{name}: panel {k} ({p[0]}) has {frac:.2%} of its bytes in a band"
        if p[0] == "FLOW":
            assert not ((p[1][..., 1] == 0) & (p[1][..., 0] > 0)).any()       # nothing at the wrap
        got.append(emulate32(p[0], p[1], p[2] if len(p) > 2 else None, cam))
    RC.check_bytes(np.concatenate(got, axis=1), L, b, name)


def test_bands_follow_the_operation_count():
    """Orders of magnitude of b, from u = 2^-24 alone: one product for RGB, a handful of operations for the quotients,
    the angle's 4 ulp times 27 times the slope for FLOW."""
    H, W = 13, 17
    cam = RC.camera(H, W)
    u255 = 255 * RC.U
    b = {k: RC.band(*(RC.source(k, H, W, 3) + ((None,) if k != "ERROR" else ())), cam).max() for k in RC.KINDS}
    assert b["RGB"] <= 1.01 * u255 and b["GREY"] <= 1.01 * u255
    assert u255 < b["GREY_DIV_MAX"] <= 3 * u255 and u255 < b["SIGNED3"] <= 3 * u255
    assert 3 * u255 < b["ERROR"] <= 40 * u255
    assert b["FLOW"] >= 0.8 * 255 * (64 / 255) * 27 * RC.ATAN2_ULPS * 2 * RC.U * 0.1 and b["FLOW"] <= 2e-2
    assert b["NORMALS_FD"] <= 2e-2


def test_check_bytes_rejects_what_the_rule_forbids():
    L = np.array([[[10.4, 11.999999, 12.000001]]])
    b = np.full_like(L, 1e-5)
    RC.check_bytes(np.array([[[10, 11, 12]]]), L, b, "exact")
    RC.check_bytes(np.array([[[10, 12, 11]]]), L, b, "both one level off inside their bands")
    for wrong in ([11, 11, 12], [10, 13, 12], [10, 11, 10], [9, 11, 12]):
        with pytest.raises(AssertionError):
            RC.check_bytes(np.array([[wrong]]), L, b, "outside")
