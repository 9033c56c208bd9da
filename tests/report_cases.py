"""The seeded inputs of the report-sheet GPU tests (tests/test_gpu_report.py), the rule their bytes are held to, and where
its bound comes from.  tests/test_report_cases_cpu.py checks the cases themselves without a GPU.

Rule.  With x the float64 restatement's value (tests/report_restatement.py) and L = 255 clip(x, 0, 1), a byte must equal
floor(L) unless L lies within `b` of an integer; there it may also be the neighbouring level on that integer's other side.
So: floor(L - b) <= byte <= floor(L + b).

Where b comes from: a forward error analysis of the kernel's fp32 statements, evaluated per byte on the case's own inputs
(class Err: every value carries a bound on |fp32 result - exact result|).  Each fp32 operation adds one rounding, u |r|
with u = 2^-24; a difference of nearly equal numbers, such as a finite difference of back-projected points, passes its
operands' bounds on unamplified in absolute terms, which is what makes the bound large relative to the small result, and
that is followed through the cross product, the normalisation and the final * 255.  For FLOW the bound also carries the
error of atan2f times the slope of the colour in the wheel position: neighbouring wheel entries differ by at most 64
levels, so |d col / d fk| <= 64 / 255 ~ 0.25 (the analysis uses the two entries a pixel mixes, and this bound where the
floor of the wheel position may differ).  No
ulp table for HIP's device math functions is installed next to the compiler here, so atan2f is ASSUMED to be within
ATAN2_ULPS = 4 ulp.  b never comes from a run of the kernels.

Cap (a condition on the cases, not a measurement): at most CAP = 0.5 % of a panel's bytes may lie in such a band, so that the
rule pins the rest exactly.  The seeds below are chosen so that this holds for every case.

Wrap: the colour is discontinuous only between a = -1 and a = +1, i.e. at v == 0 with u > 0, where the sign of the zero
decides.  The random flows have no zero component; the explicit wrap cases use +0 / -0, where fp32 is unambiguous.
"""
import numpy as np

import report_restatement as R

U = 2.0 ** -24          # unit round-off of fp32, round to nearest
ATAN2_ULPS = 4          # assumed bound of the device's atan2f (1 ulp <= 2 U |result|)
CAP = 0.005
KINDS = ("RGB", "GREY", "GREY_DIV_MAX", "ERROR", "SIGNED3", "NORMALS_FD", "FLOW")
# (H, W, P): the row lengths 3 P W are 6, 90, 255, 960, 1800 and 21 bytes = 2, 2, 3, 0, 0, 1 modulo 4
SIZES = ((2, 2, 1), (3, 5, 6), (13, 17, 5), (48, 80, 4), (270, 300, 2), (5, 7, 1))
STAT_SIZES = ((1, 1), (3, 5), (13, 17), (48, 80), (270, 300))


class Err:
    """A float64 value (array) and a bound on how far the kernel's fp32 result can be from it."""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape).copy()

    @staticmethod
    def of(x):
        return x if isinstance(x, Err) else Err(x)

    def _rounded(self, v, e):
        return Err(v, e + U * (np.abs(v) + e))

    def _sum(self, o, v):
        r = self._rounded(v, self.e + o.e)
        # x + 0 and 0 + x are exact
        r.e = np.where((o.v == 0) & (o.e == 0), self.e, np.where((self.v == 0) & (self.e == 0), o.e, r.e))
        return r

    def __add__(self, o):
        o = Err.of(o)
        return self._sum(o, self.v + o.v)

    def __sub__(self, o):
        o = Err.of(o)
        return self._sum(o, self.v - o.v)

    def __rsub__(self, o):
        return Err.of(o) - self

    __radd__ = __add__

    def __mul__(self, o):
        o = Err.of(o)
        return self._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Err.of(o)
        den = np.maximum(np.abs(o.v) - o.e, 1e-300)
        q = self.v / o.v
        return self._rounded(q, (self.e + np.abs(q) * o.e) / den)

    def __neg__(self):
        return Err(-self.v, self.e)

    def sqrt(self):
        r = np.sqrt(self.v)
        lo = np.sqrt(np.maximum(self.v - self.e, 0.0))
        return self._rounded(r, np.maximum(r - lo, np.sqrt(self.v + self.e) - r))

    def exact_scale(self, s):
        """times a power of two: no rounding"""
        return Err(self.v * s, self.e * abs(s))

    def __getitem__(self, idx):
        return Err(self.v[idx], self.e[idx])

    def amin(self):
        return Err(self.v.min(), self.e.max())

    def amax(self):
        return Err(self.v.max(), self.e.max())


def const32(c):
    """a literal the kernel holds in fp32"""
    return Err(c, U * abs(c))


def _hwc(a):
    return np.asarray(a, dtype=np.float64).transpose(1, 2, 0)


def _band_of(x: Err):
    """the bound of 255 clamp01(x): the clamp does not widen it, the product adds one rounding; a value that both
    evaluations clamp (beyond 0 or 1 by more than its bound) is exactly 0 or 255"""
    lv = Err(np.clip(x.v, 0.0, 1.0), x.e) * 255.0
    return np.where((x.v - x.e >= 1.0) | (x.v + x.e <= 0.0), 0.0, lv.e)


def band(kind, a, b=None, cam=None, clip=None):
    """-> float64 [H,W,3]: b per byte of the panel."""
    if kind in ("RGB", "GREY"):
        x = Err(R.panel(kind, a))
    elif kind == "GREY_DIV_MAX":
        g = Err(R.grey(a))
        x = g / g.amax() if g.v.max() != 0 else Err(np.zeros_like(g.v))
        x.e = np.where(g.v == g.v.max(), 0.0, x.e)     # the maximum is one of the inputs, and a / a is exactly 1
    elif kind == "ERROR":
        d = Err(_hwc(a)) - Err(_hwc(b))
        e = d * d
        lo, hi = e.amin(), e.amax()
        span = hi - lo
        den = span if span.v - span.e > 1e-8 else Err(np.maximum(span.v, 1e-8), span.e)
        x = (e - lo) / den
        # the pixel that holds the maximum (if no other comes within the bound of it) is d / d = 1 exactly
        top = np.sort(e.v.ravel())[-2:]
        if e.v.size > 1 and top[1] - top[0] > 2 * e.e.max() and den is span:
            x.e = np.where(e.v == top[1], 0.0, x.e)
    elif kind == "SIGNED3":
        x = (Err(_hwc(a)) + 1.0).exact_scale(0.5)
    elif kind == "NORMALS_FD":
        x = _normals_err(a, cam)
    elif kind == "FLOW":
        x = _flow_err(a, clip)
    else:
        raise ValueError(kind)
    return _band_of(x)


def _normals_err(depth, cam):
    z = Err(np.asarray(depth, dtype=np.float64).reshape(np.asarray(depth).shape[-2:])) + const32(1e-6)
    H, W = z.v.shape
    focal, cx, cy, skew, offset = (float(c) for c in cam)
    py, px = np.meshgrid(np.arange(H, dtype=np.float64) + offset, np.arange(W, dtype=np.float64) + offset, indexing="ij")
    y = (Err(py) - cy) / focal          # (pixel + offset is exact in fp32; so are the intrinsics the cases use)
    xd = ((Err(px) - cx) - y * skew) / focal
    p = [xd * z, y * z, z]
    rep_c = np.minimum(np.arange(W), W - 2)
    rep_r = np.minimum(np.arange(H), H - 2)
    du = [(c[:, rep_c + 1] - c[:, rep_c]) for c in p]
    dv = [(c[rep_r + 1, :] - c[rep_r, :]) for c in p]
    n = [dv[1] * du[2] - du[1] * dv[2], dv[2] * du[0] - du[2] * dv[0], dv[0] * du[1] - du[0] * dv[1]]
    length = ((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]).sqrt()
    out = [((c / length) + 1.0).exact_scale(0.5) for c in n]
    return Err(np.stack([o.v for o in out], -1), np.stack([o.e for o in out], -1))


def _flow_err(flow_uv, clip):
    f = np.asarray(flow_uv, dtype=np.float64)
    if clip is not None:
        f = np.clip(f, 0.0, clip)
    u0, v0 = Err(f[..., 0]), Err(f[..., 1])
    rad_max = ((u0 * u0 + v0 * v0).sqrt()).amax()
    den = rad_max + const32(1e-5)
    u, v = u0 / den, v0 / den
    rad = (u * u + v * v).sqrt()
    # angle: the bound of the arguments seen from the origin, plus atan2f's own error, then the division by fp32 pi
    r2 = np.maximum(u.v * u.v + v.v * v.v, 1e-300)
    ang = np.arctan2(-v.v, -u.v)
    ang_e = (np.abs(v.v) * u.e + np.abs(u.v) * v.e) / r2 + ATAN2_ULPS * 2 * U * np.abs(ang)
    ang_e = np.where((u.v == 0) & (v.v == 0), 0.0, ang_e)      # atan2f(-0, -0) is -pi_f itself
    a = Err(ang, ang_e) / const32(np.pi)
    # (at the explicit wrap pixels -pi_f / pi_f is exactly -1: their bound below is an over-estimate, not a licence)
    fk = (a + 1.0).exact_scale(0.5) * float(R.NCOLS - 1)
    k0 = np.clip(np.floor(fk.v).astype(np.int64), 0, R.NCOLS - 1)
    k1 = np.where(k0 + 1 == R.NCOLS, 0, k0 + 1)
    frac = fk.v - k0
    w = Err(frac)
    near = (frac < fk.e + U) | (1.0 - frac < fk.e + U)     # the kernel's floor(fk) may be the neighbouring entry
    wheel = R.wheel().astype(np.float64)
    out = []
    for c in range(3):
        # wheel / 255 is one rounding, none for 0 and 255; the kernel mixes as c0 + f (c1 - c0), exact where c0 == c1
        c0 = Err(wheel[k0, c] / 255.0, U * (wheel[k0, c] % 255 != 0))
        c1 = Err(wheel[k1, c] / 255.0, U * (wheel[k1, c] % 255 != 0))
        col = c0 + w * (c1 - c0)
        # the wheel position's own bound (+ the rounding of f = fk - floor(fk)) times the slope of the colour in it: the
        # two entries' difference, or the steepest the wheel has (64 levels per entry) where the floor may differ -- col
        # is continuous in fk across the entries
        slope = np.where(near, 64.0 / 255.0, np.abs(c1.v - c0.v))
        col = Err(col.v, col.e + (fk.e + U) * slope)
        out.append(1.0 - rad * (1.0 - col))
    return Err(np.stack([o.v for o in out], -1), np.stack([o.e for o in out], -1))


# ---- inputs -----------------------------------------------------------------------------------------------------------
def camera(H, W, use_center=True):
    """(focal, cx, cy, skew, offset): fp32-exact numbers, skew != 0"""
    return (max(H, W) + 0.5, W / 2.0 + 0.25, H / 2.0 - 0.5, 0.125, 0.5 if use_center else 0.0)


# The bound of a finite-difference normal grows with the pixel's distance from the principal point: x z is formed with an
# error of a few u |x z|, and the difference of two neighbours is z / focal, so its relative error is a few u |px - cx|.
# On a 300-pixel-wide random depth map that puts more than CAP of the bytes into a band, whatever the seed.  The larger
# maps are therefore FACETS: four planes m . P = d seen through the case's camera, whose finite-difference normal is the
# plane's own at every interior pixel, with planes drawn until 255 x sits at least 0.25 from an integer in every channel.
# The bytes in a band are then those of the few pixels whose differences straddle two facets.
FACETS_FROM = 13 * 17


def facets(H, W, g):
    cam = camera(H, W)
    dirs = R.view_dirs(H, W, cam)
    depth = np.empty((H, W), dtype=np.float32)
    rows, cols = (slice(0, H // 2 - 2), slice(H // 2 - 2, H)), (slice(0, W // 2 + 3), slice(W // 2 + 3, W))
    for r in rows:
        for c in cols:
            for _ in range(1000):
                m = np.array([g.uniform(-0.4, 0.4), g.uniform(-0.4, 0.4), 1.0])
                plane = (g.uniform(2.0, 3.0) / np.tensordot(m, dirs, axes=1)).astype(np.float32)
                frac = R.level(R.normals_fd(plane[None], cam))[H // 2, W // 2] % 1.0
                if (np.abs(frac - 0.5) <= 0.25).all():
                    break
            else:
                raise AssertionError("no plane found")
            depth[r, c] = plane[r, c]
    return depth[None]


def source(kind, H, W, seed):
    """-> the panel tuple (kind, a[, b]) with float32 arrays"""
    g = np.random.RandomState(seed)
    f32 = np.float32
    if kind == "RGB":
        return (kind, g.uniform(-0.1, 1.1, (3, H, W)).astype(f32))
    if kind == "GREY":
        return (kind, g.uniform(0.0, 1.0, (1, H, W)).astype(f32))
    if kind == "GREY_DIV_MAX":
        return (kind, g.uniform(0.2, 5.0, (1, H, W)).astype(f32))
    if kind == "ERROR":
        return (kind, g.uniform(0.0, 1.0, (3, H, W)).astype(f32), g.uniform(0.0, 1.0, (3, H, W)).astype(f32))
    if kind == "SIGNED3":
        return (kind, g.uniform(-1.0, 1.0, (3, H, W)).astype(f32))
    if kind == "NORMALS_FD":
        if H * W <= FACETS_FROM:
            return (kind, g.uniform(1.0, 3.0, (1, H, W)).astype(f32))
        return (kind, facets(H, W, g))
    if kind == "FLOW":
        flow = g.normal(0.0, 2.0, (H, W, 2)).astype(f32)
        assert not (flow == 0).any()
        return (kind, flow)
    raise ValueError(kind)


SEED0 = 7100


def compose_cases():
    """-> [(id, H, W, [panel tuples])]: for every size one sheet per kind (P panels of that kind, each with its own
    seed) and one mixed sheet that cycles through the kinds."""
    cases = []
    for si, (H, W, P) in enumerate(SIZES):
        for ki, kind in enumerate(KINDS + ("MIXED",)):
            kinds = [kind] * P if kind != "MIXED" else [KINDS[(si + k) % len(KINDS)] for k in range(P)]
            panels = [source(k, H, W, SEED0 + 1000 * si + 50 * ki + p) for p, k in enumerate(kinds)]
            cases.append((f"{H}x{W}x{P}-{kind}", H, W, panels))
    return cases


def expected(panels, H, W):
    """-> (level L [H, P W, 3], band b [H, P W, 3]) of a side-by-side sheet"""
    cam = camera(H, W)
    xs, bs = [], []
    for p in panels:
        args = (p[0], p[1], p[2] if len(p) > 2 else None, cam, p[3] if len(p) > 3 else None)
        xs.append(R.panel(*args))
        bs.append(band(*args))
    return R.level(np.concatenate(xs, axis=1)), np.concatenate(bs, axis=1)


def in_band(L, b):
    """where the rule admits two levels (a level that the clamp pins to 0 or 255 admits one, whatever b)"""
    return np.floor(np.clip(L - b, 0.0, 255.0)) != np.floor(np.clip(L + b, 0.0, 255.0))


def check_bytes(got, L, b, what):
    """The rule: floor(L - b) <= byte <= floor(L + b).  Prints the figures before it asserts."""
    got = np.asarray(got).astype(np.int64)
    assert got.shape == L.shape, f"{what}: shape {got.shape} vs {L.shape}"
    lo = np.floor(np.clip(L - b, 0.0, 255.0))
    hi = np.floor(np.clip(L + b, 0.0, 255.0))
    off = got != np.floor(L)
    bad = (got < lo) | (got > hi)
    print(f"[report] {what}: {int(off.sum())}/{got.size} bytes one level off the float64 floor, {int(bad.sum())} outside "
          f"the rule; {int(in_band(L, b).sum())} in a band, largest b {float(b.max()):.2e}")
    assert not bad.any(), f"{what}: {int(bad.sum())} bytes outside the one-level rule, first at " \
                          f"{tuple(np.argwhere(bad)[0])}: got {got[bad][0]}, level {L[bad][0]!r}, b {b[bad][0]:.2e}"
