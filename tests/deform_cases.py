"""Deterministic cases for the two autograd functions of mobgs_amd.deformation (`_HexPlane`, `_MlpUpdate`), their float64
and fp32 references from oracle/deform_torch.py, and the comparator of tests/test_gpu_deform_kernels.py.  Torch on the CPU
and the oracle only: nothing of the package under test is imported here; tests/test_deform_cases_cpu.py checks from the
oracle alone that every case reaches the edge it is named after.

Near-kink filter.  Random rows are drawn at twice the wanted count, the float64 oracle looks at them and the first N rows
that are not near a kink are kept, so that fp32 and float64 take the same branch everywhere and no comparison needs a
flip allowance:
  * HexPlane: a row is near a kink when a grid coordinate ix of one of its 18 x 2 plane axes lies within 1e-4 of an
    integer (coordinates clipped to the border sit exactly ON 0 or r - 1 in every precision: no kink), or when a normalised
    coordinate lies within 1e-5 of +-1;
  * MLP: when one of its 128 + 3 x 128 pre-activations satisfies |z| <= 64 * 2^-24 * (sum |w x| + |b|), the fp32
    dot-product error bound of that unit, or a scale update ds lies that close to +-log 100.
A case that drops more than 5 % of its candidates raises.

Planted rows (the border case): aabb +-1 / +-2, coordinates and times dyadic with at most 4 fractional bits.  Their
grid coordinates are exact in fp32 and in float64 at every resolution, so a point on a face, an edge, a corner or outside
the box lands in the same cell with the same fraction in both.  (The planes have 7, 15 and 31 intervals per axis and 3 in
time: the only dyadic coordinates on a grid line are the faces themselves, which are grid lines of every level.)"""
import functools
import math
from types import SimpleNamespace

import torch

from oracle import deform_torch as D

LOG100 = math.log(100)
MULTIRES = (1, 2, 4)
HOT_MAX = 24 * 1024  # cells of the time planes above which the backward leaves its LDS table (csrc/hexplane_bwd.hip)
MAX_DROP = 0.05
W_KEYS = ("w0", "b0", "pos_w1", "pos_b1", "pos_w2", "pos_b2", "scl_w1", "scl_b1", "scl_w2", "scl_b2", "rot_w1", "rot_b1",
          "rot_w2", "rot_b2")
AABB = torch.tensor([[1.3, 0.9, 2.1], [-1.1, -1.4, -0.7]])  # row 0 = xyz_max, row 1 = xyz_min
OUTSIDE = 1.0172  # points uniform in the box grown by this factor per axis: 1 - 1.0172^-3 = 5 % outside


# ---- comparator --------------------------------------------------------------------------------------------------------
def needed_k(got, ref64, ref32):
    """-> (err, gap, floor, k needed): err = max |got - ref64|, gap = max |ref32 - ref64|, floor = 2^-23 max |ref64| and
    the smallest k with err <= k gap + floor."""
    got, ref32 = got.detach().cpu().double(), ref32.detach().double()
    if ref64.numel() == 0:
        return 0.0, 0.0, 0.0, 0.0
    err = float((got - ref64).abs().max())
    gap = float((ref32 - ref64).abs().max())
    floor = 2.0 ** -23 * float(ref64.abs().max())
    if err <= floor:
        return err, gap, floor, 0.0
    return err, gap, floor, ((err - floor) / gap if gap > 0 else math.inf)


def close_to_f64(got, ref64, ref32, k, what):
    """max |got - ref64| <= k max |ref32 - ref64| + 2^-23 max |ref64|, and got == 0 wherever ref64 == 0 exactly.
    Prints the figures before it asserts and returns the k the tensor needed."""
    assert tuple(got.shape) == tuple(ref64.shape), f"{what}: shape {tuple(got.shape)} != {tuple(ref64.shape)}"
    err, gap, floor, need = needed_k(got, ref64, ref32)
    print(f"RATIO {what}: err {err:.3e} gap {gap:.3e} floor {floor:.3e} needs k {need:.3f} (allowed {k})")
    g = got.detach().cpu().double()
    stray = int(((ref64 == 0) & (g != 0)).sum())
    assert stray == 0, f"{what}: {stray} entries are not 0 where the float64 reference is exactly 0"
    assert err <= k * gap + floor, f"{what}: max |diff| {err:.3e} > {k} x {gap:.3e} + {floor:.3e}"
    return need


def _keep_first(bad, n, what):
    """Indices of the first n candidates that are not `bad`, and the share of ALL candidates that is."""
    dropped = float(bad.double().mean()) if bad.numel() else 0.0
    if dropped > MAX_DROP:
        raise ValueError(f"{what}: the near-kink filter drops {dropped:.1%} of the candidates (cap {MAX_DROP:.0%})")
    good = torch.nonzero(~bad).reshape(-1)
    if good.numel() < n:
        raise ValueError(f"{what}: {good.numel()} usable candidates for {n} rows")
    return good[:n], dropped


# ---- HexPlane ----------------------------------------------------------------------------------------------------------
def plane_shapes(base):
    """[1, 32, rb, ra] of the 18 planes (level-major, D.COMBS order) for base resolution [x, y, z, t]."""
    out = []
    for m in MULTIRES:
        reso = [base[0] * m, base[1] * m, base[2] * m, base[3]]
        out += [(1, 32, reso[b], reso[a]) for a, b in D.COMBS]
    return out


def hot_cells(base):
    """Cells of the planes that have a time axis."""
    return sum(s[2] * s[3] for s, (a, b) in zip(plane_shapes(base), D.COMBS * 3) if b == 3)


def normalised(pts, times, aabb):
    """float64 [n, 4]: the unclamped normalised coordinates and the time."""
    a = aabb.double()
    return torch.cat([(pts.double() - a[0]) * (2.0 / (a[1] - a[0])) - 1.0, times.double()], dim=1)


def grid_coordinate(q, r):
    return (q.clamp(-1.0, 1.0) + 1.0) * 0.5 * (r - 1)


def hex_near_kink(pts, times, aabb, base):
    q = normalised(pts, times, aabb)
    bad = ((q.abs() - 1.0).abs() < 1e-5).any(dim=1)
    for axis in range(4):
        for m in (MULTIRES if axis < 3 else (1,)):
            ix = grid_coordinate(q[:, axis], base[axis] * m)
            bad |= (q[:, axis].abs() < 1.0) & ((ix - ix.round()).abs() < 1e-4)
    return bad


def hex_cells(case):
    """float64 base cell (y0 * ra + x0) of every (row, plane): [N, 18]."""
    q = normalised(case.pts, case.times, case.aabb)
    cols = []
    for (_, _, rb, ra), (a, b) in zip(plane_shapes(case.base), D.COMBS * 3):
        cols.append(grid_coordinate(q[:, b], rb).floor().long() * ra + grid_coordinate(q[:, a], ra).floor().long())
    return torch.stack(cols, dim=1)


def _box_points(n, g):
    u = 0.5 + OUTSIDE * (torch.rand(n, 3, generator=g) - 0.5)
    return AABB[0] + (AABB[1] - AABB[0]) * u


def _planted_rows():
    """64 rows in normalised coordinates v (the world coordinate is -v or -2 v) and their times."""
    rows = [[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)]  # 8 corners
    for free in range(3):  # 12 edges
        for s1 in (-1.0, 1.0):
            for s2 in (-1.0, 1.0):
                v = [s1, s2]
                v.insert(free, 0.3125)
                rows.append(v)
    for axis in range(3):  # 6 faces, 6 x outside on one side
        for s in (-1.0, 1.0):
            for far in (1.0, 1.5):
                v = [-0.5625, 0.3125]
                v.insert(axis, s * far)
                rows.append(v)
    rows += [[1.25, -1.5, 0.0625], [-1.25, 0.4375, 1.5], [1.5, 1.5, -1.5], [-1.5, 1.0, 0.25], [1.0, -1.25, -1.0],
             [0.0, 0.0, 0.0]]  # outside on two / three axes, outside next to a face, the centre
    g = torch.Generator().manual_seed(77)
    while len(rows) < 64:  # interior dyadic rows
        rows.append((torch.randint(-15, 16, (3,), generator=g).double() / 16.0).tolist())
    v = torch.tensor(rows, dtype=torch.float64)
    tvals = (-1.0, 1.0, 1.5, -1.5, 0.0, 0.25)
    t = torch.tensor([tvals[(i + i // 6) % 6] for i in range(64)], dtype=torch.float64)
    return v, t


HEX_SIZES = (0, 1, 2, 3, 31, 33, 511, 512, 513, 1025)
HEX_CASES = tuple(f"n{n}" for n in HEX_SIZES) + ("border", "pileup", "hot_full", "cold", "cold_ref")
_HEX_SHAPED = {"hot_full": (513, [16, 16, 16, 73], False), "cold": (513, [16, 16, 16, 74], False),
               "cold_ref": (1025, [64, 64, 64, 25], True)}  # N, base, one shared time


@functools.lru_cache(maxsize=None)
def hex_case(name):
    """-> namespace(name, N, base, pts [N,3], times [N,1], aabb [2,3], planes 18 x [1,32,rb,ra] channels-last in
    [0.5, 1.5], cot [N,96], dropped): fp32 CPU tensors."""
    g = torch.Generator().manual_seed(1000 + HEX_CASES.index(name))
    base, aabb, dropped = [8, 8, 8, 4], AABB, 0.0
    if name == "border":
        n = 64
        aabb = torch.tensor([[1.0, 2.0, 1.0], [-1.0, -2.0, -1.0]])
        v, t = _planted_rows()
        pts, times = (-v * aabb[0].double()).float(), t.float().reshape(n, 1)
    elif name == "pileup":
        n = 600
        # cell 11 of the 31 intervals of the finest level lies inside one cell of the 15- and the 7-interval levels
        u = (11.0 + 0.1 + 0.8 * torch.rand(2 * n, 3, generator=g)) / 31.0
        pts, times = AABB[0] + (AABB[1] - AABB[0]) * u, torch.full((2 * n, 1), 0.3)
    else:
        n, base, shared = _HEX_SHAPED.get(name) or (int(name[1:]), base, False)
        pts = _box_points(2 * n, g)
        times = torch.full((2 * n, 1), 11.0 / 23.0) if shared else 2.4 * torch.rand(2 * n, 1, generator=g) - 1.2
    if name != "border":
        keep, dropped = _keep_first(hex_near_kink(pts, times, aabb, base), n, "HexPlane case " + name)
        pts, times = pts[keep].contiguous(), times[keep].contiguous()
    planes = [(0.5 + torch.rand(s, generator=g)).contiguous(memory_format=torch.channels_last)
              for s in plane_shapes(base)]
    return SimpleNamespace(name=name, N=n, base=base, pts=pts, times=times, aabb=aabb, planes=planes,
                           cot=torch.randn(n, 96, generator=g), dropped=dropped)


def hex_eval(case, dtype, keep=None):
    """The oracle's HexPlane statements in `dtype` on the rows `keep` (all): feat, v_pts, v_times, plane0 .. plane17."""
    pts, times, cot = (t if keep is None else t[keep] for t in (case.pts, case.times, case.cot))
    planes = [p.to(dtype, copy=True).contiguous().requires_grad_(True) for p in case.planes]
    if pts.shape[0] == 0:  # grid_sample takes no empty grid: nothing is sampled and nothing scattered
        out = {"feat": torch.zeros(0, 96, dtype=dtype), "v_pts": torch.zeros(0, 3, dtype=dtype),
               "v_times": torch.zeros(0, 1, dtype=dtype)}
        out.update({f"plane{i}": torch.zeros_like(p) for i, p in enumerate(planes)})
        return out
    pts, times = (t.to(dtype, copy=True).requires_grad_(True) for t in (pts, times))
    feat = D.hexplane_features(pts, times, case.aabb.to(dtype), [planes[6 * l:6 * l + 6] for l in range(3)])
    feat.backward(cot.to(dtype))
    out = {"feat": feat.detach(), "v_pts": pts.grad, "v_times": times.grad}
    out.update({f"plane{i}": p.grad for i, p in enumerate(planes)})
    return out


@functools.lru_cache(maxsize=None)
def hex_reference(name):
    """(float64, fp32) references of a case, computed once and shared: leave them unchanged."""
    case = hex_case(name)
    return hex_eval(case, torch.float64), hex_eval(case, torch.float32)


# ---- MLP + update rules ------------------------------------------------------------------------------------------------
def _linear(out_f, in_f, g):
    """nn.Linear's default initialisation (weight and bias uniform in +-1 / sqrt(fan_in)), times 2."""
    b = 2.0 / math.sqrt(in_f)
    return b * (2 * torch.rand(out_f, in_f, generator=g) - 1), b * (2 * torch.rand(out_f, generator=g) - 1)


def _weights(g):
    W = {}
    W["w0"], W["b0"] = _linear(128, 96, g)
    for h, nout in (("pos", 7), ("scl", 3), ("rot", 4)):
        W[h + "_w1"], W[h + "_b1"] = _linear(128, 128, g)
        W[h + "_w2"], W[h + "_b2"] = _linear(nout, 128, g)
    return W


def mlp_near_kink(feat, W):
    """-> (near a kink [n] bool, ds [n,3]) in float64."""
    E = 64 * 2.0 ** -24
    f = feat.double()
    Wd = {k: v.double() for k, v in W.items()}
    z0 = f @ Wd["w0"].t() + Wd["b0"]
    bad = (z0.abs() <= E * (f.abs() @ Wd["w0"].abs().t() + Wd["b0"].abs())).any(dim=1)
    a1 = torch.relu(z0)
    ds = None
    for h in ("pos", "scl", "rot"):
        z1 = a1 @ Wd[h + "_w1"].t() + Wd[h + "_b1"]
        bad |= (z1.abs() <= E * (a1 @ Wd[h + "_w1"].abs().t() + Wd[h + "_b1"].abs())).any(dim=1)
        if h == "scl":
            a2 = torch.relu(z1)
            ds = a2 @ Wd["scl_w2"].t() + Wd["scl_b2"]
            lim = E * (a2 @ Wd["scl_w2"].abs().t() + Wd["scl_b2"].abs())
            bad |= (((ds - LOG100).abs() <= lim) | ((ds + LOG100).abs() <= lim)).any(dim=1)
    return bad, ds


MLP_SIZES = (0, 1, 63, 64, 65, 127, 128)
MLP_CASES = tuple(f"n{n}" for n in MLP_SIZES) + ("parked", "clamp")
_MLP_N = {"parked": 16449, "clamp": 130}


@functools.lru_cache(maxsize=None)
def mlp_case(name):
    """-> namespace(name, N, feat [N,96] in [0,2], pts, scales, rots (unnormalised), W (dict, W_KEYS), cots (3), ds
    [N,3] float64, dropped): fp32 CPU tensors."""
    g = torch.Generator().manual_seed(2000 + MLP_CASES.index(name))
    n = _MLP_N.get(name) or int(name[1:])
    W = _weights(g)
    if name == "clamp":
        W["scl_b2"] = torch.tensor([6.0, -6.0, 0.0])
    feat = 2.0 * torch.rand(2 * n, 96, generator=g)
    bad, ds = mlp_near_kink(feat, W)
    keep, dropped = _keep_first(bad, n, "MLP case " + name)
    return SimpleNamespace(name=name, N=n, feat=feat[keep].contiguous(), pts=torch.randn(n, 3, generator=g),
                           scales=0.5 * torch.randn(n, 3, generator=g), rots=torch.randn(n, 4, generator=g), W=W,
                           cots=[torch.randn(n, c, generator=g) for c in (3, 3, 4)], ds=ds[keep], dropped=dropped)


def mlp_eval(case, dtype, keep=None):
    """The oracle's MLP heads and update rules (oracle/deform_torch.py deform_forward after the features) in `dtype` on
    the rows `keep` (all): out_pts / out_scales / out_rots, g_feat / g_pts / g_scales / g_rots and a gradient per
    W_KEYS name."""
    rows = [t if keep is None else t[keep] for t in (case.feat, case.pts, case.scales, case.rots)]
    feat, pts, scales, rots = (t.to(dtype, copy=True).requires_grad_(True) for t in rows)
    W = {k: case.W[k].to(dtype, copy=True).requires_grad_(True) for k in W_KEYS}
    dx, ds, dr = D.mlp_heads(feat, W)
    o_pts = D.quat2mat5(dx[:, 3:]).bmm((pts + dx[:, 0:3]).view(-1, 3, 1)).view(-1, 3)
    o_scl = scales + torch.clamp(ds, -LOG100, LOG100)
    o_rot = D.quat_mul_normalized(rots + dr, dx[:, 3:])
    torch.autograd.backward([o_pts, o_scl, o_rot], [(c if keep is None else c[keep]).to(dtype) for c in case.cots])
    out = {"out_pts": o_pts.detach(), "out_scales": o_scl.detach(), "out_rots": o_rot.detach(), "g_feat": feat.grad,
           "g_pts": pts.grad, "g_scales": scales.grad, "g_rots": rots.grad}
    out.update({k: W[k].grad for k in W_KEYS})
    return out


@functools.lru_cache(maxsize=None)
def mlp_reference(name):
    """(float64, fp32) references of a case, computed once and shared: leave them unchanged."""
    case = mlp_case(name)
    return mlp_eval(case, torch.float64), mlp_eval(case, torch.float32)
