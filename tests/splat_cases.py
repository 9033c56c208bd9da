"""Deterministic cases for the per-splat kernels -- the projection (csrc/project.hip: project_fwd_kernel, project_bwd_kernel,
camera_sum_kernel, viewmat_reduce_kernel) and the state build (csrc/prep.hip + csrc/prep_shared.h) -- their float64 and fp32
references, and the comparators of tests/test_gpu_project_kernels.py and tests/test_gpu_prep_kernels.py.  Torch on the CPU and
the oracle only: nothing of the package under test is imported here; tests/test_splat_cases_cpu.py checks from the oracle
alone that every case reaches the edge it is named after.

Projection.  The reference is oracle.gsplat_torch.fully_fused_projection in float64 and in fp32, gradients by autograd for
random normal cotangents of means2d / depths / conics.  Splats are PLACED: rays uniform over three image widths and heights
(the frustum clamp of persp_setup starts 0.15 widths outside the image, so more than half of the rows clamp in x, in y or in
both), depths 0.5 .. 6.5, every 16th row swept across the near plane, log-normal sizes with every 7th row 8 x as large (large
splats reach into the image from outside), un-normalised anisotropic quaternions, a camera with fx != fy and an off-centre
principal point that is rotated and translated against the world (and per camera for C > 1).

Near-kink filter (as tests/deform_cases.py): candidates are drawn in excess, the float64 restatement `project_terms` looks at
them and the first N rows that are not near a kink are kept, so that fp32 and float64 take the same branch everywhere and no
comparison needs a flip allowance.  A row is near a kink when in any camera one of
  * z against near_plane / far_plane,
  * x / z, y / z against the four clamp limits,
  * 3 sqrt(v1) against an integer (the radius is its ceiling) or against radius_clip,
  * mean2d +- radius against 0 / width / height,
  * det against 0 (det <= 1e-4 a d: the difference a d - b^2 has lost four digits)
lies within 1e-4 relative of its threshold.  A case that drops more than 5 % of its candidates raises.

Prep.  The reference `prep_eval` restates prep.hip's header in any dtype on top of oracle.render_torch.hermite (pinned by
tests/golden/hermite.npz): exp, sigmoid, rotation + tfp omega un-normalised, [f_dc | tfp f_t] with the static f_t times zero,
x 1e-2, static rows first.  Its only kink is floor(t (n - 1)) and that one is NOT filtered: the spline and its control-point
gradient are continuous across a knot, so times exactly on knots are legitimate points (shown in the CPU test).

Comparators.  `close_to_f64` of tests/deform_cases.py per tensor, and per ROW within a stratum (`rows_close_to_f64`):
    e_i = |got_i - ref64_i|_inf / (|ref64_i|_inf + f),   f = 1e-3 x the median row norm of the stratum,
max_i e_i and median_i e_i each at most k x the same statistic of the fp32 reference.  The per-row maximum of the fp32
reference has a heavy tail from ill-conditioned rows, so the median carries the sharpness and the maximum catches a single
bad row.  A row whose gradient is small against the tensor's maximum is invisible to a per-tensor bound and visible here."""
import functools
import math
from types import SimpleNamespace

import torch

from deform_cases import MAX_DROP, _keep_first, close_to_f64, needed_k  # noqa: F401  (re-exported to the tests)
from oracle import gsplat_torch as G
from oracle.render_torch import hermite

EPS2D = 0.3
KINK = 1e-4
STRATA = ("ordinary", "x-clamped", "y-clamped", "both")


# ---- comparators -------------------------------------------------------------------------------------------------------
COLS = {"means2d": 2, "depths": 1, "conics": 3, "v_means": 3, "v_quats": 4, "v_scales": 3,  # elements per row
        "means": 3, "quats": 4, "scales": 3, "opac": 1, "colors": 9, "s_xyz": 3, "s_scaling": 3, "s_rotation": 4,
        "s_opacity": 1, "s_fdc": 6, "s_ft": 3, "d_control": 36, "d_scaling": 3, "d_rotation": 4, "d_omega": 4,
        "d_opacity": 1, "d_fdc": 6, "d_ft": 3}


def _rows2d(t, rows, cols):
    return t.detach().cpu().double().reshape(-1, cols)[rows]


def shrink(got, ref64, allow):
    """`got` moved towards ref64 by up to `allow` per element: a derived allowance (one rounding to half) taken off the
    difference before a comparator sees it."""
    got = got.detach().cpu().double()
    d = got - ref64
    return ref64 + torch.sign(d) * (d.abs() - allow).clamp_min(0.0)


def half_allowance(ref64):
    """One rounding of x to IEEE half: 2^-11 |x|, or half a subnormal step 2^-25."""
    return torch.maximum(2.0 ** -11 * ref64.abs(), torch.full_like(ref64, 2.0 ** -25))


def row_stats(got, ref64, rows, cols):
    """-> (max_i e_i, median_i e_i) over the rows `rows` of the tensors flattened to [-1, cols]."""
    g, r = _rows2d(got, rows, cols), _rows2d(ref64, rows, cols)
    norm = r.abs().amax(dim=1)
    err = (g - r).abs().amax(dim=1)
    den = norm + 1e-3 * float(norm.median())
    e = torch.where(den > 0, err / den.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0).double())
    return float(e.max()), float(e.median())


def _ratio(a, b):
    return 0.0 if a == 0.0 else (a / b if b > 0 else math.inf)


def needed_k_rows(got, ref64, ref32, rows, cols):
    """-> (max got, max fp32, median got, median fp32, the k this stratum needs)."""
    if rows.numel() == 0:
        return 0.0, 0.0, 0.0, 0.0, 0.0
    gmax, gmed = row_stats(got, ref64, rows, cols)
    rmax, rmed = row_stats(ref32, ref64, rows, cols)
    return gmax, rmax, gmed, rmed, max(_ratio(gmax, rmax), _ratio(gmed, rmed))


SMALL = 32  # strata with fewer rows than this are small samples (see rows_close_to_f64)


def rows_close_to_f64(got, ref64, ref32, strata, cols, k, what, k_small=None):
    """Per stratum {name: row indices of the tensors flattened to [-1, cols]}: max_i e_i <= k max_i e32_i and
    median_i e_i <= k median_i e32_i.  Prints the figures of every stratum before it asserts and returns the largest k a
    stratum needed.  k_small: the factor for strata of fewer than SMALL rows.  Two fp32 evaluations of one row that
    associate differently draw their errors independently, and the per-row error has a heavy tail: over the 10 665
    ordinary rows of `many_rows` the fp32 oracle's own e_i for the scale gradient has median 2.3e-7, 99th percentile
    1.4e-6, and the medians of two independent samples of n rows differ by more than 3 x in 1 % of the pairs up to n = 11
    (2.4 x at n = 16, 1.8 x at n = 32), their maxima by 6 x at any n -- in a large stratum the maximum sits on an
    ill-conditioned row, which is bad for every evaluation, in a small one there is none."""
    assert tuple(got.shape) == tuple(ref64.shape), f"{what}: shape {tuple(got.shape)} != {tuple(ref64.shape)}"
    worst, failed = 0.0, []
    for name, rows in strata.items():
        if rows.numel() == 0:
            continue
        kk = k_small if (k_small is not None and rows.numel() < SMALL) else k
        gmax, rmax, gmed, rmed, need = needed_k_rows(got, ref64, ref32, rows, cols)
        print(f"ROWS {what} <{name}, {rows.numel()} rows>: max {gmax:.3e} (fp32 {rmax:.3e}) median {gmed:.3e} "
              f"(fp32 {rmed:.3e}) needs k {need:.3f} (allowed {kk})")
        worst = max(worst, need)
        if not (gmax <= kk * rmax and gmed <= kk * rmed):
            failed.append(f"{name}: max {gmax:.3e} vs {kk} x {rmax:.3e}, median {gmed:.3e} vs {kk} x {rmed:.3e}")
    assert not failed, f"{what}: " + "; ".join(failed)
    return worst


def max_scaled_close(got, ref, frac=5e-4, rtol=1e-3):
    """The per-tensor rule of the end-to-end parity tests: |got - ref| <= frac max |ref| + rtol |ref| everywhere."""
    got, ref = got.detach().double(), ref.detach().double()
    return bool(((got - ref).abs() <= frac * float(ref.abs().max()) + rtol * ref.abs()).all())


# ---- projection --------------------------------------------------------------------------------------------------------
#              (N, C); the image is 160 x 96, 72 x 56 in `many_rows`
PROJ_SHAPES = {
    "n1": (1, 1), "n63": (63, 1), "n64": (64, 1), "n65": (65, 1), "n255": (255, 1), "n256": (256, 1), "n257": (257, 1),
    "n1100": (1100, 1), "n1100_only2d": (1100, 1), "n1100_onlydepth": (1100, 1), "n1100_onlyconic": (1100, 1),
    "c3_shared": (1100, 3), "c3_own": (1100, 3), "clip": (1100, 1), "all_culled": (300, 2), "many_rows": (65793, 1)}
PROJ_CASES = tuple(PROJ_SHAPES)
_SEEDS = {"n1": 3039}  # the single row is visible and clamped in x and in y (tests/test_splat_cases_cpu.py)
_ONLY = {"n1100_only2d": (True, False, False), "n1100_onlydepth": (False, True, False),
         "n1100_onlyconic": (False, False, True)}


def _rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    X = torch.tensor([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=torch.float64)
    Y = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=torch.float64)
    Z = torch.tensor([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], dtype=torch.float64)
    return Z @ Y @ X


def _rigid(R, t):
    V = torch.eye(4, dtype=torch.float64)
    V[:3, :3], V[:3, 3] = R, torch.tensor(t, dtype=torch.float64)
    return V


def _viewmats(C, roll_only):
    """Camera 0 is rotated and translated against the world; camera c > 0 against camera 0, and 3 c further back (smaller
    radii: see _draw) -- roll_only: about the optical axis, which keeps every point behind the camera behind it."""
    V0 = _rigid(_rotation(0.21, -0.33, 0.12), (0.4, -0.25, 0.6))
    out = [V0]
    for c in range(1, C):
        D = _rigid(_rotation(0.0, 0.0, 0.4 * c), (0.2 * c, -0.1, 0.1 * c)) if roll_only else \
            _rigid(_rotation(0.06 * c, -0.09 * c, 0.05 * c), (0.25 * c, -0.1 * c, 3.0 * c))
        out.append(D @ V0)
    return torch.stack(out)


def _draw(n, C, W, H, V, K, g, behind, own, small_rows=False, mu=-2.25, aniso=0.4):
    """n candidate rows in float64: placed in camera 0's frame, stored in the world's.  Sizes: log-normal, sigma 1.2 around
    e^mu per row, 0.4 per axis on top, every 7th row x 8.  mu = -2.25: the radius criterion of the near-kink filter drops
    2e-4 r of the rows per camera, r the radius in pixels, and the rows that reach into the image from outside have r of
    25 .. 1000; at mu = -2 three cameras lose 9 % of the candidates, past the 5 % cap."""
    R = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)  # noqa: E731
    Nn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    u, v = W * (3.0 * R(n) - 1.0), H * (3.0 * R(n) - 1.0)
    z = 0.5 + 6.0 * R(n)
    idx = torch.arange(n)
    if behind:
        z = -z
    else:
        sweep = idx % 16 == 5
        k = int(sweep.sum())  # (in shuffled order: keeping the first N candidates must not cut the sweep's far end off)
        z[sweep] = torch.linspace(-0.2, 0.03, k, dtype=torch.float64)[torch.randperm(k, generator=g)]
    p = torch.stack([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z], dim=1)
    means = (p - V[0, :3, 3]) @ V[0, :3, :3]  # R^T (p - t)
    scales = torch.exp(mu + 1.2 * Nn(n, 1)) * torch.exp(aniso * Nn(n, 3))
    scales[idx % 7 == 3] *= 8.0
    if small_rows:
        scales[idx % 5 == 1] *= 0.1  # (`clip`: rows for radius_clip to cull)
    quats = Nn(n, 4) * torch.tensor([1.6, 0.6, 1.0, 0.35], dtype=torch.float64) * torch.exp(0.5 * Nn(n, 1))
    if own:
        means = means[None] + 0.05 * Nn(C, n, 3)
        quats = quats[None] + 0.15 * Nn(C, n, 4)
    return means.float(), quats.float(), scales.float()


def project_terms(means, quats, scales, viewmats, Ks, width, height, near_plane, far_plane, radius_clip, dtype=torch.float64,
                  straight_x=False):
    """The statements of oracle.gsplat_torch.fully_fused_projection with their intermediate quantities kept, for geometry
    shared by the cameras ([N,3] / [N,4]) or per camera ([C,N,3] / [C,N,4]).  straight_x: a deliberately WRONG backward --
    where x / z is clamped, tx keeps its clamped value but takes the unclamped branch's derivative (d tx = d x), the two
    branches of persp_setup's vector-Jacobian product swapped for those rows."""
    means, quats, scales, V, K = (t.to(dtype) for t in (means, quats, scales, viewmats, Ks))
    C = V.shape[0]
    R, t = V[:, :3, :3], V[:, :3, 3]
    m = means if means.dim() == 3 else means[None].expand(C, -1, -1)
    q = quats if quats.dim() == 3 else quats[None].expand(C, -1, -1)
    p = torch.einsum("cij,cnj->cni", R, m) + t[:, None, :]
    M = G.quat_to_rotmat(q) * scales[None, :, None, :]
    covar_c = torch.einsum("cij,cnjk,clk->cnil", R, M @ M.transpose(-1, -2), R)
    fx, fy, cx, cy = K[:, 0, 0][:, None], K[:, 1, 1][:, None], K[:, 0, 2][:, None], K[:, 1, 2][:, None]
    x, y, z = p.unbind(-1)
    zok = (z >= near_plane) & (z <= far_plane)
    zs = torch.where(zok, z, torch.ones_like(z))
    lim_x_pos, lim_x_neg = (width - cx) / fx + 0.3 * (0.5 * width / fx), cx / fx + 0.3 * (0.5 * width / fx)
    lim_y_pos, lim_y_neg = (height - cy) / fy + 0.3 * (0.5 * height / fy), cy / fy + 0.3 * (0.5 * height / fy)
    rz = 1.0 / zs
    xr, yr = x * rz, y * rz
    tx = zs * torch.minimum(lim_x_pos, torch.maximum(-lim_x_neg, xr))
    ty = zs * torch.minimum(lim_y_pos, torch.maximum(-lim_y_neg, yr))
    x_clamped = (xr > lim_x_pos) | (xr < -lim_x_neg)
    y_clamped = (yr > lim_y_pos) | (yr < -lim_y_neg)
    if straight_x:
        tx = torch.where(x_clamped, tx.detach() + (x - x.detach()), tx)
    O = torch.zeros_like(z)
    J = torch.stack([fx * rz, O, -fx * tx * rz * rz, O, fy * rz, -fy * ty * rz * rz], dim=-1).reshape(C, -1, 2, 3)
    cov2d = J @ covar_c @ J.transpose(-1, -2)
    mean2d = torch.stack([fx * x * rz + cx, fy * y * rz + cy], dim=-1)
    a, b, d = cov2d[..., 0, 0] + EPS2D, cov2d[..., 0, 1], cov2d[..., 1, 1] + EPS2D
    det = a * d - b * b
    valid = zok & (det > 0)
    dets = torch.where(valid, det, torch.ones_like(det))
    conics = torch.stack([d / dets, -b / dets, a / dets], dim=-1)
    with torch.no_grad():
        bb = 0.5 * (a + d)
        r_cont = 3.0 * torch.sqrt(bb + torch.sqrt(torch.clamp(bb * bb - det, min=0.01)))
        radius = torch.ceil(r_cont)
        valid = valid & (radius > radius_clip) & ~((mean2d[..., 0] + radius <= 0) | (mean2d[..., 0] - radius >= width) |
                                                   (mean2d[..., 1] + radius <= 0) | (mean2d[..., 1] - radius >= height))
        radii = torch.where(valid, radius, torch.zeros_like(radius)).to(torch.int32)
    vm = valid[..., None]
    return SimpleNamespace(
        z=z, zok=zok, xr=xr, yr=yr, lims=(lim_x_pos, lim_x_neg, lim_y_pos, lim_y_neg), x_clamped=x_clamped,
        y_clamped=y_clamped, a=a, d=d, det=det, r_cont=r_cont, radius=radius, mean2d=mean2d, radii=radii,
        means2d=torch.where(vm, mean2d, torch.zeros_like(mean2d)), depths=torch.where(valid, z, torch.zeros_like(z)),
        conics=torch.where(vm, conics, torch.zeros_like(conics)))


def proj_near_kink(T, width, height, near_plane, far_plane, radius_clip):
    """[N] bool from the float64 terms T: the row is near a kink in some camera."""
    def near(v, thr):
        return (v - thr).abs() <= KINK * abs(thr) if not torch.is_tensor(thr) else (v - thr).abs() <= KINK * thr.abs()
    bad = near(T.z, near_plane) | near(T.z, far_plane)
    lxp, lxn, lyp, lyn = T.lims
    inner = near(T.xr, lxp) | near(T.xr, -lxn) | near(T.yr, lyp) | near(T.yr, -lyn)
    inner |= (T.r_cont - T.r_cont.round()).abs() <= KINK * T.r_cont
    if radius_clip > 0:
        inner |= near(T.r_cont, radius_clip)
    mx, my, r = T.mean2d[..., 0], T.mean2d[..., 1], T.radius
    for v, edge in ((mx + r, 0.0), (mx - r, float(width)), (my + r, 0.0), (my - r, float(height))):
        inner |= (v - edge).abs() <= KINK * (r + edge)
    inner |= T.det <= KINK * T.a * T.d
    return (bad | (T.zok & inner)).any(dim=0)


@functools.lru_cache(maxsize=None)
def proj_case(name):
    """-> namespace(name, N, C, W, H, near_plane, far_plane, radius_clip, own, means [N,3] | [C,N,3], quats [N,4] | [C,N,4],
    scales [N,3], viewmats [C,4,4], Ks [C,3,3], opacities [N], cots (v_means2d [C,N,2], v_depths [C,N], v_conics [C,N,3];
    None = that output gets no cotangent), dropped): fp32 CPU tensors."""
    n, C = PROJ_SHAPES[name]
    g = torch.Generator().manual_seed(_SEEDS.get(name, 3000 + PROJ_CASES.index(name)))
    W, H = (72, 56) if name == "many_rows" else (160, 96)
    far_plane, radius_clip = (5.0, 4.0) if name == "clip" else (1e10, 0.0)
    own, behind = name == "c3_own", name == "all_culled"
    fx = 0.9 * W
    K = torch.tensor([[fx, 0.0, 0.47 * W], [0.0, 1.1 * fx, 0.55 * H], [0.0, 0.0, 1.0]], dtype=torch.float64)
    V = _viewmats(C, roll_only=behind)
    cand = n + n // 8 + 64
    means, quats, scales = _draw(cand, C, W, H, V, K, g, behind, own, small_rows=name == "clip")
    V32, K32 = V.float(), K.float()[None].repeat(C, 1, 1)
    T = project_terms(means, quats, scales, V32, K32, W, H, 0.01, far_plane, radius_clip)
    keep, dropped = _keep_first(proj_near_kink(T, W, H, 0.01, far_plane, radius_clip), n, "projection case " + name)
    means, quats = means[..., keep, :].contiguous(), quats[..., keep, :].contiguous()
    cots = [torch.randn(C, n, 2, generator=g), torch.randn(C, n, generator=g), torch.randn(C, n, 3, generator=g)]
    cots = [c if use else None for c, use in zip(cots, _ONLY.get(name, (True, True, True)))]
    return SimpleNamespace(name=name, N=n, C=C, W=W, H=H, near_plane=0.01, far_plane=far_plane, radius_clip=radius_clip,
                           own=own, means=means, quats=quats, scales=scales[keep].contiguous(), viewmats=V32, Ks=K32,
                           opacities=0.05 + 0.9 * torch.rand(n, generator=g), cots=cots, dropped=dropped)


def proj_terms_of(case, dtype=torch.float64, **kw):
    return project_terms(case.means, case.quats, case.scales, case.viewmats, case.Ks, case.W, case.H, case.near_plane,
                         case.far_plane, case.radius_clip, dtype, **kw)


def proj_strata(case):
    """[C,N] long from the float64 oracle: -1 culled, else 0 ordinary / 1 x-clamped only / 2 y-clamped only / 3 both."""
    T = proj_terms_of(case)
    return torch.where(T.radii > 0, T.x_clamped.long() + 2 * T.y_clamped.long(), torch.full_like(T.radii, -1).long())


def strata_rows(code):
    """{stratum: flat row indices} of a [C,N] (per camera and row) or [N] code."""
    flat = code.reshape(-1)
    return {name: torch.nonzero(flat == i).reshape(-1) for i, name in enumerate(STRATA)}


def union_strata(code):
    """[N] code of a gradient that sums over the cameras: culled when culled in every camera, else clamped in x (y) when
    a camera that sees the row clamps it in x (y)."""
    seen = code >= 0
    xc = (seen & ((code == 1) | (code == 3))).any(dim=0)
    yc = (seen & ((code == 2) | (code == 3))).any(dim=0)
    return torch.where(seen.any(dim=0), xc.long() + 2 * yc.long(), torch.full_like(xc, -1, dtype=torch.long))


PROJ_OUTPUTS = ("means2d", "depths", "conics")
PROJ_GRADS = ("v_means", "v_quats", "v_scales")


def _backward(outs, cots, dtype):
    pairs = [(o, c.to(dtype)) for o, c in zip(outs, cots) if c is not None]
    torch.autograd.backward([o for o, _ in pairs], [c for _, c in pairs])


def proj_eval(case, dtype, project=None):
    """radii, means2d, depths, conics and v_means / v_quats / v_scales / v_viewmats of oracle.gsplat_torch's
    fully_fused_projection in `dtype` (per-camera geometry: one call per camera, the shared leaves' gradients summed by
    autograd).  project: a function of the five leaves instead (the wrong-backward variant of the CPU test)."""
    means, quats, scales, V = (t.to(dtype, copy=True).requires_grad_(True)
                               for t in (case.means, case.quats, case.scales, case.viewmats))
    Ks = case.Ks.to(dtype)
    kw = dict(eps2d=EPS2D, near_plane=case.near_plane, far_plane=case.far_plane, radius_clip=case.radius_clip)
    if project is not None:
        T = project(means, quats, scales, V, Ks)
        outs = (T.radii, T.means2d, T.depths, T.conics)
    elif case.own:
        per = [G.fully_fused_projection(means[c], None, quats[c], scales, V[c:c + 1], Ks[c:c + 1], case.W, case.H, **kw)
               for c in range(case.C)]
        outs = tuple(torch.cat([p[i] for p in per], dim=0) for i in range(4))
    else:
        outs = G.fully_fused_projection(means, None, quats, scales, V, Ks, case.W, case.H, **kw)[:4]
    _backward(outs[1:], case.cots, dtype)
    return {"radii": outs[0], "means2d": outs[1].detach(), "depths": outs[2].detach(), "conics": outs[3].detach(),
            **{"v_" + k: t.grad if t.grad is not None else torch.zeros_like(t)  # (no path: means2d / depths and quats, scales)
               for k, t in (("means", means), ("quats", quats), ("scales", scales), ("viewmats", V))}}


@functools.lru_cache(maxsize=None)
def proj_reference(name):
    """(float64, fp32) references of a case, computed once and shared: leave them unchanged."""
    case = proj_case(name)
    return proj_eval(case, torch.float64), proj_eval(case, torch.float32)


def proj_row_strata(case, key):
    """{stratum: rows} for output / gradient `key`: per (camera, row) for [C,N,.] tensors, the union over the cameras for
    the [N,.] gradients that sum over them."""
    code = proj_strata(case)
    if key in PROJ_OUTPUTS or (case.own and key in ("v_means", "v_quats")):
        return strata_rows(code)
    return strata_rows(union_strata(code))


# ---- prep --------------------------------------------------------------------------------------------------------------
LEAVES = ("s_xyz", "s_scaling", "s_rotation", "s_opacity", "s_fdc", "s_ft", "d_control", "d_scaling", "d_rotation",
          "d_omega", "d_opacity", "d_fdc", "d_ft")  # the order of ops._LEAF_NAMES and of PrepSplats' gradient buffers
HALF_LEAVES = tuple(k for k in LEAVES if k not in ("s_xyz", "d_control"))  # attributes: stored as halves in `half`
PREP_OUTPUTS = ("means", "quats", "scales", "opac", "colors")
KNOTS = tuple(range(4, 13))
T_IN = (0.37, 0.37)  # interior: 0.37 (n - 1) is no integer for n = 4 .. 12
#             (Ns, Nd)     times [2] = (t_feat, t_curve) or [K,2]
PREP_SHAPES = {
    "s0_d1": ((0, 1), T_IN), "s1_d0": ((1, 0), T_IN),
    "wave_63_2": ((63, 2), T_IN), "wave_64_64": ((64, 64), T_IN), "wave_100_157": ((100, 157), T_IN),
    "d257": ((0, 257), T_IN), "s300": ((300, 0), T_IN),
    "ends_0": ((40, 300), (0.0, 0.0)), "ends_1": ((40, 300), (1.0, 1.0)),
    "on_knots_2": ((40, 300), (1 / 2, 1 / 2)), "on_knots_3": ((40, 300), (1 / 3, 1 / 3)),
    "on_knots_4": ((40, 300), (1 / 4, 1 / 4)),
    "outside_lo": ((40, 300), (-0.3, 0.0)), "outside_hi": ((40, 300), (1.4, 1.0)),
    "k3": ((100, 157), ((0.2, 0.2), (0.55, 0.55), (1.1, 1.0))),
    "accumulate": ((100, 157), T_IN), "half": ((100, 157), T_IN)}
PREP_CASES = tuple(PREP_SHAPES)
# case: (q, the knot counts for which t = 1 / q is a knot)
ON_KNOTS = {"on_knots_2": (2, (5, 7, 9, 11)), "on_knots_3": (3, (4, 7, 10)), "on_knots_4": (4, (5, 9))}
T_SECOND = (0.81, 0.81)  # the second pass of `accumulate`


@functools.lru_cache(maxsize=None)
def prep_case(name):
    """-> namespace(name, Ns, Nd, K, times [2] | [K,2], leaves {LEAVES name: tensor}, d_ncp [Nd,1] int64 cycling through
    4 .. 12, d_trbf [Nd,1], cots (v_means, v_quats, v_scales, v_opac, v_colors), cots2 (the second pass of `accumulate`),
    half): fp32 CPU tensors (in `half` the attribute leaves hold half-representable values)."""
    (Ns, Nd), times = PREP_SHAPES[name]
    g = torch.Generator().manual_seed(4000 + PREP_CASES.index(name))
    N = Ns + Nd
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    L = {"s_xyz": 2.0 * rn(Ns, 3), "s_scaling": -2.0 + 0.8 * rn(Ns, 3), "s_rotation": rn(Ns, 4), "s_opacity": 2.0 * rn(Ns, 1),
         "s_fdc": torch.rand(Ns, 6, generator=g), "s_ft": 0.3 * rn(Ns, 3),
         "d_control": 200.0 * rn(Nd, 1, 3) + torch.cumsum(15.0 * rn(Nd, 12, 3), dim=1),  # centimetres, a random walk
         "d_scaling": -2.0 + 0.8 * rn(Nd, 3), "d_rotation": rn(Nd, 4), "d_omega": 0.5 * rn(Nd, 4),
         "d_opacity": 2.0 * rn(Nd, 1), "d_fdc": torch.rand(Nd, 6, generator=g), "d_ft": 0.3 * rn(Nd, 3)}
    half = name == "half"
    if half:
        L = {k: (v.half().float() if k in HALF_LEAVES else v) for k, v in L.items()}
    times = torch.tensor(times, dtype=torch.float32)
    lead = (times.shape[0],) if times.dim() == 2 else ()

    def cots():
        return [rn(*lead, N, 3), rn(*lead, N, 4), rn(N, 3), rn(N), rn(*lead, N, 9)]
    return SimpleNamespace(name=name, Ns=Ns, Nd=Nd, K=lead[0] if lead else 1, times=times, leaves=L,
                           d_ncp=(4 + torch.arange(Nd) % 9).reshape(Nd, 1), d_trbf=torch.rand(Nd, 1, generator=g),
                           cots=cots(), cots2=cots() if name == "accumulate" else None, half=half)


def prep_state(L, d_ncp, d_trbf, times):
    """prep.hip's header in the dtype of the leaves `L` at one instant times = (t_feat, t_curve): static rows first.
    -> means [N,3], quats [N,4] (un-normalised), scales [N,3], opac [N], colors [N,9]."""
    dtype = L["s_xyz"].dtype
    t_feat, t_curve = times.to(dtype)
    tfp = t_feat - d_trbf.to(dtype)  # [Nd,1]
    d_means = hermite(L["d_control"], t_curve, d_ncp) * 1e-2
    d_quats = L["d_rotation"] + tfp * L["d_omega"]
    d_cols = torch.cat([L["d_fdc"], tfp * L["d_ft"]], dim=1)
    s_cols = torch.cat([L["s_fdc"], 0.0 * L["s_ft"]], dim=1)
    return (torch.cat([L["s_xyz"], d_means]), torch.cat([L["s_rotation"], d_quats]),
            torch.exp(torch.cat([L["s_scaling"], L["d_scaling"]])),
            torch.sigmoid(torch.cat([L["s_opacity"], L["d_opacity"]])).squeeze(-1), torch.cat([s_cols, d_cols]))


def prep_eval(case, dtype, times=None, cots=None):
    """The five outputs (with a leading K for means / quats / colors when times is [K,2]) and the 13 leaf gradients for
    the cotangents `cots` (the case's), in `dtype`."""
    times = case.times if times is None else times
    cots = case.cots if cots is None else cots
    L = {k: v.to(dtype, copy=True).requires_grad_(True) for k, v in case.leaves.items()}
    if times.dim() == 2:
        per = [prep_state(L, case.d_ncp, case.d_trbf, t) for t in times]
        outs = [torch.stack([p[0] for p in per]), torch.stack([p[1] for p in per]), per[0][2], per[0][3],
                torch.stack([p[4] for p in per])]
    else:
        outs = list(prep_state(L, case.d_ncp, case.d_trbf, times))
    torch.autograd.backward(outs, [c.to(dtype) for c in cots])
    out = {k: o.detach() for k, o in zip(PREP_OUTPUTS, outs)}
    out.update({k: L[k].grad if L[k].grad is not None else torch.zeros_like(L[k]) for k in LEAVES})
    return out


@functools.lru_cache(maxsize=None)
def prep_reference(name):
    """(float64, fp32) references of a case, computed once and shared: leave them unchanged.  `accumulate`: the outputs
    of the first pass and the SUM of the two passes' gradients (fp32: summed in fp32, as the kernel does)."""
    case = prep_case(name)
    refs = []
    for dtype in (torch.float64, torch.float32):
        r = prep_eval(case, dtype)
        if name == "accumulate":
            r["first"] = {k: r[k] for k in LEAVES}
            second = prep_eval(case, dtype, torch.tensor(T_SECOND), case.cots2)
            r.update({k: r[k] + second[k] for k in LEAVES})
        refs.append(r)
    return tuple(refs)


def prep_row_strata(case, key):
    """{stratum: flat row indices} of output / gradient `key`: static and dynamic rows, and the dynamic rows per knot count
    where the knot count enters (means, d_control)."""
    Ns, Nd, N = case.Ns, case.Nd, case.Ns + case.Nd
    ncp = case.d_ncp.reshape(-1)
    if key in PREP_OUTPUTS:
        reps = case.K if key in ("means", "quats", "colors") else 1
        lead = (torch.arange(reps) * N)[:, None]
        on = lambda rows: (lead + rows[None, :]).reshape(-1)  # noqa: E731
        strata = {"static": on(torch.arange(Ns)), "dynamic": on(Ns + torch.arange(Nd))}
        if key == "means":
            strata.update({f"knots{n}": on(Ns + torch.nonzero(ncp == n).reshape(-1)) for n in KNOTS})
        return strata
    if key.startswith("s_"):
        return {"static": torch.arange(Ns)}
    strata = {"dynamic": torch.arange(Nd)}
    if key == "d_control":
        strata.update({f"knots{n}": torch.nonzero(ncp == n).reshape(-1) for n in KNOTS})
    return strata
