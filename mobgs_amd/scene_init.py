"""Building a Gaussian set from data: what the reference does before its first render().

    knn3_mean_dist2(points)                       simple_knn._C.distCUDA2 (CUDA-only upstream) -> csrc/knn.hip
    inverse_cubic_hermite(curves, times, N_pts)   /root/reference/scene/gaussian_model.py:18-88
    scene_initialization(viewpoints, ...)         /root/reference/train.py:58-199 -> csrc/scene_seed.hip
    static_init(...) / dynamic_init(...)          the tensors of create_from_pcd (:495-582) / create_from_pcd_dynamic
                                                  (:406-493), as the constructor dictionaries of
                                                  densify.TrainableGaussians (from_pcd / from_pcd_dynamic)

The 3-NN kernel is exact for any row order and prunes by boxes of consecutive rows; `knn3_mean_dist2` hands it the
points sorted along a 63-bit Morton curve (21 bits per axis over the cloud's bounding cube, one torch.sort) and
scatters the result back.  The spline fit of the reference is one least-squares problem per point over a design
matrix that is the same for every point in every call the reference makes: that case is one float64
pseudo-inverse on the host and one matrix product on the device.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream

SH_C0 = 0.28209479177387814   # utils/sh_utils.py:26
CONTROL_NUM = 12              # GaussianModel.control_num (:111)


# ---- 3-NN mean squared distance ----------------------------------------------------------------------------------
def morton_order(points: torch.Tensor) -> torch.Tensor:
    """int64 [N]: the rows of `points` [N,3] along a Z-order curve, 21 bits per axis over the bounding CUBE (one scale
    for the three axes: cells stay cubes in space, however flat the cloud).  rendering.spatial_order is the 10-bit
    precedent; at 1 M points 10 bits leave hundreds of points per cell."""
    m = points.detach().reshape(-1, 3).to(torch.float32)
    lo, hi = m.min(0).values, m.max(0).values
    scale = 2097151.0 / (hi - lo).max().clamp_min(1e-30)
    q = ((m - lo) * scale).clamp_(0, 2097151).to(torch.int64)

    def spread(v):  # 21 bits -> every third bit
        v = (v | (v << 32)) & 0x1F00000000FFFF
        v = (v | (v << 16)) & 0x1F0000FF0000FF
        v = (v | (v << 8)) & 0x100F00F00F00F00F
        v = (v | (v << 4)) & 0x10C30C30C30C30C3
        v = (v | (v << 2)) & 0x1249249249249249
        return v
    code = spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2)
    return torch.argsort(code)


def knn3_sorted(points: torch.Tensor) -> torch.Tensor:
    """mobgs_knn3_mean_dist2 on the rows as they are (fast when neighbouring rows are neighbours in space)."""
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be [N,3], got {tuple(points.shape)}")
    lib = _lib.load()
    pts = _lib.f32c(points.detach())
    n = int(pts.shape[0])
    p = ptr(pts)   # (raises for CPU tensors: there is no CPU path)
    nbytes = int(lib.mobgs_knn3_scratch_bytes(n))
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=pts.device)
    out = torch.empty(n, dtype=torch.float32, device=pts.device)
    check(lib.mobgs_knn3_mean_dist2(n, p, ptr(out), ptr(scratch), nbytes, stream()), "mobgs_knn3_mean_dist2")
    return out


def knn3_mean_dist2(points: torch.Tensor) -> torch.Tensor:
    """[N] float32: for every point the mean of the squared distances to its three nearest neighbours (the point itself
    excluded by index; fp32 (dx dx + dy dy) + dz dz).  Exact, bit-reproducible and independent of the row order."""
    if not points.is_cuda:
        raise RuntimeError("mobgs_amd: tensors must live on a HIP device (device='cuda'); there is no CPU path")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be [N,3], got {tuple(points.shape)}")
    pts = _lib.f32c(points.detach())
    if pts.shape[0] < 4:
        return knn3_sorted(pts)   # refused by the library with its message, before any launch
    order = morton_order(pts)
    d_sorted = knn3_sorted(pts[order])
    out = torch.empty_like(d_sorted)
    out[order] = d_sorted
    return out


# ---- spline fit ----------------------------------------------------------------------------------------------------
def hermite_design(times: torch.Tensor, N_pts: int) -> torch.Tensor:
    """float64 [..., T, N_pts]: row t holds the weights with which the N_pts control points give the cubic Hermite spline
    at times[..., t] (gaussian_model.py:24-81: segment index clamped to [0, N-2], neighbours clamped to [0, N-1],
    one-sided derivatives where the clamp bites)."""
    N = int(N_pts)
    ts = times.to(torch.float64) * (N - 1)
    idx = torch.clamp(torch.floor(ts).long(), 0, N - 2)
    il = torch.clamp(idx - 1, 0, N - 1)
    ir = torch.clamp(idx + 1, 0, N - 1)
    irr = torch.clamp(idx + 2, 0, N - 1)
    t = ts - idx.to(torch.float64)
    h00 = (1 + 2 * t) * (1 - t) ** 2
    h10 = t * (1 - t) ** 2
    h01 = t ** 2 * (3 - 2 * t)
    h11 = t ** 2 * (t - 1)
    zero = torch.zeros_like(t)
    first, last = il == idx, irr == ir
    p0 = torch.where(first, zero, -h10 / 2)
    p1 = h00 + torch.where(first, -h10, zero) + torch.where(last, -h11, -h11 / 2)
    p2 = h01 + torch.where(first, h10, h10 / 2) + torch.where(last, h11, zero)
    p3 = torch.where(last, zero, h11 / 2)
    A = torch.zeros(tuple(times.shape) + (N,), dtype=torch.float64, device=times.device)
    for i, c in ((il, p0), (idx, p1), (ir, p2), (irr, p3)):
        A.scatter_add_(-1, i[..., None], c[..., None])
    return A


def _times_2d(times: torch.Tensor, B: int) -> torch.Tensor:
    t = times
    if t.dim() == 3 and t.shape[-1] == 1:
        t = t[..., 0]
    if t.dim() == 1:
        t = t[None, :].expand(B, -1)
    if t.dim() != 2 or t.shape[0] != B:
        raise ValueError(f"times must be [B,T,1], [B,T] or [T] with B = {B}, got {tuple(times.shape)}")
    return t


def inverse_cubic_hermite(curves: torch.Tensor, times: torch.Tensor, N_pts: int = CONTROL_NUM, scale: float = 0.8,
                          return_error: bool = False):
    """gaussian_model.py:18-88: control points [B, N_pts, C] of the cubic Hermite splines that fit `curves` [B, T, C]
    sampled at `times` [B, T, 1] in the least-squares sense.  (`scale` is unused there too.)

    Shared times -- one vector expanded over the batch, as in every call the reference makes (:436-439) -- take no
    per-point factorisation: one float64 pseudo-inverse of the [T, N_pts] design matrix on the host, applied to the
    whole batch with one float64 matrix product on the curves' device.  Rows with differing times go through a
    batched float64 torch.linalg.lstsq (correct, not fast).  A rank-deficient design (T < N_pts among others) raises
    ValueError: the reference returns whatever its LAPACK driver makes of it."""
    if curves.dim() != 3:
        raise ValueError(f"curves must be [B,T,C], got {tuple(curves.shape)}")
    B, T, _ = curves.shape
    N = int(N_pts)
    t2 = _times_2d(times, B)
    if t2.shape[1] != T:
        raise ValueError(f"times has {t2.shape[1]} samples, curves {T}")
    if N < 2:
        raise ValueError("N_pts must be at least 2")
    if T < N:
        raise ValueError(f"rank-deficient fit: {T} samples cannot determine {N} control points")
    shared = B <= 1 or t2.stride(0) == 0 or bool((t2 == t2[:1]).all())
    if shared:
        A = hermite_design(t2[0].detach().cpu(), N)                      # [T, N] float64, host
        if int(torch.linalg.matrix_rank(A)) < N:
            raise ValueError(f"rank-deficient fit: the [{T}, {N}] design matrix of these times has rank "
                             f"{int(torch.linalg.matrix_rank(A))}")
        pinv = torch.linalg.pinv(A).to(curves.device)                    # [N, T]
        sol = torch.einsum("kt,btc->bkc", pinv, curves.detach().to(torch.float64))
    else:
        A = hermite_design(t2.detach(), N)                               # [B, T, N] float64
        rank = torch.linalg.matrix_rank(A)
        if bool((rank < N).any()):
            raise ValueError(f"rank-deficient fit: {int((rank < N).sum())} of {B} design matrices have rank < {N}")
        sol = torch.linalg.lstsq(A, curves.detach().to(torch.float64)).solution
    control = sol.to(curves.dtype)
    if return_error:
        alt = torch.linalg.pinv(hermite_design(t2.detach(), N)) @ curves.detach().to(torch.float64)
        return control, torch.dist(sol, alt).to(curves.dtype)
    return control


# ---- the initial state of a set ------------------------------------------------------------------------------------
def _pcd_tensors(pcd) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    # (a tensor may live on the device -- scene_initialization leaves its clouds there -- np.asarray cannot read those)
    f = lambda a: (a.detach() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))).float().cpu()  # noqa: E731
    points, colors, times = f(pcd.points), f(pcd.colors), f(pcd.times)
    if points.dim() != 2 or points.shape[1] != 3 or colors.shape != points.shape:
        raise ValueError(f"pcd.points / pcd.colors must be [N,3], got {tuple(points.shape)} / {tuple(colors.shape)}")
    return points, colors, times.reshape(points.shape[0], -1)


def _common_init(pcd, device, sh_degree: int, trbfslinit: Optional[float]):
    """The part create_from_pcd and create_from_pcd_dynamic share (:408-425 / :497-519, :445-476 / :534-565).  A point
    cloud arrives on the host; the closed-form tensors (RGB -> SH, the opacity constant) are formed there, so that they
    are the reference's values to the bit, and copied once.  Only the scales are computed on the device."""
    points, colors, times = _pcd_tensors(pcd)
    n = points.shape[0]
    sh = ((colors - 0.5) / SH_C0).to(device)
    points = points.to(device)
    dist2 = torch.clamp_min(knn3_mean_dist2(points), 0.0000001)
    z = lambda *s: torch.zeros(n, *s, dtype=torch.float32, device=device)  # noqa: E731
    rots = z(4)
    rots[:, 0] = 1
    tenth = 0.1 * torch.ones(n, 1, dtype=torch.float)
    params = {"xyz": points, "scaling": torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3), "rotation": rots,
              "opacity": torch.log(tenth / (1 - tenth)).to(device), "features_dc": torch.cat((sh, sh), dim=1),
              "features_t": z(3)}
    extras = {"omega": z(4), "zeta": z(1), "motion": z(9), "trbf_center": times.contiguous().to(device),
              "trbf_scale": torch.full((n, 1), 0.0 if trbfslinit is None else float(trbfslinit), dtype=torch.float32,
                                       device=device),
              "f_rest": z((sh_degree + 1) ** 2, 3),
              "current_control_num": torch.full((n, 1), CONTROL_NUM, dtype=torch.int64, device=device)}
    return params, extras


def static_init(pcd, device="cuda", sh_degree: int = 0, trbfslinit: Optional[float] = None
                ) -> Tuple[Dict[str, torch.Tensor], Dict[str, torch.Tensor]]:
    """(params, extras) of create_from_pcd.  control_xyz is absent: the reference fills it with random numbers (:527)
    that nothing reads for a static set, GaussianParams' default stands in."""
    return _common_init(pcd, device, sh_degree, trbfslinit)


def dynamic_init(pcd, dyn_tracjectory, device="cuda", sh_degree: int = 0, trbfslinit: Optional[float] = None
                 ) -> Tuple[Dict[str, torch.Tensor], Dict[str, torch.Tensor]]:
    """(params, extras) of create_from_pcd_dynamic: as the static set, plus the control points fitted to the tracked
    trajectories [N, T, 3] at T uniform times (:436-440)."""
    params, extras = _common_init(pcd, device, sh_degree, trbfslinit)
    traj = torch.as_tensor(dyn_tracjectory).float().to(device)
    n = params["xyz"].shape[0]
    if traj.dim() != 3 or traj.shape[0] != n or traj.shape[2] != 3:
        raise ValueError(f"dyn_tracjectory must be [{n}, T, 3], got {tuple(traj.shape)}")
    T = traj.shape[1]
    time_step = 1 / (T - 1.0)
    t_step = torch.arange(0, 1 + time_step, time_step).float()[:T].to(device)
    t_step = t_step[None, :, None].expand(n, -1, -1)
    extras["control_xyz"] = inverse_cubic_hermite(traj * 1e2, t_step, N_pts=CONTROL_NUM)
    return params, extras


# ---- motion-adaptive splines: one control point down -----------------------------------------------------------------
MIN_CONTROL_NUM = 4           # onedown_control_pts floors the count here (:279)
_one_down_cache: Dict[str, torch.Tensor] = {}


def one_down_design(n: int) -> torch.Tensor:
    """float64 [n, n-1]: the design matrix of refitting a spline of n control points (knot times k / (n - 1)) with
    n - 1 points: rows 0..n-1 / columns 0..n-2 of the [12, 11] system of inverse_cubic_hermite_for_prune (:310-371); its
    remaining rows only force the remaining columns to zero."""
    n = int(n)
    if not MIN_CONTROL_NUM < n <= CONTROL_NUM:
        raise ValueError(f"one_down_design: n must be in {MIN_CONTROL_NUM + 1}..{CONTROL_NUM}, got {n}")
    return hermite_design(torch.arange(n, dtype=torch.float64) / (n - 1), n - 1)


def one_down_tables(device=None) -> torch.Tensor:
    """float32 [8, 11, 12] (cached, host copy + one per device): block n - 5 holds pinv(one_down_design(n)) in its
    first n - 1 rows and n columns, zeros elsewhere, so that new[:11] = table[n - 5] @ old[:12] whatever the unused slots
    of a row hold once they are masked.  Built in float64.  A rank-deficient design raises ValueError."""
    if "cpu" not in _one_down_cache:
        table = torch.zeros(CONTROL_NUM - MIN_CONTROL_NUM, CONTROL_NUM - 1, CONTROL_NUM, dtype=torch.float64)
        for n in range(MIN_CONTROL_NUM + 1, CONTROL_NUM + 1):
            A = one_down_design(n)
            rank = int(torch.linalg.matrix_rank(A))
            if rank < n - 1:
                raise ValueError(f"rank-deficient fit: the [{n}, {n - 1}] one-down design matrix has rank {rank}")
            table[n - 5, :n - 1, :n] = torch.linalg.pinv(A)
        _one_down_cache["cpu"] = table.float().contiguous()
    if device is None or torch.device(device).type == "cpu":
        return _one_down_cache["cpu"]
    key = str(torch.device(device))
    if key not in _one_down_cache:
        _one_down_cache[key] = _one_down_cache["cpu"].to(device)
    return _one_down_cache[key]


def _one_down_launch(control_xyz, control_num, viewmats, times, focal, cx, cy, threshold, want_new: bool, commit: bool):
    """mobgs_control_onedown on tensors that are already what the kernel wants.  -> (error [N], new [N,11,3] | None,
    counters int32 [2] = (rows pruned, rows with a count outside 4..12)); no host synchronisation."""
    ptr(control_xyz), ptr(control_num)   # (raises for CPU tensors: there is no CPU path)
    if control_xyz.dim() != 3 or tuple(control_xyz.shape[1:]) != (CONTROL_NUM, 3) or control_xyz.dtype != torch.float32:
        raise ValueError(f"control_xyz must be float32 [N,{CONTROL_NUM},3], got {control_xyz.dtype} "
                         f"{tuple(control_xyz.shape)}")
    n = int(control_xyz.shape[0])
    if control_num.dtype != torch.int64 or control_num.numel() != n:
        raise ValueError(f"current_control_num must be int64 with {n} entries, got {control_num.dtype} "
                         f"{tuple(control_num.shape)}")
    dev = control_xyz.device
    viewmats = _lib.f32c(viewmats.detach().to(dev))
    times = _lib.f32c(times.detach().to(dev)).reshape(-1)
    V = int(times.shape[0])
    if tuple(viewmats.shape) != (V, 4, 4):
        raise ValueError(f"viewmats must be [{V},4,4] for {V} times, got {tuple(viewmats.shape)}")
    err = torch.empty(n, dtype=torch.float32, device=dev)
    new = torch.empty(n, CONTROL_NUM - 1, 3, dtype=torch.float32, device=dev) if want_new else None
    counters = torch.zeros(2, dtype=torch.int32, device=dev)
    if n == 0:   # (an empty tensor has no address to hand over)
        return err, new, counters
    check(_lib.load().mobgs_control_onedown(n, V, ptr(viewmats), ptr(times), float(focal), float(cx), float(cy),
                                            ptr(one_down_tables(dev)), float(threshold), ptr(control_xyz),
                                            ptr(control_num), ptr(err),
                                            ptr(new), ptr(counters), 1 if commit else 0, stream()),
          "mobgs_control_onedown")
    return err, new, counters


def _raise_on_bad_counts(counters: torch.Tensor) -> None:
    bad = int(counters[1])
    if bad:
        raise ValueError(f"current_control_num: {bad} rows hold a count outside {MIN_CONTROL_NUM}..{CONTROL_NUM} "
                         "(reported by mobgs_control_onedown; those rows were skipped)")


def one_down_fit(control_xyz: torch.Tensor, current_control_num: torch.Tensor, viewmats: torch.Tensor,
                 times: torch.Tensor, focal: float, width: float, height: float
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Dry run of onedown_control_pts: (new_control [N,11,3], new_num [N,1], error [N]) and no input is written.
    viewmats [V,4,4] are world-to-camera matrices in the column-vector convention (the TRANSPOSE of the reference's
    world_view_transform), times [V]; the first and the last view are skipped and K = [focal, focal, width / 2,
    height / 2] as in compute_prune_error (:292-308).  Rows whose count is already 4 report their own points, their own
    count and error 0.  Checks the counts on the host (one read-back): a count outside 4..12 raises ValueError."""
    ctrl = _lib.f32c(control_xyz.detach())
    num = current_control_num.detach().contiguous()
    err, new, counters = _one_down_launch(ctrl, num, viewmats, times, focal, width / 2, height / 2, 0.0, True, False)
    _raise_on_bad_counts(counters)
    flat = num.reshape(-1)
    new_num = torch.where(flat > MIN_CONTROL_NUM, flat - 1, flat).reshape(-1, 1)
    return new, new_num, err


_last_counters: Optional[torch.Tensor] = None   # device counters of the last onedown_control_pts call


def check_last_prune() -> None:
    """Raise ValueError if the last onedown_control_pts met a count outside 4..12 (it skipped those rows).  The call
    itself does not synchronise; this does."""
    if _last_counters is not None:
        _raise_on_bad_counts(_last_counters)


def viewpoint_arrays(viewpoints, device) -> Tuple[torch.Tensor, torch.Tensor, float, float, float]:
    """(viewmats [V,4,4], times [V], focal, cx, cy) read from cameras exactly as compute_prune_error reads them
    (:293-304): fx = fy = viewpoints[0].metadata.focal_length, cx = image_width / 2, cy = image_height / 2 (not the
    principal point), viewpoint.time, and world_view_transform, which holds the transposed world-to-camera matrix."""
    if len(viewpoints) < 3:
        raise ValueError(f"onedown_control_pts needs at least 3 viewpoints (the first and the last are skipped), got "
                         f"{len(viewpoints)}")
    v0 = viewpoints[0]
    focal = float(v0.metadata.focal_length)
    cx, cy = float(v0.image_width / 2), float(v0.image_height / 2)
    # stacked on the target device: matrices that already live there (the reference keeps them on the GPU) are not read back
    mats = torch.stack([torch.as_tensor(v.world_view_transform).detach().to(device=device, dtype=torch.float32)
                        for v in viewpoints])
    times = torch.tensor([float(v.time) for v in viewpoints], dtype=torch.float32).to(device)
    return mats.transpose(1, 2).contiguous(), times, focal, cx, cy


@torch.no_grad()
def onedown_control_pts(pc, viewpoints, error_threshold: Optional[float] = None) -> torch.Tensor:
    """GaussianModel.onedown_control_pts (:274-290) for any object with `control_xyz` [N,12,3] and
    `current_control_num` [N,1] (an unchanged reference GaussianModel included): every row with more than 4 control
    points is refitted with one point fewer, and keeps the shorter spline -- count n - 1, fitted points in slots
    0..n-2, zeros up to slot 10, slot 11 untouched -- where the mean pixel distance between the two trajectories over
    the interior `viewpoints` is at most `error_threshold` (default: pc.error_threshold, else 1.0).  In place, one
    launch, no host synchronisation and nothing printed.  -> the number of rows pruned, a 0-dim int32 device tensor.

    Deliberately unlike the reference: rows that already have 4 points are left bit for bit as they are (the reference
    refits them with 4 points against a dummy equation that pins the fourth one, which halves it).  The Adam moments of
    control_xyz are left alone, as in the reference.  A count outside 4..12 makes the kernel skip the row and count it;
    check_last_prune() raises for it.  With an fp32 master (`control_xyz.master`, GaussianParams.enable_fp32_masters)
    the master is pruned and copied into the stored tensor."""
    stored = pc.control_xyz
    master = getattr(stored, "master", None)
    target = master if master is not None else stored
    if target.dtype != torch.float32 or not target.is_contiguous():
        raise ValueError("onedown_control_pts: control_xyz (or its master) must be a contiguous float32 tensor; it is "
                         "written in place")
    num = pc.current_control_num
    if not num.is_contiguous():
        raise ValueError("onedown_control_pts: current_control_num must be contiguous; it is written in place")
    thr = error_threshold if error_threshold is not None else getattr(pc, "error_threshold", 1.0)
    mats, times, focal, cx, cy = viewpoint_arrays(viewpoints, target.device)
    _, _, counters = _one_down_launch(target.detach(), num.detach(), mats, times, focal, cx, cy, thr, False, True)
    # the kernel wrote through raw pointers: move the version counters so that caches keyed on them see it
    torch.autograd.graph.increment_version(target)
    torch.autograd.graph.increment_version(num)
    if master is not None:
        stored.detach().copy_(master)
    global _last_counters
    _last_counters = counters
    return counters[0]


# ---- seeding the two sets from depth maps, poses and 2-D tracks ------------------------------------------------------
class SeedMaps(NamedTuple):
    accum_error: torch.Tensor    # [V,H,W] float32: the masked photometric error summed over all views
    inconsistent: torch.Tensor   # [V,H,W] uint8: accum_error > the view's own mean
    cls: torch.Tensor            # [V,H,W] uint8: 0 static candidate, 1 dynamic candidate, 2 neither
    points: torch.Tensor         # [V,H,W,3] float32: the world point of every pixel


class PointCloud(NamedTuple):
    """The fields of the reference's BasicPointCloud (utils/graphics_utils.py)."""
    points: torch.Tensor
    colors: torch.Tensor
    normals: None
    times: torch.Tensor


def _rt64(w2c: torch.Tensor, K: torch.Tensor):
    w = torch.as_tensor(w2c).detach().to("cpu", torch.float64)
    k = torch.as_tensor(K).detach().to("cpu", torch.float64)
    if w.dim() != 3 or tuple(w.shape[1:]) != (3, 4) or tuple(k.shape) != (w.shape[0], 3, 3):
        raise ValueError(f"w2c must be [V,3,4] and K [V,3,3], got {tuple(w.shape)} and {tuple(k.shape)}")
    return w[:, :, :3], w[:, :, 3], k


def pair_table(w2c: torch.Tensor, K: torch.Tensor) -> torch.Tensor:
    """float32 [V,V,12] on the host: entry (i, j) is the row-major 3x4 matrix K_j [R_j R_i^T | t_j - R_j R_i^T t_i] K_i^-1
    that takes (d u, d v, d, 1) of pixel (u, v) with depth d in view i to the homogeneous pixel of view j.  Formed in
    float64 and rounded once, as one_down_tables is."""
    R, t, k = _rt64(w2c, K)
    Rij = torch.einsum("jab,icb->ijac", R, R)                        # R_j R_i^T
    A = torch.einsum("jab,ijbc,icd->ijad", k, Rij, torch.linalg.inv(k))
    b = torch.einsum("jab,ijb->ija", k, t[None, :, :] - torch.einsum("ijab,ib->ija", Rij, t))
    V = R.shape[0]
    return torch.cat([A, b[..., None]], dim=-1).reshape(V, V, 12).float().contiguous()


def unproject_table(w2c: torch.Tensor, K: torch.Tensor) -> torch.Tensor:
    """float32 [V,12] on the host: the row-major 3x4 matrix [R_i^T K_i^-1 | -R_i^T t_i] (float64, rounded once) that takes
    (d u, d v, d, 1) to the world point of the pixel (points_from_DRTK)."""
    R, t, k = _rt64(w2c, K)
    Rt = R.transpose(1, 2)
    A = Rt @ torch.linalg.inv(k)
    b = -(Rt @ t[..., None])
    return torch.cat([A, b], dim=-1).reshape(-1, 12).float().contiguous()


def nearest_pixel(u: torch.Tensor) -> torch.Tensor:
    """The pixel that grid_sample(mode="nearest", align_corners=False) reads for the pixel coordinate u after the
    reference's u / W * 2 - 1 (train.py:184-187): nearbyint(u - 0.5), ties to even."""
    return torch.round(u - 0.5)


def _check_views(images, depths, w2c, K, motion=None):
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f"images must be [V,3,H,W], got {tuple(images.shape)}")
    V, _, H, W = images.shape
    if V < 2:
        raise ValueError(f"scene seeding compares every view with the others: at least 2 views are needed, got {V}")
    if H < 2 or W < 2:
        raise ValueError(f"images must be at least 2 x 2 pixels, got {H} x {W}")
    if tuple(depths.shape) != (V, H, W):
        raise ValueError(f"depths must be [{V},{H},{W}] like the images, got {tuple(depths.shape)}")
    if tuple(w2c.shape) != (V, 3, 4) or tuple(K.shape) != (V, 3, 3):
        raise ValueError(f"w2c must be [{V},3,4] and K [{V},3,3], got {tuple(w2c.shape)} and {tuple(K.shape)}")
    if motion is not None and tuple(motion.shape) != (V, H, W):
        raise ValueError(f"motion_masks must be [{V},{H},{W}], got {tuple(motion.shape)}")
    # one read-back; everything after it is enqueued without another
    if not bool((torch.isfinite(depths) & (depths > 0)).all()):
        raise ValueError("depths must be finite and positive everywhere (a pixel without depth has no world point)")
    return V, H, W


def _motion_bytes(motion: torch.Tensor) -> torch.Tensor:
    """uint8: 0 where the mask is exactly 0, 1 where it is exactly 1, 2 elsewhere (the reference selects with
    `motion_error == 0` / `== 1`, train.py:132-139: any other value is in neither set)."""
    two = torch.full(motion.shape, 2, dtype=torch.uint8, device=motion.device)
    return torch.where(motion == 0, torch.zeros_like(two), torch.where(motion == 1, torch.ones_like(two), two))


def _seed_maps_host(images, depths, w2c, K, motion):
    """The float64 composition for tensors on the host (no kernel runs there): the reference's own steps, view by view.
    One of three statements of the sampling rules, with csrc/scene_seed.hip and tests/seed_restatement.py: they change
    together."""
    V, _, H, W = images.shape
    img, d = images.double(), depths.double()
    R, t, k = _rt64(w2c, K)
    vv, uu = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    pix = torch.stack([uu, vv, torch.ones_like(uu)], 0).reshape(3, -1)
    accum = torch.zeros(V, H * W, dtype=torch.float64)
    points = torch.empty(V, H * W, 3, dtype=torch.float64)
    for i in range(V):
        cam = (torch.linalg.inv(k[i]) @ pix) * d[i].reshape(1, -1)
        world = R[i].T @ cam - (R[i].T @ t[i])[:, None]
        points[i] = world.T
        for j in range(V):
            c2 = R[j] @ world + t[j][:, None]
            z = torch.where(c2[2].abs() < 1e-6, torch.full_like(c2[2], 1e-6), c2[2])
            p2 = k[j] @ (c2 / z)
            xn, yn = 2 * p2[0] / (W - 1) - 1, 2 * p2[1] / (H - 1) - 1
            inside = (xn >= -1) & (xn <= 1) & (yn >= -1) & (yn <= 1)
            ix, iy = (xn + 1) / 2 * (W - 1), (yn + 1) / 2 * (H - 1)
            x0, y0 = torch.floor(ix), torch.floor(iy)
            s = torch.zeros(3, H * W, dtype=torch.float64)
            for ox, oy in ((0, 0), (1, 0), (0, 1), (1, 1)):
                xs, ys = x0 + ox, y0 + oy
                w = (1 - (ix - xs).abs()) * (1 - (iy - ys).abs())
                ok = inside & (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
                at = (ys.clamp(0, H - 1) * W + xs.clamp(0, W - 1)).long()
                at = torch.where(ok, at, torch.zeros_like(at))
                s = s + torch.where(ok, w, torch.zeros_like(w)) * img[j].reshape(3, -1)[:, at]
            mask = (s.sum(0) > 0).double()
            accum[i] += (mask * (s - img[i].reshape(3, -1)).abs()).mean(0)
    mean = accum.mean(1)
    inc = accum > mean[:, None]
    mo = motion.reshape(V, -1)
    cls = torch.full((V, H * W), 2, dtype=torch.uint8)
    cls[~inc & (mo == 0)] = 0
    cls[inc & (mo == 1)] = 1
    return (accum.float().reshape(V, H, W), mean.float(), inc.to(torch.uint8).reshape(V, H, W), cls.reshape(V, H, W),
            points.float().reshape(V, H, W, 3))


def _seed_launch(images, depths, w2c, K, motion):
    """-> (accum_error, mean [V], inconsistent, cls, points).  Device tensors: mobgs_seed_consistency, then
    mobgs_seed_classify, on the current stream.  Host tensors: the float64 composition."""
    images, depths = _lib.f32c(images.detach()), _lib.f32c(depths.detach())
    V, H, W = _check_views(images, depths, w2c, K, motion)
    dev = images.device
    mbytes = torch.zeros(V, H, W, dtype=torch.uint8, device=dev) if motion is None else \
        _motion_bytes(motion.detach().to(dev)).contiguous()
    if not images.is_cuda:
        return _seed_maps_host(images, depths, w2c, K, mbytes)
    depths = depths.to(dev)
    lib = _lib.load()
    nbytes = int(lib.mobgs_seed_scratch_bytes(V, H, W))
    if nbytes == 0:
        raise ValueError(f"scene seeding: {V} views of {H} x {W} pixels are outside what mobgs_seed_* accepts "
                         "(2..4096 views, H * W <= 2^28)")
    pairs, unproj = pair_table(w2c, K).to(dev), unproject_table(w2c, K).to(dev)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    accum = torch.empty(V, H, W, dtype=torch.float32, device=dev)
    check(lib.mobgs_seed_consistency(V, H, W, ptr(images), ptr(depths), ptr(pairs), ptr(accum), ptr(scratch), nbytes,
                                     stream()), "mobgs_seed_consistency")
    inc = torch.empty(V, H, W, dtype=torch.uint8, device=dev)
    cls = torch.empty(V, H, W, dtype=torch.uint8, device=dev)
    points = torch.empty(V, H, W, 3, dtype=torch.float32, device=dev)
    mean = torch.empty(V, dtype=torch.float32, device=dev)
    check(lib.mobgs_seed_classify(V, H, W, ptr(accum), ptr(scratch), nbytes, ptr(depths), ptr(mbytes), ptr(unproj),
                                  ptr(inc), ptr(cls), ptr(points), ptr(mean), stream()), "mobgs_seed_classify")
    return accum, mean, inc, cls, points


@torch.no_grad()
def view_consistency(images: torch.Tensor, depths: torch.Tensor, w2c: torch.Tensor, K: torch.Tensor
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(accum_error [V,H,W], mean [V]): every view warped into every other through the target's depth map, the masked
    photometric error summed per target pixel (train.py:90-108), and its mean per view.  images [V,3,H,W], depths
    [V,H,W] (finite, positive), w2c [V,3,4], K [V,3,3]."""
    accum, mean, _, _, _ = _seed_launch(images, depths, w2c, K, None)
    return accum, mean


@torch.no_grad()
def seed_maps(images: torch.Tensor, depths: torch.Tensor, w2c: torch.Tensor, K: torch.Tensor,
              motion_masks: torch.Tensor) -> SeedMaps:
    """view_consistency plus, per pixel, the thresholded error, the candidate class against `motion_masks` [V,H,W]
    (0 = still, 1 = moving) and the world point (train.py:108-158).  Two launches, one read-back (the depth check)."""
    accum, _, inc, cls, points = _seed_launch(images, depths, w2c, K, motion_masks)
    return SeedMaps(accum, inc, cls, points)


@torch.no_grad()
def track_trajectories(coords: torch.Tensor, tracklet: torch.Tensor, points: torch.Tensor
                       ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(track_index [N] int32, trajectory [N,T,3]): for every pixel coordinate coords[n] the track whose start
    tracklet[0] is nearest (fp32 squared distance, ties to the lowest index), and points[t] read at that track's position
    in every frame t (nearest_pixel; zeros where the track has left the image).  tracklet [T,M,2], points [V,H,W,3] with
    T == V (train.py:171-189)."""
    if points.dim() != 4 or points.shape[3] != 3:
        raise ValueError(f"points must be [V,H,W,3], got {tuple(points.shape)}")
    V, H, W, _ = points.shape
    if tracklet.dim() != 3 or tracklet.shape[2] != 2 or tracklet.shape[1] < 1:
        raise ValueError(f"tracklet must be [T,M,2] with M >= 1, got {tuple(tracklet.shape)}")
    T, M, _ = tracklet.shape
    if T != V:
        raise ValueError(f"the tracklet has {T} frames and the point maps {V} views: one frame per view is needed")
    if coords.dim() != 2 or coords.shape[1] != 2:
        raise ValueError(f"coords must be [N,2], got {tuple(coords.shape)}")
    dev = points.device
    coords, tracklet = _lib.f32c(coords.detach().to(dev)), _lib.f32c(tracklet.detach().to(dev))
    points = _lib.f32c(points.detach())
    N = int(coords.shape[0])
    if not points.is_cuda:
        d = torch.square(coords[:, None, :] - tracklet[0][None]).sum(-1)       # fp32, as the reference forms it
        index = d.argmin(-1)
        uv = tracklet[:, index, :].double()                                    # [T,N,2]
        x, y = nearest_pixel(uv[..., 0]), nearest_pixel(uv[..., 1])
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        at = torch.where(ok, y * W + x, torch.zeros_like(x)).long()
        got = torch.gather(points.reshape(V, H * W, 3), 1, at[..., None].expand(-1, -1, 3))
        got = torch.where(ok[..., None], got, torch.zeros_like(got))
        return index.to(torch.int32), got.permute(1, 0, 2).contiguous()
    index = torch.empty(N, dtype=torch.int32, device=dev)
    traj = torch.empty(N, T, 3, dtype=torch.float32, device=dev)
    if N:
        check(_lib.load().mobgs_seed_trajectories(N, T, M, V, H, W, ptr(coords), ptr(tracklet), ptr(points), ptr(index),
                                                  ptr(traj), stream()), "mobgs_seed_trajectories")
    return index, traj


def seed_view_arrays(viewpoints, device=None):
    """(images [V,3,H,W], depths [V,H,W], w2c [V,3,4] float64 host, K [V,3,3] float64 host, motion [V,H,W], times [V],
    tracklet [T,M,2]) read from cameras as scene_initialization reads them (train.py:71-99,128,171): original_image,
    depth, R (stored transposed: the world-to-camera rotation is R.T), T, focal, metadata.principal_point_x / _y, mask,
    time, and the tracklet of the FIRST view."""
    if len(viewpoints) < 2:
        raise ValueError(f"scene_initialization compares every view with the others: at least 2 viewpoints are "
                         f"needed, got {len(viewpoints)}")
    shapes = {tuple(v.original_image.shape) for v in viewpoints}
    if len(shapes) != 1:
        raise ValueError(f"all views must have one image size, got {sorted(shapes)}")
    dev = torch.device(device) if device is not None else viewpoints[0].original_image.device
    T_ = lambda a: a.detach() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))  # noqa: E731
    images = torch.stack([T_(v.original_image).to(dev, torch.float32) for v in viewpoints])
    V, _, H, W = images.shape
    depths = torch.stack([T_(v.depth).to(dev, torch.float32).reshape(H, W) for v in viewpoints])
    motion = torch.stack([T_(v.mask).to(dev, torch.float32).reshape(H, W) for v in viewpoints])
    w2c = torch.zeros(V, 3, 4, dtype=torch.float64)
    K = torch.zeros(V, 3, 3, dtype=torch.float64)
    for i, v in enumerate(viewpoints):
        w2c[i, :, :3] = T_(v.R).to("cpu", torch.float64).T
        w2c[i, :, 3] = T_(v.T).to("cpu", torch.float64)
        K[i, 0, 0] = K[i, 1, 1] = float(v.focal)
        K[i, 0, 2], K[i, 1, 2] = float(v.metadata.principal_point_x), float(v.metadata.principal_point_y)
        K[i, 2, 2] = 1.0
    times = torch.tensor([float(v.time) for v in viewpoints], dtype=torch.float32)
    tracklet = T_(viewpoints[0].tracklet).to(dev, torch.float32)
    if tracklet.dim() != 3 or tracklet.shape[0] != V:
        raise ValueError(f"the tracklet of the first view must be [T,M,2] with one frame per view (T = {V}), got "
                         f"{tuple(tracklet.shape)}")
    return images, depths, w2c, K, motion, times, tracklet


@torch.no_grad()
def scene_initialization(viewpoints, stat_npts: int, dyn_npts: int, *, generator: Optional[torch.Generator] = None,
                         select=None, device=None):
    """The reference's scene_initialization (train.py:58-199) -> (stat_pc, dyn_pc, dyn_tracjectory), ready for
    TrainableGaussians.from_pcd(stat_pc, ...) and from_pcd_dynamic(dyn_pc, ..., dyn_tracjectory).  The clouds carry the
    fields of BasicPointCloud; their tensors stay on the device of the images (or `device`).

    Static points are drawn without replacement from the static candidates of ALL views (in view order, row-major inside
    a view, as the reference concatenates them); dynamic points from the dynamic candidates of view 0 only, with
    replacement when there are fewer than `dyn_npts`.  The draw comes from `generator` (torch; the reference uses
    Python's `random`, whose sequence is not reproduced); `select=(stat_idx, dyn_idx)` -- indices into the two candidate
    lists -- replaces it: `stat_npts` and `dyn_npts` are then unused (the clouds have as many points as `select` names) and
    only the indices' range is checked.  `device` moves the views there first (default: where the first image lives).  Raises ValueError for fewer than 2 views, a tracklet whose frame count is not the view
    count, mixed image sizes, a depth that is not finite and positive, more static points asked for than there are
    candidates, and no dynamic candidate at all."""
    images, depths, w2c, K, motion, times, tracklet = seed_view_arrays(viewpoints, device)
    V, _, H, W = images.shape
    maps = seed_maps(images, depths, w2c, K, motion)
    dev = images.device
    stat_flat = torch.nonzero(maps.cls.reshape(-1) == 0).reshape(-1)          # index into [V * H * W]
    dyn_flat = torch.nonzero(maps.cls[0].reshape(-1) == 1).reshape(-1)        # view 0: index into [H * W]
    n_stat, n_dyn = int(stat_flat.shape[0]), int(dyn_flat.shape[0])
    if select is not None:
        stat_idx = torch.as_tensor(np.asarray(select[0])).long().reshape(-1)
        dyn_idx = torch.as_tensor(np.asarray(select[1])).long().reshape(-1)
        if stat_idx.numel() and not (0 <= int(stat_idx.min()) and int(stat_idx.max()) < n_stat):
            raise ValueError(f"select: static indices must lie in 0..{n_stat - 1}")
        if n_dyn == 0 or (dyn_idx.numel() and not (0 <= int(dyn_idx.min()) and int(dyn_idx.max()) < n_dyn)):
            raise ValueError(f"select: dynamic indices must lie in 0..{n_dyn - 1}")
    else:
        if int(stat_npts) > n_stat:
            raise ValueError(f"stat_npts = {stat_npts} but only {n_stat} static candidates exist (pixels that are "
                             "consistent across the views and outside the motion masks)")
        if n_dyn == 0:
            raise ValueError("no dynamic candidate in the first view (no pixel is both inconsistent across the views "
                             "and inside its motion mask)")
        stat_idx = torch.randperm(n_stat, generator=generator)[:int(stat_npts)]
        if n_dyn < int(dyn_npts):
            dyn_idx = torch.randint(n_dyn, (int(dyn_npts),), generator=generator)
        else:
            dyn_idx = torch.randperm(n_dyn, generator=generator)[:int(dyn_npts)]
    stat_at, dyn_at = stat_flat[stat_idx.to(dev)], dyn_flat[dyn_idx.to(dev)]
    colors = images.permute(0, 2, 3, 1).reshape(-1, 3)
    points = maps.points.reshape(-1, 3)
    times = times.to(dev)
    stat_pc = PointCloud(points=points[stat_at], colors=colors[stat_at], normals=None,
                         times=times[torch.div(stat_at, H * W, rounding_mode="floor")].reshape(-1, 1))
    dyn_pc = PointCloud(points=points[dyn_at], colors=colors[dyn_at], normals=None,
                        times=times[0].expand(dyn_at.shape[0]).reshape(-1, 1).contiguous())
    coords = torch.stack([dyn_at % W, torch.div(dyn_at, W, rounding_mode="floor")], dim=1).to(torch.float32)
    _, trajectory = track_trajectories(coords, tracklet, maps.points)
    return stat_pc, dyn_pc, trajectory
