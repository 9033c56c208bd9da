"""Grid regularisers of the HexPlane (boundary B1): the reference's `scene/regulation.py:13-28` (compute_plane_tv,
compute_plane_smoothness) and `GaussianModel.compute_regulation` (`scene/gaussian_model.py:1373-1415`) on the HIP path.

    from mobgs_amd.regulation import grid_regulation
    loss = loss + grid_regulation(net.deformation_net.grid.grids, time_smoothness_weight, l1_time_planes_weight,
                                  plane_tv_weight)

`grids` is a list of levels.  A level of 6 planes has them in itertools.combinations(range(4), 2) order: 0, 1 and 3 are
spatial, 2, 4 and 5 carry time along dim 2 (h); a level of exactly 3 planes contributes nothing to any term.

    plane = sum of compute_plane_smoothness over planes 0, 1, 3      (the reference weighs it with plane_tv_weight, but it
                                                                      is the smoothness function, along h only: kept)
    time  = sum of compute_plane_smoothness over planes 2, 4, 5
    l1    = sum of mean |1 - t| over planes 2, 4, 5                  (d/dt = -sign(1 - t) with sign(0) = 0, as torch.abs
                                                                      has it: fresh time planes are exactly 1 and get a
                                                                      zero l1 gradient)
    compute_regulation = plane_tv_weight plane + time_smoothness_weight time + l1_time_planes_weight l1

Device tensors: every plane of a call goes through ONE autograd node -- one streaming launch plus a one-workgroup finish
forward, one launch backward (csrc/gridreg.hip), no plane-sized temporaries; a plane's gradient comes back with a
channels-last parameter's own strides.  The weights are read from device memory: Python floats are uploaded once per
distinct triple (warm a call up before recording it into a graph), 0-d device tensors are stacked; they get no gradient.
CPU tensors take the same terms composed from torch ops, so the same functions run in the CPU tests.
"""
from __future__ import annotations

from typing import List, Sequence

import torch

from . import _lib
from ._lib import check, ptr, stream

SPATIAL_PLANES, TIME_PLANES = (0, 1, 3), (2, 4, 5)
NAN_BELOW_3 = ("compute_plane_smoothness needs h >= 3 (dim 2): the reference takes the mean of an empty tensor there "
               "and yields NaN")


# ---- the CPU path: the same terms from plain torch ops (also the composition scripts/bench_deform.py times) -----------
def _diff(t, dim):
    """Neighbour differences t[k + 1] - t[k] along dim, one fp32 subtraction each."""
    n = t.shape[dim]
    return t.narrow(dim, 1, n - 1) - t.narrow(dim, 0, n - 1)


def _smoothness_torch(t):
    """Mean square of the second difference along dim 2, the second difference taken of the first."""
    return _diff(_diff(t, 2), 2).square().mean()


def _tv_torch(t):
    """Twice the sum over both image directions of (sum of squared neighbour differences) / (their number + 1e-6)."""
    total = 0.0
    for dim in (2, 3):
        d = _diff(t, dim)
        total = total + d.square().sum() / (d.numel() + 1e-6)
    return 2 * total


def _l1_torch(t):
    return (1 - t).abs().mean()


# ---- the device path -------------------------------------------------------------------------------------------------
def _defines():
    return _lib._DEFINES


def _check_plane(t, smooth: bool):
    if not torch.is_tensor(t):
        raise TypeError("mobgs_amd.regulation: a plane must be a tensor")
    if t.dim() != 4:
        raise ValueError(f"mobgs_amd.regulation: a plane must be [B, C, h, w], got {tuple(t.shape)}")
    if min(t.shape) < 1:
        raise ValueError(f"mobgs_amd.regulation: empty plane {tuple(t.shape)}")
    if smooth and t.shape[2] < 3:
        raise ValueError(f"mobgs_amd.regulation: {NAN_BELOW_3} (got h = {t.shape[2]})")


def _kernel_view(t: torch.Tensor) -> torch.Tensor:
    """What the kernel reads: fp32 with a unit-stride direction (channels-last: stride of C is 1; NCHW: stride of w is 1);
    any other stride pattern is copied."""
    x = t.detach()
    if x.dtype != torch.float32:
        x = x.float()
    _, C, _, w = x.shape
    if not (C == 1 or x.stride(1) == 1 or w == 1 or x.stride(3) == 1) or x.data_ptr() % 4:
        x = x.contiguous()
    return x


def _grad_strides(x: torch.Tensor):
    """Dense strides of the gradient the kernel writes for x: [h][w][C] for the channels-last arm, [C][h][w] otherwise."""
    _, C, h, w = x.shape
    if C == 1 or x.stride(1) == 1:
        return (C * h * w, 1, w * C, C)
    return (C * h * w, h * w, w, 1)


def _table(views: Sequence[torch.Tensor], kinds, slots, grads=None):
    D = _defines()
    n = sum(x.shape[0] for x in views)
    if n > D["MOBGS_GRIDREG_MAX_PLANES"]:
        raise ValueError(f"mobgs_amd.regulation: {n} planes in one call, the kernel's table holds "
                         f"{D['MOBGS_GRIDREG_MAX_PLANES']}")
    tab = (_lib.MobgsGridPlane * n)()
    k = 0
    for idx, (x, kind, slot) in enumerate(zip(views, kinds, slots)):
        B, C, h, w = x.shape
        if kind == D["MOBGS_GRIDREG_TV"]:
            inv0, inv1 = 1.0 / (B * C * (h - 1) * w + 1e-6), 1.0 / (B * C * h * (w - 1) + 1e-6)
        else:
            inv0, inv1 = (1.0 / (B * C * (h - 2) * w) if h > 2 else 0.0), 1.0 / (B * C * h * w)
        for b in range(B):
            r = tab[k]
            r.t = x.data_ptr() + 4 * b * x.stride(0)
            r.grad = grads[idx].data_ptr() + 4 * b * grads[idx].stride(0) if grads is not None else None
            r.C, r.h, r.w, r.kind, r.slot = C, h, w, kind, slot
            r.sc, r.sh, r.sw = x.stride(1), x.stride(2), x.stride(3)
            r.inv0, r.inv1 = inv0, inv1
            k += 1
    return n, tab


def _alloc_grads(views):
    """The gradients as views of ONE buffer (one allocation), each starting on a 16-byte boundary."""
    offs, total = [], 0
    for x in views:
        offs.append(total)
        total += (x.numel() + 3) // 4 * 4
    flat = torch.empty(total, dtype=torch.float32, device=views[0].device)
    return [torch.as_strided(flat, tuple(x.shape), _grad_strides(x), o) for x, o in zip(views, offs)]


_plan_memo = {}


def _plan(planes, views, kinds, slots, n_slots):
    """(n, table, workgroups) of a call.  Describing 18 planes to the C ABI costs ~0.1 ms of host time, more than the
    kernels run, so the table is remembered per tuple of plane OBJECTS and reused while every one of them is the same
    object at the same address with the same shape and strides.  An entry holds weak references and numbers only: it
    keeps no storage alive, and while the plane objects live their storage cannot be handed to another tensor.  Only
    tables whose views alias the planes are kept (a converted or copied plane gets a new address every call)."""
    key = (kinds, slots, n_slots, tuple(id(p) for p in planes))
    sig = [(p.data_ptr(), p.shape, p.stride()) for p in planes]
    hit = _plan_memo.get(key)
    if hit is not None and hit[1] == sig and all(r() is p for r, p in zip(hit[0], planes)):
        return hit[2]
    n, tab = _table(views, kinds, slots)
    plan = (n, tab, _lib.load().mobgs_gridreg_blocks(n, tab, n_slots))
    if all(v.data_ptr() == p.data_ptr() and v.stride() == p.stride() for v, p in zip(views, planes)):
        import weakref
        if len(_plan_memo) > 8:
            _plan_memo.clear()
        _plan_memo[key] = ([weakref.ref(p) for p in planes], sig, plan)
    return plan


class _GridReg(torch.autograd.Function):
    """(kinds, slots, n_slots, weights [n_slots] or None, planes...) -> the weighted total (0-d) with weights, else the
    n_slots terms."""

    @staticmethod
    def forward(ctx, kinds, slots, n_slots, weights, *planes):
        lib = _lib.load()
        views = [_kernel_view(p) for p in planes]
        n, tab, blocks = _plan(planes, views, kinds, slots, n_slots)
        dev = views[0].device
        partial = torch.empty(max(blocks, 1), 2, dtype=torch.float64, device=dev)
        out = torch.empty(n_slots, dtype=torch.float32, device=dev)
        total = torch.empty((), dtype=torch.float32, device=dev) if weights is not None else None
        check(lib.mobgs_gridreg_fwd(n, tab, n_slots, ptr(weights), ptr(partial), ptr(out), ptr(total), stream()),
              "mobgs_gridreg_fwd")
        ctx.save_for_backward(*views)
        ctx.spec = (n, tab, n_slots, weights)
        ctx.dtypes = [p.dtype for p in planes]
        return total if weights is not None else out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, v_out):
        lib = _lib.load()
        n, tab, n_slots, weights = ctx.spec
        views = ctx.saved_tensors
        v_out = _lib.f32c(v_out).reshape(-1)
        grads = _alloc_grads(views)
        tab = type(tab).from_buffer_copy(tab)       # (the forward's table may be a remembered one)
        k = 0
        for g in grads:
            for b in range(g.shape[0]):
                tab[k].grad = g.data_ptr() + 4 * b * g.stride(0)
                k += 1
        check(lib.mobgs_gridreg_bwd(n, tab, n_slots, ptr(weights), ptr(v_out), stream()), "mobgs_gridreg_bwd")
        grads = [g if g.dtype == dt else g.to(dt) for g, dt in zip(grads, ctx.dtypes)]
        return (None, None, None, None, *[g if need else None for g, need in zip(grads, ctx.needs_input_grad[4:])])


_weight_memo = {}


def _weights_dev(weights, device) -> torch.Tensor:
    """[n] fp32 on the device.  Python numbers: uploaded once per distinct tuple and device.  Tensors: stacked (no gradient)."""
    if not any(torch.is_tensor(w) for w in weights):
        key = (tuple(float(w) for w in weights), str(device))
        hit = _weight_memo.get(key)
        if hit is None:
            if len(_weight_memo) > 64:
                _weight_memo.clear()
            _weight_memo[key] = hit = torch.tensor(key[0], dtype=torch.float32, device=device)
        return hit
    return torch.stack([w.detach().to(device=device, dtype=torch.float32).reshape(()) if torch.is_tensor(w)
                        else torch.tensor(float(w), dtype=torch.float32, device=device) for w in weights])


def _on_device(planes) -> bool:
    cuda = [bool(p.is_cuda) for p in planes]
    if any(cuda) and not all(cuda):
        raise RuntimeError("mobgs_amd.regulation: planes on a HIP device and on the host in one call")
    return all(cuda)


def _single(t, kind_name: str, torch_fn):
    _check_plane(t, smooth=kind_name == "MOBGS_GRIDREG_SMOOTH")
    if not t.is_cuda:
        return torch_fn(t)
    return _GridReg.apply((_defines()[kind_name],), (0,), 1, None, t).reshape(())   # (a view: no launch either way)


def compute_plane_tv(t: torch.Tensor) -> torch.Tensor:
    """scene/regulation.py:13-19: twice (sum of squared differences / (their count + 1e-6)) along h plus along w, of a
    [B, C, h, w] tensor."""
    return _single(t, "MOBGS_GRIDREG_TV", _tv_torch)


def compute_plane_smoothness(t: torch.Tensor) -> torch.Tensor:
    """scene/regulation.py:22-28: the mean squared second difference along dim 2 of a [B, C, h, w] tensor."""
    return _single(t, "MOBGS_GRIDREG_SMOOTH", _smoothness_torch)


def _split(grids) -> tuple:
    """(spatial planes, time planes) of the levels that contribute (a level of exactly 3 planes does not)."""
    spatial: List[torch.Tensor] = []
    time: List[torch.Tensor] = []
    for level in grids:
        if len(level) == 3:
            continue
        spatial += [level[i] for i in SPATIAL_PLANES]
        time += [level[i] for i in TIME_PLANES]
    for p in spatial + time:
        _check_plane(p, smooth=True)
    return spatial, time


def _terms_torch(spatial, time):
    plane = sum(_smoothness_torch(p) for p in spatial)
    tsm = sum(_smoothness_torch(p) for p in time)
    l1 = sum(_l1_torch(p) for p in time)
    return plane, tsm, l1


def _terms_device(spatial, time, weights):
    D = _defines()
    kinds = (D["MOBGS_GRIDREG_SMOOTH"],) * len(spatial) + (D["MOBGS_GRIDREG_SMOOTH_L1"],) * len(time)
    slots = (0,) * len(spatial) + (1,) * len(time)
    return _GridReg.apply(kinds, slots, 3, weights, *spatial, *time)


def _device_of(grids):
    return next((p.device for level in grids for p in level), torch.device("cpu"))


def regulation_terms(grids) -> torch.Tensor:
    """[3]: the unweighted (_plane_regulation, _time_regulation, _l1_regulation), for logging (differentiable)."""
    spatial, time = _split(grids)
    if not spatial:
        return torch.zeros(3, device=_device_of(grids))
    if not _on_device(spatial + time):
        return torch.stack(_terms_torch(spatial, time))
    return _terms_device(spatial, time, None)


def grid_regulation(grids, time_smoothness_weight, l1_time_planes_weight, plane_tv_weight) -> torch.Tensor:
    """GaussianModel.compute_regulation (scene/gaussian_model.py:1414-1415) as a 0-d tensor."""
    spatial, time = _split(grids)
    if not spatial:
        return torch.zeros((), device=_device_of(grids))
    if not _on_device(spatial + time):
        plane, tsm, l1 = _terms_torch(spatial, time)
        return plane_tv_weight * plane + time_smoothness_weight * tsm + l1_time_planes_weight * l1
    w = _weights_dev((plane_tv_weight, time_smoothness_weight, l1_time_planes_weight), spatial[0].device)
    return _terms_device(spatial, time, w)
