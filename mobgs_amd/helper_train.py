"""The densification controller of the reference's training loop (/root/reference/helper_train.py:167-258 and
/root/reference/train.py:634-648, :809-820), under the reference's names and argument order.

    batch_densification_stats(stat, dyn, outs, W, H)      train.py:634-648 + :813-817   one launch per set, or one in all
    message_densification_stats(stat, dyn, slots, W, H)   the same from the gradient message of the sharded loop
    DensificationController(opt, extent).step(it, s, d)   train.py:206-228 + :819-820     the loop's state and schedule
    controlgaussians(opt, gaussians, 2, iteration, ...)   helper_train.py:222-258       the schedule of mode 2
    removeminmax(gaussians, maxbounds, minbounds)         helper_train.py:167-180
    densification_step(opt, iteration, stat, dyn, ...)    train.py:809-820              both of the above, both sets

The statistics of an iteration are formed ONCE over the views of its batch: the screen-space gradients are summed over
the views first (fp32, in view order), scaled by W / 2 and H / 2, and the norm of that sum is accumulated -- not the sum
of the per-view norms; the radii are the maximum and the visibility the union over the views
(mobgs_densify_stats_batch, csrc/densify_ctl.hip).  Every resize goes through TrainableGaussians' planned methods
(mobgs_densify_plan: two launches and one read-back of four counts)."""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import check, ptr, stream

MAX_VIEWS = _lib._DEFINES["MOBGS_STATS_MAX_VIEWS"]   # include/mobgs_hip.h: the kernel's table has as many slots


def controlgaussians(opt, gaussians, densify, iteration, scene, visibility_filter, radii, viewspace_point_tensor, flag,
                     traincamerawithdistance=None, maxbounds=None, minbounds=None, type='', is_dynamic=False, *,
                     samples=None):
    """helper_train.py:183-289 for densify == 2, the mode train.py:208 fixes.  -> flag.

    While iteration < opt.densify_until_iter: at iterations past opt.densify_from_iter that opt.densification_interval
    divides, either clone + split (while flag < opt.desicnt; the gradient threshold is halved for the dynamic set, two
    children per split parent, and only the static set's calls count in flag) or the opacity prune at opt.opthr; and
    reset_opacity() whenever 3000 divides the iteration.  size_threshold is computed and passed on nowhere, as the
    reference computes it and its densify_pruneclone ignores it.  `scene` is read for .cameras_extent only;
    visibility_filter, radii, viewspace_point_tensor, traincamerawithdistance, the bounds and `type` are unused in this
    mode, as in the reference.  samples (keyword, not in the reference): explicit normal samples for the split children.

    torch.cuda.empty_cache() is NOT called after the prune: the table lives in capacity-sized buffers that a resize
    does not free, and returning the allocator's cache costs a device synchronisation.

    Modes 1 and 3 raise NotImplementedError: mode 1 needs the omega freeze (zero_omegabymotion and the gradient masks of
    freezweightsbymasknounsqueeze), mode 3 stops in a breakpoint() before its first resize in the reference."""
    if densify == 1:
        raise NotImplementedError("controlgaussians: densify = 1 needs the omega freeze (zero_omegabymotion, "
                                  "freezweightsbymasknounsqueeze), which is not ported; train.py fixes densify = 2")
    if densify == 3:
        raise NotImplementedError("controlgaussians: densify = 3 stops in a breakpoint() before its first resize in "
                                  "the reference (helper_train.py:274); train.py fixes densify = 2")
    if densify != 2:
        raise NotImplementedError(f"controlgaussians: densify = {densify!r} (the reference returns None here)")
    if iteration < opt.densify_until_iter:
        if iteration > opt.densify_from_iter and iteration % opt.densification_interval == 0:
            if flag < opt.desicnt:
                size_threshold = 20 if iteration > opt.opacity_reset_interval else None  # noqa: F841 (unused, as there)
                grad_thres = opt.densify_grad_threshold * 5e-1 if is_dynamic else opt.densify_grad_threshold
                gaussians.pruneclone_planned(grad_thres, scene.cameras_extent, splitN=2, samples=samples)
                if not is_dynamic:
                    flag += 1
            else:
                gaussians.prune_opacity_below(opt.opthr)
        if iteration % 3000 == 0:
            gaussians.reset_opacity()
    return flag


def removeminmax(gaussians, maxbounds, minbounds):
    """helper_train.py:167-180: drop the rows with a coordinate strictly outside the box.  The bounds may be 0-dim device
    tensors, as train.py:217-228 makes them; they are not read back (no .item()), and the cache is not emptied."""
    gaussians.prune_outside(minbounds, maxbounds)


def _set_rows(pc) -> int:
    return int(pc.get_xyz.shape[0])


def _stats_sets(stat, dyn, ns, nd, g_tab, grad_stride, r_tab, encoding, width, height):
    """mobgs_densify_stats_sets on rows [0, ns) for the static and [ns, ns + nd) for the dynamic set: one launch."""
    check(_lib.load().mobgs_densify_stats_sets(
        len(g_tab), g_tab, int(grad_stride), r_tab, _lib._DEFINES[encoding], float(width) * 0.5, float(height) * 0.5,
        0, ns, ptr(stat.xyz_gradient_accum), ptr(stat.denom), ptr(stat.max_radii2D),
        ns, nd, ptr(dyn.xyz_gradient_accum), ptr(dyn.denom), ptr(dyn.max_radii2D), stream()), "mobgs_densify_stats_sets")


def message_densification_stats(stat, dyn, slots, width, height):
    """batch_densification_stats on the gradient message of the sharded loop: `slots` are the statistics slots of the
    batch's views (FlatGradients.extra(name), 3 N fp32 each, N = both sets' rows) AFTER the all-reduce, as
    SubframeShard.put_densification_stats filled them -- the first 2 N floats the [N, 2] gradient rows, the last N the radii
    as fp32-coded integers.  ONE launch reads them where they lie (no slice copy, no cast, no compare) and updates both
    sets.  The sum over ranks put the owner's numbers next to zeros, so the result is bit for bit what
    batch_densification_stats gives the owner."""
    ns, nd = _set_rows(stat), _set_rows(dyn)
    n = ns + nd
    if not 1 <= len(slots) <= MAX_VIEWS:
        raise ValueError(f"message_densification_stats: {len(slots)} views (1 .. {MAX_VIEWS})")
    for k, slot in enumerate(slots):
        if slot.dim() != 1 or slot.shape[0] != 3 * n or slot.dtype != torch.float32 or slot.stride(0) != 1:
            raise ValueError(f"message_densification_stats: slot {k} is {slot.dtype} {tuple(slot.shape)} with stride "
                             f"{slot.stride()}; {3 * n} contiguous float32 are needed for {ns} + {nd} rows")
        if not slot.is_cuda:
            raise RuntimeError(f"message_densification_stats: {_lib.NO_CPU_PATH}")
    K = len(slots)
    g_tab = (ctypes.c_void_p * K)(*[s.data_ptr() for s in slots])
    r_tab = (ctypes.c_void_p * K)(*[s.data_ptr() + 8 * n for s in slots])
    _stats_sets(stat, dyn, ns, nd, g_tab, 2, r_tab, "MOBGS_RADII_FP32", width, height)


def batch_densification_stats(stat, dyn, outs, width, height, want_outputs=False, one_launch=False):
    """train.py:634-648 and :813-817.  outs: the mid-exposure render dict of every view of the batch (render() or
    render_many(); 1 .. 16 views), after backward.  One launch per set updates its xyz_gradient_accum, denom and
    max_radii2D.  want_outputs: -> ((grad [n,2], visibility [n] bool, radii [n] int32) of the static set, the same of the
    dynamic set), what train.py:819-820 passes on to controlgaussians; otherwise None.
    one_launch=True: both sets in ONE launch (mobgs_densify_stats_sets), the same bits; it has no optional outputs, so
    want_outputs must stay False.

    The kernel validates nothing, so this raises ValueError on: no view or more than 16, a view without a gradient, row
    counts that differ from the two sets' total, gradients that are not fp32 rows of one common stride with unit inner
    stride, radii that are not contiguous int32."""
    from .gaussian_renderer import viewspace_grad
    ns, nd = _set_rows(stat), _set_rows(dyn)
    if one_launch and want_outputs:
        raise ValueError("batch_densification_stats: one_launch=True has no optional outputs (want_outputs=False)")
    if not 1 <= len(outs) <= MAX_VIEWS:
        raise ValueError(f"batch_densification_stats: {len(outs)} views (1 .. {MAX_VIEWS})")
    grads, radii = [], []
    for k, out in enumerate(outs):
        g, r = viewspace_grad(out), out["radii"]
        if g is None:
            raise ValueError(f"batch_densification_stats: view {k} has no gradient yet (call it after backward)")
        if g.dim() != 2 or g.shape[0] != ns + nd or g.shape[1] < 2 or r.dim() != 1 or r.shape[0] != ns + nd:
            raise ValueError(f"batch_densification_stats: view {k} has gradients {tuple(g.shape)} and radii "
                             f"{tuple(r.shape)}, the sets have {ns} + {nd} rows")
        if g.dtype != torch.float32 or r.dtype != torch.int32:
            raise ValueError(f"batch_densification_stats: view {k} has {g.dtype} gradients and {r.dtype} radii "
                             "(float32 and int32)")
        if g.stride(1) != 1 or g.stride(0) < 2 or g.stride(0) != (grads[0].stride(0) if grads else g.stride(0)) \
                or r.stride(0) != 1:
            raise ValueError(f"batch_densification_stats: view {k} has gradient strides {g.stride()} and radii stride "
                             f"{r.stride()}: rows of one common stride with unit inner stride are needed")
        if not (g.is_cuda and r.is_cuda):
            raise RuntimeError(f"batch_densification_stats: {_lib.NO_CPU_PATH}")
        grads.append(g)
        radii.append(r)
    K = len(outs)
    g_tab = (ctypes.c_void_p * K)(*[g.data_ptr() for g in grads])
    r_tab = (ctypes.c_void_p * K)(*[r.data_ptr() for r in radii])
    lib, dev = _lib.load(), grads[0].device
    if one_launch:
        _stats_sets(stat, dyn, ns, nd, g_tab, grads[0].stride(0), r_tab, "MOBGS_RADII_INT32", width, height)
        return None
    triples = []
    for pc, row0, n in ((stat, 0, ns), (dyn, ns, nd)):
        extra = (None, None, None)
        if want_outputs:
            extra = (torch.empty(n, 2, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                     torch.empty(n, dtype=torch.uint8, device=dev))
        check(lib.mobgs_densify_stats_batch(K, g_tab, grads[0].stride(0), r_tab, row0, n, float(width) * 0.5,
                                            float(height) * 0.5, ptr(pc.xyz_gradient_accum), ptr(pc.denom),
                                            ptr(pc.max_radii2D), *[ptr(t) for t in extra], stream()),
              "mobgs_densify_stats_batch")
        if want_outputs:
            triples.append((extra[0], extra[2].view(torch.bool), extra[1]))
    return tuple(triples) if want_outputs else None


def densification_step(opt, iteration, stat, dyn, outs, width, height, scene, flags, bounds=None):
    """train.py:809-820 whole (the caller skips it in the "warm" stage, as :810 does): while iteration <
    opt.densify_until_iter, the batch statistics of both sets, then controlgaussians(densify = 2) for the dynamic set and
    for the static set, in the reference's order.  flags = (flag_d, flag_s) -> (flag_d, flag_s).
    bounds (optional): (maxbounds_d, minbounds_d, maxbounds_s, minbounds_s), handed through as the reference hands them."""
    flag_d, flag_s = flags
    max_d, min_d, max_s, min_s = bounds if bounds is not None else (None, None, None, None)
    with torch.no_grad():
        if iteration < opt.densify_until_iter:
            batch_densification_stats(stat, dyn, outs, width, height)
            # (mode 2 reads none of visibility_filter, radii, viewspace_point_tensor: they are not materialised)
            flag_d = controlgaussians(opt, dyn, 2, iteration, scene, None, None, None, flag_d,
                                      traincamerawithdistance=None, maxbounds=max_d, minbounds=min_d, is_dynamic=True)
            flag_s = controlgaussians(opt, stat, 2, iteration, scene, None, None, None, flag_s,
                                      traincamerawithdistance=None, maxbounds=max_s, minbounds=min_s)
    return flag_d, flag_s


def scheduled_operations(opt, iteration, flag):
    """The operations controlgaussians(opt, ., 2, iteration, ., flag) performs, in its order: a subset of
    ("pruneclone" | "prune_opacity", "reset_opacity")."""
    ops = []
    if iteration < opt.densify_until_iter:
        if iteration > opt.densify_from_iter and iteration % opt.densification_interval == 0:
            ops.append("pruneclone" if flag < opt.desicnt else "prune_opacity")
        if iteration % 3000 == 0:
            ops.append("reset_opacity")
    return ops


class DensificationController:
    """What train.py:206-228 and :809-820 keep in local variables around controlgaussians, as one object a loop owns:
    flag_d and flag_s, the two pairs of bounds (torch.amax / amin of each set's positions, 0-dim device tensors that are
    never read back, taken when the sets are handed over), scene.cameras_extent and the options.

        step(iteration, stat, dyn) -> bool   controlgaussians(densify = 2) for the dynamic set, then for the static set
                                             (train.py:819-820); True when a table was resized or had its opacity reset,
                                             i.e. when the sets' Parameters are new objects
        log                                  one record per operation: [iteration, "dyn" | "stat", operation, rows before,
                                             rows after, the set's flag before the call]
        state_dict() / load_state_dict()     plain numbers and lists: fits save_training_state(counters=...)

    The statistics of an iteration are not formed here (batch_densification_stats / message_densification_stats inside
    the iteration, where the gradients are)."""

    def __init__(self, opt, cameras_extent, stat=None, dyn=None):
        import types
        self.opt = opt
        self.scene = types.SimpleNamespace(cameras_extent=float(cameras_extent))
        self.flag_d = self.flag_s = 0
        self.log = []
        self.maxbounds_d = self.minbounds_d = self.maxbounds_s = self.minbounds_s = None
        if dyn is not None:
            self.maxbounds_d, self.minbounds_d = self._bounds(dyn)
        if stat is not None:
            self.maxbounds_s, self.minbounds_s = self._bounds(stat)

    @staticmethod
    def _bounds(pc):
        with torch.no_grad():
            xyz = pc._xyz
            if xyz.shape[0] == 0:
                return None, None
            return ([torch.amax(xyz[:, k]) for k in range(3)], [torch.amin(xyz[:, k]) for k in range(3)])

    def _control(self, iteration, pc, name, flag, is_dynamic, maxbounds, minbounds):
        ops = scheduled_operations(self.opt, iteration, flag)
        rows = _set_rows(pc)
        new_flag = controlgaussians(self.opt, pc, 2, iteration, self.scene, None, None, None, flag,
                                    traincamerawithdistance=None, maxbounds=maxbounds, minbounds=minbounds,
                                    is_dynamic=is_dynamic)
        after = _set_rows(pc)
        for k, op in enumerate(ops):   # (a reset follows the resize of its iteration and moves no row)
            self.log.append([int(iteration), name, op, rows if k == 0 else after, after, int(flag)])
        return new_flag, bool(ops)

    def due(self, iteration) -> bool:
        """Whether step(iteration, ...) will operate on a table: a loop that replays a recorded iteration asks before it
        brings its optimisers' host state up to date."""
        return bool(scheduled_operations(self.opt, iteration, self.flag_d)
                    or scheduled_operations(self.opt, iteration, self.flag_s))

    def step(self, iteration, stat, dyn) -> bool:
        with torch.no_grad():
            self.flag_d, changed_d = self._control(iteration, dyn, "dyn", self.flag_d, True, self.maxbounds_d,
                                                   self.minbounds_d)
            self.flag_s, changed_s = self._control(iteration, stat, "stat", self.flag_s, False, self.maxbounds_s,
                                                   self.minbounds_s)
        return changed_d or changed_s

    def state_dict(self) -> dict:
        host = lambda b: None if b is None else [float(x) for x in b]  # noqa: E731  (a read-back: between iterations)
        return {"flag_d": int(self.flag_d), "flag_s": int(self.flag_s), "cameras_extent": self.scene.cameras_extent,
                "log": [list(r) for r in self.log],
                "bounds": [host(self.maxbounds_d), host(self.minbounds_d), host(self.maxbounds_s), host(self.minbounds_s)]}

    def load_state_dict(self, state: dict, device=None):
        self.flag_d, self.flag_s = int(state["flag_d"]), int(state["flag_s"])
        self.scene.cameras_extent = float(state["cameras_extent"])
        self.log = [list(r) for r in state["log"]]
        dev = lambda b: None if b is None else [torch.tensor(x, dtype=torch.float32, device=device) for x in b]  # noqa: E731
        self.maxbounds_d, self.minbounds_d, self.maxbounds_s, self.minbounds_s = (dev(b) for b in state["bounds"])
        return self
