"""Densification and optimiser surgery of a Gaussian set.

`TrainableGaussians` carries the 14 per-splat optimiser groups of the reference's GaussianModel
(/root/reference/scene/gaussian_model.py:598-617), a torch.optim.Adam over them (eps 1e-15, :645) and the five
per-splat statistics arrays, and offers the reference's method names with the reference's semantics:

    training_setup(opt)                      :590-661 (per-splat groups + decoder)
    add_densification_stats(vsp_grad, vis)   :1352-1356   (+ update_max_radii(): helper_train.py:263)
    densify_and_clone(grads, thr, extent)    :1480-1506
    densify_and_splitv2(grads, thr, extent, N)   :1207-1244
    densify_pruneclone(thr, min_opacity, extent, max_screen_size, splitN)   :1417-1434
    prune_points(mask)                       :1066-1089
    onedown_control_pts(viewpoints)          :274-371 (scene_init.onedown_control_pts: csrc/control_prune.hip)
    reset_opacity()                          :897-903
    pruneclone_planned / prune_opacity_below / prune_outside   the tables of densify_pruneclone / prune_points(opacity
                                             mask) / helper_train.removeminmax from ONE plan (csrc/densify_ctl.hip, K34)

Where the reference re-allocates every group with ~50 index / cat / repeat calls per operation, every field lives
here in a capacity-sized buffer pair; a resize builds ONE row list and moves all fields (parameters, Adam moments,
statistics) with one mobgs_rows_gather launch into the other buffer of the pair.  Parameters are views [:n] of the
current buffers; as in the reference they are NEW nn.Parameter objects after each resize and the optimiser's
groups/state are re-keyed to them.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, List, Optional

import torch
from torch import nn

from . import _lib
from ._lib import check, ptr, stream
from .gaussian_model import GaussianParams

# optimiser group name -> attribute (reference :598-617); shapes per splat
GROUPS = [("xyz", "_xyz"), ("control_xyz", "control_xyz"), ("current_control_num", "current_control_num"),
          ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("f_t", "_features_t"), ("opacity", "_opacity"),
          ("scaling", "_scaling"), ("rotation", "_rotation"), ("omega", "_omega"), ("zeta", "_zeta"),
          ("trbf_center", "_trbf_center"), ("trbf_scale", "_trbf_scale"), ("motion", "_motion")]
STATS = ["xyz_gradient_accum", "denom", "max_radii2D", "_deformation_accum"]  # reset by every append
_LR = {"xyz": lambda o, s: o.position_lr_init * s, "control_xyz": lambda o, s: 10 * o.position_lr_init * s,
       "current_control_num": lambda o, s: 0.0, "f_dc": lambda o, s: o.feature_lr,
       "f_rest": lambda o, s: o.feature_lr / 20.0, "f_t": lambda o, s: o.featuret_lr,
       "opacity": lambda o, s: o.opacity_lr, "scaling": lambda o, s: o.scaling_lr,
       "rotation": lambda o, s: o.rotation_lr, "omega": lambda o, s: o.omega_lr, "zeta": lambda o, s: o.zeta_lr,
       "trbf_center": lambda o, s: o.trbfc_lr, "trbf_scale": lambda o, s: o.trbfs_lr,
       "motion": lambda o, s: o.position_lr_init * s * 0.5 * o.movelr}


class _Field:
    """One per-splat array: two capacity-sized buffers (current / spare) and the per-row shape."""

    def __init__(self, data: torch.Tensor, capacity: int, zero_new: bool):
        self.row_shape = tuple(data.shape[1:])
        self.dtype = data.dtype
        self.zero_new = zero_new
        self.buf = [torch.empty((capacity,) + self.row_shape, dtype=data.dtype, device=data.device) for _ in range(2)]
        self.cur = 0
        self.buf[0][:data.shape[0]] = data

    @property
    def row_bytes(self) -> int:
        n = 1
        for d in self.row_shape:
            n *= d
        return n * self.buf[0].element_size()

    def view(self, n: int) -> torch.Tensor:
        return self.buf[self.cur][:n]

    def grow(self, capacity: int, n: int):
        for k in range(2):
            old = self.buf[k]
            new = torch.empty((capacity,) + self.row_shape, dtype=self.dtype, device=old.device)
            if k == self.cur:
                new[:n] = old[:n]
            self.buf[k] = new


class TrainableGaussians(GaussianParams):
    def __init__(self, params: Dict[str, torch.Tensor], dynamic: Optional[Dict[str, torch.Tensor]] = None,
                 decoder=None, device="cuda", capacity_factor: float = 1.5):
        super().__init__(params, dynamic, decoder, device=device, requires_grad=False)
        n = self._xyz.shape[0]
        dev = self._xyz.device
        z = lambda *s: torch.zeros(n, *s, dtype=torch.float32, device=dev)  # noqa: E731
        dyn = dynamic or {}
        self._opacity = self._opacity.reshape(n, 1)
        self._features_rest = dyn["f_rest"].to(dev) if "f_rest" in dyn else z(0, 3)
        self._zeta = dyn["zeta"].to(dev) if "zeta" in dyn else z(1)
        self._trbf_scale = dyn["trbf_scale"].to(dev) if "trbf_scale" in dyn else z(1)
        self._motion = dyn["motion"].to(dev) if "motion" in dyn else z(9)
        self.current_control_num = self.current_control_num.reshape(n, 1)
        self._deformation_table = (dyn["_deformation_table"].to(dev) if "_deformation_table" in dyn
                                   else torch.ones(n, dtype=torch.bool, device=dev))
        self.xyz_gradient_accum, self.denom, self._deformation_accum = z(1), z(1), z(3)
        self.max_radii2D = torch.zeros(n, dtype=torch.float32, device=dev)
        self.percent_dense = 0.01
        self.spatial_lr_scale = 1.0
        self.optimizer = None
        self._n = n
        self._capacity = max(int(n * capacity_factor) + 1024, n)
        self._factor = capacity_factor
        self._fields: Dict[str, _Field] = {}
        for g, attr in GROUPS:
            self._fields[g] = _Field(getattr(self, attr).detach(), self._capacity, False)
        self._fields["_deformation_table"] = _Field(self._deformation_table.to(torch.uint8), self._capacity, False)
        for s in STATS:
            self._fields[s] = _Field(getattr(self, s), self._capacity, True)
        self._publish(rekey=False)

    # ---- views <-> attributes ------------------------------------------------------------------------------------
    def _publish(self, rekey: bool):
        """Point the reference-named attributes at the current buffers; with an optimiser, re-key its groups and
        state to the new Parameters (what replace/cat/prune do group by group in the reference)."""
        n = self._n
        groups = {gr["name"]: gr for gr in self.optimizer.param_groups} if self.optimizer is not None else {}
        for g, attr in GROUPS:
            t = self._fields[g].view(n)
            if g == "current_control_num":
                new = t  # integer knot count: a plain tensor in the reference's optimiser group too (:601)
            else:
                new = nn.Parameter(t.requires_grad_(True))
            if g in groups:
                old = groups[g]["params"][0]
                st = self.optimizer.state.pop(old, None)
                if st is not None and "exp_avg" in st:
                    st["exp_avg"] = self._fields[g + ".exp_avg"].view(n)
                    st["exp_avg_sq"] = self._fields[g + ".exp_avg_sq"].view(n)
                    self.optimizer.state[new] = st
                groups[g]["params"][0] = new
            setattr(self, attr, new)
        self._deformation_table = self._fields["_deformation_table"].view(n).view(torch.bool)
        for s in STATS:
            setattr(self, s, self._fields[s].view(n))

    def training_setup(self, training_args):
        """Per-splat groups + decoder of the reference's training_setup (:598-617, :645); the deformation / pose
        groups belong to modules outside this class and can be added with optimizer.add_param_group()."""
        self.percent_dense = training_args.percent_dense
        for s in ("xyz_gradient_accum", "denom", "_deformation_accum"):
            getattr(self, s).zero_()
        scale = self.spatial_lr_scale
        groups = [{"params": [getattr(self, attr)], "lr": _LR[g](training_args, scale), "name": g}
                  for g, attr in GROUPS]
        groups.append({"params": list(self.rgbdecoder.parameters()), "lr": training_args.rgb_lr, "name": "decoder"})
        from .optim import FusedAdam   # torch.optim.Adam whose step() is ONE launch (the caller's loop stays unchanged)
        self.optimizer = FusedAdam(groups, lr=0.0, eps=1e-15)

    # ---- learning-rate schedules (reference :625-661 and :663-680) ---------------------------------------------------
    _SCHEDULES = ("xyz_scheduler_args", "grid_scheduler_args", "deformation_scheduler_args", "pose_scheduler_args")

    def setup_schedules(self, training_args, stage="coarse"):
        """The schedules the reference's training_setup builds next to its optimiser: xyz from position_lr_init / _final,
        deformation and grid from their own pairs (all three times spatial_lr_scale), posenet from pose_lr_init (a tenth of
        it in the fine stage) / pose_lr_final; every one over position_lr_max_steps.  A schedule whose values the
        arguments do not carry is left out, and update_learning_rate() raises if a group then asks for it.
        training_setup() does not call this: its result stays what it was."""
        from .general_utils import get_expon_lr_func
        o, scale = training_args, self.spatial_lr_scale
        has = lambda *names: all(hasattr(o, n) for n in names)  # noqa: E731
        for name in self._SCHEDULES:
            self.__dict__.pop(name, None)
        if not has("position_lr_max_steps"):
            return self
        steps = o.position_lr_max_steps
        if has("position_lr_init", "position_lr_final"):
            self.xyz_scheduler_args = get_expon_lr_func(lr_init=o.position_lr_init * scale,
                                                        lr_final=o.position_lr_final * scale, max_steps=steps)
        if has("deformation_lr_init", "deformation_lr_final"):
            self.deformation_scheduler_args = get_expon_lr_func(lr_init=o.deformation_lr_init * scale,
                                                                lr_final=o.deformation_lr_final * scale, max_steps=steps)
        if has("grid_lr_init", "grid_lr_final"):
            self.grid_scheduler_args = get_expon_lr_func(lr_init=o.grid_lr_init * scale, lr_final=o.grid_lr_final * scale,
                                                         max_steps=steps)
        if has("pose_lr_init", "pose_lr_final"):
            self.pose_scheduler_args = get_expon_lr_func(
                lr_init=o.pose_lr_init / 10 if stage == "fine" else o.pose_lr_init, lr_final=o.pose_lr_final,
                max_steps=steps)
        return self

    def schedule_of(self, group_name: str):
        """The schedule update_learning_rate() applies to a group of this name (the reference's tests, in its order:
        == "xyz", "grid" in name, == "deformation", == "posenet"), or None for a group that keeps its rate."""
        if group_name == "xyz":
            attr = "xyz_scheduler_args"
        elif "grid" in group_name:
            attr = "grid_scheduler_args"
        elif group_name == "deformation":
            attr = "deformation_scheduler_args"
        elif group_name == "posenet":
            attr = "pose_scheduler_args"
        else:
            return None
        fn = getattr(self, attr, None)
        if fn is None:
            raise AttributeError(f"TrainableGaussians: the group {group_name!r} is scheduled by {attr}, which does not "
                                 "exist: call setup_schedules(training_args) with arguments that carry its rates")
        return fn

    def update_learning_rate(self, iteration):
        """gaussian_model.py:663-680: the scheduled groups' rates for this iteration."""
        for group in self.optimizer.param_groups:
            fn = self.schedule_of(group["name"])
            if fn is not None:
                group["lr"] = fn(iteration)

    def schedules(self) -> dict:
        """{(optimizer, group name): schedule} for the scheduled groups the optimiser holds now: what
        mobgs_amd.optim.DeviceAdam takes."""
        out = {}
        for group in self.optimizer.param_groups:
            fn = self.schedule_of(group["name"])
            if fn is not None:
                out[(self.optimizer, group["name"])] = fn
        return out

    def adopt_optimizer_state(self):
        """Move the Adam moments torch allocated on the first step() into table fields (so that they are resized with
        the parameters).  Called lazily by every resize."""
        n = self._n
        for gr in self.optimizer.param_groups:
            g = gr["name"]
            if g not in self._fields or len(gr["params"]) != 1:
                continue
            st = self.optimizer.state.get(gr["params"][0], None)
            if st is None or "exp_avg" not in st:
                continue
            for k in ("exp_avg", "exp_avg_sq"):
                name = f"{g}.{k}"
                f = self._fields.get(name)
                if f is None:
                    f = self._fields[name] = _Field(st[k], self._capacity, True)
                elif st[k].data_ptr() != f.view(n).data_ptr():
                    f.view(n).copy_(st[k])
                st[k] = f.view(n)

    # ---- per-step statistics ---------------------------------------------------------------------------------------
    @torch.no_grad()
    def add_densification_stats(self, viewspace_point_tensor, update_filter, radii=None):
        """gaussian_model.py:1352-1356; with `radii` also helper_train.py:263 (max_radii2D) in the same launch.
        `viewspace_point_tensor` is the GRADIENT tensor [N, >=2], as passed by train.py:814-817."""
        g = viewspace_point_tensor
        if g.dim() == 3:
            g = g[0]
        g = g if (g.dtype == torch.float32 and g.is_contiguous()) else g.float().contiguous()
        vis = update_filter.reshape(-1).to(torch.uint8) if update_filter is not None else None
        r = radii.reshape(-1).to(torch.int32).contiguous() if radii is not None else None
        check(_lib.load().mobgs_densify_stats(self._n, ptr(g), g.shape[-1], ptr(vis), ptr(r),
                                             ptr(self.xyz_gradient_accum), ptr(self.denom),
                                             ptr(self.max_radii2D) if r is not None else None, stream()),
              "mobgs_densify_stats")

    # ---- resize machinery -----------------------------------------------------------------------------------------
    def _indices_of(self, mask_u8: torch.Tensor, want: int):
        n = mask_u8.shape[0]
        idx = torch.empty(n, dtype=torch.int32, device=mask_u8.device)
        cnt = torch.empty(1, dtype=torch.int32, device=mask_u8.device)
        check(_lib.load().mobgs_mask_indices(n, ptr(mask_u8), want, ptr(idx), ptr(cnt), stream()),
              "mobgs_mask_indices")
        return idx[:int(cnt.item())]

    @torch.no_grad()
    def spatial_sort_(self) -> torch.Tensor:
        """GaussianParams.spatial_sort_ for the whole table: parameters, Adam moments and densification statistics move
        together in ONE gather.  `keep_sorted = True` makes every densification end with it."""
        from .rendering import spatial_order
        order = spatial_order(self.sort_positions()).to(torch.int32)
        self._rebuild(order, reset_stats=False)
        self.rows_coherent = self._n
        return order.long()

    keep_sorted = False

    def _rebuild(self, index: torch.Tensor, reset_stats: bool):
        """Table := rows `index` (int32; negative = NEW copy of row -(i+1)) of the current table."""
        self.rows_coherent = -1
        from . import gaussian_renderer as _GR
        _GR.parameters_changed()   # (rows move in place: no version counter sees it -- ADVICE r5)
        if self.optimizer is not None:
            self.adopt_optimizer_state()
        n_out = int(index.shape[0])
        if n_out > self._capacity:
            self._capacity = int(n_out * self._factor) + 1024
            for f in self._fields.values():
                f.grow(self._capacity, self._n)
        names = [k for k in self._fields if not (reset_stats and k in STATS)]
        fields = [self._fields[k] for k in names]
        nf = len(fields)
        src = (ctypes.c_void_p * nf)(*[f.buf[f.cur].data_ptr() for f in fields])
        dst = (ctypes.c_void_p * nf)(*[f.buf[1 - f.cur].data_ptr() for f in fields])
        rb = (ctypes.c_int32 * nf)(*[f.row_bytes for f in fields])
        zn = (ctypes.c_int32 * nf)(*[1 if f.zero_new else 0 for f in fields])
        index = index.contiguous()
        check(_lib.load().mobgs_rows_gather(nf, src, dst, rb, zn, ptr(index) if n_out else None, n_out, 0, stream()),
              "mobgs_rows_gather")
        for f in fields:
            f.cur = 1 - f.cur
        if reset_stats:
            for s in STATS:
                self._fields[s].view(n_out).zero_()
        self._n = n_out
        self._publish(rekey=True)

    def _select(self, n_grads: int, grad_threshold: float, scene_extent: float):
        n = self._n
        dev = self._xyz.device
        clone = torch.empty(n, dtype=torch.uint8, device=dev)
        split = torch.empty(n, dtype=torch.uint8, device=dev)
        check(_lib.load().mobgs_densify_select(n, n_grads, ptr(self._sel_accum), ptr(self._sel_denom),
                                              ptr(self._fields["scaling"].view(n)), float(grad_threshold),
                                              float(self.percent_dense * scene_extent), ptr(clone), ptr(split),
                                              stream()), "mobgs_densify_select")
        return clone, split

    def _grads_as_ratio(self, grads):
        """The selection kernel forms accum / denom itself; explicit `grads` [n,1] are passed as grads / 1."""
        g = grads.reshape(-1).to(torch.float32).contiguous()
        self._sel_accum, self._sel_denom = g, torch.ones_like(g)
        return g.shape[0]

    # ---- the reference's operations ----------------------------------------------------------------------------
    @torch.no_grad()
    def prune_points(self, mask):
        keep = self._indices_of(mask.reshape(-1).to(torch.uint8), 0)
        coherent = self.rows_coherent == self._n
        self._rebuild(keep, reset_stats=False)
        if coherent:  # a subsequence of ordered rows is ordered
            self.rows_coherent = self._n

    @torch.no_grad()
    def densify_and_clone(self, grads, grad_threshold, scene_extent, *_unused, **_unused_kw):
        n_grads = self._grads_as_ratio(grads)
        clone, _ = self._select(n_grads, grad_threshold, scene_extent)
        sel = self._indices_of(clone, 1)
        every = torch.arange(self._n, dtype=torch.int32, device=sel.device)
        self._rebuild(torch.cat([every, -(sel + 1)]), reset_stats=True)
        if self.keep_sorted:
            self.spatial_sort_()

    @torch.no_grad()
    def densify_and_splitv2(self, grads, grad_threshold, scene_extent, N=2, samples=None):
        n_grads = self._grads_as_ratio(grads)
        _, split = self._select(n_grads, grad_threshold, scene_extent)
        keep = self._indices_of(split, 0)
        sel = self._indices_of(split, 1)
        self._split_into(keep, [], sel, N, samples)

    def _split_into(self, keep, clones, sel, N, samples):
        parents = -(sel + 1)
        index = torch.cat([keep, *clones, *([parents] * N)])
        first = int(keep.shape[0]) + sum(int(c.shape[0]) for c in clones)
        n_children = N * int(sel.shape[0])
        if samples is None and n_children:
            stds = torch.exp(self._fields["scaling"].view(self._n)[sel.long()]).repeat(N, 1)
            samples = torch.normal(mean=torch.zeros_like(stds), std=stds)
        self._rebuild(index, reset_stats=True)
        if n_children:
            samples = samples.to(torch.float32).contiguous()
            check(_lib.load().mobgs_split_children(n_children, first, N, ptr(samples),
                                                  ptr(self._fields["rotation"].view(self._n)),
                                                  ptr(self._fields["xyz"].view(self._n)),
                                                  ptr(self._fields["scaling"].view(self._n)), stream()),
                  "mobgs_split_children")
        if self.keep_sorted:
            self.spatial_sort_()

    @torch.no_grad()
    def densify_pruneclone(self, max_grad, min_opacity, extent, max_screen_size, splitN=2, samples=None):
        """:1417-1434: clone + splitv2 on grads = xyz_gradient_accum / denom (the reference also forms a prune mask
        there and never applies it).  One selection pass and ONE gather: the result equals the two separate steps
        ([kept originals | clones | split children])."""
        self._sel_accum, self._sel_denom = self.xyz_gradient_accum.reshape(-1), self.denom.reshape(-1)
        clone, split = self._select(self._n, max_grad, extent)
        keep = self._indices_of(split, 0)
        sel = self._indices_of(split, 1)
        cl = self._indices_of(clone, 1)
        self._split_into(keep, [-(cl + 1)], sel, splitN, samples)

    # ---- planned resizes (include/mobgs_hip.h K34, csrc/densify_ctl.hip) ---------------------------------------------
    # The row list of a resize from ONE plan: two launches and one read-back of four counts, where the methods above
    # take a selection launch, up to three single-workgroup list launches with a read-back each, and arange / cat glue.
    # Everything after the list (_rebuild, the children kernel) is shared with them, so the results are the same tables.
    def _plan(self, op_name: str, n_split: int = 1, **inputs):
        """-> (index int32 [n max(2, n_split)], kept, clones, split parents, n_out) of mobgs_densify_plan on the live
        rows; the four counts come to the host in one copy."""
        n, dev = self._n, self._xyz.device
        arr = lambda k: ptr(inputs[k]) if k in inputs else None  # noqa: E731
        index = torch.empty(n * max(2, n_split), dtype=torch.int32, device=dev)
        counts = torch.empty(4, dtype=torch.int32, device=dev)
        scratch = torch.empty(3 * ((n + 1023) // 1024), dtype=torch.int32, device=dev)
        check(_lib.load().mobgs_densify_plan(
            _lib._DEFINES["MOBGS_PLAN_" + op_name], n, n_split, arr("accum"), arr("denom"), arr("scaling"),
            float(inputs.get("grad_threshold", 0.0)), float(inputs.get("size_threshold", 0.0)), arr("opacity"),
            float(inputs.get("min_opacity", 0.0)), arr("xyz"), arr("bounds"), arr("mask"),
            ptr(index) if n else None, ptr(counts), ptr(scratch) if n else None, stream()), "mobgs_densify_plan")
        kept, clones, parents, n_out = counts.tolist()
        return index, kept, clones, parents, n_out

    def _prune_planned(self, op_name: str, **inputs):
        index, _, _, _, n_out = self._plan(op_name, **inputs)
        coherent = self.rows_coherent == self._n
        self._rebuild(index[:n_out], reset_stats=False)
        if coherent:  # a subsequence of ordered rows is ordered
            self.rows_coherent = self._n

    @torch.no_grad()
    def pruneclone_planned(self, max_grad, extent, splitN=2, samples=None):
        """The table densify_pruneclone(max_grad, ., extent, ., splitN, samples) leaves ([kept originals | clones | split
        children]), with torch.normal consuming the generator as it does there."""
        n = self._n
        scaling = self._fields["scaling"].view(n)
        index, kept, clones, parents, n_out = self._plan(
            "PRUNECLONE", splitN, accum=self.xyz_gradient_accum.reshape(-1), denom=self.denom.reshape(-1),
            scaling=scaling, grad_threshold=max_grad, size_threshold=self.percent_dense * extent)
        n_children = splitN * parents
        if samples is None and n_children:
            sel = -(index[n_out - parents:n_out] + 1)   # the list's tail: the split parents, ascending
            stds = torch.exp(scaling[sel.long()]).repeat(splitN, 1)
            samples = torch.normal(mean=torch.zeros_like(stds), std=stds)
        self._rebuild(index[:n_out], reset_stats=True)
        if n_children:
            samples = samples.to(torch.float32).contiguous()
            check(_lib.load().mobgs_split_children(n_children, kept + clones, splitN, ptr(samples),
                                                  ptr(self._fields["rotation"].view(self._n)),
                                                  ptr(self._fields["xyz"].view(self._n)),
                                                  ptr(self._fields["scaling"].view(self._n)), stream()),
                  "mobgs_split_children")
        if self.keep_sorted:
            self.spatial_sort_()

    @torch.no_grad()
    def prune_opacity_below(self, min_opacity):
        """The table prune_points((get_opacity < min_opacity).squeeze()) leaves, with the sigmoid and the comparison inside
        the plan: 1 / (1 + expf(-x)) in fp32 there, torch.sigmoid here.  The two agree except for a row whose sigmoid lies
        within a few ulp of min_opacity, which the two routes may decide differently; every other row, and every table
        without such a row, comes out bit for bit the same."""
        self._prune_planned("PRUNE_OPACITY", opacity=self._fields["opacity"].view(self._n).reshape(-1),
                            min_opacity=min_opacity)

    @torch.no_grad()
    def prune_outside(self, minbounds, maxbounds):
        """The table helper_train.removeminmax leaves: rows with a coordinate strictly above `maxbounds` or strictly
        below `minbounds` go.  The bounds (three numbers or 0-dim tensors each) reach the kernel as six fp32 on the
        device: no value is read back."""
        dev = self._xyz.device
        bounds = torch.stack([torch.as_tensor(b, dtype=torch.float32, device=dev).reshape(())
                              for b in (*maxbounds, *minbounds)])
        self._prune_planned("PRUNE_BOUNDS", xyz=self._fields["xyz"].view(self._n), bounds=bounds)

    @torch.no_grad()
    def onedown_control_pts(self, viewpoints):
        """gaussian_model.py:274-290 on the live rows of the table: scene_init.onedown_control_pts (one launch, in
        place, no host synchronisation) -> the number of rows pruned as a 0-dim device tensor.  Shapes, Parameters and
        the optimiser's keys stay what they were (a captured iteration stays valid); the Adam moments of control_xyz are
        left alone, as in the reference.  The kernel writes through raw pointers: the renderer's caches are told, and
        the version counters of the two tensors move."""
        from . import gaussian_renderer as _GR
        from .scene_init import onedown_control_pts
        pruned = onedown_control_pts(self, viewpoints, self.error_threshold)
        _GR.parameters_changed()
        return pruned

    @torch.no_grad()
    def reset_opacity(self):
        op = torch.sigmoid(self._opacity)
        x = torch.min(op, torch.ones_like(op) * 0.01)
        new = torch.log(x / (1 - x))
        if torch.isnan(new).any():
            raise FloatingPointError("opacities_new is nan")  # the reference prints and exit()s here
        self._fields["opacity"].view(self._n).copy_(new)
        if self.optimizer is not None:
            self.adopt_optimizer_state()
            for k in ("opacity.exp_avg", "opacity.exp_avg_sq"):
                if k in self._fields:
                    self._fields[k].view(self._n).zero_()
        self._publish(rekey=True)

    # ---- checkpoint interchange (scene/gaussian_model.py:761-804, :934-1040) ---------------------------------------
    def save_ply(self, path: str):
        from . import ply_io
        ply_io.save_ply(self, path)

    @classmethod
    def from_ply(cls, path: str, device="cuda", decoder=None):
        from . import ply_io
        params, dynamic = ply_io.load_ply(path)
        pc = cls(params, dynamic, decoder=decoder, device=device)
        pt = path.replace(".ply", ".pt")
        if decoder is None and os.path.exists(pt):
            pc.rgbdecoder.load_state_dict(torch.load(pt, map_location=device))
        return pc

    # ---- training checkpoints (mobgs_amd/checkpoint.py; include/mobgs_hip.h K29) -----------------------------------------
    def state_dict(self) -> dict:
        """The whole table (parameters, Adam moments, statistics, deformation table) as ONE packed device block with its
        checksum, the field list and the optimiser's rates / step counts: checkpoint.set_state_dict."""
        from . import checkpoint
        return checkpoint.set_state_dict(self)

    def load_state_dict(self, state: dict):
        """state_dict()'s result back into this set (any row count; the optimiser, if both have one, is re-keyed)."""
        from . import checkpoint
        checkpoint.load_set_state(self, state)
        return self

    # ---- creation from data (scene/gaussian_model.py:495-582, :406-493) ------------------------------------------------
    @classmethod
    def _from_init(cls, params, extras, spatial_lr_scale, is_dynamic, device, decoder, capacity_factor, spatial_sort):
        pc = cls(params, extras, decoder=decoder, device=device, capacity_factor=capacity_factor)
        pc.is_dynamic = is_dynamic   # (rows of a static set are ordered by their positions, not by control points)
        pc.spatial_lr_scale = spatial_lr_scale
        pc.pcd_order = pc.spatial_sort_() if spatial_sort else None
        return pc

    @classmethod
    def from_pcd(cls, pcd, spatial_lr_scale: float, time_line: int = 0, *, sh_degree: int = 0, trbfslinit=None,
                 device="cuda", decoder=None, capacity_factor: float = 1.5, spatial_sort: bool = True):
        """create_from_pcd (:495-582): a static set from a point cloud `pcd` (.points [N,3], .colors [N,3] in [0,1],
        .times [N,1]); `time_line` is unused, as in the reference.  Initial scales: the 3-NN kernel (csrc/knn.hip).
        One deviation: the reference draws the static set's control_xyz from a normal distribution (:527) and no
        kernel reads it; here it keeps GaussianParams' default.  spatial_sort: store the rows along a Morton curve
        (spatial_sort_(); row i of the set is then row pcd_order[i] of `pcd`), False keeps the order of `pcd`."""
        from . import scene_init
        params, extras = scene_init.static_init(pcd, device, sh_degree, trbfslinit)
        return cls._from_init(params, extras, spatial_lr_scale, False, device, decoder, capacity_factor, spatial_sort)

    @classmethod
    def from_pcd_dynamic(cls, pcd, spatial_lr_scale: float, time_line: int, dyn_tracjectory, *, sh_degree: int = 0,
                         trbfslinit=None, device="cuda", decoder=None, capacity_factor: float = 1.5,
                         spatial_sort: bool = True):
        """create_from_pcd_dynamic (:406-493): as from_pcd, with 12 spline control points per point fitted to its tracked
        trajectory `dyn_tracjectory` [N, T, 3] at T uniform times (scene_init.inverse_cubic_hermite)."""
        from . import scene_init
        params, extras = scene_init.dynamic_init(pcd, dyn_tracjectory, device, sh_degree, trbfslinit)
        return cls._from_init(params, extras, spatial_lr_scale, True, device, decoder, capacity_factor, spatial_sort)

    # ---- introspection for tests ------------------------------------------------------------------------------------
    def table_state(self) -> Dict[str, torch.Tensor]:
        if self.optimizer is not None:
            self.adopt_optimizer_state()
        out = {k: f.view(self._n) for k, f in self._fields.items()}
        out["_deformation_table"] = out["_deformation_table"].view(torch.bool)
        return out
