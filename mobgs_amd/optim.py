"""One Adam step for several torch.optim.Adam optimisers in ONE kernel launch (include/mobgs_hip.h K16).

The reference steps three optimisers per iteration (/root/reference/train.py:790-807); with one-tensor parameter groups
(scene/gaussian_model.py:598-617) torch's multi-tensor path degenerates to ~8 launches per group: 3.3 ms per iteration at
300 k Gaussians.  `fused_adam_step` performs exactly torch.optim.Adam's update (amsgrad = False, weight_decay = 0,
maximize = False) for every fp32 CUDA parameter of the given optimisers, on their own state tensors (`exp_avg`,
`exp_avg_sq`, `step` -- created on first use like torch does, so state_dict() / densification surgery see what they expect),
and falls back to `optimizer.step()` for anything else (other dtypes, weight decay, amsgrad, CPU tensors).

`DeviceAdam` (include/mobgs_hip.h K27) is the same step for a loop replayed from a graph: the learning rates of every iteration
and the bias corrections of every step count are tabulated on the host once and looked up on the device, so the step has no
host scalars and graphed.GraphedCallable can record it with forward and backward.
"""
from __future__ import annotations

import ctypes
import math
from typing import Iterable, List

import torch

from . import _lib
from ._lib import check, stream


class _AdamTensor(ctypes.Structure):
    _fields_ = _lib._STRUCTS["MobgsAdamTensor"]  # read from include/mobgs_hip.h


def _fusable(opt: torch.optim.Optimizer, group: dict, p: torch.Tensor) -> bool:
    return (isinstance(opt, torch.optim.Adam) and not group.get("amsgrad", False) and not group.get("maximize", False)
            and group.get("weight_decay", 0) == 0 and not group.get("capturable", False)
            and not group.get("differentiable", False) and p.is_cuda and p.dtype == torch.float32
            and p.is_contiguous() and p.grad is not None and p.grad.dtype == torch.float32
            and p.grad.is_contiguous() and not p.grad.is_sparse)


@torch.no_grad()
def fused_adam_step(optimizers: Iterable[torch.optim.Optimizer]) -> int:
    """Step all the optimisers; -> number of tensors that went through the fused kernel."""
    lib = _lib.load()
    batches = {}   # (beta1, beta2, eps) -> descriptors
    keep: List[torch.Tensor] = []
    fused = 0
    for opt in optimizers:
        leftovers = []
        for group in opt.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not _fusable(opt, group, p):
                    leftovers.append(p)
                    continue
                st = opt.state[p]
                if len(st) == 0:   # torch.optim.Adam._init_group
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                t = float(st["step"])
                lr = float(group["lr"])
                step_size = lr / (1.0 - b1 ** t)
                bias2_sqrt = math.sqrt(1.0 - b2 ** t)
                m, v = st["exp_avg"], st["exp_avg_sq"]
                if not (m.is_contiguous() and v.is_contiguous()):
                    st["step"] -= 1
                    leftovers.append(p)
                    continue
                fused += 1
                if p.numel() == 0:   # (an empty group, e.g. f_rest of a degree-0 model: state and step count only)
                    continue
                keep += [p, p.grad, m, v]
                batches.setdefault((float(b1), float(b2), float(group["eps"])), []).append(
                    _AdamTensor(p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), step_size,
                                bias2_sqrt))
        if leftovers:  # torch's own step for what the kernel does not cover (grads of the fused ones hidden meanwhile)
            hidden = [(p, p.grad) for g in opt.param_groups for p in g["params"]
                      if p.grad is not None and all(p is not q for q in leftovers)]
            for p, _ in hidden:
                p.grad = None
            try:
                opt.step()
            finally:
                for p, g in hidden:
                    p.grad = g
    if batches:
        # the kernel writes the parameters through raw pointers: the render-side caches that are told directly
        # (gaussian_renderer._shared_mid_state: ADVICE r5) ...
        from . import gaussian_renderer as _GR
        _GR.parameters_changed()
    for (b1, b2, eps), descs in batches.items():
        for i in range(0, len(descs), 64):
            chunk = descs[i:i + 64]
            arr = (_AdamTensor * len(chunk))(*chunk)
            check(lib.mobgs_adam_step(len(chunk), arr, b1, b2, eps, stream()), "mobgs_adam_step")
    # ... and Tensor._version, which everything else keys on (deformation._packed, _lib.DerivedCache, blce.py): moved
    # by hand for every parameter the kernel wrote, as torch's own in-place step would have (host only)
    for i in range(0, len(keep), 4):
        torch.autograd.graph.increment_version(keep[i])
    return fused


# ---- the same step with its factors formed on the device (include/mobgs_hip.h K27): recordable into a graph ---------------
class _DevSchedule(ctypes.Structure):
    _fields_ = _lib._STRUCTS["MobgsAdamDevSchedule"]


class _DevTensor(ctypes.Structure):
    _fields_ = _lib._STRUCTS["MobgsAdamDevTensor"]


class MultiplicativeLR:
    """The rate of a group whose owner multiplies it by `factor` after every step (blceKernel.adjust_lr, train.py:807), as
    a function of the iteration: `lr` at `first_iteration` (and before), one multiplication per later iteration --
    repeated multiplication in Python floats, as `group["lr"] *= factor` forms it, not a power."""

    def __init__(self, lr: float, factor: float, first_iteration: int = 1):
        self.rates, self.factor, self.first = [lr], factor, int(first_iteration)

    def __call__(self, iteration):
        k = max(int(iteration) - self.first, 0)
        while len(self.rates) <= k:
            self.rates.append(self.rates[-1] * self.factor)
        return self.rates[k]


def lr_table(schedules, horizon: int) -> torch.Tensor:
    """float64 [horizon + 1, len(schedules)] on the host: row `it` holds schedule(it) of every column, evaluated once with
    the caller's own callables -- what update_learning_rate(it) would have put into group["lr"]."""
    rows = [[float(fn(it)) for fn in schedules] for it in range(int(horizon) + 1)]
    return torch.tensor(rows, dtype=torch.float64).reshape(int(horizon) + 1, len(schedules))


def bias_tables(beta1, beta2, max_t: int):
    """(1.0 - beta1 ** t, math.sqrt(1.0 - beta2 ** t)) for t = 0 .. max_t with t a Python float, as fused_adam_step forms
    them: two float64 [max_t + 1] host tensors."""
    ts = [float(t) for t in range(int(max_t) + 1)]
    return (torch.tensor([1.0 - beta1 ** t for t in ts], dtype=torch.float64),
            torch.tensor([math.sqrt(1.0 - beta2 ** t) for t in ts], dtype=torch.float64))


def rate_layout(columns, groups, n_columns: int, horizon: int):
    """Where each planned tensor finds its rate.  columns[i]: the table column of tensor i's group, or None for a group
    without a schedule; groups[i]: its group dict.  -> (constants, layout): the float64 rates of the unscheduled groups, one
    per distinct group, and per tensor (in_table, offset, stride, rows) -- a scheduled tensor reads table[row, offset] with
    stride n_columns over horizon + 1 rows, an unscheduled one reads constants[offset] with stride 0: one value."""
    const_groups, layout = [], []
    for col, group in zip(columns, groups):
        if col is not None:
            layout.append((True, int(col), int(n_columns), int(horizon) + 1))
            continue
        if not any(group is g for g in const_groups):
            const_groups.append(group)
        layout.append((False, next(k for k, g in enumerate(const_groups) if g is group), 0, 1))
    return torch.tensor([float(g["lr"]) for g in const_groups], dtype=torch.float64), layout


def _to_device_bytes(array, dev) -> torch.Tensor:
    return torch.frombuffer(bytearray(bytes(array)), dtype=torch.uint8).to(dev)


class DeviceAdam:
    """fused_adam_step for a loop that is replayed from a graph: the learning-rate schedules and Adam's bias corrections are
    tabulated ONCE on the host, with the statements the eager path uses, and looked up on the device by counters that live
    there, so nothing of a step is a host scalar and `step()` can be recorded with the rest of the iteration:

        schedules = list(stat.schedules().items()) + list(dyn.schedules().items()) \
            + [(g, MultiplicativeLR(g["lr"], blce.lr_factor)) for g in blce.optimizer.param_groups]
        adam = DeviceAdam([stat.optimizer, dyn.optimizer, blce.optimizer], schedules, horizon=30000)
        def iteration():
            loss = trainer.forward_backward()
            adam.step()                       # two launches: factors from the tables, then the update
            return loss
        fb = GraphedCallable(iteration, warmup=0)
        for it in ...:
            loss = fb()                       # (the call that captures replays once as well)
            adam.after_replay()               # host side of the replayed step: version counters, caches, the mirror

    Step k (k = 0, 1, ...) runs with the rates of iteration first_iteration + k, i.e. what update_learning_rate(iteration)
    followed by fused_adam_step gives in a loop that starts at first_iteration: parameters and moments are bit-equal to that
    loop's (tests/test_gpu_device_adam.py).  schedules: a dict {(optimizer, group name): callable of the iteration} or a list of
    (key, callable) pairs whose key is such a tuple or the group dict itself; a group without one keeps its present rate.  The plan holds every fusable tensor that has a
    .grad when it is built (state created like torch does); a tensor without a gradient is not stepped and its step count
    stays; anything else (other dtypes, weight decay, amsgrad, CPU tensors) raises -- there is no fallback inside a graph.
    The gradients must live where they lived at build time (persistent .grad tensors, distributed.FlatGradients).
    After densification / pruning / a late gradient: rebuild(), and record the graph again.  Before anything on the host
    reads the optimisers (state_dict(), a continuation with fused_adam_step): sync_to_host()."""

    def __init__(self, optimizers: Iterable[torch.optim.Optimizer], schedules=None, horizon: int = 0,
                 first_iteration: int = 1):
        self.optimizers = list(optimizers)
        pairs = list(schedules.items()) if isinstance(schedules, dict) else list(schedules or [])
        self.horizon, self.first_iteration = int(horizon), int(first_iteration)
        if not 0 <= self.first_iteration <= self.horizon:
            raise ValueError(f"DeviceAdam: first_iteration = {first_iteration} must lie in 0 .. horizon = {horizon}")
        self._sched_keys = [k for k, _ in pairs]
        self._columns: List = []                 # distinct callables, one table column each
        self._column_of_key = []
        for _, fn in pairs:
            if not callable(fn):
                raise TypeError("DeviceAdam: a schedule must be a callable of the iteration")
            if not any(fn is c for c in self._columns):
                self._columns.append(fn)
            self._column_of_key.append(next(i for i, c in enumerate(self._columns) if c is fn))
        self.lr_rows = lr_table(self._columns, self.horizon)     # host copy (sync_to_host reads it)
        self.iteration = self.first_iteration                     # host mirror of the device's iteration counter
        self._plan = None
        self.rebuild()

    # ---- plan ----------------------------------------------------------------------------------------------------------
    def _column(self, opt, group):
        for key, col in zip(self._sched_keys, self._column_of_key):
            if key is group or (isinstance(key, tuple) and len(key) == 2 and key[0] is opt
                                and key[1] == group.get("name")):
                return col
        return None

    @torch.no_grad()
    def rebuild(self):
        """(Re)build the plan from the optimisers as they are now: new pointers and sizes, step counts carried over through
        the state dicts, unscheduled rates read again.  A graph that recorded step() must be recorded again."""
        if self._plan is not None:
            self.sync_to_host()
        entries, dev = [], None
        for opt in self.optimizers:
            for group in opt.param_groups:
                b1, b2 = group["betas"]
                for p in group["params"]:
                    if p.grad is None:
                        continue
                    if not _fusable(opt, group, p):
                        raise RuntimeError(f"DeviceAdam: a tensor of group {group.get('name')!r} cannot go through the "
                                           "kernel (needs torch.optim.Adam without amsgrad / maximize / weight decay / "
                                           "capturable, contiguous fp32 device tensors and gradients)")
                    st = opt.state[p]
                    if len(st) == 0:   # torch.optim.Adam._init_group
                        st["step"] = torch.tensor(0.0, dtype=torch.float32)
                        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    m, v = st["exp_avg"], st["exp_avg_sq"]
                    if not (m.is_contiguous() and v.is_contiguous() and m.is_cuda and v.is_cuda
                            and m.dtype == v.dtype == torch.float32 and m.numel() == v.numel() == p.numel()):
                        raise RuntimeError(f"DeviceAdam: the moments of group {group.get('name')!r} are not contiguous "
                                           "fp32 device tensors of the parameter's size")
                    if dev is None:
                        dev = p.device
                    if p.device != dev or p.grad.device != dev:
                        raise RuntimeError("DeviceAdam: all tensors of a plan must live on one device")
                    entries.append(dict(opt=opt, group=group, p=p, grad=p.grad, grad_ptr=p.grad.data_ptr(), st=st, m=m,
                                        v=v, n=p.numel(), step=int(float(st["step"])), betas=(b1, b2),
                                        eps=float(group["eps"]), column=self._column(opt, group)))
        self._plan = entries
        n = len(entries)
        self._longest = max([e["n"] for e in entries], default=0)
        if n == 0:
            return self
        if n > 65535:
            raise RuntimeError(f"DeviceAdam: {n} tensors (at most 65535 per plan)")
        remaining = self.horizon - self.iteration + 1
        S = self.lr_rows.shape[1]
        self._lr_sched = self.lr_rows.to(dev)
        self.lr_const, layout = rate_layout([e["column"] for e in entries], [e["group"] for e in entries], S, self.horizon)
        self._lr_const = self.lr_const.to(dev)
        self._bias = {}
        max_t = max(e["step"] for e in entries) + max(remaining, 0) + 1
        for e in entries:
            key = (float(e["betas"][0]), float(e["betas"][1]))
            if key not in self._bias:
                bc1, bc2s = bias_tables(e["betas"][0], e["betas"][1], max_t)
                self._bias[key] = (bc1.to(dev), bc2s.to(dev))
        scheds, tensors = (_DevSchedule * n)(), (_DevTensor * n)()
        for i, e in enumerate(entries):
            bc1, bc2s = self._bias[(float(e["betas"][0]), float(e["betas"][1]))]
            in_table, offset, stride, rows = layout[i]
            lr_ptr = (self._lr_sched if in_table else self._lr_const).data_ptr() + 8 * offset
            scheds[i] = _DevSchedule(lr_ptr, bc1.data_ptr(), bc2s.data_ptr(), stride, rows, max_t + 1, 0)
            b1, b2 = float(e["betas"][0]), float(e["betas"][1])
            empty = e["n"] == 0   # (an empty group, e.g. f_rest of a degree-0 model: state and step count only)
            tensors[i] = _DevTensor(0 if empty else e["p"].data_ptr(), 0 if empty else e["grad_ptr"],
                                    0 if empty else e["m"].data_ptr(), 0 if empty else e["v"].data_ptr(), e["n"],
                                    1.0 - b1, b2, 1.0 - b2, e["eps"])
        self._sched_dev, self._tensor_dev = _to_device_bytes(scheds, dev), _to_device_bytes(tensors, dev)
        self._counters = torch.tensor([self.iteration] + [e["step"] for e in entries], dtype=torch.int32).to(dev)
        self._factors = torch.zeros(n, 2, dtype=torch.float32, device=dev)
        self._device = dev
        return self

    # ---- one step ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self):
        """The two launches on the current stream, then (unless a capture is recording them: after_replay() then follows
        every replay) the host side of the step.  Raises before launching when the step lies past the horizon, and, outside
        a capture, when a planned tensor's .grad is no longer the one the plan holds."""
        if self.iteration > self.horizon:
            raise RuntimeError(f"DeviceAdam: iteration {self.iteration} is past the horizon {self.horizon} the schedules "
                               "were tabulated for")
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            for e in self._plan:
                g = e["p"].grad
                if g is None or g.data_ptr() != e["grad_ptr"]:
                    raise RuntimeError(f"DeviceAdam: the .grad of a tensor of group {e['group'].get('name')!r} is not the "
                                       "one the plan was built with (gradients must be persistent): call rebuild()")
                if e["st"].get("exp_avg") is not e["m"] and (e["st"].get("exp_avg") is None
                                                              or e["st"]["exp_avg"].data_ptr() != e["m"].data_ptr()
                                                              or e["st"]["exp_avg_sq"].data_ptr() != e["v"].data_ptr()):
                    raise RuntimeError(f"DeviceAdam: the moments of group {e['group'].get('name')!r} were moved since the "
                                       "plan was built (densification surgery, load_state_dict): call rebuild()")
        n = len(self._plan)
        if n:
            lib = _lib.load()
            with torch.cuda.device(self._device):
                s = stream()
                check(lib.mobgs_adam_dev_factors(n, self._sched_dev.data_ptr(), self._counters.data_ptr(),
                                                 self._factors.data_ptr(), s), "mobgs_adam_dev_factors")
                check(lib.mobgs_adam_dev_step(n, self._tensor_dev.data_ptr(), self._factors.data_ptr(), self._longest, s),
                      "mobgs_adam_dev_step")
        if not capturing:
            self._host_side()

    def after_replay(self):
        """The host side of a step that a graph replay just ran: Tensor._version of every written parameter, the render-side
        cache notice, the iteration mirror.  Raises when that replay lay past the horizon (the device clamped to the last
        row: the step ran, with the last tabulated rates)."""
        if self.iteration > self.horizon:
            raise RuntimeError(f"DeviceAdam: the replayed step (iteration {self.iteration}) lies past the horizon "
                               f"{self.horizon}; the device used the last tabulated row")
        self._host_side()

    def _host_side(self):
        wrote = [e["p"] for e in self._plan if e["n"]]
        if wrote:
            from . import gaussian_renderer as _GR
            _GR.parameters_changed()
        for p in wrote:
            torch.autograd.graph.increment_version(p)
        self.iteration += 1

    # ---- what the host sees ----------------------------------------------------------------------------------------------
    def counters(self) -> torch.Tensor:
        """[iteration, step of every planned tensor] from the device (one copy; synchronises)."""
        return self._counters.cpu() if self._plan else torch.tensor([self.iteration], dtype=torch.int32)

    def factors(self) -> torch.Tensor:
        """[n, 2] (step_size, bias2_sqrt) of the last step, from the device."""
        return self._factors.cpu() if self._plan else torch.zeros(0, 2)

    @torch.no_grad()
    def sync_to_host(self):
        """One device-to-host copy of the counters into state[p]["step"]; every scheduled group's "lr" becomes the table
        row last used.  state_dict(), densification surgery and a continuation with fused_adam_step then see what the eager
        loop would have left."""
        c = self.counters().tolist()
        if c[0] != self.iteration:
            raise RuntimeError(f"DeviceAdam: the device is at iteration {c[0]}, the host mirror at {self.iteration}: "
                               "after_replay() must follow every replay of a recorded step(), once")
        for e, s in zip(self._plan, c[1:]):
            e["st"]["step"] = torch.tensor(float(s), dtype=torch.float32)
            e["step"] = s
        last = self.iteration - 1
        if last >= self.first_iteration:
            row = self.lr_rows[min(last, self.horizon)]
            for opt in self.optimizers:
                for group in opt.param_groups:
                    col = self._column(opt, group)
                    if col is not None:
                        group["lr"] = float(row[col])
        return self


class FusedAdam(torch.optim.Adam):
    """torch.optim.Adam whose step() is the one-launch kernel above: what the modules of this package that stand in for
    the reference's own (densify.TrainableGaussians for scene/gaussian_model.py GaussianModel.training_setup, :598-617;
    blce.blceKernel for scene/blce.py) hand to an UNCHANGED training loop -- /root/reference/train.py:790-807 calls
    `optimizer.step()` on whatever training_setup() created.  Same update, same state tensors
    (`exp_avg`, `exp_avg_sq`, `step`), state_dict()-compatible; anything the kernel does not cover (closure, amsgrad, weight
    decay, non-fp32 / CPU tensors) goes through torch's own step.  MOBGS_FUSED_ADAM=0: plain torch.optim.Adam.step()."""

    @torch.no_grad()
    def step(self, closure=None):
        import os
        if closure is not None or os.environ.get("MOBGS_FUSED_ADAM", "1") == "0":
            return super().step(closure)
        # (fused_adam_step falls back to torch's step for the tensors it cannot take: reach it through the base class,
        # not through this override)
        real, self.step = self.step, super().step
        try:
            fused_adam_step([self])
        finally:
            self.step = real
        return None
