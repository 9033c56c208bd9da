"""Multi-GPU sharding of the K latent sub-frame renders of blurry training views (one process per GPU,
torch.distributed over RCCL/xGMI; backend "nccl" IS RCCL on ROCm, "gloo" on CPU for tests).

The reference is single-GPU: train.py:441-541 renders, for every view of the batch, the mid frame in train mode and
the other K - 1 = 8 latent sharp frames one after the other and averages them, `pred = mean_k(render_k) + 1e-10`.
The sub-frames only depend on the (replicated) Gaussians and on their own camera / exposure offset, so the
(view, sub-frame) units shard with exactly two exchange steps per training iteration:

  forward   all_reduce(SUM) of the rank-local partial image sums, one [V,3,H,W] fp32 tensor for the V views of the
            batch (16.4 MB per view at 1352x1014) -> every rank holds the identical blurry predictions and computes
            the identical photometric loss;
  backward  dL/dpred is already replicated, so that all-reduce back-propagates as the identity (no traffic); each
            rank back-propagates through its own sub-frames, then ONE in-place all_reduce(SUM) of a persistent flat
            buffer that holds every parameter gradient (<= 57 floats per Gaussian, decoder, BLCE) AND the mid-frame
            densification statistics (means2d.grad [N,2] and radii [N] of each view's mid render, train.py:634-648,
            which only the rank that rendered the mid frame has) gives every rank the full gradient and statistics.

Which loss terms may be formed where (the SUM counts every rank's backward once):
  * terms that are functions of the all-reduced prediction (L1 / SSIM, train.py:621-628): on EVERY rank, unscaled --
    each rank's backward reaches only its own sub-frames;
  * terms on the outputs of one sub-frame render (depth / mask losses on the mid render, train.py:651-655): only the
    rank that rendered that unit has them (`owns()`), unscaled;
  * terms every rank can form identically from replicated data alone (regularisers on parameters): scale them with
    `replicated_term()` (1 / world) or form them on one rank only, otherwise the SUM counts them world times.

Full replicas of the parameters live on every rank (300k x 57 floats = 68 MB, trivial next to 288 GB HBM).
"""
from __future__ import annotations

from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import torch
from contextlib import nullcontext as _nullcontext
import torch.distributed as dist


_comm_streams: Dict[int, "torch.cuda.Stream"] = {}
# (tag, start event, done event) of every asynchronous device all-reduce when MOBGS_COMM_LOG=1 -- how the overlap tests
# and scripts/rccl_world1_check.py see WHERE an exchange ran relative to the compute stream's own events
comm_log: List[Tuple[str, "torch.cuda.Event", "torch.cuda.Event"]] = []
COMM_LOG_MAX = 4096  # most recent exchanges kept with MOBGS_COMM_LOG=1
wait_log: List[Tuple[str, "torch.cuda.Event", "torch.cuda.Event"]] = []  # (tag, before, after) around each consumer-side wait


def _comm_logging() -> bool:
    import os
    return os.environ.get("MOBGS_COMM_LOG") == "1"


def comm_stream(device) -> "torch.cuda.Stream":
    """The one side stream per device on which asynchronous exchanges are ENQUEUED (HIP streams: collectives beside
    compute).  RCCL runs a collective on its own internal stream, ordered behind the stream that is current when the
    call is made; issuing it from this side stream -- after the side stream has waited for the producer -- keeps it
    independent of whatever the compute stream enqueues next."""
    idx = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    st = _comm_streams.get(idx)
    if st is None:
        st = _comm_streams[idx] = torch.cuda.Stream(device=idx)
    return st


class _StreamWork:
    """Handle of an exchange enqueued on the communication stream: wait() makes the CURRENT stream wait for its
    completion event (no host block)."""

    def __init__(self, done: "torch.cuda.Event", keep=(), device=None, tag: str = ""):
        self.done, self.keep, self.device, self.tag = done, keep, device, tag

    def wait(self, timeout=None):
        # the current stream OF THE TENSOR'S DEVICE (not of whatever device happens to be current: ADVICE r4)
        st = torch.cuda.current_stream(self.device)
        if _comm_logging():
            # how long the CONSUMER's stream stalls on this exchange = what of it is exposed (not hidden behind compute):
            # bench.py --gpus N reports it per rank (wait_log)
            before = torch.cuda.Event(enable_timing=True)
            before.record(st)
            st.wait_event(self.done)
            after = torch.cuda.Event(enable_timing=True)
            after.record(st)
            wait_log.append((self.tag, before, after))
            del wait_log[:-COMM_LOG_MAX]
            return True
        st.wait_event(self.done)
        return True

    def is_completed(self):
        return self.done.query()


def _all_reduce_sum(t: torch.Tensor, group=None, async_op: bool = False, tag: str = ""):
    """In-place SUM.  A gloo group gets device tensors staged through the host (functional tests of the N > 1 path on
    a one-GPU box; the RCCL path reduces in place on the device).  async_op on a device tensor with the nccl (= RCCL)
    backend: enqueued from the communication stream (see comm_stream) -> _StreamWork."""
    if t.is_cuda and dist.get_backend(group) == "gloo":
        h = t.detach().cpu()
        dist.all_reduce(h, op=dist.ReduceOp.SUM, group=group)
        t.copy_(h)
        return _DoneWork() if async_op else None  # synchronous here; callers of async_op get a handle all the same
    if async_op and t.is_cuda:
        import os
        side, main = comm_stream(t.device), torch.cuda.current_stream(t.device)
        log = os.environ.get("MOBGS_COMM_LOG") == "1"
        side.wait_stream(main)                      # the producer of `t` has finished before the exchange starts
        with torch.cuda.stream(side):
            start = torch.cuda.Event(enable_timing=log)
            start.record(side)
            work = dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group, async_op=True)
            work.wait()                             # the SIDE stream waits for RCCL's stream (no host block)
            done = torch.cuda.Event(enable_timing=log)
            done.record(side)
        t.record_stream(side)
        if log:
            comm_log.append((tag, start, done))
            del comm_log[:-COMM_LOG_MAX]   # bounded: a long run with MOBGS_COMM_LOG=1 keeps the most recent exchanges
        return _StreamWork(done, (t, work), t.device, tag)
    return dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group, async_op=async_op)


class _DoneWork:
    """A completed `Work`: what the host-staged gloo path hands to callers that asked for async_op=True."""

    def wait(self, timeout=None):
        return True

    def is_completed(self):
        return True


class _CopyBackWork:
    """Handle of an asynchronous all-reduce that ran on an fp32 COPY of a half-precision buffer: wait() awaits the
    exchange and rounds the sum back into the buffer (once)."""

    def __init__(self, work, dst: torch.Tensor, src: torch.Tensor):
        self.work, self.dst, self.src, self.done = work, dst, src, False

    def wait(self, timeout=None):
        if not self.done:
            if self.work is not None:
                self.work.wait()
            with torch.cuda.device(self.dst.device) if self.dst.is_cuda else _nullcontext():
                self.dst.copy_(self.src)  # (on the current stream of the BUFFER's device: ADVICE r4)
            self.done = True
        return True

    def is_completed(self):
        return self.done or self.work is None or self.work.is_completed()


class _SumAcrossRanks(torch.autograd.Function):
    """y = sum_r x_r (all-reduce).  reduce_backward=False: the caller's loss is a function of y that is IDENTICAL on
    every rank, so the gradient of that single loss w.r.t. this rank's x_r is dL/dy itself -- backward is the identity.
    reduce_backward=True: the ranks put DIFFERENT terms on y (each the loss terms of the units it owns, e.g. the
    flow losses of its get_flow calls, which read the blurry prediction): the gradient of the total w.r.t. x_r is the
    SUM over ranks of their dL_r/dy -- backward all-reduces.
    donate=True: x is a fresh temporary nobody else reads (the stacked partial sums) -- reduced in place, no copy."""

    @staticmethod
    def forward(ctx, x, group, donate, reduce_backward=False):
        ctx.group, ctx.reduce_backward = group, bool(reduce_backward)
        y = x.detach()
        donate = bool(donate) and y.is_contiguous()  # a strided temporary cannot be reduced in place: reduce a copy
        if not donate:
            y = y.clone(memory_format=torch.contiguous_format)
        _all_reduce_sum(y, group)
        if donate:
            ctx.mark_dirty(x)
            return x
        return y

    @staticmethod
    def backward(ctx, g):
        if ctx.reduce_backward:
            g = g.contiguous().clone()
            _all_reduce_sum(g, ctx.group)
        return g, None, None, None


class _SumAcrossRanksAsync(torch.autograd.Function):
    """_SumAcrossRanks whose forward only STARTS the all-reduce (async_op=True: it runs on the backend's own stream,
    ordered behind the work already enqueued on the current stream) and returns before it has finished; the caller
    awaits `ctx_work` (apply_async) before anything reads the result.  The input is a temporary: reduced in place."""

    @staticmethod
    def forward(ctx, x, group, reduce_backward, box):
        ctx.group, ctx.reduce_backward = group, bool(reduce_backward)
        y = x.detach()
        if not y.is_contiguous():
            y = y.clone(memory_format=torch.contiguous_format)
            box.append(_all_reduce_sum(y, group, async_op=True, tag="image"))
            return y
        box.append(_all_reduce_sum(y, group, async_op=True, tag="image"))
        ctx.mark_dirty(x)
        return x

    @staticmethod
    def backward(ctx, g):
        if ctx.reduce_backward:
            g = g.contiguous().clone()
            _all_reduce_sum(g, ctx.group)
        return g, None, None, None

    @staticmethod
    def apply_async(x, group, reduce_backward):
        box: list = []
        if x.is_leaf:            # mark_dirty needs a non-leaf (a partial sum of renders is one; a zero image is not)
            x = x.clone()
        return _SumAcrossRanksAsync.apply(x, group, reduce_backward, box), (box[0] if box else None)


class FlatGradients:
    """One persistent flat buffer per parameter dtype (fp32; fp16 for attribute arrays stored in half precision);
    every parameter's .grad is a VIEW of it, so backward passes accumulate in place and the exchange is an in-place
    all-reduce per buffer (no torch.cat, no copy back).  `extra` reserves named fp32 slots for per-step statistics
    that ride in the same message (name -> number of floats)."""

    GROWTH = 1.5   # rebind(): a storage that no longer fits grows to this times the need (+ 1024), as the tables do

    def __init__(self, params: Sequence[torch.Tensor], extra: Optional[Dict[str, int]] = None):
        self.params: List[torch.Tensor] = []
        self.views: List[torch.Tensor] = []
        self._store: Dict[torch.dtype, Optional[torch.Tensor]] = {torch.float32: None, torch.float16: None}
        self._device = torch.device("cpu")
        self._lay(params, extra, grow=False)

    def _lay(self, params, extra, grow: bool) -> None:
        """The layout over `params` and `extra`: fp32 parameters in order, then the named slots, in `flat`; fp16
        parameters in order in `flat_half`.  Both are prefixes of their storage, which is kept when it holds the layout
        and otherwise allocated anew (grow: with GROWTH's headroom)."""
        params = [p for p in params if p.requires_grad]
        if any(p.dtype not in (torch.float32, torch.float16) for p in params):
            raise NotImplementedError("FlatGradients holds fp32 / fp16 parameters")
        self.params = params
        if params:
            self._device = params[0].device
        self.extra_slices: Dict[str, slice] = {}
        sizes = {torch.float32: 0, torch.float16: 0}
        for p in self.params:
            sizes[p.dtype] += p.numel()
        off = sizes[torch.float32]
        self.param_floats = off   # fp32 words holding parameter gradients (the statistics slots follow)
        for name, k in (extra or {}).items():
            self.extra_slices[name] = slice(off, off + int(k))
            off += int(k)
        sizes[torch.float32] = off
        for dtype, need in sizes.items():
            st = self._store[dtype]
            if st is None or st.numel() < need or st.device != self._device:
                room = int(need * self.GROWTH) + 1024 if grow else need
                self._store[dtype] = torch.zeros(room, dtype=dtype, device=self._device)
        self.flat = self._store[torch.float32][:sizes[torch.float32]]
        self.flat_half = self._store[torch.float16][:sizes[torch.float16]]
        self.views = []
        o = {torch.float32: 0, torch.float16: 0}
        for p in self.params:
            buf = self.flat if p.dtype == torch.float32 else self.flat_half
            self.views.append(buf[o[p.dtype]:o[p.dtype] + p.numel()].view_as(p))
            o[p.dtype] += p.numel()

    def rebind(self, params: Sequence[torch.Tensor], extra: Optional[Dict[str, int]] = None) -> "FlatGradients":
        """Lay the views over `params` as they are NOW -- after a resize, an opacity reset or a load the sets' Parameters
        are new objects and their row counts may differ -- and over new `extra` slot sizes (None: no slots).  The storage
        is kept when the new layout fits in it (a smaller layout never shrinks it) and otherwise replaced by one of
        GROWTH times the need, so a run that resizes every 100 iterations allocates a handful of times.  Afterwards every
        parameter's .grad is its view, both buffers are zero, attached() / extra(name) / param_floats / buffers() describe
        the new layout, and no parameter -- old or new -- holds an old view."""
        stale = {v.data_ptr() for v in self.views}
        for p in self.params:
            if p.grad is not None and p.grad.data_ptr() in stale:
                p.grad = None
        self._lay(params, extra, grow=True)
        self.zero()
        return self

    def buffers(self) -> List[torch.Tensor]:
        return [b for b in (self.flat, self.flat_half) if b.numel()]

    def zero(self) -> None:
        """Start of an iteration: clear the buffers and (re-)attach the views as .grad."""
        for b in self.buffers():
            b.zero_()
        for p, v in zip(self.params, self.views):
            p.grad = v

    def attached(self) -> bool:
        return all(p.grad is not None and p.grad.data_ptr() == v.data_ptr() for p, v in zip(self.params, self.views))

    def gather_stray(self) -> None:
        """A .grad that was replaced by another tensor since zero() (an optimizer with set_to_none, a LeafGradSink
        that installed its own buffer) is folded back into the flat buffer."""
        for p, v in zip(self.params, self.views):
            if p.grad is None:
                p.grad = v
            elif p.grad.data_ptr() != v.data_ptr():
                v.add_(p.grad)
                p.grad = v

    def extra(self, name: str) -> torch.Tensor:
        return self.flat[self.extra_slices[name]]


class SubframeShard:
    def __init__(self, world_size: Optional[int] = None, rank: Optional[int] = None, group=None):
        if world_size is None:
            world_size = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        if rank is None:
            rank = dist.get_rank(group) if dist.is_available() and dist.is_initialized() else 0
        self.world, self.rank, self.group = int(world_size), int(rank), group
        # the exchanges run when there is more than one rank -- or when asked to anyway (MOBGS_FORCE_COLLECTIVES=1 with an
        # initialised process group: a ONE-rank RCCL group on a one-GPU box runs every collective of the N > 1 path on
        # the real backend, identity sums; scripts/rccl_world1_check.py)
        import os
        self.collective = self.world > 1 or (os.environ.get("MOBGS_FORCE_COLLECTIVES") == "1"
                                              and dist.is_available() and dist.is_initialized())

    # ---- partition ----------------------------------------------------------------------------------
    def units(self, n_units: int, offset: int = 0) -> List[int]:
        """Unit indices this rank renders: (u + offset) mod world == rank (round-robin keeps 9 units over 8 ranks at
        ceil(9/8) = 2 on one rank, 1 elsewhere; 18 units -- two views, the reference's batch -- at 3,3,2,...).
        `offset` rotates the assignment: a second family of units (the get_flow calls of the same batch) started at
        offset = number of units of the first hands ITS surplus to the ranks the first family left short."""
        return [u for u in range(n_units) if (u + offset) % self.world == self.rank]

    def owner(self, unit: int, offset: int = 0) -> int:
        return (unit + offset) % self.world

    def owns(self, unit: int, offset: int = 0) -> bool:
        return (unit + offset) % self.world == self.rank

    def view_units(self, n_views: int, n_sub: int, offset: int = 0) -> List[Tuple[int, int]]:
        """(view, sub-frame) pairs of this rank for a batch of `n_views` views with `n_sub` sub-frames each; the
        global unit index is view * n_sub + sub-frame."""
        return [(u // n_sub, u % n_sub) for u in self.units(n_views * n_sub, offset)]

    # ---- cost-weighted partition (round 3) ----------------------------------------------------------
    # Relative device time of the unit kinds of one training iteration at the headline size (bench.py, 1 x MI355X): a
    # lean latent render 1.05 ms = 1; the train-mode mid render (static / dynamic layers, depth, alphas) 2.4 ms; one
    # get_flow() call 1.8 ms.
    COST_LATENT, COST_MID, COST_FLOW = 1.0, 2.3, 1.7

    @staticmethod
    def plan(costs: Sequence[float], world: int, carry: Optional[Sequence[float]] = None):
        """Longest-processing-time-first assignment of units with the given costs to `world` ranks: heaviest unit first,
        each to the rank with the smallest load so far (ties: lowest rank).  `carry`: loads the ranks already have from
        another family of units.  Deterministic and a pure function of its arguments -- every rank computes the same
        plan.  -> (owner per unit, load per rank)."""
        loads = [float(x) for x in carry] if carry is not None else [0.0] * world
        owners = [0] * len(costs)
        for u in sorted(range(len(costs)), key=lambda i: (-float(costs[i]), i)):
            r = min(range(world), key=lambda q: (loads[q], q))
            owners[u] = r
            loads[r] += float(costs[u])
        return owners, loads

    def iteration_plan(self, n_views: int, n_sub: int, with_flows: bool = True):
        """The (view, sub-frame) render units and get_flow units of one training iteration, dealt by cost: the mid
        frames (train mode, 2.3 x a latent render) first, then the flow calls, then the latent renders, each to the
        least-loaded rank.  Round-robin (view_units) ignores that the two mid frames cost 2.3 units: 18 render units on
        8 ranks give loads of 3.3 / 3.0 against 2.58 on average (78 %); by cost the heaviest rank has 3.0 (86 %), and
        with the 18 flow units in the same pool 7.0 against 6.4 (91 %; 97 % on 4 ranks).
        -> {"render": owners [V * K], "flow": owners [V * K] or None, "loads": per rank}."""
        half = n_sub // 2
        rc = [self.COST_MID if (u % n_sub) == half else self.COST_LATENT for u in range(n_views * n_sub)]
        if with_flows:
            fc = [self.COST_FLOW] * (n_views * n_sub)
            owners, loads = self.plan(rc + fc, self.world)
            return {"render": owners[:len(rc)], "flow": owners[len(rc):], "loads": loads}
        owners, loads = self.plan(rc, self.world)
        return {"render": owners, "flow": None, "loads": loads}

    def planned_units(self, owners: Sequence[int], n_sub: int) -> List[Tuple[int, int]]:
        """This rank's (view, sub-frame) pairs under a plan, in view order (a view's partial sum is complete as early
        as possible: its image exchange can start while the next view renders)."""
        return [(u // n_sub, u % n_sub) for u, r in enumerate(owners) if r == self.rank]

    def replicated_term(self, loss_term: torch.Tensor) -> torch.Tensor:
        """Scale a loss term that EVERY rank forms identically from replicated data (not through the all-reduced
        prediction, not on the outputs of one rank's render) so that the gradient SUM counts it once."""
        return loss_term if self.world == 1 else loss_term / self.world

    # ---- forward exchange ---------------------------------------------------------------------------
    def mean_of_subframes(self, local_sum: torch.Tensor, n_units: int, donate: bool = False,
                          reduce_backward: bool = False) -> torch.Tensor:
        """local_sum = sum of THIS rank's sub-frame renders (any leading batch dimensions) -> mean over all n_units
        sub-frames (+1e-10, as train.py:541), identical on every rank.  With one process and one unit it is the
        render itself.  reduce_backward: see _SumAcrossRanks -- needed as soon as some loss term on the prediction
        exists on ONE rank only (then every term all ranks form identically on it goes through replicated_term())."""
        if not self.collective:
            return local_sum if n_units == 1 else local_sum / n_units + 1e-10
        if reduce_backward and not local_sum.requires_grad:
            # a rank without a render unit (more ranks than units) still forms loss terms on the prediction and must
            # take part in the backward all-reduce: give the exchange node an input that requires grad
            local_sum = local_sum.detach().requires_grad_(True).clone()  # (a non-leaf: `donate` reduces in place)
        total = _SumAcrossRanks.apply(local_sum, self.group, donate, reduce_backward)
        return total / n_units + 1e-10

    def render_blurry_view(self, render_unit: Callable[[int], torch.Tensor], n_units: int,
                           like: Optional[torch.Tensor] = None) -> torch.Tensor:
        """render_unit(k) -> sharp latent image of sub-frame k.  Returns the blurry prediction (all ranks).
        A rank that owns no sub-frame (world > n_units) contributes zeros; its prediction then does not require
        grad, so it must skip loss.backward() but still call all_reduce_gradients()."""
        mine = self.units(n_units)
        local = None
        for k in mine:
            img = render_unit(k)
            local = img if local is None else local + img
        if local is None:  # more ranks than sub-frames
            if like is None:
                raise ValueError("rank without sub-frames needs `like` to know the image shape")
            local = torch.zeros_like(like)
        return self.mean_of_subframes(local, n_units)

    def render_blurry_views(self, render_unit: Callable[[int, int], torch.Tensor], n_views: int, n_sub: int,
                            like: torch.Tensor, reduce_backward: bool = False,
                            units: Optional[Sequence[Tuple[int, int]]] = None, overlap: bool = False,
                            as_list: bool = False):
        """Batch form (train.py:430-541 loops over the views of the batch): render_unit(view, k) -> [3,H,W].
        Returns the blurry predictions [n_views,3,H,W] on every rank.  `units`: this rank's (view, sub-frame) pairs
        (default: the round-robin view_units).  overlap=False: ONE all-reduce for the whole batch.  overlap=True: one
        all-reduce PER VIEW, issued asynchronously as soon as this rank has rendered its last unit of the view -- the
        exchange of view v then runs on RCCL's stream while view v + 1 renders (8.2 MB per view at 1352x1014; VERDICT r2
        item 6b); the results are awaited together before the predictions are used."""
        mine = list(units) if units is not None else self.view_units(n_views, n_sub)
        sums: List[Optional[torch.Tensor]] = [None] * n_views
        if not (overlap and self.collective):
            for v, k in mine:
                img = render_unit(v, k)
                sums[v] = img if sums[v] is None else sums[v] + img
            if as_list:
                return [self.mean_of_subframes(s if s is not None else torch.zeros_like(like), n_sub,
                                               reduce_backward=reduce_backward) for s in sums]
            local = torch.stack([s if s is not None else torch.zeros_like(like) for s in sums])
            return self.mean_of_subframes(local, n_sub, donate=True, reduce_backward=reduce_backward)
        totals: List[Optional[torch.Tensor]] = [None] * n_views
        counts = [0] * n_views
        works = []

        def exchange(v):
            part = sums[v] if sums[v] is not None else torch.zeros_like(like)
            if counts[v] == 1:
                # the partial "sum" of a rank with ONE unit of the view IS that unit's render -- a tensor the caller
                # keeps reading (the mid frame's outputs feed the depth / flow terms): never reduce it in place
                # (8 MB per view at 1352x1014).  Two or more units: the sum is a fresh temporary.
                part = part.clone()
            if reduce_backward and not part.requires_grad:
                part = part.detach().requires_grad_(True).clone()
            tot, work = _SumAcrossRanksAsync.apply_async(part, self.group, reduce_backward)
            totals[v] = tot
            works.append(work)

        # collectives of one group are matched by ISSUE ORDER: every rank starts the exchanges in view order (a rank
        # with no unit of a view joins its exchange as soon as the earlier views are done)
        for v in range(n_views):
            for vv, k in mine:
                if vv == v:
                    img = render_unit(v, k)
                    sums[v] = img if sums[v] is None else sums[v] + img
                    counts[v] += 1
            exchange(v)
        for w in works:
            if w is not None:
                w.wait()
        if as_list:   # per-view tensors without a common stack node: backward_by_view walks each view's graph on its own
            return [t / n_sub + 1e-10 for t in totals]
        return torch.stack(totals) / n_sub + 1e-10

    # ---- backward exchange --------------------------------------------------------------------------
    def all_reduce_gradients(self, params, async_op: bool = False):
        """ONE all_reduce(SUM) over all parameter gradients.  `params`: a FlatGradients (in place on its persistent
        buffer, statistics slots included) or a plain sequence of tensors (packed into a temporary flat buffer;
        missing grads count as zero)."""
        if isinstance(params, FlatGradients):
            params.gather_stray()
            if not self.collective:
                return None
            works = []
            for b in params.buffers():
                if b.dtype == torch.float16:
                    # a half-precision SUM over 8 ranks saturates / loses the small terms: reduce the half slice in
                    # fp32 and round once.  (The trainable fp16-storage mode keeps no half
                    # gradients at all: GaussianParams(attr_dtype=float16, master=True) accumulates them in fp32.)
                    w32 = b.float()
                    if async_op:  # the fp32 copy is reduced asynchronously; wait() rounds it back once
                        works.append(_CopyBackWork(_all_reduce_sum(w32, self.group, True, tag="grad16"), b, w32))
                    else:
                        _all_reduce_sum(w32, self.group)
                        b.copy_(w32)
                else:
                    works.append(_all_reduce_sum(b, self.group, async_op, tag="grad"))
            return works if async_op else None
        if not self.collective:
            return None
        params = [p for p in params if p.requires_grad]
        if not params:
            return None
        flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1).to(torch.float32)
                          for p in params])
        _all_reduce_sum(flat, self.group)
        off = 0
        for p in params:  # the reduced gradients stay in the flat buffer: every .grad becomes a view of it
            n = p.numel()
            g = flat[off:off + n].view_as(p)
            p.grad = g if p.dtype == torch.float32 else g.to(p.dtype)
            off += n
        return None

    def backward_by_view(self, buckets: Sequence[FlatGradients], view_backward: Callable[[int], None],
                         after_view: Optional[Callable[[int], None]] = None) -> FlatGradients:
        """The backward pass of an iteration, one VIEW at a time, with one gradient message per view:

            for v: buckets[v] becomes the .grad storage; view_backward(v) back-propagates the loss terms of view v (and
                   only them: the caller keeps per-view loss terms apart -- the photometric mean over V equal-sized
                   images is the mean of the per-view terms); after_view(v) may deposit that view's densification
                   statistics in buckets[v]; its all-reduce STARTS asynchronously on the communication stream
            then:  await them in order, buckets[0] += buckets[1:] (one multi-tensor add), re-attach buckets[0].

        The exchange of view v's 68-MB message thus runs while view v + 1 back-propagates; only the last view's is
        exposed.  Gradients afterwards live in buckets[0] (returned); every view's statistics
        slots stay in its own bucket.  Without a process group: the same loop without exchanges."""
        works = []
        for v, b in enumerate(buckets):
            b.zero()
            view_backward(v)
            if after_view is not None:
                after_view(v)
            works.append(self.all_reduce_gradients(b, async_op=True))
        for ws in works:
            for w in (ws or []):
                w.wait()
        first = buckets[0]
        for name in ("flat", "flat_half"):
            rest = [getattr(b, name) for b in buckets[1:] if getattr(b, name).numel()]
            if rest:
                n_par = getattr(first, name).numel() if name == "flat_half" else first.param_floats
                dst = getattr(first, name)[:n_par]
                for r in rest:   # (parameter part only: every bucket's statistics slots are its own)
                    dst.add_(r[:n_par])
        for p, view in zip(first.params, first.views):
            p.grad = view
        return first

    def put_densification_stats(self, bucket: FlatGradients, name: str, viewspace_grad: Optional[torch.Tensor],
                                radii: Optional[torch.Tensor]) -> None:
        """The rank that rendered a view's mid frame deposits `viewspace_points.grad` [.., N, 2] and `radii` [N]
        (train.py:634-648 reads them for add_densification_stats) in the slot `name` (3 N floats) of the gradient
        message; the other ranks leave zeros, so the SUM hands them to everyone."""
        slot = bucket.extra(name)
        n = slot.numel() // 3
        if viewspace_grad is not None:
            slot[:2 * n].copy_(viewspace_grad.reshape(-1)[:2 * n])
        if radii is not None:
            slot[2 * n:].copy_(radii.reshape(-1).to(torch.float32))

    @staticmethod
    def get_densification_stats(bucket: FlatGradients, name: str) -> Tuple[torch.Tensor, torch.Tensor]:
        slot = bucket.extra(name)
        n = slot.numel() // 3
        return slot[:2 * n].view(n, 2), slot[2 * n:].to(torch.int32)


def broadcast_parameters(params: Iterable[torch.Tensor], src: int = 0, group=None) -> None:
    """Make every rank start from rank `src`'s replica."""
    if not (dist.is_available() and dist.is_initialized()):
        return
    for p in params:
        dist.broadcast(p.data, src=src, group=group)
