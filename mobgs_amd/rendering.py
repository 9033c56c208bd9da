"""Operator API (boundary B2): drop-in for `gsplat.rendering` as MoBGS uses it.

    from mobgs_amd.rendering import rasterization, fully_fused_projection

replaces `from gsplat.rendering import rasterization, fully_fused_projection`
(/root/reference/gaussian_renderer/__init__.py:15).  Keyword names, return tuple and `meta` keys follow
gsplat v1.4.0; every stage runs in libmobgs_hip.so (hand-written gfx950 kernels) through the C ABI of
include/mobgs_hip.h.  Options the reference never uses raise NotImplementedError.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from . import _fast, _lib, ops, profiler
from ._lib import DerivedCache, check, f32c, ptr, stream, stream_int

TILE = 16
# statistics of the most recent build_tile_lists() call (read by bench.py for the roofline line)
last_stats = {}


def _lib_():
    return _lib.load()


# --------------------------------------------------------------------------------------------------
# projection
# --------------------------------------------------------------------------------------------------
class _Project(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, quats, scales, viewmats, Ks, width, height, eps2d, near_plane, far_plane, radius_clip):
        lib = _lib_()
        means, quats, scales, viewmats, Ks = map(f32c, (means, quats, scales, viewmats, Ks))
        C, N = viewmats.shape[0], means.shape[0]
        dev = means.device
        radii = torch.empty(C, N, dtype=torch.int32, device=dev)
        means2d = torch.empty(C, N, 2, dtype=torch.float32, device=dev)
        depths = torch.empty(C, N, dtype=torch.float32, device=dev)
        conics = torch.empty(C, N, 3, dtype=torch.float32, device=dev)
        tiles_per_gauss = torch.empty(C, N, dtype=torch.int32, device=dev)
        check(lib.mobgs_project_fwd(C, N, ptr(means), ptr(quats), ptr(scales), ptr(viewmats), ptr(Ks), width, height,
                                    eps2d, near_plane, far_plane, radius_clip, ptr(radii), ptr(means2d), ptr(depths),
                                    ptr(conics), ptr(tiles_per_gauss), stream()), "mobgs_project_fwd")
        ctx.save_for_backward(means, quats, scales, viewmats, Ks, radii, conics)
        ctx.dims = (width, height, eps2d)
        ctx.mark_non_differentiable(radii, tiles_per_gauss)
        ctx.set_materialize_grads(False)  # no zero tensors for the outputs nothing back-propagates through
        return radii, means2d, depths, conics, tiles_per_gauss

    @staticmethod
    def backward(ctx, _v_radii, v_means2d, v_depths, v_conics, _v_tpg):
        return (*_project_bwd(ctx.saved_tensors, ctx.dims, v_means2d, v_depths, v_conics), None, None, None, None, None, None,
                None)


def _project_bwd(saved, dims, v_means2d, v_depths, v_conics):
    """The projection's backward pass on what _Project.forward (and the binning nodes' forwards) save: saved = (means, quats,
    scales, viewmats, Ks, radii, conics), dims = (width, height, eps2d).  -> (v_means, v_quats, v_scales, v_viewmats)."""
    lib = _lib_()
    means, quats, scales, viewmats, Ks, radii, conics = saved
    width, height, eps2d = dims
    F = _fast.get()
    if F is not None:  # the same body in C++ (csrc/fastpath.cpp)
        return F.project_bwd(width, height, eps2d, means, quats, scales, viewmats, Ks, radii, conics, v_means2d, v_depths,
                             v_conics, stream_int())
    C, N = viewmats.shape[0], means.shape[-2]
    dev = means.device
    v_means = torch.empty_like(means)
    v_quats = torch.empty_like(quats)
    v_scales = torch.empty_like(scales)
    v_viewmats = torch.empty_like(viewmats)
    partial = torch.empty(lib.mobgs_project_bwd_scratch_floats(C, N), dtype=torch.float32, device=dev)
    g2 = f32c(v_means2d) if v_means2d is not None else None
    gd = f32c(v_depths) if v_depths is not None else None
    gc = f32c(v_conics) if v_conics is not None else None
    check(lib.mobgs_project_bwd(C, N, 1 if means.dim() == 3 else 0, ptr(means), ptr(quats), ptr(scales),
                                ptr(viewmats), ptr(Ks), width, height, eps2d, ptr(radii), ptr(conics), ptr(g2),
                                ptr(gd), ptr(gc), ptr(v_means), ptr(v_quats), ptr(v_scales), ptr(v_viewmats),
                                ptr(partial), stream()), "mobgs_project_bwd")
    return v_means, v_quats, v_scales, v_viewmats


def fully_fused_projection(
    means: Tensor,
    covars: Optional[Tensor],
    quats: Optional[Tensor],
    scales: Optional[Tensor],
    viewmats: Tensor,
    Ks: Tensor,
    width: int,
    height: int,
    eps2d: float = 0.3,
    near_plane: float = 0.01,
    far_plane: float = 1e10,
    radius_clip: float = 0.0,
    packed: bool = False,
    sparse_grad: bool = False,
    calc_compensations: bool = False,
    camera_model: str = "pinhole",
) -> Tuple[Tensor, Tensor, Tensor, Tensor, Optional[Tensor]]:
    """gsplat.fully_fused_projection (unpacked, pinhole, quats+scales).  Returns
    (radii i32[C,N], means2d [C,N,2], depths [C,N], conics [C,N,3], compensations=None)."""
    if covars is not None or quats is None or scales is None:
        raise NotImplementedError("mobgs_amd: only the quats+scales parameterisation is supported")
    if packed or sparse_grad or calc_compensations or camera_model != "pinhole":
        raise NotImplementedError("mobgs_amd: packed / sparse_grad / compensations / non-pinhole are not supported")
    radii, means2d, depths, conics, _ = _Project.apply(means, quats, scales, viewmats, Ks, int(width), int(height),
                                                       float(eps2d), float(near_plane), float(far_plane),
                                                       float(radius_clip))
    return radii, means2d, depths, conics, None


# --------------------------------------------------------------------------------------------------
# tile intersection lists (no autograd)
# --------------------------------------------------------------------------------------------------
class TileLists:
    """Per-tile depth-ordered splat lists of one rasterization call.

    Lists built speculatively (SPECULATIVE_BINNING) are usable by the compositing kernels at once -- those read the
    lists through device pointers only -- while the three counts {n_box, n_isects, max_tile_len} are still on their
    way to the host.  Reading a count (or a count-sized view: flatten_ids, isect_ids) calls resolve(), which waits
    for them; if the arena was too small the kernels saw EMPTY lists and resolve() rebuilds the lists synchronously
    with a larger arena and returns True, upon which the caller re-issues what it had enqueued."""

    __slots__ = ("C", "N", "tile_w", "tile_h", "cum_tiles", "keep_scan", "tile_offsets", "tile_order",
                 "flatten_arena", "_n_box", "_n_isects", "_max_tile_len", "_flatten_ids", "_isect_ids", "_pending",
                 "rebuilds", "defer", "records", "tiles_per_gauss", "order")

    def __init__(self):
        self._pending = None
        self.rebuilds = 0     # how many times resolve() had to rebuild the lists (arena overflow)
        self.defer = False    # True: compositing calls do not resolve; the caller does, later, and re-issues them
        self.records = None   # compositor records written by the projection kernel (SharedProjection(pack_colors=))
        # [C*N] bounding-box tile counts: splat g's gradient slots span cum_tiles[g] .. + tiles_per_gauss[g] (the reductions
        # take it so that the lists may have been built with an enumeration order, see SharedProjection(order=))
        self.tiles_per_gauss = None
        self.order = None     # the enumeration order the lists were built with (None: splat order)

    @property
    def pending(self) -> bool:
        return self._pending is not None

    def resolve(self) -> bool:
        p, self._pending = self._pending, None
        return p.finish(self) if p is not None else False

    def _fill(self, C, N, tile_w, tile_h, cum_tiles, keep_scan, tile_offsets, tile_order, tiles_per_gauss, order=None):
        """Geometry and buffers of one binning call (the counts and the count-sized views follow: _set_counts)."""
        self.C, self.N, self.tile_w, self.tile_h = C, N, tile_w, tile_h
        self.cum_tiles, self.keep_scan, self.tile_offsets, self.tile_order = cum_tiles, keep_scan, tile_offsets, tile_order
        self.tiles_per_gauss, self.order = tiles_per_gauss, order

    def _set_counts(self, n_box, n_isects, max_len, flatten_arena, isect_arena):
        self._n_box, self._n_isects, self._max_tile_len = n_box, n_isects, max_len
        self.flatten_arena = flatten_arena
        self._flatten_ids = flatten_arena[:n_isects]
        self._isect_ids = isect_arena[:n_isects] if isect_arena is not None else None

    n_box = property(lambda self: (self.resolve(), self._n_box)[1])
    n_isects = property(lambda self: (self.resolve(), self._n_isects)[1])
    max_tile_len = property(lambda self: (self.resolve(), self._max_tile_len)[1])
    flatten_ids = property(lambda self: (self.resolve(), self._flatten_ids)[1])
    isect_ids = property(lambda self: (self.resolve(), self._isect_ids)[1])


class _StatsSlots:
    """Page-locked landing slots (4 x int64 each: three counts + a sequence word the device writes last) for the
    asynchronous count read-back, one pool per process."""

    def __init__(self, n=256):
        self.block = torch.zeros(n, 4, dtype=torch.int64, pin_memory=True)
        self.view = self.block.numpy()  # same memory: polled without going through the dispatcher
        self.base = self.block.data_ptr()
        self.free = list(range(n))
        self.seq = 0

    def take(self):
        """-> (row: numpy view of 4 int64, slot index | None, host address of the row, owner keeping it alive)"""
        if self.free:
            i = self.free.pop()
            return self.view[i], i, self.base + 32 * i, self.block
        extra = torch.zeros(4, dtype=torch.int64, pin_memory=True)  # pool exhausted: a one-off pinned row
        return extra.numpy(), None, extra.data_ptr(), extra

    def next_seq(self) -> int:
        self.seq += 1
        return self.seq

    def give(self, i):
        if i is not None:
            self.free.append(i)


_stats_slots = None


class _PendingCounts:
    """The read-back half of a speculative mobgs_project_and_bin_speculative call."""

    def __init__(self, row, slot, event, caps, arenas, rebuild_args, seq=0, owner=None):
        self.row, self.slot, self.event, self.seq = row, slot, event, seq  # row: numpy view of the pinned words
        self.caps, self.arenas, self.rebuild_args = caps, arenas, rebuild_args
        self.owner = owner  # the pinned tensor behind `row`

    def __del__(self):
        # dropped without finish() (exception, unused result): the device may still be about to write this slot, so
        # it goes back to the pool only when its sequence word has arrived; otherwise it is simply retired
        if self.slot is None or _stats_slots is None:
            return
        import sys
        if sys is None or sys.is_finalizing():  # interpreter shutdown: torch / HIP may already be torn down
            return
        try:
            arrived = int(self.row[3]) == self.seq if self.event is None else bool(self.event.query())
        except Exception:  # noqa: BLE001
            arrived = False
        if arrived:
            _stats_slots.give(self.slot)
        self.slot = None

    def _wait(self):
        if self.event is not None:
            self.event.synchronize()
            return
        # the device stores the counts and then the sequence number into the pinned row: poll it (no event was
        # recorded, so nothing sits between the binning kernels and what was enqueued behind them)
        import time
        word = self.row
        if int(word[3]) == self.seq:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("mobgs: render() cannot be captured into a HIP graph (the host reads the intersection "
                               "counts of the frame between binning and the end of the forward pass)")
        # The counts are normally there within ~0.2 ms of the call: spin for that long (a sleep costs 50+ us of wake-up
        # latency), then yield the core between polls -- the wait is bounded by TIME, not by an iteration count that is a
        # different duration on every host (up to 20 000 iterations of busy-spinning)
        t0 = time.monotonic()
        while int(word[3]) != self.seq:
            dt = time.monotonic() - t0
            if dt < 250e-6:
                continue
            if dt > 10.0:
                torch.cuda.synchronize()
                if int(word[3]) != self.seq:
                    raise RuntimeError("mobgs: the intersection counts never arrived (device fault?)")
            time.sleep(20e-6 if dt < 2e-3 else (100e-6 if dt < 0.05 else 1e-3))  # queue full of other work: stop burning a core

    def finish(self, tl) -> bool:
        self._wait()
        n_box, n_isects, max_len = (int(v) for v in self.row[:3])
        _stats_slots.give(self.slot)
        self.slot = None
        key, cap_box, cap_listed, seg_stride = self.caps
        hints = hint_record(key)
        if n_box <= cap_box and n_isects <= cap_listed and (seg_stride == 0 or max_len <= seg_stride):
            tl._set_counts(n_box, n_isects, max_len, *self.arenas)
            hints.resolved(n_box, n_isects, max_len)
            last_stats.update(n_isects=n_isects, n_box=n_box, max_tile_len=max_len,
                              n_tiles=tl.C * tl.tile_w * tl.tile_h)
            return False
        # arena too small (first frame of a scene, or the scene grew) or, with single-pass lists, a tile's list longer
        # than its key segment: every kernel enqueued so far saw empty lists; rebuild synchronously with the two-pass
        # entry points -- the projection outputs do not depend on the arena
        if seg_stride and max_len > seg_stride:
            seg_overflows[0] += 1
        hints.overflowed(n_box)
        fresh = build_tile_lists(*self.rebuild_args)
        # (order = None: the two-pass rebuild enumerates in splat order)
        tl._fill(tl.C, tl.N, tl.tile_w, tl.tile_h, fresh.cum_tiles, fresh.keep_scan, fresh.tile_offsets, fresh.tile_order,
                 fresh.tiles_per_gauss)
        tl._set_counts(fresh._n_box, fresh._n_isects, fresh._max_tile_len, fresh.flatten_arena, fresh._isect_ids)
        hints.rebuilt(fresh._n_isects, fresh._max_tile_len)
        tl.rebuilds += 1
        list_rebuilds[0] += 1
        return True


list_rebuilds = [0]  # speculative binning calls whose arena was too small (lists rebuilt synchronously) -- diagnostics
seg_overflows = [0]  # ... of them, single-pass calls in which a tile's list outgrew its key segment
fused_calls = [0]    # binning calls that took the single-pass path (diagnostics / tests)
# Single-pass tile lists (round 5; include/mobgs_hip.h mobgs_project_and_bin_fused): the binning kernel writes every sort
# key straight into its tile's segment of a strided arena sized from the previous frame's longest list x SEG_SLACK; the
# first frame of a workload (no hint yet), lists beyond the one-launch sort (2048 entries) and arenas beyond
# FUSED_ARENA_BYTES take the two-pass path, as does the synchronous rebuild after an overflow.  Outputs are identical.
FUSED_LISTS = os.environ.get("MOBGS_FUSED_LISTS", "1") != "0"
SEG_SLACK = 1.3
# cap of the single-pass key arena (nt x 8 copies x seg_stride x 8 bytes: ~145 MB for one 1352x1014 camera, ~1.3 GB for
# an 8-camera batch); beyond it the call takes the two-pass path (cap_listed x 8 bytes).  MOBGS_FUSED_ARENA_MB overrides
# (peak memory had no knob short of switching the path off)
FUSED_ARENA_BYTES = int(float(os.environ.get("MOBGS_FUSED_ARENA_MB", "2048")) * (1 << 20))
_FUSED_COPIES = 8  # counter copies of the binning kernel (csrc/isect.hip TC_COPIES)


class _Hints:
    """What one workload (_workload_key) carries from frame to frame: arena capacities, the longest tile list (selects the
    binning / sort variant and sizes the key segments), the last resolved counts (StaticCapacity sizes from them) and the
    key-segment stride in use.  Performance only -- a wrong hint costs a rebuild, never a result.  The methods below are
    the only code of this module that writes the fields, one method per event (DESIGN.md has the table).
    cap_box: capacity of the keep-flag buffer (grows geometrically, never shrinks); cap_listed: of the listed-intersection
    buffers; longest: longest per-tile list of the previous frames; last_counts: (I_box, I_listed) of the most recent
    resolved frame; seg_stride: key-segment stride of the single-pass path (sticky, see stride())."""

    __slots__ = ("cap_box", "cap_listed", "longest", "last_counts", "seg_stride")

    def __init__(self):
        self.cap_box = self.cap_listed = self.longest = self.seg_stride = 0
        self.last_counts = (0, 0)

    def caps(self, C, N):
        """-> (cap_box, cap_listed, len_hint) a call takes by default."""
        box = max(self.cap_box, 16 * (C * N) + 1024)
        return box, max(self.cap_listed, box // 2), self.longest

    def static_caps(self, C, N, margin):
        """... and under StaticCapacity(margin): the last resolved frame's counts times `margin`, once there is one."""
        box, listed, _ = self.caps(C, N)
        seen_box, seen_listed = self.last_counts
        if seen_box:
            box = max(int(seen_box * margin) + 1024, 4096)
            listed = max(int(seen_listed * margin) + 1024, 4096)
        return box, listed, int(self.longest * margin)

    def stride(self, len_hint, C, N, nt, cap_box) -> int:
        """Key-segment capacity per tile for the single-pass path, or 0 = use the two-pass path.
        The stride is STICKY per workload: the hint breathes by a few per cent from view to view, and an arena whose size
        changes with it defeats the caching allocator (a slightly larger block is a fresh hipMalloc, which synchronises the
        device; DESIGN.md has the measurement).  A needed stride within [prev / 2, prev] keeps `prev`; a larger one grows
        with 25 % headroom; only a workload that shrank to less than half gives memory back."""
        if not FUSED_LISTS or N <= 0 or len_hint <= 0 or cap_box < 4 * C * N + 2:
            return 0
        stride = max(64, (int(len_hint * SEG_SLACK) + 15) // 16 * 16)
        limit = _lib_().mobgs_fused_max_seg_stride()
        prev = self.seg_stride
        if prev >= stride > prev // 2:
            stride = prev
        else:
            grown = (int(stride * 1.25) + 15) // 16 * 16 if prev else stride
            if grown <= limit and nt * _FUSED_COPIES * grown * 8 <= FUSED_ARENA_BYTES:
                stride = grown
        if stride > limit or nt * _FUSED_COPIES * stride * 8 > FUSED_ARENA_BYTES:
            return 0
        self.seg_stride = stride
        return stride

    def keep_caps(self, cap_box, cap_listed):
        """The capacities a call was issued with (speculative: before its counts are known) or ended with (synchronous)."""
        self.cap_box, self.cap_listed = cap_box, cap_listed

    def _decay_to(self, max_len):
        # the hint decays slowly (5 % per frame), so that a camera path whose longest list fluctuates does not overflow
        # its segments every other frame
        self.longest = max(int(max_len), int(self.longest * 0.95))

    def resolved(self, n_box, n_isects, max_len):
        """A speculative frame resolved within its arenas."""
        self._decay_to(max_len)
        self.last_counts = (n_box, n_isects)

    def overflowed(self, n_box):
        """A speculative frame overflowed: grow the box arena BEFORE the synchronous rebuild (which sizes from it) ..."""
        self.cap_box = max(self.cap_box, int(n_box * 1.25) + 1024)

    def rebuilt(self, n_isects, max_len):
        """... and the listed arena from what the rebuild counted."""
        self.cap_listed = max(self.cap_listed, int(n_isects * 1.25) + 1024)
        self._decay_to(max_len)

    def measured(self, cap_box, max_len):
        """A synchronous build_tile_lists ended with this arena and this longest list (the hint is overwritten, no decay)."""
        self.cap_box, self.longest = cap_box, max_len

    def observed(self, n_box, n_isects, max_len):
        """StaticCapacity.check() read these counts from a landing row: running maxima."""
        self.last_counts = (max(n_box, self.last_counts[0]), max(n_isects, self.last_counts[1]))
        self.longest = max(max_len, self.longest)


_hints = {}  # workload key -> _Hints


def hint_record(key) -> _Hints:
    """The record of a workload key (created empty on first use)."""
    rec = _hints.get(key)
    if rec is None:
        rec = _hints[key] = _Hints()
    return rec


def forget_hints() -> None:
    """Tests / experiments: every workload starts afresh (first-frame guesses, two-pass lists)."""
    _hints.clear()


_tile_culling = True
# Caller-side policy handed to the library with every call (include/mobgs_hip.h MobgsTuning; the library itself keeps
# no state).  tuning.heavy_tile_len / tuning.quadrant_culling / tuning.block_walk may be changed by tests and
# experiments.
tuning = _lib.MobgsTuning()
if os.environ.get("MOBGS_BWD_MFMA") is not None:  # A/B arm of the round-4 backward compositor (1 / 0; unset = library default)
    tuning.bwd_mfma = int(os.environ["MOBGS_BWD_MFMA"])


def _tuning_with_hint(key):
    """`tuning` plus the longest list the previous frame on this device had (selects the dense binning variant)."""
    t = tuning.copy(longest_list_hint=hint_record(key).longest, geometry_per_camera=0)
    _tuning_keepalive.append(t)
    del _tuning_keepalive[:-8]
    return t.ref()


_tuning_keepalive = []

# Zero-cotangent gate (include/mobgs_hip.h MobgsTuning.gate_zero_cotangent): compositing nodes created while the gate is
# on probe their cotangents on the device in backward and skip the pass when all of them are zero -- a loss term
# multiplied by a zero weight (train.py:675 with lambda_flow_loss = 0) then costs a probe, not a backward pass.
# get_flow() / get_flow_many() switch it on for their nodes; render() leaves it off (its images always carry a loss).
_zero_gate = [0]


class zero_cotangent_gate:
    """with zero_cotangent_gate(): compositing nodes recorded inside skip their backward pass when every cotangent is
    exactly zero (decided on the device: no synchronisation).  Gradients are bit-identical otherwise."""

    def __init__(self, on=True):
        self.on = 1 if on else 0

    def __enter__(self):
        self.prev = _zero_gate[0]
        _zero_gate[0] = self.on
        return self

    def __exit__(self, *exc):
        _zero_gate[0] = self.prev
        return False


_probe_flags = {}


def cotangents_all_zero(tensors) -> bool:
    """Are all elements of all given float32 HIP tensors exactly zero?  One streaming probe on the device
    (mobgs_cotangent_probe) and ONE 4-byte read-back -- a host synchronisation: callers use it where dropping a whole
    backward sub-graph is worth one (gaussian_renderer._FlowHead), never inside a HIP-graph capture."""
    ts = [f32c(t) for t in tensors if t is not None and t.numel() > 0]
    if not ts:
        return True
    dev = ts[0].device
    flag = _probe_flags.get(dev)
    if flag is None:
        flag = _probe_flags[dev] = torch.zeros(1, dtype=torch.int32, device=dev)
    n = len(ts)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    counts = (ctypes.c_size_t * n)(*[t.numel() for t in ts])
    check(_lib_().mobgs_cotangent_probe(n, ptrs, counts, ptr(flag), stream()), "mobgs_cotangent_probe")
    return int(flag.item()) == 0


_variant_copies = {}
# A/B switch of MobgsTuning.static_rows (round 6): 0 = render() / get_flow() never state which rows are static, every
# entry takes the full blend body (gradients are bit-identical either way except for the sign of the zeros the static
# rows' f_t receive)
STATIC_ROWS = os.environ.get("MOBGS_STATIC_ROWS", "1") != "0"


# MobgsTuning.cover_slots (round 6): the plain backward pass on the quadrant kernel writes every gradient slot itself -- no
# zero fill of the slot buffer (108 MB per 1352x1014 render).  0: the fill, as before (A/B; gradients are bit-identical)
COVER_SLOTS = os.environ.get("MOBGS_COVER_SLOTS", "1") != "0"


def _tuning_variant(gated: bool, static_rows: int = 0, cover: bool = False):
    """`tuning` with the zero-cotangent gate on and / or the static row count of the node and / or cover_slots (all are
    properties of the node, not of the module); copies are cached per (fields of `tuning`, gate, rows, cover)."""
    static_rows = int(static_rows) if STATIC_ROWS else 0
    if not gated and static_rows <= 0 and not cover:
        return tuning
    key = (tuning.heavy_tile_len, tuning.longest_list_hint, tuning.quadrant_culling, tuning.block_walk,
           tuning.bwd_block_walk, tuning.bwd_mfma, bool(gated), static_rows, bool(cover))
    t = _variant_copies.get(key)
    if t is None:
        if len(_variant_copies) > 64:
            _variant_copies.clear()
        t = _variant_copies[key] = tuning.copy(geometry_per_camera=0, gate_zero_cotangent=1 if gated else 0,
                                               static_rows=max(static_rows, 0), cover_slots=1 if cover else 0)
    return t


def _tuning_gated():
    return _tuning_variant(True, 0)


class StaticCapacity:
    """Context: speculative binning WITHOUT the count read-back (round 3: HIP-graph capture of a whole render step).

    Outside this context the host reads the frame's three counts {I_box, I_listed, longest list} mid-forward, to size
    count-dependent views and to redo the binning when an arena overflowed -- a host read no graph can contain.  Inside,
    every count-sized buffer takes its CAPACITY instead (the kernels read the true extents from device memory anyway:
    tile offsets, keep-scan bases, a tile schedule padded with -1), the counts still land in a pinned row, and nobody
    waits for them: `check()` -- after the work has completed -- tells whether any arena was too small (the kernels then
    saw EMPTY lists and the frame's outputs are invalid: grow and redo / re-capture).  Capacities are fixed at entry:
    the previous frame's counts of the same workload times `margin`."""

    def __init__(self, margin: float = 1.5, max_calls: int = 64):
        self.margin = float(margin)
        self.rows = []   # (pinned row, owner tensor, cap_box, cap_listed, key, seg_stride)
        self._prev = None
        # landing rows of the calls issued inside the context, page-locked BEFORE anything is captured (a pinned
        # allocation is not a legal call while a stream is capturing)
        self.pool = torch.zeros(max_calls, 4, dtype=torch.int64, pin_memory=True)
        self.pool_np = self.pool.numpy()

    def take_row(self):
        i = len(self.rows)
        if i >= self.pool.shape[0]:
            raise RuntimeError("StaticCapacity: more binning calls than landing rows (max_calls)")
        return self.pool_np[i], self.pool.data_ptr() + 32 * i

    def __enter__(self):
        global _static
        self._prev, _static = _static, self
        return self

    def __exit__(self, *exc):
        global _static
        _static = self._prev
        return False

    def caps(self, key, C, N):
        return hint_record(key).static_caps(C, N, self.margin)

    def check(self) -> bool:
        """True when every binning call issued under this context fitted its arenas (call after a synchronisation)."""
        ok = True
        for row, _, cap_box, cap_listed, key, seg_stride in self.rows:
            n_box, n_isects, max_len = (int(v) for v in row[:3])
            hint_record(key).observed(n_box, n_isects, max_len)
            ok = ok and n_box <= cap_box and n_isects <= cap_listed and (seg_stride == 0 or max_len <= seg_stride)
        return ok


_static = None
# True: the projection/binning call does not wait for the intersection counts (see TileLists); False: it does
SPECULATIVE_BINNING = True
# True: the compositing kernels take tiles heaviest-list-first (TileLists.tile_order); False: raster order
TILE_SCHEDULE = os.environ.get("MOBGS_TILE_SCHEDULE", "1") != "0"


# Whose hints: the renderer's entry points (gaussian_renderer.render & co) run inside hint_scope(scene token) -- a small
# integer attached to the (static, dynamic) pair of Gaussian sets the first time they are rendered -- and the token is part
# of every workload key: two scenes of equal size, or two threads rendering different scenes, no longer read and overwrite
# each other's arena capacities / list-length hints / segment strides (the hints are performance-only,
# sharing them costs rebuilds, never results).  Thread-local; token 0 = callers of the operator API without a scope.
import threading as _threading

_hint_tls = _threading.local()


class hint_scope:
    def __init__(self, token: int):
        self.token = int(token)

    def __enter__(self):
        self.prev = getattr(_hint_tls, "token", 0)
        _hint_tls.token = self.token
        return self

    def __exit__(self, *exc):
        _hint_tls.token = self.prev
        return False


_scene_counter = [0]


def scene_token(stat_pc, dyn_pc) -> int:
    """The pair's token (kept on the dynamic set's object: it dies with it; ids of dead objects are never reused)."""
    tok = getattr(dyn_pc, "_mobgs_scene_tokens", None)
    if tok is None:
        tok = {}
        try:
            dyn_pc._mobgs_scene_tokens = tok
        except AttributeError:   # (an object that takes no attributes: one shared scope)
            return 0
    t = tok.get(id(stat_pc))
    if t is None:
        _scene_counter[0] += 1
        t = tok[id(stat_pc)] = _scene_counter[0]
    return t


def _workload_key(dev, C, N, width, height):
    """Arena sizes and list-length hints carry over from the previous frame OF THE SAME WORKLOAD: scene (hint_scope),
    device, cameras, splat count (in steps of 1/8 octave, so a scene that densifies keeps its arenas) and image size -- two
    scenes or a full-set and a dynamic-only projection sharing a device do not fight over one entry."""
    n_bucket = 0 if N <= 0 else int(8 * math.log2(N))
    return (getattr(_hint_tls, "token", 0), dev.index if dev.index is not None else -1, int(C), n_bucket, int(width),
            int(height))


def set_tile_culling(flag: bool) -> None:
    """True (default): a splat is listed in a tile only if it can reach alpha >= 1/255 there -- pixels and gradients
    are bit-identical (gradients equal up to summation order), `meta["flatten_ids" / "isect_ids" / "isect_offsets"]` are then a subset of gsplat's lists.
    False: lists are exactly gsplat's (every tile the 3-sigma bounding box touches)."""
    global _tile_culling
    _tile_culling = bool(flag)


def get_tile_culling() -> bool:
    return _tile_culling


@torch.no_grad()
def build_tile_lists(means2d: Tensor, radii: Tensor, depths: Tensor, conics: Tensor, opacities: Tensor,
                     tiles_per_gauss: Tensor, width: int, height: int, want_isect_ids: bool = True) -> TileLists:
    if _static is not None:
        raise RuntimeError("StaticCapacity: build_tile_lists (the separate projection + binning of rasterization()) reads "
                           "the intersection counts back on the host -- use SharedProjection / render(), whose binning "
                           "call honours the context")
    lib = _lib_()
    C, N = radii.shape
    dev = radii.device
    tile_w, tile_h = math.ceil(width / TILE), math.ceil(height / TILE)
    nt = C * tile_w * tile_h
    tl = TileLists()
    cum_tiles = torch.empty(C * N + 1, dtype=torch.int32, device=dev)
    tile_offsets = torch.empty(nt + 1, dtype=torch.int32, device=dev)
    tile_order = torch.empty(lib.mobgs_tile_order_len(nt), dtype=torch.int32, device=dev) if TILE_SCHEDULE else None
    stats = torch.empty(3, dtype=torch.int64, device=dev)
    opac = f32c(opacities)
    key = _workload_key(dev, C, N, width, height)
    hints = hint_record(key)
    cap = hints.caps(C, N)[0]
    while True:
        keep_scan = torch.empty(lib.mobgs_keep_scan_len(cap), dtype=torch.int32, device=dev)
        scratch = torch.empty(lib.mobgs_isect_scratch_bytes(C * N, nt, cap), dtype=torch.uint8, device=dev)
        check(lib.mobgs_isect_offsets(C, N, tile_w, tile_h, width, height, int(_tile_culling), cap,
                                      ptr(tiles_per_gauss), ptr(means2d), ptr(radii), ptr(conics), ptr(opac),
                                      1 if opac.dim() == 2 else 0, ptr(cum_tiles), ptr(keep_scan),
                                      ptr(tile_offsets), ptr(tile_order), 0, ptr(stats), ptr(scratch),
                                      _tuning_with_hint(key), stream()),
              "mobgs_isect_offsets")
        n_box, n_isects, max_len = (int(v) for v in stats.tolist())  # the pipeline's one host sync (as in gsplat)
        if n_box <= cap:
            break
        cap = int(n_box * 1.25) + 1024  # first call on a denser scene: grow and redo (rare)
    hints.measured(cap, max_len)  # (the hint: dense-region variant of the next frame's binning when lists are long)
    tl._fill(C, N, tile_w, tile_h, cum_tiles, keep_scan, tile_offsets, tile_order, tiles_per_gauss)
    last_stats.update(n_isects=n_isects, n_box=n_box, max_tile_len=max_len, n_tiles=nt)
    flatten_ids = torch.empty(n_isects, dtype=torch.int32, device=dev)
    isect_ids = torch.empty(n_isects, dtype=torch.int64, device=dev) if want_isect_ids else None
    tl._set_counts(n_box, n_isects, max_len, flatten_ids, isect_ids)
    if n_isects > 0:
        keys = torch.empty(n_isects, dtype=torch.int64, device=dev)
        check(lib.mobgs_isect_emit_sort(C, N, tile_w, tile_h, cap, n_isects, max_len, ptr(depths), ptr(cum_tiles),
                                        ptr(tile_offsets), ptr(scratch), ptr(keys), ptr(flatten_ids),
                                        ptr(isect_ids), stream()), "mobgs_isect_emit_sort")
    return tl


# --------------------------------------------------------------------------------------------------
# compositing
# --------------------------------------------------------------------------------------------------
_SUPPORTED = (1, 2, 3, 4, 9, 10, 12, 16, 26)

# Which compositing kernels the passes took (tests only; None = off, the default: nothing is computed).  A test sets
# `rendering.path_log = []`, runs, and ASSERTS the selection from the entries -- dicts {"dir": "fwd" | "bwd", "D", "n_tiles",
# "class_filter", "bwd_kernel": "quadrant" | "mfma" | "mfma_team" | "block_walk", "fwd_kernel": "blocks" | "quadrant",
# "heavy_len", "heavy_tiles" (tiles the schedule composites with four waves: read back from tile_order -- a host sync),
# "decode": the Sandwich epilogue ran inside the forward compositor, "static_rows"}.  The kernel names come from
# mobgs_raster_path(), the decision functions the launchers themselves use (include/mobgs_hip.h).
path_log = None
_BWD_NAMES = ("quadrant", "mfma", "mfma_team", "block_walk")


def _log_path(direction, D, tl, class_filter=False, tn=None, **extra):
    if path_log is None:
        return
    nt = tl.C * tl.tile_w * tl.tile_h
    bits = _lib_().mobgs_raster_path(int(D), 1 if class_filter else 0, nt, (tn if tn is not None else tuning).ref())
    heavy = 0
    if tl.tile_order is not None:
        order = tl.tile_order
        heavy = int(((order >= 0) & ((order & (1 << 30)) != 0)).sum().item()) // 4
    path_log.append(dict(dir=direction, D=int(D), n_tiles=nt, class_filter=bool(class_filter),
                         bwd_kernel=_BWD_NAMES[bits & 3], fwd_kernel="blocks" if bits & 4 else "quadrant",
                         heavy_len=bits >> 8, heavy_tiles=heavy, **extra))


def _lists_total_addr(tl) -> int:
    """Address of tile_offsets[n_tiles] -- the total number of listed entries, 0 when an arena overflowed and the binning kernels
    emptied the lists.  Handed to the slot reductions as their `any_record` word wherever stage 1 sets none (cover_slots, the
    class passes): without a host in the loop (StaticCapacity / a HIP-graph replay) an overflowed frame's keep_scan and slot
    ranges must not be read (found in round 6: a graphed training loop faulted when the scene outgrew its arenas)."""
    to = tl.tile_offsets
    return to.data_ptr() + 4 * (to.numel() - 1)


_path_bits_cache = {}


def _raster_path_bits(D: int, nt: int, class_filter: int = 0) -> int:
    """mobgs_raster_path(D, class_filter, nt, tuning) -- which kernels a plain (class) pass takes -- cached per (D, grid,
    policy fields): the backward node asks once per call, and a ctypes call + a pointer object cost the host ~5 us each time."""
    key = (int(D), int(nt), tuning.heavy_tile_len, tuning.bwd_mfma, tuning.bwd_block_walk, tuning.block_walk, class_filter)
    bits = _path_bits_cache.get(key)
    if bits is None:
        if len(_path_bits_cache) > 256:
            _path_bits_cache.clear()
        bits = _path_bits_cache[key] = int(_lib_().mobgs_raster_path(int(D), class_filter, int(nt), tuning.ref()))
    return bits


def _zero_dead_channels(v_colors, static_rows, D, bits):
    """MobgsTuning.static_rows: v_colors[.., 6..8] of the static rows of a 10-channel pass is returned as 0.  Only the
    quadrant backward kernel has the short blend body that leaves those sums at their cleared zeros; the matrix-pipe and
    block-walk kernels (bits & 3 != 0) never read the field and return the real gradient, so the zeros are written here --
    whatever the rows hold: the quadrant kernel still returns the real gradient of a static row whose dead channels are
    not zero, these arms do not (found by tests/test_gpu_raster_kernels.py; the selection of the benchmark's grid is the quadrant kernel: no extra
    launch there)."""
    if static_rows > 0 and D == 10 and (bits & 3) != 0:
        v_colors[:, :static_rows, 6:9] = 0.0


def _refuse_token(colors, packed, who):
    """The fused prep path hands a colour TOKEN through render() (SharedProjection.from_raw): never-written storage that
    stands for "the records the projection kernel packed".  A consumer about to read it as an array stops here."""
    if getattr(colors, "_mobgs_colour_token", False) and packed is None:
        raise RuntimeError(f"{who}: got the fused-prep colour token without matching packed records -- the colour "
                           "features exist only inside SharedProjection.tl.records (call ops.PrepSplats for an array)")


def _pad_channels(D: int) -> int:
    for s in _SUPPORTED:
        if s >= D:
            return s
    raise NotImplementedError(f"mobgs_amd: {D} colour channels exceed the compiled maximum ({_SUPPORTED[-1]})")


_const_cache = {}


def _const(make, *shape, dev):
    """A float32 constant (make = torch.ones | torch.zeros) that kernels only read: built once per shape and device."""
    key = (make, shape, str(dev))
    t = _const_cache.get(key)
    if t is None:
        if len(_const_cache) > 16:
            _const_cache.clear()
        t = _const_cache[key] = make(*shape, dtype=torch.float32, device=dev)
    return t


def _ptr3(tensors):
    return (ctypes.c_void_p * 3)(*[None if t is None else t.data_ptr() for t in tensors])


# -- one host body per launch: the fast-path arm (csrc/fastpath.cpp, where it has one) and the ctypes arm side by side --------
def _pack_records(C, N, channels, means2d, conics, colors, opacities, extra, radii):
    """mobgs_pack_records: the compositor's per-splat records of these (float32, contiguous) inputs -> [C*N, stride]."""
    lib = _lib_()
    D = channels + (1 if extra is not None else 0)
    records = torch.empty(C * N, lib.mobgs_record_stride(D), dtype=torch.float32, device=means2d.device)
    check(lib.mobgs_pack_records(C, N, channels, ptr(means2d), ptr(conics), ptr(colors), 1 if colors.dim() == 3 else 0,
                                 ptr(opacities), 1 if opacities.dim() == 2 else 0, ptr(extra), ptr(radii), ptr(records),
                                 stream()), "mobgs_pack_records")
    return records


def _new_reach(tl, dev):
    """Per list entry: the quadrants of its tile the splat can reach -- computed by the forward kernels anyway, kept for the
    backward pass over the same lists."""
    return torch.empty(max(tl.flatten_arena.numel(), 1), dtype=torch.uint8, device=dev)


def _composite_until_resolved(tl, launch, honour_defer, reach=None):
    """Run `launch(reach) -> reach` (one forward compositing launch over tl's lists) until the lists it read are final:
    speculative lists whose arena was too small get rebuilt by tl.resolve(), then `reach` is regrown to the new arena and the
    launch issued again.  -> the reach buffer of the last launch (None for a kernel that keeps none).
    honour_defer: a caller that wants to enqueue more work before waiting for the counts sets tl.defer and resolves and
    re-issues by itself.  render() sets `defer` only around composite_decode, which composites through _Rasterize, so
    _Rasterize and _RasterizeClassAlpha (the nodes of the main image and its coverage) pass True; _RasterizeLayers and
    _RasterizeClasses have always resolved on the spot and pass False."""
    while True:
        if reach is not None and reach.numel() < tl.flatten_arena.numel():  # lists rebuilt into a larger arena
            reach = torch.empty(tl.flatten_arena.numel(), dtype=torch.uint8, device=reach.device)
        reach = launch(reach)
        if (honour_defer and tl.defer) or not tl.resolve():
            return reach


def _new_slots(tl, stride, dev, cover=False):
    """Gradient slots of one backward pass: a row per list entry + one extra row whose first word is the any_record flag of
    include/mobgs_hip.h (zeroed by the same fill; + the gate word of a gated pass).  cover (MobgsTuning.cover_slots): the
    kernel writes every slot -- no fill."""
    return (torch.empty if cover else torch.zeros)(max(tl.n_isects, 1) + 1, stride, dtype=torch.float32, device=dev)


def _slot_flag(tl, slots, source, fast):
    """The `any_record` word of a backward launch (include/mobgs_hip.h), from one of its three sources: "row" -- the first
    word of the slot buffer's extra last row (_new_slots), which stage 1 sets; "total" -- the lists' total
    (_lists_total_addr), wherever stage 1 sets none (cover_slots, the 10-channel class passes); None -- no flag.
    fast: as the C++ host bodies take it (-1 = the extra row, an address, 0 = none), else as ctypes does (c_void_p | None)."""
    if source == "row":
        return -1 if fast else ctypes.c_void_p(slots.data_ptr() + 4 * (slots.shape[0] - 1) * slots.shape[1])
    if source == "total":
        return _lists_total_addr(tl) if fast else ctypes.c_void_p(_lists_total_addr(tl))
    return 0 if fast else None


def _raster_bwd(tl, records, bg, radii, means2d, alphas, last_ids, v_render, v_alphas, reach, dims, tn, cover):
    """Stage 1 of the backward pass (mobgs_raster_bwd): per-entry gradient records -> slots.
    dims = (C, N, channels, has_extra, width, height)."""
    C, N, channels, has_extra, width, height = dims
    F = _fast.get()
    if F is not None:  # the same body in C++ (csrc/fastpath.cpp)
        with profiler.region("raster_bwd"):
            return F.raster_bwd(C, N, channels, int(has_extra), width, height, tl.n_isects, records, bg, radii, means2d,
                                tl.cum_tiles, tl.keep_scan, tl.tile_offsets, tl.tile_order, tl.flatten_ids, alphas,
                                last_ids, v_render, v_alphas, reach, tn.address(), stream_int(), cover)
    v_render = f32c(v_render)
    v_alphas = f32c(v_alphas) if v_alphas is not None else None
    slots = _new_slots(tl, records.shape[1], records.device, cover)
    flag = _slot_flag(tl, slots, None if cover else "row", False)
    lib = _lib_()
    with profiler.region("raster_bwd"):
        check(lib.mobgs_raster_bwd(C, N, channels, int(has_extra), width, height, ptr(records), ptr(bg), ptr(radii),
                                   ptr(means2d), ptr(tl.cum_tiles), ptr(tl.keep_scan), ptr(tl.tile_offsets),
                                   ptr(tl.tile_order), ptr(tl.flatten_ids), ptr(alphas), ptr(last_ids), ptr(v_render),
                                   ptr(v_alphas), ptr(slots), ptr(reach), flag, tn.ref(), stream()), "mobgs_raster_bwd")
    return slots


def _raster_bwd_decode(tl, records, bg, radii, render, alphas, last_ids, v_rgb, v_depth, v_alphas, dec, reach, dims, tn,
                       cover):
    """Stage 1 with the decoder's backward pass as the kernel's prologue (mobgs_raster_bwd_decode; dec = (intr, c2w, w1, w2)
    as the forward saved them) -> (slots, partial rows of the decoder's weight / pose gradient sums).
    dims = (C, N, width, height)."""
    C, N, width, height = dims
    intr, c2w, w1, w2 = dec
    va = v_alphas.reshape(C, height, width) if v_alphas is not None else None
    F = _fast.get()
    with profiler.region("raster_bwd"):
        if F is not None:
            return F.raster_bwd_decode(C, N, width, height, tl.n_isects, records, bg, radii, tl.cum_tiles, tl.keep_scan,
                                       tl.tile_offsets, tl.tile_order, tl.flatten_ids, render, alphas, last_ids, v_rgb,
                                       v_depth, va, intr, c2w, w1, w2, reach, tn.address(), stream_int(), cover)
        lib = _lib_()
        dev = records.device
        v_rgb = f32c(v_rgb) if v_rgb is not None else torch.zeros(C, 3, height, width, dtype=torch.float32, device=dev)
        v_depth = f32c(v_depth) if v_depth is not None else None
        va = f32c(va) if va is not None else None
        slots = _new_slots(tl, records.shape[1], dev, cover)
        partial = torch.empty(lib.mobgs_raster_bwd_decode_scratch_floats(C, width, height), dtype=torch.float32, device=dev)
        check(lib.mobgs_raster_bwd_decode(
            C, N, width, height, ptr(records), ptr(bg), ptr(radii), ptr(tl.cum_tiles), ptr(tl.keep_scan),
            ptr(tl.tile_offsets), ptr(tl.tile_order), ptr(tl.flatten_ids), ptr(render), ptr(alphas), ptr(last_ids),
            ptr(v_rgb), ptr(v_depth), ptr(va), ptr(intr), 4 if (C > 1 and intr.numel() == 4 * C) else 0, ptr(c2w),
            (c2w.numel() // C) if (C > 1 and c2w.dim() == 3) else 0, ptr(w1), ptr(w2), ptr(slots), ptr(reach),
            _slot_flag(tl, slots, None if cover else "row", False), ptr(partial), tn.ref(), stream()),
            "mobgs_raster_bwd_decode")
    return slots, partial


def _reduce_slots(tl, records, slots, flag_source, C, N, channels, has_extra):
    """Stage 2 (mobgs_raster_bwd_reduce): the slots of every splat summed
    -> (v_means2d [C,N,2], v_conics [C,N,3], v_opac [C,N], v_colors [C,N,channels], v_extra [C,N] | None)."""
    F = _fast.get()
    if F is not None:
        return F.raster_bwd_reduce(C, N, channels, int(has_extra), records, tl.cum_tiles, tl.keep_scan, slots, stream_int(),
                                   tl.tiles_per_gauss, _slot_flag(tl, slots, flag_source, True))
    dev = records.device
    v_means2d = torch.empty(C, N, 2, dtype=torch.float32, device=dev)
    v_conics = torch.empty(C, N, 3, dtype=torch.float32, device=dev)
    v_opac = torch.empty(C, N, dtype=torch.float32, device=dev)
    v_colors = torch.empty(C, N, channels, dtype=torch.float32, device=dev)
    v_extra = torch.empty(C, N, dtype=torch.float32, device=dev) if has_extra else None
    lib = _lib_()
    check(lib.mobgs_raster_bwd_reduce(C, N, channels, int(has_extra), ptr(records), ptr(tl.cum_tiles), ptr(tl.keep_scan),
                                      ptr(slots), _slot_flag(tl, slots, flag_source, False), ptr(v_means2d), ptr(v_conics),
                                      ptr(v_opac), ptr(v_colors), ptr(v_extra), ptr(tl.tiles_per_gauss), stream()),
          "mobgs_raster_bwd_reduce")
    return v_means2d, v_conics, v_opac, v_colors, v_extra


def _reduce_slots_decode(tl, records, slots, flag_source, C, N, channels, width, height, partial, c2w, w1, w2,
                         c2w_needs_grad, sunk):
    """Stage 2 after _raster_bwd_decode: the slot reduction + the decoder's weight / pose gradient sums over `partial`, which
    ride in the reduction's launch (mobgs_raster_bwd_reduce_decode) or, WGRAD_IN_REDUCE = False, take a launch of their own
    first (mobgs_raster_bwd_decode_finish, then the usual reduction).  sunk: LeafGradSink.decoder_buffers() or None.
    -> (*the five of _reduce_slots, g_c2w | None, g_w1, g_w2)."""
    F = _fast.get()
    if WGRAD_IN_REDUCE and F is not None:
        return F.raster_bwd_reduce_decode(
            C, N, width, height, records, tl.cum_tiles, tl.keep_scan, slots, tl.tiles_per_gauss,
            _slot_flag(tl, slots, flag_source, True), partial, c2w, w1, w2, bool(c2w_needs_grad),
            sunk[0] if sunk is not None else None, sunk[1] if sunk is not None else None,
            sunk[2] if sunk is not None else 0, stream_int())
    lib = _lib_()
    if sunk is not None:
        g_w1, g_w2, accumulate = sunk
    else:
        g_w1, g_w2, accumulate = torch.empty_like(w1), torch.empty_like(w2), 0
    g_c2w = torch.empty_like(c2w) if c2w_needs_grad else None
    cstr = (c2w.numel() // C) if (C > 1 and c2w.dim() == 3) else 0
    sums = (ptr(partial), cstr, ptr(g_w1), ptr(g_w2), ptr(g_c2w),
            (g_c2w.numel() // (C if cstr else 1)) if g_c2w is not None else 0, accumulate, stream())
    if not WGRAD_IN_REDUCE:
        check(lib.mobgs_raster_bwd_decode_finish(C, width, height, *sums), "mobgs_raster_bwd_decode_finish")
        return (*_reduce_slots(tl, records, slots, flag_source, C, N, channels, True), g_c2w, g_w1, g_w2)
    dev = records.device
    v_means2d = torch.empty(C, N, 2, dtype=torch.float32, device=dev)
    v_conics = torch.empty(C, N, 3, dtype=torch.float32, device=dev)
    v_opac = torch.empty(C, N, dtype=torch.float32, device=dev)
    v_colors = torch.empty(C, N, channels, dtype=torch.float32, device=dev)
    v_extra = torch.empty(C, N, dtype=torch.float32, device=dev)
    check(lib.mobgs_raster_bwd_reduce_decode(
        C, N, ptr(records), ptr(tl.cum_tiles), ptr(tl.keep_scan), ptr(slots), _slot_flag(tl, slots, flag_source, False),
        ptr(v_means2d), ptr(v_conics), ptr(v_opac), ptr(v_colors), ptr(v_extra), ptr(tl.tiles_per_gauss), width, height,
        *sums), "mobgs_raster_bwd_reduce_decode")
    return v_means2d, v_conics, v_opac, v_colors, v_extra, g_c2w, g_w1, g_w2


def _fold_cameras(v, per_camera, C):
    """A per-camera gradient [C,N,...] as its input takes it: as it is when every camera had its own rows, else summed over
    the cameras."""
    if per_camera:
        return v
    return v.sum(0) if C > 1 else v[0]


def _class_fwd(tl, records, bg, reach, C, N, Ns, cls, D, width, height, honour_defer):
    """One class-restricted forward pass (mobgs_raster_class_fwd) over the lists of the whole set: class `cls` = 1, the first
    Ns splats, or 2, the rest.  -> (render [C,H,W,D], alphas [C,H,W], last ids, reach)."""
    lib = _lib_()
    dev = records.device
    render = torch.empty(C, height, width, D, dtype=torch.float32, device=dev)
    alphas = torch.empty(C, height, width, dtype=torch.float32, device=dev)
    last = torch.empty(C, height, width, dtype=torch.int32, device=dev)

    def launch(reach):
        check(lib.mobgs_raster_class_fwd(C, N, Ns, cls, D, width, height, ptr(records), ptr(bg), ptr(tl.tile_offsets),
                                         ptr(tl.tile_order), ptr(tl.flatten_arena), ptr(render), ptr(alphas), ptr(last),
                                         ptr(reach), tuning.ref(), stream()), "mobgs_raster_class_fwd")
        return reach

    reach = _composite_until_resolved(tl, launch, honour_defer, reach)
    return render, alphas, last, reach


def _class_bwd(tl, records, bg, radii, alphas, last, v_render, v_alpha, slots, reach, flag_source, tn, C, N, Ns, cls, D,
               width, height):
    """Stage 1 of a class-restricted backward pass (mobgs_raster_class_bwd) into `slots`: the classes of one set own
    disjoint slots, so their passes may share one buffer and one reduction."""
    lib = _lib_()
    check(lib.mobgs_raster_class_bwd(C, N, Ns, cls, D, width, height, ptr(records), ptr(bg), ptr(radii), ptr(tl.cum_tiles),
                                     ptr(tl.keep_scan), ptr(tl.tile_offsets), ptr(tl.tile_order), ptr(tl.flatten_ids),
                                     ptr(alphas), ptr(last), ptr(v_render), ptr(v_alpha), ptr(slots), ptr(reach),
                                     _slot_flag(tl, slots, flag_source, False), tn.ref(), stream()),
          "mobgs_raster_class_bwd")


# True: render() lets the forward compositor decode its own image (SharedProjection.composite_decode); False: a separate
# decoder launch, as before round 5 (A/B; results are bit-identical)
FUSE_DECODER = os.environ.get("MOBGS_FUSE_DECODER", "1") != "0"
# True (round 6): the backward half too -- rgb / depth are outputs of the compositing node itself and the decoder's backward
# pass is the prologue of the backward compositor (mobgs_raster_bwd_decode); False: ops.Decode owns it (a launch of its
# own + a 55-MB cotangent image).  Splat gradients are bit-identical either way, weight / pose gradients to summation order.
FUSE_DECODER_BWD = os.environ.get("MOBGS_FUSE_DECODER_BWD", "1") != "0"
# True: the decoder's weight / pose gradient sums run as extra workgroups of the gradient-slot reduction (no launch of their
# own); False: mobgs_raster_bwd_decode_finish (A/B; same sums to summation order)
WGRAD_IN_REDUCE = os.environ.get("MOBGS_WGRAD_IN_REDUCE", "1") != "0"
# True: static-only / dynamic-only images (without the combined one) come from two class-restricted passes of the
# single-set compositor over the combined lists (every splat belongs to exactly one class, so together they do the
# work of ONE pass and share one gradient-slot buffer); False: from the generic 3-layer kernel
CLASS_PASSES = True


class _Rasterize(torch.autograd.Function):
    """rasterize_to_pixels: (means2d, conics, colors, opacities[, extra channel], backgrounds) -> image, alpha
    [, rgb, depth of the Sandwich decoder run as the compositor's epilogue]."""

    @staticmethod
    def forward(ctx, means2d, conics, colors, opacities, extra, backgrounds, radii, tl: TileLists, width, height,
                packed=None, dec=None, static_rows=0, dec_c2w=None, dec_w1=None, dec_w2=None):
        """dec = (intr, c2w, w1, w2) (detached, float32, contiguous): the Sandwich decoder runs as the kernel's epilogue
        (mobgs_raster_fwd_decode) and the node returns (render, alphas, rgb, depth) -- rgb / depth non-differentiable here:
        ops.Decode takes them as its precomputed outputs and owns their backward pass.
        dec_c2w / dec_w1 / dec_w2 (FUSE_DECODER_BWD): the caller's pose and weight TENSORS -- rgb / depth are then
        differentiable outputs of THIS node, whose backward pass runs the decoder's backward as the prologue of the backward
        compositor (_raster_bwd_decode: no decoder launch, no cotangent image in memory) whenever only rgb / depth (and
        alpha) carry cotangents and the ungated quadrant kernel is the selection; else as a launch of its own
        (_decoder_bwd_separately).
        static_rows = S > 0: the first S splats are the reference's STATIC set (include/mobgs_hip.h
        MobgsTuning.static_rows: colour channels 6.. structurally zero, their gradient multiplied by 0.0 downstream) --
        the backward compositor takes the short blend body for their entries and returns zeros for those channels."""
        lib = _lib_()
        C, N = radii.shape
        dev = means2d.device
        means2d, conics, colors, opacities = map(f32c, (means2d, conics, colors, opacities))
        extra = f32c(extra) if extra is not None else None
        channels = colors.shape[-1]
        D = channels + (1 if extra is not None else 0)
        colors_per_camera = 1 if colors.dim() == 3 else 0
        opac_per_camera = 1 if opacities.dim() == 2 else 0
        bg = f32c(backgrounds) if backgrounds is not None else None
        stride = lib.mobgs_record_stride(D)
        # `packed`: records of exactly these inputs written by the projection kernel (SharedProjection(pack_colors=)):
        # no pack launch (colors = NULL tells mobgs_raster_fwd so)
        if packed is not None and tuple(packed.shape) != (C * N, stride):
            packed = None
        _refuse_token(colors, packed, "_Rasterize")
        colors_arg = None if packed is not None else colors
        F = _fast.get()
        records, reach = packed, None
        rgb = dec_depth = None
        if dec is not None and not (D == 10 and extra is not None and tuning.block_walk != 0):
            raise NotImplementedError("decoder epilogue: 9 feature channels + depth through the block-walk kernel only")
        if F is not None:  # allocations + the launch in C++ (csrc/fastpath.cpp); buffers are reused on a redo
            d4 = dec if dec is not None else (None, None, None, None)

            def launch(reach):
                nonlocal records, render, alphas, last_ids, rgb, dec_depth
                records, render, alphas, last_ids, reach, rgb, dec_depth = F.raster_fwd(
                    C, N, channels, width, height, means2d, conics, colors_arg, colors_per_camera, opacities,
                    opac_per_camera, extra, bg, radii, tl.tile_offsets, tl.tile_order, tl.flatten_arena, records,
                    reach, tuning.address(), stream_int(), *d4)
                return reach
        else:
            if records is None:
                records = torch.empty(C * N, stride, dtype=torch.float32, device=dev)
            if dec is not None:
                rgb = torch.empty(C, 3, height, width, dtype=torch.float32, device=dev)
                dec_depth = torch.empty(C, height, width, dtype=torch.float32, device=dev)
            render = torch.empty(C, height, width, D, dtype=torch.float32, device=dev)
            alphas = torch.empty(C, height, width, dtype=torch.float32, device=dev)
            last_ids = torch.empty(C, height, width, dtype=torch.int32, device=dev)
            reach = _new_reach(tl, dev)

            def launch(reach):
                head = (C, N, channels, width, height, ptr(means2d), ptr(conics), ptr(colors_arg), colors_per_camera,
                        ptr(opacities), opac_per_camera, ptr(extra), ptr(bg), ptr(radii), ptr(tl.tile_offsets),
                        ptr(tl.tile_order), ptr(tl.flatten_arena), ptr(records), ptr(render), ptr(alphas),
                        ptr(last_ids), ptr(reach))
                if dec is not None:
                    intr, c2w, w1, w2 = dec
                    check(lib.mobgs_raster_fwd_decode(*head, ptr(intr), 4 if (C > 1 and intr.numel() == 4 * C) else 0,
                                                      ptr(c2w), (c2w.numel() // C) if (C > 1 and c2w.dim() == 3) else 0,
                                                      ptr(w1), ptr(w2), ptr(rgb), ptr(dec_depth), tuning.ref(),
                                                      stream()), "mobgs_raster_fwd_decode")
                else:
                    check(lib.mobgs_raster_fwd(*head, tuning.ref(), stream()), "mobgs_raster_fwd")
                return reach
        with profiler.region("raster_fwd"):
            reach = _composite_until_resolved(tl, launch, True, reach)
        _log_path("fwd", D, tl, decode=dec is not None)
        dec_fused = dec is not None and dec_w1 is not None
        if dec_fused:   # (+ the decoder's inputs: the composited image -- an output, saved the way outputs are -- and weights)
            ctx.save_for_backward(records, bg, radii, means2d, alphas, last_ids, reach, render, *dec)
        else:
            ctx.save_for_backward(records, bg, radii, means2d, alphas, last_ids, reach)
        ctx.set_materialize_grads(False)  # an output nothing back-propagates through costs no zero image
        ctx.tl = tl
        ctx.arena = tl.flatten_arena  # the lists `reach` belongs to (a rebuild replaces the arena)
        ctx.meta = (C, N, channels, extra is not None, width, height, colors_per_camera, opac_per_camera)
        ctx.bg_needs_grad = backgrounds is not None and backgrounds.requires_grad
        ctx.gate = _zero_gate[0]
        ctx.static_rows = int(static_rows) if D in (10, 12) else 0
        ctx.dec_fused = dec_fused
        if ctx.dec_fused:
            ctx.dec_w_inputs = (dec_w1, dec_w2)          # the caller's tensor objects (a LeafGradSink knows them by identity)
            ctx.dec_c2w_needs_grad = dec_c2w is not None and ctx.needs_input_grad[13]
            ctx.dec_c2w_shape = tuple(dec_c2w.shape) if dec_c2w is not None else None
            return render, alphas.unsqueeze(-1), rgb, dec_depth
        if dec is not None:
            ctx.mark_non_differentiable(rgb, dec_depth)
            return render, alphas.unsqueeze(-1), rgb, dec_depth
        return render, alphas.unsqueeze(-1)

    @staticmethod
    def _decoder_bwd_separately(ctx, alphas, v_rgb, v_depth):
        """decoder_bwd as a launch of its own (ops.decode_backward on this node's saved state) -> (v_feat [C,H,W,10],
        v_alphas [C,H,W,1], g_c2w | None, g_w1 | None, g_w2 | None)."""
        render, intr, c2w, w1, w2 = ctx.saved_tensors[7:12]
        C, H, W = alphas.shape
        lead = (C,) if C > 1 else ()
        feat = render.reshape(*lead, H, W, 10)
        c2w_d = c2w if (C > 1 or c2w.dim() == 2) else c2w.reshape(c2w.shape[-2:])
        if v_rgb is not None:
            v_rgb = v_rgb.reshape(*lead, 3, H, W)
        if v_depth is not None:
            v_depth = v_depth.reshape(*lead, H, W)
        g = ops.decode_backward((feat, alphas.reshape(*lead, H, W), None, intr.reshape(-1) if C == 1 else intr, c2w_d, w1, w2),
                                True, ctx.dec_w_inputs, feat.shape, False, ctx.dec_c2w_needs_grad, v_rgb, v_depth)
        g_c2w = g[4].reshape(ctx.dec_c2w_shape) if g[4] is not None else None
        return g[0].reshape(C, H, W, 10), g[1].reshape(C, H, W, 1), g_c2w, g[5], g[6]

    @staticmethod
    def backward(ctx, v_render, v_alphas, v_rgb=None, v_depth=None):
        records, bg, radii, means2d, alphas, last_ids, reach = ctx.saved_tensors[:7]
        tl = ctx.tl
        if tl.flatten_arena is not ctx.arena:  # lists rebuilt after this forward ran (deferred resolve): recompute
            reach = None
        C, N, channels, has_extra, width, height, colors_per_camera, opac_per_camera = ctx.meta
        D = channels + (1 if has_extra else 0)
        if not ctx.dec_fused:
            v_rgb = v_depth = None
        if v_render is None and v_alphas is None and v_rgb is None and v_depth is None:
            return (None,) * 16
        # plan: which kernel, with which tuning, and where the decoder's backward pass runs
        gated = bool(ctx.gate) and tuning.bwd_block_walk != 1
        nt = tl.C * tl.tile_w * tl.tile_h
        quadrant = tuning.bwd_block_walk != 1 and (_raster_path_bits(D, nt) & 3) == 0
        cover = COVER_SLOTS and quadrant and not gated   # the kernel writes every slot: no zero fill, no flag
        tn = _tuning_variant(gated, ctx.static_rows, cover)
        flag_source = "total" if cover else "row"
        decoder = v_rgb is not None or v_depth is not None
        fuse = decoder and v_render is None and not ctx.bg_needs_grad and not gated and quadrant
        g_c2w = g_w1 = g_w2 = None
        if decoder and not fuse:  # some other output carries a cotangent too (or another kernel is selected)
            v_feat, v_a_dec, g_c2w, g_w1, g_w2 = _Rasterize._decoder_bwd_separately(ctx, alphas, v_rgb, v_depth)
            v_render = v_feat if v_render is None else v_render + v_feat
            v_alphas = v_a_dec if v_alphas is None else v_alphas + v_a_dec
        if fuse:   # the decoder's backward pass inside the backward compositor
            render, intr, c2w, w1, w2 = ctx.saved_tensors[7:12]
            sunk = ops._active_sink.decoder_buffers(*ctx.dec_w_inputs) if ops._active_sink is not None else None
            _log_path("bwd", D, tl, tn=tn, static_rows=tn.static_rows, decode_bwd=True)
            slots, partial = _raster_bwd_decode(tl, records, bg, radii, render, alphas, last_ids, v_rgb, v_depth, v_alphas,
                                                (intr, c2w, w1, w2), reach, (C, N, width, height), tn, cover)
            v_means2d, v_conics, v_opac, v_colors, v_extra, g_c2w, g_w1, g_w2 = _reduce_slots_decode(
                tl, records, slots, flag_source, C, N, channels, width, height, partial, c2w, w1, w2,
                ctx.dec_c2w_needs_grad, sunk)
            if g_c2w is not None:
                g_c2w = g_c2w.reshape(ctx.dec_c2w_shape)
            if sunk is not None:
                g_w1 = g_w2 = None
        else:
            if v_render is None:  # only the alpha output was used
                v_render = torch.zeros(C, height, width, D, dtype=torch.float32, device=records.device)
            _log_path("bwd", D, tl, tn=tn, static_rows=tn.static_rows)
            slots = _raster_bwd(tl, records, bg, radii, means2d, alphas, last_ids, v_render, v_alphas, reach,
                                (C, N, channels, has_extra, width, height), tn, cover)
            v_means2d, v_conics, v_opac, v_colors, v_extra = _reduce_slots(tl, records, slots, flag_source, C, N, channels,
                                                                           has_extra)
            _zero_dead_channels(v_colors, tn.static_rows, D, _raster_path_bits(D, nt))
        v_bg = None
        if ctx.bg_needs_grad:
            v_bg = (v_render * (1.0 - alphas).unsqueeze(-1)).sum(dim=(1, 2))
        return (v_means2d, v_conics, _fold_cameras(v_colors, colors_per_camera, C), _fold_cameras(v_opac, opac_per_camera, C),
                v_extra, v_bg, None, None, None, None, None, None, None, g_c2w, g_w1, g_w2)


class _RasterizeClassAlpha(torch.autograd.Function):
    """Coverage (alpha = 1 - final transmittance) of ONE class of a projected set -- the first Ns splats (class_sel 1)
    or the rest (2) -- over the tile lists of the WHOLE set: what a rasterization of that subset alone with a ones
    colour returns as alpha, without projecting, binning and sorting the subset a second time
    (/root/reference/gaussian_renderer/__init__.py:477-490 does exactly that for the dynamic splats in get_flow()).
    A one-channel class pass (_class_fwd / _class_bwd); -> alphas [C,H,W]."""

    @staticmethod
    def forward(ctx, means2d, conics, opacities, radii, tl: TileLists, width, height, Ns, class_sel, background=None):
        C, N = radii.shape
        dev = means2d.device
        means2d, conics, opacities = map(f32c, (means2d, conics, opacities))
        records = _pack_records(C, N, 1, means2d, conics, _const(torch.ones, N, 1, dev=dev), opacities, None, radii)
        # background [C,1] (optional): the ones-colour render (1 - T) + T * bg -- what get_flow() calls latent_alpha,
        # /root/reference/gaussian_renderer/__init__.py:477-490 -- leaves the kernel directly (no rsub / mul / add glue)
        bg = f32c(background).reshape(C, 1) if background is not None else None
        render, alphas, last, reach = _class_fwd(tl, records, bg, _new_reach(tl, dev), C, N, Ns, class_sel, 1, width,
                                                 height, True)
        _log_path("fwd", 1, tl, class_filter=True, decode=False)
        ctx.save_for_backward(records, radii, alphas, last, reach, bg)
        ctx.tl, ctx.arena = tl, tl.flatten_arena
        ctx.gate = _zero_gate[0]
        ctx.meta = (C, N, width, height, opacities.dim() == 2, Ns, class_sel)
        return alphas if bg is None else render.squeeze(-1)

    @staticmethod
    def backward(ctx, v_alphas):
        C, N, width, height, opac_per_camera, Ns, class_sel = ctx.meta
        records, radii, alphas, last, reach, bg = ctx.saved_tensors
        tl = ctx.tl
        dev = records.device
        if v_alphas is None:
            return (None,) * 10
        if tl.flatten_arena is not ctx.arena:  # lists rebuilt after this forward ran: recompute the masks
            reach = None
        tn = _tuning_gated() if ctx.gate else tuning
        slots = _new_slots(tl, records.shape[1], dev)
        if bg is None:   # the cotangent belongs to the alpha output
            v_render, v_a = _const(torch.zeros, C, height, width, 1, dev=dev), f32c(v_alphas)
        else:            # ... to the 1-channel render output (background folded in by the kernel)
            v_render, v_a = f32c(v_alphas).reshape(C, height, width, 1), None
        _log_path("bwd", 1, tl, class_filter=True, tn=tn)
        _class_bwd(tl, records, bg, radii, alphas, last, v_render, v_a, slots, reach, "row", tn, C, N, Ns, class_sel, 1,
                   width, height)
        v_means2d, v_conics, v_opac, _, _ = _reduce_slots(tl, records, slots, "row", C, N, 1, False)
        return v_means2d, v_conics, _fold_cameras(v_opac, opac_per_camera, C), None, None, None, None, None, None, None


class _RasterizeLayers(torch.autograd.Function):
    """Layered compositing (csrc/raster_layers.hip): the combined, static-only and dynamic-only renders of one
    camera in a single walk over the combined tile lists.  Returns (render_all, alpha_all, render_static,
    alpha_static, render_dynamic, alpha_dynamic): render [C,H,W,10], alpha [C,H,W]; layers not in `mask` are
    empty tensors."""

    @staticmethod
    def forward(ctx, means2d, means2d_view, conics, colors, opacities, extra, backgrounds, radii, tl: TileLists,
                width, height, Ns, mask):
        # means2d_view is an autograd alias of means2d (same values): it receives the position gradient of the
        # combined layer alone, means2d that of the static / dynamic layers -- see rasterize_layers()
        lib = _lib_()
        C, N = radii.shape
        dev = means2d.device
        means2d, conics, colors, opacities, extra = map(f32c, (means2d, conics, colors, opacities, extra))
        channels = colors.shape[-1]
        D = channels + 1
        if D != 10:
            raise NotImplementedError("layered compositing is built for 9 feature channels + depth")
        _refuse_token(colors, None, "_RasterizeLayers")
        bg = f32c(backgrounds) if backgrounds is not None else None
        records = _pack_records(C, N, channels, means2d, conics, colors, opacities, extra, radii)
        renders, alphas, lasts = [], [], []
        for layer in range(3):
            on = (mask >> layer) & 1
            renders.append(torch.empty(C, height, width, D, dtype=torch.float32, device=dev) if on else None)
            alphas.append(torch.empty(C, height, width, dtype=torch.float32, device=dev) if on else None)
            lasts.append(torch.empty(C, height, width, dtype=torch.int32, device=dev) if on else None)

        def launch(_):   # (this kernel keeps no reach masks)
            check(lib.mobgs_raster_layers_fwd(C, N, Ns, mask, D, width, height, ptr(records), ptr(bg),
                                              ptr(tl.tile_offsets), ptr(tl.tile_order), ptr(tl.flatten_arena),
                                              _ptr3(renders), _ptr3(alphas), _ptr3(lasts), stream()),
                  "mobgs_raster_layers_fwd")

        with profiler.region("raster_layers_fwd"):
            _composite_until_resolved(tl, launch, False)
        ctx.save_for_backward(records, bg, radii, *[t for t in alphas + lasts if t is not None])
        ctx.tl = tl
        ctx.meta = (C, N, channels, width, height, colors.dim() == 3, opacities.dim() == 2, Ns, mask)
        empty = means2d.new_empty(0)
        out = []
        for layer in range(3):
            out += [renders[layer] if renders[layer] is not None else empty,
                    alphas[layer] if alphas[layer] is not None else empty]
        return tuple(out)

    @staticmethod
    def backward(ctx, *cots):
        lib = _lib_()
        C, N, channels, width, height, colors_per_camera, opac_per_camera, Ns, mask = ctx.meta
        records, bg, radii, *rest = ctx.saved_tensors
        tl = ctx.tl
        dev = records.device
        stride = records.shape[1]
        on = [(mask >> layer) & 1 for layer in range(3)]
        n_on = sum(on)
        it = iter(rest)
        alphas = [next(it) if o else None for o in on]
        lasts = [next(it) if o else None for o in on]
        v_render = [f32c(cots[2 * layer]) if (on[layer] and cots[2 * layer] is not None) else None
                    for layer in range(3)]
        v_alphas = [f32c(cots[2 * layer + 1]) if (on[layer] and cots[2 * layer + 1] is not None) else None
                    for layer in range(3)]
        assert n_on >= 1
        slots = torch.zeros(max(tl.n_isects, 1), 2, stride, dtype=torch.float32, device=dev)
        slots_xy0 = torch.zeros(max(tl.n_isects, 1), 2, 2, dtype=torch.float32, device=dev)
        v_means2d = torch.empty(C, N, 2, dtype=torch.float32, device=dev)
        v_means2d_l0 = torch.empty(C, N, 2, dtype=torch.float32, device=dev)
        v_conics = torch.empty(C, N, 3, dtype=torch.float32, device=dev)
        v_opac = torch.empty(C, N, dtype=torch.float32, device=dev)
        v_colors = torch.empty(C, N, channels, dtype=torch.float32, device=dev)
        v_extra = torch.empty(C, N, dtype=torch.float32, device=dev)
        with profiler.region("raster_layers_bwd"):
            check(lib.mobgs_raster_layers_bwd(C, N, Ns, mask, channels, 1, width, height, ptr(records), ptr(bg),
                                              ptr(radii), ptr(tl.cum_tiles), ptr(tl.keep_scan), ptr(tl.tile_offsets),
                                              ptr(tl.tile_order), ptr(tl.flatten_ids), _ptr3(alphas), _ptr3(lasts),
                                              _ptr3(v_render),
                                              _ptr3(v_alphas), ptr(slots), ptr(slots_xy0), ptr(v_means2d_l0),
                                              ptr(v_means2d), ptr(v_conics), ptr(v_opac), ptr(v_colors), ptr(v_extra),
                                              ptr(tl.tiles_per_gauss), stream()), "mobgs_raster_layers_bwd")
        return (v_means2d - v_means2d_l0, v_means2d_l0, v_conics, _fold_cameras(v_colors, colors_per_camera, C),
                _fold_cameras(v_opac, opac_per_camera, C), v_extra, None, None, None, None, None, None, None)


class _RasterizeClasses(torch.autograd.Function):
    """Static-only and/or dynamic-only "RGB+D" renders over the lists of the whole set: one 10-channel class pass each
    (_class_fwd / _class_bwd: csrc/raster.hip with a class filter).  Returns (render_static, alpha_static, render_dynamic,
    alpha_dynamic); classes not in `mask` (bit 1 = static, bit 2 = dynamic) are empty tensors."""

    @staticmethod
    def forward(ctx, means2d, conics, colors, opacities, extra, backgrounds, radii, tl: TileLists, width, height, Ns,
                mask, packed=None, static_rows=0):
        lib = _lib_()
        ctx.static_rows = int(static_rows)
        C, N = radii.shape
        dev = means2d.device
        means2d, conics, colors, opacities, extra = map(f32c, (means2d, conics, colors, opacities, extra))
        channels = colors.shape[-1]
        D = channels + 1
        if D != 10:
            raise NotImplementedError("class-restricted compositing is built for 9 feature channels + depth")
        bg = f32c(backgrounds) if backgrounds is not None else None
        if packed is not None and tuple(packed.shape) == (C * N, lib.mobgs_record_stride(D)):
            records = packed  # written by the projection kernel (SharedProjection(pack_colors=))
        else:
            _refuse_token(colors, None, "_RasterizeClasses")
            records = _pack_records(C, N, channels, means2d, conics, colors, opacities, extra, radii)
        outs = {}
        # one reach buffer: each forward pass writes the entries of its class, the backward passes read them back
        reach = _new_reach(tl, dev)
        with profiler.region("raster_class_fwd"):
            for cls in (1, 2):
                if not (mask >> cls) & 1:
                    continue
                *outs[cls], reach = _class_fwd(tl, records, bg, reach, C, N, Ns, cls, D, width, height, False)
                _log_path("fwd", D, tl, class_filter=True, decode=False)
        saved = [records, bg, radii]
        for cls in (1, 2):
            if cls in outs:
                saved += [outs[cls][1], outs[cls][2]]
        ctx.save_for_backward(*saved)
        ctx.tl = tl
        ctx.reach, ctx.arena = reach, tl.flatten_arena
        ctx.meta = (C, N, channels, width, height, colors.dim() == 3, opacities.dim() == 2, Ns, mask)
        empty = means2d.new_empty(0)
        res = []
        for cls in (1, 2):
            res += [outs[cls][0], outs[cls][1]] if cls in outs else [empty, empty]
        return tuple(res)

    @staticmethod
    def backward(ctx, *cots):
        C, N, channels, width, height, colors_per_camera, opac_per_camera, Ns, mask = ctx.meta
        records, bg, radii, *rest = ctx.saved_tensors
        tl = ctx.tl
        dev = records.device
        D = channels + 1
        slots = torch.zeros(max(tl.n_isects, 1), records.shape[1], dtype=torch.float32, device=dev)  # (no flag row)
        reach = ctx.reach if tl.flatten_arena is ctx.arena else None
        it = iter(rest)
        with profiler.region("raster_class_bwd"):
            for i, cls in enumerate((1, 2)):
                if not (mask >> cls) & 1:
                    continue
                alphas, last = next(it), next(it)
                v_render, v_alpha = cots[2 * i], cots[2 * i + 1]
                if v_render is None and v_alpha is None:
                    continue
                v_render = f32c(v_render) if v_render is not None else torch.zeros(C, height, width, D, device=dev)
                v_alpha = f32c(v_alpha) if v_alpha is not None else None
                # (the static class IS the reference's static set: its rows' dead channels take the short blend body)
                tn = _tuning_variant(False, ctx.static_rows if cls == 1 else 0)
                _log_path("bwd", D, tl, class_filter=True, tn=tn, static_rows=tn.static_rows)
                _class_bwd(tl, records, bg, radii, alphas, last, v_render, v_alpha, slots, reach, None, tn, C, N, Ns, cls, D,
                           width, height)
        # (any_record: the lists' total -- zero when an arena overflowed without a host in the loop: no slot is read then)
        v_means2d, v_conics, v_opac, v_colors, v_extra = _reduce_slots(tl, records, slots, "total", C, N, channels, True)
        if (mask >> 1) & 1:   # (only the static class pass touches the static rows' sums)
            _zero_dead_channels(v_colors, min(ctx.static_rows, Ns) if STATIC_ROWS else 0, D,
                                _raster_path_bits(D, tl.C * tl.tile_w * tl.tile_h, 1))
        return (v_means2d, v_conics, _fold_cameras(v_colors, colors_per_camera, C),
                _fold_cameras(v_opac, opac_per_camera, C), v_extra, None, None, None, None, None, None, None, None, None)


def _project_and_bin(means, quats, scales, viewmats, Ks, opacities, tl, width, height, eps2d, near_plane, far_plane,
                     radius_clip, want_isect_ids, pack_colors=None, order=None, prep=None):
    """Projection + tile lists of one call: fills `tl`, -> ((radii, means2d, depths, conics, tiles_per_gauss), the tensors
    the projection backward needs).  The host body of _ProjectAndBin and _PrepProjectAndBin.
    order (optional): int32 [C*N], a permutation of the flat splat ids -- the enumeration order of the bounding-box
    intersections (include/mobgs_hip.h, enum_order).  Only the single-pass path takes it; results do not depend on it.
    prep (internal, _PrepProjectAndBin): the 16 raw inputs of ops.PrepSplats -- the projection kernel builds the
    per-splat state itself; means / quats / scales / opacities are then uninitialised OUTPUT buffers."""
    means, quats, scales, viewmats, Ks, opac = map(f32c, (means, quats, scales, viewmats, Ks, opacities))
    F = _fast.get() if SPECULATIVE_BINNING else None
    if prep is not None and F is None:
        raise RuntimeError("fused prep needs the C++ host fast path and speculative binning")
    C = viewmats.shape[0]
    # means [C,N,3] / quats [C,N,4]: every camera has its own positions / rotations of the N splats (the K sub-frames
    # of a blurry view as ONE batch; MobgsTuning.geometry_per_camera).  Speculative path only.
    if means.dim() == 3:
        if not (quats.dim() == 3 and means.shape[0] == C and quats.shape[0] == C and SPECULATIVE_BINNING):
            raise ValueError("per-camera geometry: means [C,N,3] and quats [C,N,4] with C = number of cameras")
        call_tuning = tuning.copy(geometry_per_camera=1)
    else:
        call_tuning = tuning
    if isinstance(order, str):  # COHERENT: the splats are STORED in a spatially coherent order (no indirection)
        if order == COHERENT:
            call_tuning = call_tuning if call_tuning is not tuning else tuning.copy()
            call_tuning.coherent_order = 1
        order = None
    if call_tuning is not tuning:
        _tuning_keepalive.append(call_tuning)
        del _tuning_keepalive[:-8]
    args = (means, quats, scales, viewmats, Ks, opac, width, height, eps2d, near_plane, far_plane, radius_clip)
    if F is None and _static is not None:
        # what is left reads the frame's counts back on the host (an event wait or a poll of the pinned sequence
        # word) -- inside a StaticCapacity context (HIP-graph capture: no kernel runs) that would raise a capture
        # error or spin forever.  Say what is missing instead.
        raise RuntimeError("StaticCapacity needs the C++ host fast path and speculative binning: "
                           f"fast path {'loaded' if _fast.get() is not None else 'NOT loaded (MOBGS_FASTPATH=0 or the build failed)'}, "
                           f"SPECULATIVE_BINNING = {SPECULATIVE_BINNING}")
    if SPECULATIVE_BINNING:  # allocations + the orchestrator call in C++ (csrc/fastpath.cpp), or their twin in Python
        outs = _bin_speculative(F.project_and_bin_speculative if F is not None else _project_and_bin_speculative, tl, args,
                                want_isect_ids, pack_colors, order, prep, call_tuning)
    else:
        outs = _bin_synchronous(tl, args, want_isect_ids)
    radii, conics = outs[0], outs[3]
    return outs, (means, quats, scales, viewmats, Ks, radii, conics)


def _bin_speculative(callee, tl, args, want_isect_ids, pack_colors, order, prep, call_tuning):
    """The speculative binning call: capacities, hint and stride from the workload's record (or from the StaticCapacity
    context), a landing row for the counts, the call, and `tl` filled with buffers whose counts are still on their way
    (tl._pending; under StaticCapacity nobody waits: the capacities stand in).  callee: F.project_and_bin_speculative or
    its Python twin below."""
    global _stats_slots
    if _stats_slots is None:
        _stats_slots = _StatsSlots()
    means, opac, viewmats, width, height = args[0], args[5], args[3], args[6], args[7]
    C, N = viewmats.shape[0], means.shape[-2]
    tile_w, tile_h = math.ceil(width / TILE), math.ceil(height / TILE)
    tl.records = None
    pack = f32c(pack_colors) if pack_colors is not None else None
    key = _workload_key(means.device, C, N, width, height)
    hints = hint_record(key)
    if _static is not None:  # fixed capacities, no read-back (StaticCapacity)
        cap_box, cap_listed, len_hint = _static.caps(key, C, N)
        row, row_addr = _static.take_row()  # this call's own landing row (kept for the context's lifetime)
        slot, owner = None, _static.pool
    else:
        cap_box, cap_listed, len_hint = hints.caps(C, N)
        row, slot, row_addr, owner = _stats_slots.take()
    seq = _stats_slots.next_seq()
    row[3] = 0
    seg_stride = hints.stride(len_hint, C, N, C * tile_w * tile_h, cap_box)
    fused_calls[0] += 1 if seg_stride else 0
    if order is not None and (not seg_stride or order.numel() != C * N or order.dtype != torch.int32):
        order = None  # (the two-pass path enumerates in splat order)
    rc, outs, tile_order, isect_ids, tl.records = callee(
        *args, int(_tile_culling), bool(want_isect_ids), bool(TILE_SCHEDULE), pack, cap_box, cap_listed, len_hint, row_addr,
        seq, call_tuning.address(), stream_int(), seg_stride, order, prep if prep is not None else [])
    radii, means2d, depths, conics, tiles_per_gauss, cum_tiles, tile_offsets, keep_scan, flatten_ids = outs
    event = None
    if rc == 1 and _static is None:  # counts by asynchronous copy: wait on an event (0: poll the sequence word)
        event = torch.cuda.Event()
        event.record()
    tl._fill(C, N, tile_w, tile_h, cum_tiles, keep_scan, tile_offsets, tile_order, tiles_per_gauss, order)
    tl.flatten_arena = flatten_ids
    if _static is not None:
        _static.rows.append((row, owner, cap_box, cap_listed, key, seg_stride))
        tl._pending = None
        tl._set_counts(cap_box, cap_listed, len_hint, flatten_ids, isect_ids)
    else:
        tl._pending = _PendingCounts(row, slot, event, (key, cap_box, cap_listed, seg_stride), (flatten_ids, isect_ids),
                                     (means2d, radii, depths, conics, opac, tiles_per_gauss, width, height, want_isect_ids),
                                     seq, owner)
        hints.keep_caps(cap_box, cap_listed)
    return radii, means2d, depths, conics, tiles_per_gauss


def _alloc_outputs(lib, C, N, nt, dev, tile_schedule):
    """What a binning call allocates whatever its arenas: -> (radii, means2d, depths, conics, tiles_per_gauss, cum_tiles,
    tile_offsets, tile_order | None, stats_dev)."""
    i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
    return (torch.empty(C, N, **i32), torch.empty(C, N, 2, **f32), torch.empty(C, N, **f32), torch.empty(C, N, 3, **f32),
            torch.empty(C, N, **i32), torch.empty(C * N + 1, **i32), torch.empty(nt + 1, **i32),
            torch.empty(lib.mobgs_tile_order_len(nt), **i32) if tile_schedule else None,
            torch.empty(3, dtype=torch.int64, device=dev))


def _alloc_arenas(lib, C, N, nt, dev, cap_box, cap_listed, seg_stride, want_isect_ids):
    """... and its arenas: -> (keep_scan, scratch, flatten_ids, sort_keys, isect_ids | None)."""
    return (torch.empty(lib.mobgs_keep_scan_len(cap_box), dtype=torch.int32, device=dev),
            torch.empty(lib.mobgs_isect_scratch_bytes(C * N, nt, cap_box), dtype=torch.uint8, device=dev),
            torch.empty(cap_listed, dtype=torch.int32, device=dev),
            torch.empty(lib.mobgs_fused_seg_keys_len(nt, seg_stride) if seg_stride else cap_listed, dtype=torch.int64,
                        device=dev),
            torch.empty(cap_listed, dtype=torch.int64, device=dev) if want_isect_ids else None)


def _bin_head(args, tile_culling, outs, cap_box, cap_listed, arenas):
    """The 31 leading arguments mobgs_project_and_bin, _speculative and _fused share (C .. sort_keys)."""
    means, quats, scales, viewmats, Ks, opac, width, height, eps2d, near_plane, far_plane, radius_clip = args
    keep_scan, scratch, flatten_ids, sort_keys, _ = arenas
    return (viewmats.shape[0], means.shape[-2], ptr(means), ptr(quats), ptr(scales), ptr(viewmats), ptr(Ks), ptr(opac),
            1 if opac.dim() == 2 else 0, width, height, eps2d, near_plane, far_plane, radius_clip, tile_culling,
            *map(ptr, outs), cap_box, ptr(keep_scan), ptr(scratch), cap_listed, ptr(flatten_ids), ptr(sort_keys))


def _project_and_bin_speculative(means, quats, scales, viewmats, Ks, opac, width, height, eps2d, near_plane, far_plane,
                                 radius_clip, tile_culling, want_isect_ids, tile_schedule, pack, cap_box, cap_listed, len_hint,
                                 row_addr, seq, tuning_addr, stream_addr, seg_stride, order, prep):
    """F.project_and_bin_speculative (csrc/fastpath.cpp) with the allocations in Python and the call through ctypes: same
    arguments, same return tuple (rc, the nine outputs, tile_order, isect_ids, records)."""
    if prep:
        raise RuntimeError("fused prep needs the C++ host fast path and speculative binning")
    lib = _lib_()
    C, N, dev = viewmats.shape[0], means.shape[-2], means.device
    nt = C * math.ceil(width / TILE) * math.ceil(height / TILE)
    outs = _alloc_outputs(lib, C, N, nt, dev, tile_schedule)
    # optional: the projection kernel also writes the compositor's packed records (colours + depth channel)
    records = None
    if pack is not None and lib.mobgs_raster_channels_supported(pack.shape[-1] + 1):
        records = torch.empty(C * N, lib.mobgs_record_stride(pack.shape[-1] + 1), dtype=torch.float32, device=dev)
    arenas = _alloc_arenas(lib, C, N, nt, dev, cap_box, cap_listed, seg_stride, want_isect_ids)
    head = _bin_head((means, quats, scales, viewmats, Ks, opac, width, height, eps2d, near_plane, far_plane, radius_clip),
                     tile_culling, outs, cap_box, cap_listed, arenas)
    tail = (ptr(arenas[4]), len_hint, ctypes.c_void_p(row_addr), seq, ptr(pack) if records is not None else None,
            1 if (records is not None and pack.dim() == 3) else 0, pack.shape[-1] if records is not None else 0, ptr(records),
            ctypes.c_void_p(tuning_addr), ctypes.c_void_p(stream_addr))
    if seg_stride:  # single-pass lists (see FUSED_LISTS)
        rc = lib.mobgs_project_and_bin_fused(*head, seg_stride, ptr(order), *tail)
    else:
        rc = lib.mobgs_project_and_bin_speculative(*head, *tail)
    if rc not in (0, 1):
        check(rc, "mobgs_project_and_bin_speculative")
    return rc, (*outs[:7], arenas[0], arenas[2]), outs[7], arenas[4], records


def _bin_synchronous(tl, args, want_isect_ids):
    """mobgs_project_and_bin: one C call that reads the counts back itself (SPECULATIVE_BINNING off); on MOBGS_E_CAPACITY
    the arenas grow and the call is redone."""
    lib = _lib_()
    means, viewmats, width, height = args[0], args[3], args[6], args[7]
    C, N, dev = viewmats.shape[0], means.shape[-2], means.device
    tile_w, tile_h = math.ceil(width / TILE), math.ceil(height / TILE)
    nt = C * tile_w * tile_h
    outs = _alloc_outputs(lib, C, N, nt, dev, TILE_SCHEDULE)
    stats_host = (ctypes.c_int64 * 3)()
    tl.records = None
    key = _workload_key(dev, C, N, width, height)
    hints = hint_record(key)
    cap_box, cap_listed, _ = hints.caps(C, N)
    while True:
        arenas = _alloc_arenas(lib, C, N, nt, dev, cap_box, cap_listed, 0, want_isect_ids)
        rc = lib.mobgs_project_and_bin(*_bin_head(args, int(_tile_culling), outs, cap_box, cap_listed, arenas), ptr(arenas[4]),
                                       stats_host, _tuning_with_hint(key), stream())
        if rc != -4:  # MOBGS_E_CAPACITY: grow the arena (first call on a denser scene) and redo
            check(rc, "mobgs_project_and_bin")
            break
        cap_box = max(cap_box, int(stats_host[0] * 1.25) + 1024)
        cap_listed = max(cap_listed, int(stats_host[1] * 1.25) + 1024)
    hints.keep_caps(cap_box, cap_listed)
    n_box, n_isects, max_len = int(stats_host[0]), int(stats_host[1]), int(stats_host[2])
    tl._fill(C, N, tile_w, tile_h, outs[5], arenas[0], outs[6], outs[7], outs[4])
    tl._set_counts(n_box, n_isects, max_len, arenas[2], arenas[4])
    last_stats.update(n_isects=n_isects, n_box=n_box, max_tile_len=max_len, n_tiles=nt)
    return outs[:5]


class _ProjectAndBin(torch.autograd.Function):
    """Projection + tile lists through the native orchestrator mobgs_project_and_bin (one C call, one read-back).
    The TileLists object passed in `tl` is filled as a side effect; backward is the projection backward."""

    @staticmethod
    def forward(ctx, means, quats, scales, viewmats, Ks, opacities, tl, width, height, eps2d, near_plane, far_plane,
                radius_clip, want_isect_ids, pack_colors=None, order=None):
        outs, saved = _project_and_bin(means, quats, scales, viewmats, Ks, opacities, tl, width, height, eps2d, near_plane,
                                       far_plane, radius_clip, want_isect_ids, pack_colors, order)
        ctx.save_for_backward(*saved)
        ctx.dims = (width, height, eps2d)
        ctx.mark_non_differentiable(outs[0], outs[4])
        ctx.set_materialize_grads(False)  # no zero tensors for the outputs nothing back-propagates through
        return outs

    @staticmethod
    def backward(ctx, _v_radii, v_means2d, v_depths, v_conics, _v_tpg):
        return (*_project_bwd(ctx.saved_tensors, ctx.dims, v_means2d, v_depths, v_conics), None, None, None, None, None, None,
                None, None, None, None, None, None)


# _PrepProjectAndBin.backward as one launch (A/B: MOBGS_FUSE_PREP_BWD=0 runs the projection backward and the prep
# backward one after the other, as the separate nodes do)
FUSE_PREP_BWD = os.environ.get("MOBGS_FUSE_PREP_BWD", "1") != "0"


class _PrepProjectAndBin(torch.autograd.Function):
    """ops.PrepSplats + _ProjectAndBin as ONE node whose forward is one kernel fewer (round 5): the
    projection kernel evaluates the spline / activations of its splat itself (mobgs_prep_project_and_bin_fused; the
    arithmetic of prep_fwd_kernel, bit for bit), so the activated state is not written by one launch and read back by
    the next, and the 9 colour features go straight into the compositor's records.
    -> (means, quats, scales, opac, cols, radii, means2d, depths, conics, tiles_per_gauss).  `cols` [N,9] is a TOKEN: the
    tensor through which the compositing node hands its colour gradient back; its storage is never written (the
    features live in tl.records) -- SharedProjection.from_raw() does not expose it as data.
    Backward: the projection backward followed by the prep backward, exactly the two separate nodes' kernels."""

    @staticmethod
    def forward(ctx, times, s_xyz, s_scaling, s_rotation, s_opacity, s_fdc, s_ft, d_control, d_ncp, d_scaling,
                d_rotation, d_omega, d_opacity, d_fdc, d_ft, d_trbf, viewmats, Ks, tl, width, height, eps2d,
                near_plane, far_plane, radius_clip, order):
        leaf_inputs = (s_xyz, s_scaling, s_rotation, s_opacity, s_fdc, s_ft, d_control, d_scaling, d_rotation,
                       d_omega, d_opacity, d_fdc, d_ft)
        d_ncp_c = d_ncp if (d_ncp.dtype == torch.int64 and d_ncp.is_contiguous()) else d_ncp.to(torch.int64).contiguous()
        prep = [f32c(times), f32c(s_xyz), f32c(s_scaling), f32c(s_rotation), f32c(s_opacity), f32c(s_fdc), f32c(s_ft),
                f32c(d_control), d_ncp_c, f32c(d_scaling), f32c(d_rotation), f32c(d_omega), f32c(d_opacity), f32c(d_fdc),
                f32c(d_ft), f32c(d_trbf)]
        times_c, d_trbf_c = prep[0], prep[15]
        Ns, Nd = s_xyz.shape[0], d_control.shape[0]
        means, quats, scales, opac, cols = _fast.get().prep_state_buffers(Ns + Nd, s_xyz)
        (radii, means2d, depths, conics, tiles_per_gauss), saved = _project_and_bin(
            means, quats, scales, viewmats, Ks, opac, tl, width, height, eps2d, near_plane, far_plane, radius_clip, False,
            None, order, prep)
        ctx.save_for_backward(*saved, times_c, d_ncp_c, d_trbf_c, opac)
        ctx.dims = (width, height, eps2d)
        ctx.sizes = (Ns, Nd)
        ctx.leaf_inputs = leaf_inputs
        ctx.mark_non_differentiable(radii, tiles_per_gauss)
        ctx.set_materialize_grads(False)
        return means, quats, scales, opac, cols, radii, means2d, depths, conics, tiles_per_gauss

    @staticmethod
    def backward(ctx, v_means, v_quats, v_scales, v_opac, v_cols, _v_radii, v_means2d, v_depths, v_conics, _v_tpg):
        saved = ctx.saved_tensors
        means, quats, scales = saved[0], saved[1], saved[2]
        times, d_ncp, d_trbf, opac = saved[7:11]
        F = _fast.get()
        if FUSE_PREP_BWD and F is not None:
            # ONE launch: the state cotangents never leave the registers (mobgs_project_prep_bwd_fused)
            sink = ops._active_sink
            use_sink = sink is not None and sink.accepts(ctx.leaf_inputs)
            have = use_sink and sink.buffers is not None
            Ns, Nd = ctx.sizes
            width, height, eps2d = ctx.dims
            bufs, v_viewmats = F.project_prep_bwd(
                width, height, eps2d, means, quats, scales, saved[3], saved[4], saved[5], saved[6], v_means2d, v_depths,
                v_conics, v_means, v_quats, v_scales, Ns, Nd, times, d_ncp, d_trbf, opac, v_opac, v_cols,
                [sink.buffers[n_] for n_ in ops._LEAF_NAMES] if have else [], 1 if have else 0, stream_int(),
                bool(ctx.needs_input_grad[16]))
            g = sink.buffers if have else dict(zip(ops._LEAF_NAMES, bufs))
            if use_sink:
                sink.buffers = g
                return (None,) * 16 + (v_viewmats,) + (None,) * 9
            return (None, g["s_xyz"], g["s_scaling"], g["s_rotation"], g["s_opacity"], g["s_fdc"], g["s_ft"],
                    g["d_control"], None, g["d_scaling"], g["d_rotation"], g["d_omega"], g["d_opacity"], g["d_fdc"],
                    g["d_ft"], None, v_viewmats) + (None,) * 9
        pm = pq = ps = v_viewmats = None
        if v_means2d is not None or v_depths is not None or v_conics is not None:
            pm, pq, ps, v_viewmats = _project_bwd(saved[:7], ctx.dims, v_means2d, v_depths, v_conics)
        # cotangents that reach the state directly (a loss on out["d_means3d"], a scale regulariser, ...)
        pm = v_means if pm is None else (pm if v_means is None else pm + v_means)
        pq = v_quats if pq is None else (pq if v_quats is None else pq + v_quats)
        ps = v_scales if ps is None else (ps if v_scales is None else ps + v_scales)
        # (the state this node built is float32 whatever the leaves are: no half kernel, no cast back)
        g = ops.prep_backward((times, d_ncp, d_trbf, scales, opac), ctx.sizes, ctx.leaf_inputs, False, (), pm, pq, ps, v_opac,
                              v_cols)
        return (*g, v_viewmats, None, None, None, None, None, None, None, None, None)


_bg_ext_cache = DerivedCache()


# SharedProjection(order=COHERENT): "the rows of this set are already stored along a space-filling curve" -- the binning
# kernel then behaves as with an enumeration order, without one (MobgsTuning.coherent_order)
COHERENT = "coherent"


@torch.no_grad()
def spatial_order(means: Tensor, cameras: int = 1) -> Tensor:
    """int32 [cameras * N]: the splats along a Morton (Z-order) curve of their 3-D positions `means` [N,3] (10 bits per
    axis over the cloud's bounding box), camera after camera -- an enumeration order for SharedProjection(order=).  Splats
    that are neighbours in space are neighbours in the order, for any camera; a few dozen small torch launches and one
    sort (~0.5 ms at 300 k splats): callers recompute it every few hundred frames, not per frame."""
    m = means.detach().reshape(-1, 3).to(torch.float32)
    lo, hi = m.min(0).values, m.max(0).values
    q = ((m - lo) / (hi - lo).clamp_min(1e-20) * 1023.0).clamp_(0, 1023).to(torch.int64)

    def spread(v):  # 10 bits -> every third bit
        v = (v | (v << 16)) & 0x030000FF
        v = (v | (v << 8)) & 0x0300F00F
        v = (v | (v << 4)) & 0x030C30C3
        v = (v | (v << 2)) & 0x09249249
        return v
    code = spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2)
    order = torch.argsort(code).to(torch.int32)
    if cameras > 1:
        n = order.numel()
        order = (order[None, :] + n * torch.arange(cameras, device=order.device, dtype=torch.int32)[:, None]).reshape(-1)
    return order.contiguous()


class SharedProjection:
    """One projection + one tile binning/sort of a splat set, reusable by several compositing passes of the same
    camera (`composite` = the usual single-set pass, `composite_layers` = static-only / dynamic-only layers)."""

    def __init__(self, means, quats, scales, opacities, viewmats, Ks, width, height, near_plane=0.01, far_plane=1e10,
                 radius_clip=0.0, eps2d=0.3, want_isect_ids=False, pack_colors=None, order=None):
        """pack_colors: the colours composite() / composite_layers() will be called with, when already known: the
        projection kernel then writes the compositor's packed records itself (one launch and one pass over the
        projection outputs fewer); passing other colours later simply packs again.
        order: int32 [C*N] permutation of the flat splat ids in which the binning enumerates the splats (see spatial_order():
        a spatially coherent one makes the binning kernel ~2x faster; lists, images and gradients do not depend on it),
        or COHERENT: the rows themselves are stored in such an order (GaussianParams.spatial_sort_())."""
        self.width, self.height = int(width), int(height)
        self.C, self.N = viewmats.shape[0], means.shape[-2]
        self.opacities = opacities
        self.static_rows = 0   # set by render() & co: the first rows are the reference's static set (_Rasterize.forward)
        self.tl = TileLists()
        (self.radii, self.means2d, self.depths, self.conics, self.tiles_per_gauss) = _ProjectAndBin.apply(
            means, quats, scales, viewmats, Ks, opacities.detach(), self.tl, self.width, self.height, float(eps2d),
            float(near_plane), float(far_plane), float(radius_clip), bool(want_isect_ids),
            pack_colors.detach() if pack_colors is not None else None, order)
        self._packed_colors = pack_colors if self.tl.records is not None else None
        # autograd alias used by composite() and exposed as meta["means2d"] / viewspace_points: its .grad is the
        # position gradient of the whole-set render alone (the reference's static / dynamic passes have their own,
        # un-retained means2d tensors, gaussian_renderer/__init__.py:218-223)
        self.means2d_main = self.means2d.view_as(self.means2d)

    @classmethod
    def from_raw(cls, times, raw, viewmats, Ks, width, height, near_plane=0.01, far_plane=1e10, radius_clip=0.0,
                 eps2d=0.3, order=None):
        """The projection of ops.PrepSplats.apply(times, *raw)'s state without the prep launch: `raw` = the 15 tensors
        ops.PrepSplats takes behind `times` (float32 attributes, one time instant, one camera).  -> (sp, means, quats,
        scales, opac); sp.state_colors is the token composite() / composite_decode() must be called with (the colour
        features exist only inside the packed records).  See _PrepProjectAndBin."""
        self = cls.__new__(cls)
        self.width, self.height = int(width), int(height)
        self.static_rows = 0
        self.tl = TileLists()
        (means, quats, scales, opac, cols, self.radii, self.means2d, self.depths, self.conics,
         self.tiles_per_gauss) = _PrepProjectAndBin.apply(times, *raw, viewmats, Ks, self.tl, self.width, self.height,
                                                          float(eps2d), float(near_plane), float(far_plane),
                                                          float(radius_clip), order)
        self.C, self.N = 1, means.shape[0]
        self.opacities = opac
        # `cols` is a TOKEN (uninitialised storage; the features live in tl.records): make it say so, and make every
        # consumer that would read it as data refuse (_RasterizeLayers used to composite garbage silently)
        cols._mobgs_colour_token = True
        self.state_colors = cols
        self._packed_colors = cols if self.tl.records is not None else None
        if self._packed_colors is None:
            raise RuntimeError("fused prep: the projection kernel did not leave packed records")
        self.means2d_main = self.means2d.view_as(self.means2d)
        return self, means, quats, scales, opac

    def _bg(self, backgrounds):
        if backgrounds is None:
            return None
        return _bg_ext_cache.get((backgrounds,),
                                 lambda: torch.cat([backgrounds, backgrounds.new_zeros(self.C, 1)], dim=-1))

    def _packed_for(self, colors):
        return self.tl.records if (self._packed_colors is not None and colors is self._packed_colors) else None

    def composite(self, colors, backgrounds=None):
        """"RGB+D" compositing of the whole set: (render [C,H,W,D+1], alphas [C,H,W,1])."""
        return rasterize_to_pixels(self.means2d_main, self.conics, colors, self.opacities, self.radii, self.tl,
                                   self.width, self.height, backgrounds=self._bg(backgrounds), extra=self.depths,
                                   packed=self._packed_for(colors), static_rows=self.static_rows)

    def composite_decode(self, colors, backgrounds, rays, w1, w2):
        """composite() followed by ops.decode(img, alphas, rays, w1, w2, True) -- (img, alphas, rgb [3,H,W] | [C,3,H,W],
        depth) -- with the decoder as the EPILOGUE of the compositing kernel when it can be (round 5: 9 features + depth,
        block-walk kernel, pinhole rays given as (intr, c2w)): no decoder launch, no re-read of the feature image; the
        results are bit-identical and the backward pass is ops.Decode's either way."""
        from .ops import Decode, decode
        fused = (FUSE_DECODER and isinstance(rays, (tuple, list)) and colors.shape[-1] == 9 and tuning.block_walk != 0)
        if fused:
            intr, c2w = rays
            C = self.C
            if C == 1:
                intr, c2w = intr.reshape(4), (c2w.reshape(c2w.shape[-2:]) if c2w.dim() == 3 else c2w)
            ok = intr.numel() in (4, 4 * C) and c2w.shape[-2] in (3, 4) and c2w.shape[-1] == 4 and \
                (c2w.dim() == 2 or (c2w.dim() == 3 and c2w.shape[0] == C))
            fused = ok and not (C > 1 and c2w.dim() == 2 and c2w.requires_grad)  # (decode expands that case itself)
        if not fused:
            img, alphas = self.composite(colors, backgrounds)
            rgb, depth = decode(img, alphas, rays, w1, w2, True)
            return img, alphas, rgb, depth
        dec = (f32c(intr.detach()), f32c(c2w.detach()), f32c(w1.detach()), f32c(w2.detach()))
        if FUSE_DECODER_BWD:
            img, alphas, rgb, depth = _Rasterize.apply(self.means2d_main, self.conics, colors, self.opacities, self.depths,
                                                       self._bg(backgrounds), self.radii, self.tl, self.width,
                                                       self.height, self._packed_for(colors), dec, self.static_rows,
                                                       c2w, w1, w2)
            if C == 1:   # (views, not [0]: a select's backward is a zero image + a copy)
                rgb, depth = rgb.view(3, self.height, self.width), depth.view(self.height, self.width)
            return img, alphas, rgb, depth
        img, alphas, rgb0, depth0 = _Rasterize.apply(self.means2d_main, self.conics, colors, self.opacities, self.depths,
                                                     self._bg(backgrounds), self.radii, self.tl, self.width, self.height,
                                                     self._packed_for(colors), dec, self.static_rows)
        lead = (C,) if C > 1 else ()
        feat = img.reshape(*lead, self.height, self.width, 10)
        a2 = alphas.reshape(*lead, self.height, self.width)
        if C == 1:
            rgb0, depth0 = rgb0[0], depth0[0]
        rgb, depth = Decode.apply(feat, a2, None, intr, c2w, w1, w2, True, rgb0, depth0)
        return img, alphas, rgb, depth

    def composite_layers(self, colors, Ns, backgrounds=None, want_all=False, want_static=True, want_dynamic=True):
        """Layered "RGB+D" compositing over the SAME lists: lists (render, alphas) indexed by layer
        (0 = all, 1 = the first Ns splats, 2 = the rest); None for layers that were not requested."""
        mask = (1 if want_all else 0) | (2 if want_static else 0) | (4 if want_dynamic else 0)
        if mask == 0:
            return [None] * 3, [None] * 3
        if CLASS_PASSES and not want_all and colors.shape[-1] == 9:
            rs, a_s, rd, a_d = _RasterizeClasses.apply(self.means2d, self.conics, colors, self.opacities, self.depths,
                                                       self._bg(backgrounds), self.radii, self.tl, self.width,
                                                       self.height, int(Ns), mask, self._packed_for(colors),
                                                       min(int(Ns), self.static_rows))
            return ([None, rs if want_static else None, rd if want_dynamic else None],
                    [None, a_s if want_static else None, a_d if want_dynamic else None])
        m2d_view = self.means2d.view_as(self.means2d)
        outs = _RasterizeLayers.apply(self.means2d, m2d_view, self.conics, colors, self.opacities, self.depths,
                                      self._bg(backgrounds), self.radii, self.tl, self.width, self.height, int(Ns),
                                      mask)
        on = [(mask >> layer) & 1 for layer in range(3)]
        return ([outs[2 * layer] if on[layer] else None for layer in range(3)],
                [outs[2 * layer + 1] if on[layer] else None for layer in range(3)])

    def class_alpha(self, Ns, class_sel, background=None):
        """Coverage [C,H,W] of the first Ns splats (class_sel = 1) or of the rest (2) composited on their own, from
        the lists of the whole set (see _RasterizeClassAlpha).  background [C,1] / [1]: the ones-colour render over
        that background instead, (1 - T) + T * bg."""
        return _RasterizeClassAlpha.apply(self.means2d, self.conics, self.opacities, self.radii, self.tl, self.width,
                                          self.height, int(Ns), int(class_sel), background)

    def meta(self):
        tl = self.tl
        return {"radii": self.radii, "means2d": self.means2d_main, "depths": self.depths, "conics": self.conics,
                "tiles_per_gauss": self.tiles_per_gauss, "flatten_ids": tl.flatten_ids,
                "isect_offsets": tl.tile_offsets[:-1].reshape(self.C, tl.tile_h, tl.tile_w), "width": self.width,
                "height": self.height, "tile_size": TILE, "n_cameras": self.C}


def rasterize_layers(means, quats, scales, opacities, colors, viewmats, Ks, width, height, Ns, backgrounds=None,
                     want_static=True, want_dynamic=True, near_plane=0.01, far_plane=1e10, radius_clip=0.0,
                     eps2d=0.3):
    """One projection + one binning/sort + one layered compositing pass for the three splat sets of a train-mode
    render(): all, static (first Ns splats), dynamic (the rest); "RGB+D" semantics (9 features + accumulated depth).
    Returns (render, alphas, meta): lists indexed by layer (0 = all, 1 = static, 2 = dynamic; None when not
    requested) of [C,H,W,10] / [C,H,W] tensors.  meta["means2d"] receives the position gradient of the combined
    layer only (the reference's viewspace_points semantics)."""
    sp = SharedProjection(means, quats, scales, opacities, viewmats, Ks, width, height, near_plane, far_plane,
                          radius_clip, eps2d)
    mask = 1 | (2 if want_static else 0) | (4 if want_dynamic else 0)
    m2d_view = sp.means2d.view_as(sp.means2d)
    outs = _RasterizeLayers.apply(sp.means2d, m2d_view, sp.conics, colors, opacities, sp.depths, sp._bg(backgrounds),
                                  sp.radii, sp.tl, sp.width, sp.height, int(Ns), mask)
    render = [outs[0], outs[2] if want_static else None, outs[4] if want_dynamic else None]
    alphas = [outs[1], outs[3] if want_static else None, outs[5] if want_dynamic else None]
    meta = sp.meta()
    meta["means2d"] = m2d_view
    return render, alphas, meta


def rasterize_to_pixels(means2d, conics, colors, opacities, radii, tl: TileLists, width, height, backgrounds=None,
                        extra=None, packed=None, static_rows=0):
    """Composite; channel counts without a compiled variant are zero-padded up to the next one.
    packed: records of exactly these inputs already written by the projection kernel (see SharedProjection).
    static_rows: see _Rasterize.forward (only passes of exactly 10 / 12 total channels honour it)."""
    C = radii.shape[0]
    channels = colors.shape[-1]
    D = channels + (1 if extra is not None else 0)
    Dp = _pad_channels(D)
    if Dp == D:
        return _Rasterize.apply(means2d, conics, colors, opacities, extra, backgrounds, radii, tl, width, height,
                                packed if extra is not None else None, None, static_rows)
    parts = [colors if colors.dim() == 3 else colors.unsqueeze(0).expand(C, *colors.shape)]
    if extra is not None:
        parts.append(extra.unsqueeze(-1))
    parts.append(parts[0].new_zeros(*parts[0].shape[:-1], Dp - D))
    colors_p = torch.cat(parts, dim=-1)
    bg_p = None
    if backgrounds is not None:
        bg_p = torch.cat([backgrounds, backgrounds.new_zeros(C, Dp - D)], dim=-1)
    render, alphas = _Rasterize.apply(means2d, conics, colors_p, opacities, None, bg_p, radii, tl, width, height)
    return render[..., :D], alphas


# --------------------------------------------------------------------------------------------------
# rasterization()
# --------------------------------------------------------------------------------------------------
def rasterization(
    means: Tensor,
    quats: Tensor,
    scales: Tensor,
    opacities: Tensor,
    colors: Tensor,
    viewmats: Tensor,
    Ks: Tensor,
    width: int,
    height: int,
    near_plane: float = 0.01,
    far_plane: float = 1e10,
    radius_clip: float = 0.0,
    eps2d: float = 0.3,
    sh_degree: Optional[int] = None,
    packed: bool = True,
    tile_size: int = 16,
    backgrounds: Optional[Tensor] = None,
    render_mode: str = "RGB",
    sparse_grad: bool = False,
    absgrad: bool = False,
    rasterize_mode: str = "classic",
    channel_chunk: int = 32,
    distributed: bool = False,
    camera_model: str = "pinhole",
    covars: Optional[Tensor] = None,
) -> Tuple[Tensor, Tensor, Dict]:
    """gsplat.rendering.rasterization for the options MoBGS uses (packed=False, classic, pinhole,
    render_mode in RGB / D / ED / RGB+D / RGB+ED, tile_size 16).  Returns (colors [C,H,W,X], alphas [C,H,W,1], meta)."""
    if packed:
        raise NotImplementedError("mobgs_amd.rasterization: packed=True is not supported (MoBGS passes packed=False)")
    if sh_degree is not None or covars is not None or absgrad or sparse_grad or distributed:
        raise NotImplementedError("mobgs_amd.rasterization: sh_degree / covars / absgrad / sparse_grad / distributed")
    if rasterize_mode != "classic" or camera_model != "pinhole" or tile_size != TILE:
        raise NotImplementedError("mobgs_amd.rasterization: only classic / pinhole / tile_size=16")
    if render_mode not in ("RGB", "D", "ED", "RGB+D", "RGB+ED"):
        raise ValueError(f"unknown render_mode {render_mode}")
    width, height = int(width), int(height)
    C, N = viewmats.shape[0], means.shape[0]
    if backgrounds is not None and backgrounds.shape[0] != C:
        raise ValueError("backgrounds must be [C, D]")

    radii, means2d, depths, conics, tiles_per_gauss = _Project.apply(
        means, quats, scales, viewmats, Ks, width, height, float(eps2d), float(near_plane), float(far_plane),
        float(radius_clip))
    tl = build_tile_lists(means2d.detach(), radii, depths.detach(), conics.detach(), opacities.detach(),
                          tiles_per_gauss, width, height)

    extra = None
    bg = backgrounds
    if render_mode in ("RGB+D", "RGB+ED"):
        extra = depths
        if bg is not None:
            bg = torch.cat([bg, bg.new_zeros(C, 1)], dim=-1)
        cols = colors
    elif render_mode in ("D", "ED"):
        cols = depths.unsqueeze(-1)
        if bg is not None:
            bg = bg.new_zeros(C, 1)
    else:
        cols = colors
    render_colors, render_alphas = rasterize_to_pixels(means2d, conics, cols, opacities, radii, tl, width, height,
                                                       backgrounds=bg, extra=extra)
    if render_mode in ("ED", "RGB+ED"):
        render_colors = torch.cat(
            [render_colors[..., :-1], render_colors[..., -1:] / render_alphas.clamp(min=1e-10)], dim=-1)
    meta = {
        "camera_ids": None,
        "gaussian_ids": None,
        "radii": radii,
        "means2d": means2d,
        "depths": depths,
        "conics": conics,
        "opacities": opacities[None].expand(C, N) if opacities.dim() == 1 else opacities,
        "tile_width": tl.tile_w,
        "tile_height": tl.tile_h,
        "tiles_per_gauss": tiles_per_gauss,
        "isect_ids": tl.isect_ids,
        "flatten_ids": tl.flatten_ids,
        "isect_offsets": tl.tile_offsets[:-1].reshape(C, tl.tile_h, tl.tile_w),
        "width": width,
        "height": height,
        "tile_size": tile_size,
        "n_cameras": C,
    }
    return render_colors, render_alphas, meta
