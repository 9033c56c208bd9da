"""A whole render() training step -- forward, loss cotangents, backward -- captured ONCE into a HIP graph and replayed.

The reference's own operating point is small: 512x288 images and ~30 k Gaussians at the start of training
(/root/reference/scene/dataset_readers.py:1448-1460, arguments/stereo/seesaw.py:13-14), ~81 rasterizations per blurry
view (train.py:441-584).  At that size a render() forward + backward is seventeen kernels of a few microseconds each and
the step is bound by launch overheads.  `GraphedRenderStep` removes the host from the loop:

    step = GraphedRenderStep(stat_pc, dyn_pc, width, height, K, bg)
    out = step(w2c, time, v_render, v_depth)    # copies the camera / cotangents into static buffers, replays the graph
    step.check()                                # after a synchronisation: did every arena fit?  (else: step.recapture())

What makes render() capturable (rendering.StaticCapacity): the intersection counts are not read back mid-forward;
count-sized buffers take their capacity, fixed from a warm-up frame times a margin; the kernels read true extents from
device memory as they always did.  Arena overflow cannot be repaired inside a graph: the kernels then see empty lists,
`check()` reports it from the pinned count rows and `recapture()` re-records with the larger sizes it has learnt.
Outputs and gradients are bit-identical to the eager step (tests/test_gpu_graphed.py).
Each replay OVERWRITES the leaves' .grad (static tensors owned by the graph) with the step's gradients: gradients
accumulated before capture() are discarded, and the step is NOT compatible with gradient storage that lives elsewhere --
distributed.FlatGradients (views of a flat buffer), LeafGradSink / fp32 masters -- capture() raises when it sees them.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import rendering as _R
from .camera import PinholeCamera
from .gaussian_renderer import render


class _StaticCamera(PinholeCamera):
    """A PinholeCamera whose pose and time live in ONE device buffer that is rewritten in place between replays (one
    184-byte device copy of a cached state per call).  Only what the in-kernel ray path of render() reads is kept
    current -- w2c, world_view_transform, ray_c2w, the times; camera_center / full_proj_transform / cam_ray keep the
    identity pose of construction, which is why GraphedRenderStep refuses to capture with INKERNEL_RAYS off."""

    def __init__(self, width, height, K, device):
        super().__init__(width, height, K, torch.eye(4), time=0.0, max_time=1, device=device)
        self.buf = torch.zeros(46, dtype=torch.float32, device=device)
        self._w2c = self.buf[0:16].view(4, 4)
        self.world_view_transform = self.buf[16:32].view(4, 4)   # the reference stores the transpose
        self.ray_c2w = self.buf[32:44].view(3, 4)
        self.static_times = self.buf[44:46]                       # [t, clamp(t, 0, 1)]
        self.set(torch.eye(4), 0.0)

    @torch.no_grad()
    def make_state(self, w2c: torch.Tensor, time: float) -> torch.Tensor:
        """The 46 floats of a pose + time, computed ONCE per training view with the same device arithmetic as
        PinholeCamera.__init__ (torch.inverse on the device: a replay is then bit-identical to an eager render() with a
        PinholeCamera of this pose).  Binding a cached state costs one 184-byte device copy per step."""
        dev = self.buf.device
        w = w2c.detach().to(dev, torch.float32)
        t = float(time)
        tt = torch.tensor([t, min(max(t, 0.0), 1.0)], dtype=torch.float32).to(dev)
        return torch.cat([w.reshape(-1), w.t().reshape(-1), torch.inverse(w)[:3, :].reshape(-1), tt])

    @torch.no_grad()
    def bind(self, state: torch.Tensor, time: float = None):
        self.buf.copy_(state)
        if time is not None:
            self.time = float(time)

    def set(self, w2c: torch.Tensor, time: float):
        self.bind(self.make_state(w2c, time), time)


class GraphedRenderStep:
    def __init__(self, stat_pc, dyn_pc, width: int, height: int, K: torch.Tensor, bg_color: torch.Tensor,
                 margin: float = 1.5, warmup: int = 3):
        self.stat, self.dyn = stat_pc, dyn_pc
        self.dev = dyn_pc.get_xyz.device
        self.W, self.H = int(width), int(height)
        self.cam = _StaticCamera(self.W, self.H, K, self.dev)
        self.bg = bg_color.to(self.dev)
        self.v_render = torch.zeros(3, self.H, self.W, device=self.dev)
        self.v_depth = torch.zeros(1, self.H, self.W, device=self.dev)
        self.margin, self.warmup = float(margin), int(warmup)
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.static: Optional[_R.StaticCapacity] = None
        self.out: Dict[str, torch.Tensor] = {}
        self.params = list(stat_pc.leaf_tensors(False).values()) + list(dyn_pc.leaf_tensors(True).values()) \
            + list(dyn_pc.rgbdecoder.parameters())

    # ---- eager body (also the warm-up that teaches the capacities) ---------------------------------------------
    def _body(self):
        out = render(self.cam, self.stat, self.dyn, None, self.bg)
        torch.autograd.backward([out["render"], out["depth"]], [self.v_render, self.v_depth])
        return out

    def zero_grad(self):
        for p in self.params:
            if p.grad is not None:
                p.grad.zero_()

    def capture(self, w2c: torch.Tensor, time: float):
        """Warm up eagerly at this camera (sizes the arenas), then record forward + backward into one graph."""
        from . import gaussian_renderer as _G
        if not getattr(_G, "INKERNEL_RAYS", True):
            raise RuntimeError("GraphedRenderStep needs the in-kernel rays (gaussian_renderer.INKERNEL_RAYS = True): the "
                               "static camera does not refresh cam_ray / camera_center")
        for p in self.params:
            # the recorded backward ASSIGNS graph-owned .grad tensors: gradients that live as views of a flat buffer
            # (distributed.FlatGradients) or are sunk into fp32 masters (LeafGradSink) would silently be detached
            if p.grad is not None and p.grad._base is not None:
                raise RuntimeError("GraphedRenderStep: a leaf's .grad is a view of a flat gradient buffer; the captured "
                                   "backward would replace it -- copy step.params' .grad into the buffer after replay "
                                   "instead, or capture before FlatGradients is built")
            if getattr(p, "master", None) is not None:
                raise RuntimeError("GraphedRenderStep does not support half-precision attributes with fp32 masters")
        self.cam.set(w2c, time)
        prev_mt = torch.autograd.is_multithreading_enabled()
        torch.autograd.set_multithreading_enabled(False)  # backward on the capturing thread / stream
        try:
            for p in self.params:
                p.grad = None
            for _ in range(self.warmup):
                self._body()
            torch.cuda.synchronize()
            for p in self.params:
                p.grad = None  # the capture allocates the .grad tensors from the graph's private pool
            self.static = _R.StaticCapacity(self.margin)
            self.graph = torch.cuda.CUDAGraph()
            with self.static, torch.cuda.graph(self.graph):
                out = self._body()
            self.out = {"render": out["render"], "depth": out["depth"], "radii": out["radii"]}
        finally:
            torch.autograd.set_multithreading_enabled(prev_mt)
        return self

    def __call__(self, w2c: Optional[torch.Tensor] = None, time: Optional[float] = None,
                 v_render: Optional[torch.Tensor] = None, v_depth: Optional[torch.Tensor] = None,
                 state: Optional[torch.Tensor] = None):
        """Replay at a new camera / time / cotangents (None: keep the previous ones; `state`: a camera_state() computed
        once per training view -- the cheap way to change the camera every step).  The leaves' .grad tensors are
        OVERWRITTEN with this step's gradients (the capture began with .grad = None, so the recorded backward assigns
        rather than accumulates).  -> {"render", "depth", "radii"}: static tensors, overwritten by the next call."""
        if self.graph is None:
            self.capture(w2c if w2c is not None else torch.eye(4), time or 0.0)
        if state is not None:      # a cached camera_state(): one small device copy
            self.cam.bind(state)
        elif w2c is not None or time is not None:
            self.cam.set(w2c if w2c is not None else self.cam._w2c.clone(), self.cam.time if time is None else time)
        if v_render is not None:
            self.v_render.copy_(v_render)
        if v_depth is not None:
            self.v_depth.copy_(v_depth)
        self.graph.replay()
        return self.out

    def camera_state(self, w2c: torch.Tensor, time: float) -> torch.Tensor:
        return self.cam.make_state(w2c, time)

    def check(self) -> bool:
        """After a synchronisation: True when every arena of the replayed frames fitted."""
        return self.static.check() if self.static is not None else True

    def recapture(self, w2c: torch.Tensor, time: float):
        self.graph, self.static = None, None
        return self.capture(w2c, time)


class GraphedCallable:
    """ANY host function over persistent device tensors -- e.g. the forward + loss + backward of a whole training iteration
    (render_many + get_flow_many + the loss kernels + backward into a distributed.FlatGradients buffer through ops.LeafGradSink)
    -- captured once into a HIP graph and replayed (round 6, VERDICT r5 item 7: the reference's own 512x288 operating point is
    bound by the host's ~1400 launches per iteration, not by the device).

        trainer.iteration()                              # an ordinary eager iteration first: arenas and hints exist
        fb = GraphedCallable(trainer.forward_backward, warmup=0)   # reads parameters / cameras / targets, writes the gradients
        loss = fb()                                      # first call: capture + one replay; then: one graph launch
        fused_adam_step(optimizers)                      # outside: ITS bias corrections are host scalars of the step count
        fb.check() / fb.recapture()                      # as GraphedRenderStep

    The Adam step CAN be recorded as well, through optim.DeviceAdam: its learning rates and bias corrections are tabulated on
    the host once and looked up on the device by counters that live there, so nothing of the step is a host scalar --

        adam = DeviceAdam(optimizers, schedules, horizon)
        fb = GraphedCallable(lambda: (trainer.forward_backward(), adam.step())[0], warmup=0)
        loss = fb(); adam.after_replay()                 # per iteration: one graph launch + the host side of the step

    (examples/train_deblur_synth.py --graph --graph-optimizer; recapture(): adam.rebuild() first when tensors were resized).

    Contract for `fn`: no arguments; everything it reads lives in tensors that are updated IN PLACE between calls (parameters
    by the optimiser, cameras / targets by .copy_); its gradient destination is persistent (FlatGradients / LeafGradSink or
    .grad tensors that exist before the capture and are accumulated into -- zero them inside fn); no host read-back (the
    zero-cotangent host gate of get_flow switches itself off inside a capture); host-side scalars it computes (an iteration
    counter, a learning-rate schedule) are FROZEN at their capture-time values.  What it returns is static storage,
    overwritten by the next call.  Densification changes the tensor shapes: recapture() after it."""

    def __init__(self, fn, warmup: int = 3, margin: float = 1.5):
        self.fn, self.warmup, self.margin = fn, int(warmup), float(margin)
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.static: Optional[_R.StaticCapacity] = None
        self.result = None

    def capture(self):
        prev_mt = torch.autograd.is_multithreading_enabled()
        torch.autograd.set_multithreading_enabled(False)  # backward on the capturing thread / stream
        try:
            for _ in range(self.warmup):
                self.fn()
            torch.cuda.synchronize()
            self.static = _R.StaticCapacity(self.margin)
            self.graph = torch.cuda.CUDAGraph()
            with self.static, torch.cuda.graph(self.graph):
                self.result = self.fn()
        finally:
            torch.autograd.set_multithreading_enabled(prev_mt)
        return self

    def __call__(self):
        """One execution of fn (a capture records, it does not execute: the call that captures replays once as well).  With
        warmup > 0 that first call ALSO ran fn eagerly `warmup` times -- harmless for a pure function of the parameters, not
        for one that accumulates (densification statistics): capture with warmup = 0 after an ordinary eager iteration then."""
        if self.graph is None:
            self.capture()
        self.graph.replay()
        return self.result

    def check(self) -> bool:
        """True when every arena of the replayed frames fitted.  After a synchronisation: of ALL replays so far; without one:
        of the replays that have COMPLETED (the counts land in pinned host rows) -- a training loop can call this every
        iteration for free; the host enqueues replays far faster than they run, so bound its run-ahead (an event per iteration,
        wait for the one two iterations back: examples/train_deblur_synth.py) and an outgrown arena is noticed that late.  A frame whose arena overflowed saw EMPTY
        tile lists: a background image, zero splat gradients, no out-of-bounds access (scripts/r06/overflow_probe.py) --
        recapture() records the function again with the sizes it has learnt."""
        return self.static.check() if self.static is not None else True

    def recapture(self):
        self.graph, self.static = None, None
        return self.capture()
