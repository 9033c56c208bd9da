#!/usr/bin/env python
"""The deblur loop of examples/train_deblur_synth.py with checkpoints (mobgs_amd.checkpoint): stop it, continue it, get the
same bits.

    python examples/resume_deblur_synth.py --iters 60 --save-every 20 --path /tmp/run.mobgs [--graph]
    python examples/resume_deblur_synth.py --iters 60 --resume /tmp/run.mobgs [--graph]

The loop is train()'s with lr_schedule=True -- update_learning_rate(it) before the iteration, blcekernel.adjust_lr() after
it -- plus what a long run does between iterations: densification (densify_pruneclone on the gradient statistics) and the
opacity reset.  --graph: forward + backward + the Adam step replayed as ONE graph (GraphedCallable + DeviceAdam); after a
densification, an opacity reset or a load the tensors are new ones, so the flat gradient buffer is rebuilt over them, the
DeviceAdam plan is built again with first_iteration = the next iteration and the graph is recorded again.

A save is asynchronous: the snapshot launches are enqueued behind the iteration's optimiser step and the loop goes on while
the blocks travel and the file is written; the handle is waited for at the next save and at the end.  With
lambda_flow = 0 (the shipped configs) every kernel of the iteration is deterministic and a resumed run reproduces the
uninterrupted one bit for bit (tests/test_gpu_checkpoint.py).
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mobgs_amd.checkpoint import export_reference_layout, load_training_state, save_training_state  # noqa: E402
from mobgs_amd.distributed import FlatGradients  # noqa: E402
from mobgs_amd.graphed import GraphedCallable  # noqa: E402
from train_deblur_synth import DeblurTrainer  # noqa: E402


def rebind(t):
    """After densification, an opacity reset or a load the sets' Parameters are new objects and the row counts may have
    changed: the trainer's sizes and its flat gradient buffer over the Parameters as they are now."""
    t.ns, t.nd = t.stat._n, t.dyn._n
    params = [p for gr in t.stat.optimizer.param_groups + t.dyn.optimizer.param_groups for p in gr["params"]] \
        + list(t.blce.model.get_params())
    t.bucket = FlatGradients(params, extra={f"view{v}": 3 * (t.ns + t.nd) for v in range(t.n_views)})
    t.bucket.zero()   # (attaches the views as .grad: a DeviceAdam plan built next finds every tensor's gradient)


def adopt(t, state):
    """The loaded sets and blur kernel in place of the trainer's own (cameras and targets are functions of the seed)."""
    t.stat, t.dyn, t.blce = state.stat, state.dyn, state.blce
    rebind(t)


@torch.no_grad()
def densify(t, quantile=0.9, extent=5.0):
    """densify_pruneclone on both sets with the threshold at a quantile of the mean screen-space gradients, so that a
    tenth of the rows is cloned or split whatever the scene; the split samples come from the device generator."""
    for pc in (t.stat, t.dyn):
        g = (pc.xyz_gradient_accum / pc.denom).nan_to_num(0.0).reshape(-1)
        thr = max(float(torch.quantile(g, quantile)), 1e-12)   # (a host read: between two iterations)
        pc.densify_pruneclone(thr, 0.005, extent, None)
    rebind(t)


def warm_hints(t):
    """One eager forward + backward whose only lasting effect is on the renderer's arena hints: fresh sets (a load) have
    none, and a graph recorded without them would be recorded with arenas that may not fit.  The densification statistics
    the pass adds to are put back; the gradients are zeroed by the next pass anyway."""
    keep = [(x, x.clone()) for pc in (t.stat, t.dyn) for x in (pc.xyz_gradient_accum, pc.denom, pc.max_radii2D)]
    t.forward_backward()
    with torch.no_grad():
        for x, c in keep:
            x.copy_(c)


def run(dev="cuda:0", iters=40, *, ns=4000, nd=2000, width=256, height=192, n_views=2, seed=0, lambda_flow=0.0, graph=False,
        path=None, save_every=0, save_at=(), resume=None, stop_at=None, densify_at=(), reset_opacity_at=(),
        estimate_exposure_at=(), blocking=False, log=0, controller=False):
    """controller (True, or a mapping of option overrides: DeblurTrainer): the reference's densification on its schedule
    (helper_train.DensificationController) instead of densify_at; its flags, bounds and log travel in the checkpoint's
    counters.  After one of its operations a --graph run makes the next iteration eagerly and records the one after it.
    -> (loss history of the iterations run here, trainer, save handles, arenas_fit).  Runs iterations start + 1 .. stop_at
    (default iters) where start is the checkpoint's iteration (0 without --resume); `iters` is the run's planned length (the
    horizon of the schedules and of the blur kernel's rate) and must be what the interrupted run was given."""
    if controller:
        t = DeblurTrainer(dev, ns, nd, width, height, n_views, seed, lambda_flow, None, iters, False, True,
                          controller=controller)
    else:
        t = DeblurTrainer(dev, ns, nd, width, height, n_views, seed, lambda_flow, None, iters, False, True)
    start, fresh, record_at = 0, False, 0
    if resume:
        state = load_training_state(resume, device=dev, training_args=t.opt)
        adopt(t, state)
        start, fresh = state.iteration, True
        if t.controller is not None:
            t.controller.load_state_dict(state.counters["controller"], device=dev)
            record_at = int(state.counters.get("record_at", 0))
        if state.counters.get("blce_rate_pending"):   # saved under a DeviceAdam: the rate of iteration `start`, not yet
            t.blce.adjust_lr()                        # multiplied for the next one as the eager loop leaves it
    history, handles, adam, fb, arenas_fit = [], [], None, None, True
    for it in range(start + 1, (stop_at or iters) + 1):
        if graph and fb is None and it >= 2 and it >= record_at:   # (iteration 1 of a new run is eager: arenas and hints
            if fresh:                                              # exist afterwards; so is the one after the controller)
                warm_hints(t)
            adam = t.device_adam(first_iteration=it, horizon=iters)

            def forward_backward_step():
                loss = t.forward_backward()
                adam.step()
                return loss
            fb = GraphedCallable(forward_backward_step, warmup=0)
        fresh = False
        if it in estimate_exposure_at:   # (train.py:474-492; in place and on the device: a recorded iteration reads it)
            t.estimate_exposure()
        if adam is None:
            t.update_learning_rate(it)
        if fb is not None:
            photo = fb()
            adam.after_replay()
            history.append(float(photo))
            arenas_fit = arenas_fit and fb.check()
        else:
            history.append(float(t.iteration()))
            t.blce.adjust_lr()
        due = t.controller is not None and t.controller.due(it)
        surgery = it in densify_at or it in reset_opacity_at or due
        if surgery and adam is not None:   # back to the state the eager loop holds between iterations
            adam.sync_to_host()
            t.blce.adjust_lr()
            adam, fb = None, None
        if it in densify_at:
            densify(t)
        if it in reset_opacity_at:
            t.stat.reset_opacity()
            t.dyn.reset_opacity()
            rebind(t)
        if due:
            t.control(it)
            record_at = it + 2
        if path and ((save_every and it % save_every == 0) or it in save_at):
            handles.append(save_training_state(path, stat=t.stat, dyn=t.dyn, blce=t.blce, device_adam=adam, iteration=it,
                                               counters=dict({"blce_rate_pending": adam is not None,
                                                              "last_loss": history[-1]},
                                                             **({"controller": t.controller.state_dict(),
                                                                 "record_at": record_at} if t.controller is not None else {})),
                                               blocking=blocking))
        if log and (it % log == 0 or it == start + 1):
            print(f"it {it:4d}  photometric {history[-1]:.5f}  rows {t.stat._n} + {t.dyn._n}")
    if adam is not None:
        adam.sync_to_host()
    for h in handles:
        h.result()
    return history, t, handles, arenas_fit


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60, help="planned length of the run (also of a resumed one)")
    ap.add_argument("--ns", type=int, default=20000)
    ap.add_argument("--nd", type=int, default=10000)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=288)
    ap.add_argument("--graph", action="store_true", help="replay forward + backward + Adam as one HIP graph")
    ap.add_argument("--path", default=None, help="checkpoint file written by --save-every")
    ap.add_argument("--save-every", type=int, default=0, metavar="K")
    ap.add_argument("--resume", default=None, metavar="FILE", help="continue from this checkpoint")
    ap.add_argument("--stop-at", type=int, default=None, metavar="IT", help="stop after this iteration (an interrupted run)")
    ap.add_argument("--densify-every", type=int, default=0, metavar="K")
    ap.add_argument("--reset-opacity-every", type=int, default=0, metavar="K")
    ap.add_argument("--export", default=None, metavar="DIR",
                    help="at the end also write the reference's layout (point_cloud*.ply, point_cloud.pt, blce.pth) there")
    ap.add_argument("--lambda-flow", type=float, default=0.0)
    ap.add_argument("--controller", action="store_true",
                    help="the reference's densification schedule (helper_train.DensificationController); saved and resumed")
    a = ap.parse_args()
    every = lambda k: tuple(range(k, a.iters + 1, k)) if k else ()  # noqa: E731
    history, trainer, _, fit = run(iters=a.iters, ns=a.ns, nd=a.nd, width=a.width, height=a.height, graph=a.graph,
                                   path=a.path, save_every=a.save_every, resume=a.resume, lambda_flow=a.lambda_flow,
                                   stop_at=a.stop_at, controller=a.controller,
                                   densify_at=every(a.densify_every), reset_opacity_at=every(a.reset_opacity_every), log=10)
    if a.export:
        print("exported", export_reference_layout(a.export, stat=trainer.stat, dyn=trainer.dyn, blce=trainer.blce))
    if not history:
        print("nothing left to run: the checkpoint is at the last iteration")
    else:
        print(f"last photometric {history[-1]!r}" + ("" if fit else "  (an arena was outgrown during a replay)"))
