#!/usr/bin/env python
"""A miniature of the reference's DEBLUR training iteration (train.py:430-700) on a synthetic scene, end to end on the
MI355X path and, under torchrun, sharded over GPUs:

  per view of the batch   blcekernel.get_warped_cams -> K = 9 latent renders (mid frame in train mode) -> mean = blurry
                          prediction (mobgs_amd.deblur.render_blurry_batch: ONE all-reduce for the batch)
                          K get_flow() calls (mobgs_amd.deblur.get_flow_batch, sharded like the renders)
  loss                    photometric (L1 + 0.2 D-SSIM, fused) on the prediction, depth / mask terms on the mid render,
                          the flow-consistency term of train.py:651-671 on the get_flow outputs (both grid_sample
                          warps + both masked L1 terms: mobgs_amd.loss_utils.flow_warp_loss, one fused kernel each
                          way; sharded runs: a rank-local stand-in per flow unit), a regulariser on the scales
  backward                ops.LeafGradSink + distributed.FlatGradients, ONE in-place gradient all-reduce that also carries
                          the mid-frame densification statistics
  step                    Adam on both Gaussian sets, the decoder and the BLCE parameters; densification statistics
  --controller            the reference's densification (train.py:809-820): the batch statistics in ONE launch inside the
                          iteration -- from the mid renders, or from the gradient message when sharded -- and after the
                          step helper_train.DensificationController.step(): clone + split / opacity prune / opacity reset
                          on the reference's schedule, in every mode (eager, --graph, --graph-optimizer, torchrun)

    python examples/train_deblur_synth.py [--iters 60]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 examples/train_deblur_synth.py

The "ground truth" blurry views are K-frame averages of the same scene with perturbed colours seen through jittered
cameras, so the loss has somewhere to go.  Used by tests/test_gpu_train_loop.py as an integration test.
"""
import argparse
import os
import sys

import torch

torch.autograd.set_multithreading_enabled(False)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mobgs_amd.blce import blceKernel  # noqa: E402
from mobgs_amd.camera import PinholeCamera  # noqa: E402
from mobgs_amd.deblur import get_flow_batch, render_blurry_batch  # noqa: E402
from mobgs_amd.densify import TrainableGaussians  # noqa: E402
from mobgs_amd.distributed import FlatGradients, SubframeShard  # noqa: E402
from mobgs_amd.gaussian_renderer import render  # noqa: E402
from mobgs_amd.helper_model import Sandwich  # noqa: E402
from mobgs_amd.loss_utils import flow_warp_loss, l1_loss, photometric_loss  # noqa: E402
from mobgs_amd.ops import LeafGradSink  # noqa: E402
from mobgs_amd.optim import DeviceAdam, MultiplicativeLR, fused_adam_step  # noqa: E402
from mobgs_amd.synth import SynthCamera, dynamic_extras, gaussian_cloud  # noqa: E402
from train_synth import ControlOpt, Opt  # noqa: E402  (examples/ is on sys.path when run as a script or from the test)

K = 9


class ScheduledOpt(Opt):
    """Opt with the values the reference's xyz schedule is built from (arguments/__init__.py:121-123)."""
    position_lr_final = 0.0000016
    position_lr_max_steps = 20_000


def view_pose(i):
    w2c = torch.eye(4)
    w2c[:3, 3] = torch.tensor([0.04 * i, -0.02 * i, 0.03 * i])
    return w2c


class _Intrinsics:
    """The five numbers main_utils.get_normals reads from a dycheck camera (main_utils.py:95-141)."""

    def __init__(self, K):
        self.scale_factor_x, self.scale_factor_y = float(K[0, 0]), float(K[1, 1])
        self.principal_point_x, self.principal_point_y = float(K[0, 2]), float(K[1, 2])
        self.skew = float(K[0, 1])


def sets_from_views(dev, ns, nd, width, height, dec, seed=0, n_views=12, n_tracks=2000):
    """--from-views: both sets built the way train.py builds them from a data set -- synthetic training views (a slanted
    textured plane with its analytic depth, a disc of another colour that moves across it and carries the motion mask,
    2-D tracks that follow the plane and the disc) -> scene_init.scene_initialization -> from_pcd / from_pcd_dynamic.
    12 views: the spline fit wants at least as many trajectory samples as control points."""
    import math
    import types

    from mobgs_amd.scene_init import scene_initialization
    scam = SynthCamera().scaled(width, height)
    f, cx, cy = float(scam.focal), width / 2.0, height / 2.0
    D = torch.float64
    normal, offset = torch.tensor([0.15, -0.1, 1.0], dtype=D), 3.5          # the plane normal . X = offset
    vv, uu = torch.meshgrid(torch.arange(height, dtype=D), torch.arange(width, dtype=D), indexing="ij")
    rays = torch.stack([(uu - cx) / f, (vv - cy) / f, torch.ones_like(uu)], -1).reshape(-1, 3)
    half_w = offset * width / (2 * f)
    g = torch.Generator().manual_seed(seed + 300)
    track_xy = torch.stack([(2 * torch.rand(n_tracks, generator=g, dtype=D) - 1) * 1.2 * half_w,
                            (2 * torch.rand(n_tracks, generator=g, dtype=D) - 1) * 1.2 * half_w * height / width], 1)
    disc = lambda i: torch.tensor([-0.5 * half_w + 0.08 * half_w * i, 0.05], dtype=D)  # noqa: E731
    radius = 0.22 * half_w
    follows = ((track_xy - disc(0)) ** 2).sum(1) < radius ** 2
    views, tracks = [], []
    for i in range(n_views):
        a = (i - (n_views - 1) / 2) * 0.01
        R = torch.tensor([[math.cos(a), 0, -math.sin(a)], [0, 1, 0], [math.sin(a), 0, math.cos(a)]], dtype=D)
        eye = torch.tensor([0.04 * (i - (n_views - 1) / 2), 0.0, 0.0], dtype=D)
        world_rays = rays @ R                                               # R^T applied to every camera ray
        depth = (offset - normal @ eye) / (world_rays @ normal)
        X = eye + depth[:, None] * world_rays
        on_disc = ((X[:, :2] - disc(i)) ** 2).sum(1) < radius ** 2
        colour = torch.stack([0.5 + 0.3 * torch.sin(1.7 * X[:, 0] + 0.4), 0.5 + 0.3 * torch.sin(1.3 * X[:, 1] - 0.7),
                              0.5 + 0.3 * torch.cos(0.9 * X[:, 0] - 1.6 * X[:, 1])])
        colour[:, on_disc] = torch.tensor([0.95, 0.12, 0.10], dtype=D)[:, None]
        p = track_xy + torch.where(follows[:, None], disc(i) - disc(0), torch.zeros(2, dtype=D))
        P = torch.cat([p, ((offset - normal[0] * p[:, 0] - normal[1] * p[:, 1]) / normal[2])[:, None]], 1)
        cam = (P - eye) @ R.T
        tracks.append(torch.stack([f * cam[:, 0] / cam[:, 2] + cx, f * cam[:, 1] / cam[:, 2] + cy], 1))
        views.append(types.SimpleNamespace(
            original_image=colour.reshape(3, height, width).float().to(dev), depth=depth.reshape(1, height, width).float().to(dev),
            R=R.T.float().numpy(), T=(-R @ eye).float().numpy(), focal=f, time=i / (n_views - 1.0),
            metadata=types.SimpleNamespace(principal_point_x=cx, principal_point_y=cy),
            mask=on_disc.reshape(1, height, width).float().to(dev)))
    views[0].tracklet = torch.stack(tracks).float().to(dev)
    stat_pc, dyn_pc, trajectory = scene_initialization(views, ns, nd, generator=torch.Generator().manual_seed(seed + 301))
    return (TrainableGaussians.from_pcd(stat_pc, 5.0, decoder=dec, device=dev),
            TrainableGaussians.from_pcd_dynamic(dyn_pc, 5.0, 0, trajectory, decoder=dec, device=dev))


class DeblurTrainer:
    """State of the miniature training loop; `iteration()` is ONE iteration of train.py:430-807 on this stack:
    blurry views (K latent renders each, BLCE cameras) -> K get_flow() calls per view -> photometric + depth + mask +
    normal + flow + scale terms -> backward into the flat gradient buffer -> (all-reduce) -> densification statistics ->
    Adam on both Gaussian sets (incl. the decoder) and the BLCE parameters.  bench.py times it at full size."""

    def __init__(self, dev="cuda:0", ns=4000, nd=2000, width=256, height=192, n_views=2, seed=0, lambda_flow=1e-2,
                 shard=None, iters=40, from_views=False, lr_schedule=False, *, controller=None):
        """controller: None (no densification: the statistics are added once per view, as before), a
        helper_train.DensificationController, True (one with the reference's options, train_synth.ControlOpt) or a mapping of
        option overrides ("cameras_extent" among them)."""
        from mobgs_amd.main_utils import get_normals
        self.get_normals = get_normals
        self.shard = shard = shard or SubframeShard()
        self.ns, self.nd, self.n_views, self.lambda_flow = ns, nd, n_views, lambda_flow
        scam = SynthCamera().scaled(width, height)
        torch.manual_seed(seed)
        dec = Sandwich(9, 3).to(dev)
        sp, dp = gaussian_cloud(ns, scam, seed), gaussian_cloud(nd, scam, seed + 1)
        dx = dynamic_extras(dp["xyz"], seed)
        if from_views:   # opt-in: the two sets come from synthetic views through scene_initialization
            self.stat, self.dyn = sets_from_views(dev, ns, nd, width, height, dec, seed)
        else:
            self.stat = TrainableGaussians(sp, None, dec, device=dev)
            self.dyn = TrainableGaussians(dp, dx, dec, device=dev)
        stat, dyn = self.stat, self.dyn
        self.bg = bg = torch.zeros(9, device=dev)
        g = torch.Generator().manual_seed(seed + 100)
        self.cams = cams = []
        for i in range(n_views):
            c = PinholeCamera(width, height, scam.K, view_pose(i), time=(5.0 + 6 * i) / 23.0, max_time=23, device=dev)
            c.uid = i
            cams.append(c)
        self.meta = _Intrinsics(scam.K)
        # blurry targets: mean of K renders of a colour-shifted copy of the scene at spread-out exposure offsets
        with torch.no_grad():
            tsp = dict(sp, features_dc=sp["features_dc"] + 0.4 * torch.randn(sp["features_dc"].shape, generator=g))
            tdp = dict(dp, features_dc=dp["features_dc"] + 0.4 * torch.randn(dp["features_dc"].shape, generator=g))
            tstat, tdyn = TrainableGaussians(tsp, None, dec, device=dev), TrainableGaussians(tdp, dx, dec, device=dev)
            self.targets, self.depths, self.normals = [], [], []
            for c in cams:
                outs = [render(c, tstat, tdyn, None, bg, delta_exposure=float(d))
                        for d in torch.linspace(-0.6, 0.6, K)]
                self.targets.append(torch.stack([o["render"] for o in outs]).mean(0).clamp(0, 1))
                self.depths.append(outs[K // 2]["depth"].detach())
                self.normals.append(get_normals(self.depths[-1] + 1e-6, self.meta).detach())
                c.image = self.targets[-1]  # BLCE's blur statistic reads the (blurry) input image of the view
            del tstat, tdyn
        self.gt = torch.stack(self.targets)
        torch.manual_seed(seed + 1)
        self.blce = blceKernel(num_views=n_views, num_warp=K, iteration=max(iters, 1)).to(dev)
        self.opt = opt = ScheduledOpt() if lr_schedule else Opt()
        stat.training_setup(opt)
        dyn.training_setup(opt)
        self.lr_schedule = bool(lr_schedule)
        if lr_schedule:   # gaussian_model.py:646-661: the schedules update_learning_rate() evaluates
            stat.setup_schedules(opt)
            dyn.setup_schedules(opt)
        dyn.optimizer.param_groups = [gr for gr in dyn.optimizer.param_groups if gr["name"] != "decoder"]
        params = [p for gr in stat.optimizer.param_groups + dyn.optimizer.param_groups for p in gr["params"]] \
            + list(self.blce.model.get_params())
        self.bucket = FlatGradients(params, extra={f"view{v}": 3 * (ns + nd) for v in range(n_views)})
        # N > 1: one gradient message per view, exchanged while the next view back-propagates (backward_by_view)
        self.view_buckets = ([FlatGradients(params, extra={f"view{v}": 3 * (ns + nd)}) for v in range(n_views)]
                             if shard.collective else None)
        self.controller = self._make_controller(controller) if controller is not None and controller is not False else None

    CAMERAS_EXTENT = 5.0   # scene.cameras_extent of the synthetic scene (the spatial_lr_scale sets_from_views passes)

    def _make_controller(self, controller):
        from mobgs_amd.helper_train import DensificationController
        if isinstance(controller, DensificationController):
            return controller
        overrides = dict(controller) if isinstance(controller, dict) else {}
        extent = overrides.pop("cameras_extent", self.CAMERAS_EXTENT)
        for name in ("opacity_reset_interval", "densification_interval", "densify_from_iter", "densify_until_iter",
                     "desicnt", "densify_grad_threshold"):
            setattr(self.opt, name, getattr(ControlOpt, name))
        for name, value in overrides.items():
            setattr(self.opt, name, value)
        return DensificationController(self.opt, extent, self.stat, self.dyn)

    def parameters(self):
        """The tensors the flat gradient buffers are laid over, as they are now."""
        return [p for gr in self.stat.optimizer.param_groups + self.dyn.optimizer.param_groups for p in gr["params"]] \
            + list(self.blce.model.get_params())

    def rebind(self):
        """After a resize, an opacity reset or a load the sets' Parameters are new objects and the row counts may have
        changed: the trainer's sizes, the flat gradient buffers (the per-view ones of the sharded loop too) and the
        renderer's caches follow.  The dynamic set's optimiser stays without the shared decoder's group: a resize re-keys
        the groups it has and adds none."""
        from mobgs_amd import gaussian_renderer
        self.ns, self.nd = int(self.stat.get_xyz.shape[0]), int(self.dyn.get_xyz.shape[0])
        assert all(gr["name"] != "decoder" for gr in self.dyn.optimizer.param_groups)
        params, slot = self.parameters(), 3 * (self.ns + self.nd)
        self.bucket.rebind(params, extra={f"view{v}": slot for v in range(self.n_views)})
        for v, b in enumerate(self.view_buckets or []):
            b.rebind(params, extra={f"view{v}": slot})
        gaussian_renderer.parameters_changed()

    def control(self, iteration) -> bool:
        """After the optimiser step of `iteration`: the controller's schedule on both sets (train.py:819-820); -> whether
        a table was resized or had its opacity reset (the buffers are then laid anew: rebind())."""
        if self.controller is None or not self.controller.step(iteration, self.stat, self.dyn):
            return False
        self.rebind()
        return True

    def _batch_statistics(self, mids, buckets):
        """With a controller: the statistics of the iteration over the views of its batch in ONE launch (train.py:634-648 +
        :813-817: the norm of the gradient SUMMED over the views).  buckets: None -- from the mid renders' own gradients
        and int32 radii -- or the FlatGradients whose slot "view<v>" holds view v's statistics after the all-reduce."""
        from mobgs_amd.helper_train import batch_densification_stats, message_densification_stats
        W, H = self.cams[0].image_width, self.cams[0].image_height
        with torch.no_grad():
            if buckets is None:
                batch_densification_stats(self.stat, self.dyn, [mids[v] for v in range(self.n_views)], W, H,
                                          one_launch=True)
            else:
                message_densification_stats(self.stat, self.dyn,
                                            [buckets[v].extra(f"view{v}") for v in range(self.n_views)], W, H)

    def prune_viewpoints(self, n=8):
        """Cameras for TrainableGaussians.onedown_control_pts, with the attributes the reference's compute_prune_error
        reads (metadata.focal_length, image_width / image_height, time, world_view_transform): a short path of `n` poses
        over the whole time range (the first and the last are skipped by the error measure)."""
        import types
        c0 = self.cams[0]
        md = types.SimpleNamespace(focal_length=float(c0.K[0, 0]))
        return [types.SimpleNamespace(metadata=md, image_width=c0.image_width, image_height=c0.image_height,
                                      time=i / (n - 1.0), world_view_transform=view_pose(i).transpose(0, 1).contiguous())
                for i in range(n)]

    def report(self, report_dir, iteration, seconds):
        """train.py:776-790 for the training views: the report sheets of mobgs_amd.scene_utils.render_training_image
        (image, decomp, nine flow colours and nine latent frames per view) under <report_dir>/fine_render/train/images.
        Between two iterations and outside any capture.  -> the paths of the image sheets."""
        import types

        from mobgs_amd.scene_utils import render_training_image
        for v, c in enumerate(self.cams):   # what the reference reads from a training view
            c.image_name, c.original_image = f"view{v:02d}", self.targets[v]
            c.normal, c.depth = self.normals[v][0], self.depths[v]
            c.metadata = types.SimpleNamespace(focal_length=self.meta.scale_factor_x, skew=self.meta.skew,
                                               principal_point_x=self.meta.principal_point_x,
                                               principal_point_y=self.meta.principal_point_y)
        return render_training_image(types.SimpleNamespace(model_path=report_dir), self.stat, self.dyn, self.cams, render,
                                     None, self.bg, "fine", iteration, seconds, "synthetic", is_train=True,
                                     blcekernel=self.blce)

    def estimate_exposure(self):
        """train.py:474-492 for every view of the batch: exposure_time_expo[uid] from the static flow between the view's
        neighbours and the static flow over its own exposure, halved for the first and the last view (:490).  Device
        work only; -> the per-view stats tensors."""
        cams, last = self.cams, len(self.cams) - 1
        return [self.blce.estimate_exposure_time(c, cams[max(i - 1, 0)], cams[min(i + 1, last)], self.stat, self.dyn,
                                                 None, self.bg, edge=(c.uid == 0 or c.uid == last))
                for i, c in enumerate(cams)]

    def _iteration_sharded(self) -> torch.Tensor:
        """N > 1: the same iteration with its loss kept apart per view, so that the backward pass runs view by view and
        each view's gradient message (with its densification statistics) is all-reduced on the communication stream while
        the next view back-propagates (SubframeShard.backward_by_view)."""
        shard, stat, dyn, blce, ns, V = self.shard, self.stat, self.dyn, self.blce, self.ns, self.n_views
        preds, mids = render_blurry_batch(self.cams, stat, dyn, self.bg, shard, blce=blce, n_sub=K, rank_local_terms=True,
                                          weighted=True, with_flows=True, overlap=True, as_list=True)
        flows = get_flow_batch(self.cams, stat, dyn, self.bg, shard, n_sub=K, weighted=True)
        photos = [photometric_loss(preds[v][None], self.gt[v][None], self.opt.lambda_dssim) for v in range(V)]

        def view_backward(v):
            loss = shard.replicated_term(photos[v]) / V          # the mean over V equal-sized images, view by view
            if v in mids:
                pkg = mids[v]
                for key in ("s_render", "s_depth", "d_alpha", "d_depth", "s_alpha"):
                    pkg[key]
                normal = self.get_normals(pkg["depth"] + 1e-6, self.meta)
                loss = loss + 0.05 * l1_loss(pkg["depth"], self.depths[v]) + 0.01 * pkg["d_alpha"].mean() \
                    + 0.01 * l1_loss(normal, self.normals[v])
            if self.lambda_flow != 0:
                for (vv, k), (e2m, m2e, limg, lalpha) in flows.items():
                    if vv == v:
                        loss = loss + self.lambda_flow / K * (l1_loss(limg, preds[v]) + 1e-3 * (e2m - m2e).abs().mean()
                                                              + 0.1 * lalpha.mean())
            if v == 0:
                loss = loss + shard.replicated_term(1e-4 * ((stat._scaling ** 2).mean() + (dyn._scaling ** 2).mean()))
            if loss.requires_grad:
                with LeafGradSink(stat, dyn, extra=blce.model.get_params()):
                    loss.backward()

        def after_view(v):
            if v in mids:
                shard.put_densification_stats(self.view_buckets[v], f"view{v}", mids[v]["viewspace_points"].grad,
                                              mids[v]["radii"])

        shard.backward_by_view(self.view_buckets, view_backward, after_view)
        if self.controller is not None:
            self._batch_statistics(mids, self.view_buckets)
        else:
            with torch.no_grad():
                for v in range(V):
                    grad2d, radii = shard.get_densification_stats(self.view_buckets[v], f"view{v}")
                    vis = radii > 0
                    stat.add_densification_stats(grad2d[:ns], vis[:ns], radii=radii[:ns])
                    dyn.add_densification_stats(grad2d[ns:], vis[ns:], radii=radii[ns:])
        fused_adam_step([stat.optimizer, dyn.optimizer, blce.optimizer])
        return torch.stack([p.detach() for p in photos]).mean()

    def iteration(self) -> torch.Tensor:
        if self.shard.collective:   # N > 1 (or a forced one-rank group: the same code path on one GPU)
            return self._iteration_sharded()
        photo = self.forward_backward()
        self.optimizer_step()
        return photo

    def update_learning_rate(self, iteration):
        """train.py:312-313, before the iteration's renders (lr_schedule=True only)."""
        self.dyn.update_learning_rate(iteration)
        self.stat.update_learning_rate(iteration)

    def device_adam(self, first_iteration, horizon):
        """The three optimisers as ONE mobgs_amd.optim.DeviceAdam plan whose steps run the rates of iterations
        first_iteration, first_iteration + 1, ...: the Gaussian sets' schedules as update_learning_rate() applies them, the
        blur kernel's rate as blcekernel.adjust_lr() leaves it after each step (train.py:807), starting from its present
        value.  Gradients are the views of self.bucket, which stay where they are."""
        schedules = list(self.stat.schedules().items()) + list(self.dyn.schedules().items()) \
            + [(g, MultiplicativeLR(g["lr"], self.blce.lr_factor, first_iteration)) for g in self.blce.optimizer.param_groups]
        return DeviceAdam([self.stat.optimizer, self.dyn.optimizer, self.blce.optimizer], schedules, horizon=horizon,
                          first_iteration=first_iteration)

    def optimizer_step(self):
        # train.py:790-807 steps the three optimisers one after the other (~26 one-tensor groups x 8 launches); here
        # ONE launch performs the same Adam update on all of them (mobgs_amd.optim)
        fused_adam_step([self.stat.optimizer, self.dyn.optimizer, self.blce.optimizer])

    def forward_backward(self) -> torch.Tensor:
        """Everything of the single-process iteration but the optimiser step: renders, flows, loss, backward into the flat
        gradient buffer, densification statistics -- device work over persistent tensors only, i.e. what
        mobgs_amd.graphed.GraphedCallable can record once and replay (scripts/bench_small_scene_iteration.py --graph)."""
        shard, stat, dyn, blce, bucket, ns = self.shard, self.stat, self.dyn, self.blce, self.bucket, self.ns
        bucket.zero()
        multi = shard.world > 1  # units of both families dealt by cost, per-view asynchronous image exchange
        pred, mids = render_blurry_batch(self.cams, stat, dyn, self.bg, shard, blce=blce, n_sub=K,
                                         rank_local_terms=True, weighted=multi, with_flows=True, overlap=multi)
        flows = get_flow_batch(self.cams, stat, dyn, self.bg, shard, n_sub=K, weighted=multi)
        photo = photometric_loss(pred, self.gt, self.opt.lambda_dssim)
        loss = shard.replicated_term(photo)                      # every rank forms it on the replicated prediction
        for v, pkg in mids.items():                              # the rank that rendered the mid frame
            for key in ("s_render", "s_depth", "d_alpha", "d_depth", "s_alpha"):
                pkg[key]   # train.py:445-464 reads these five auxiliary images of the mid render every iteration
            normal = self.get_normals(pkg["depth"] + 1e-6, self.meta)   # train.py:590
            loss = loss + 0.05 * l1_loss(pkg["depth"], self.depths[v]) + 0.01 * pkg["d_alpha"].mean() \
                + 0.01 * l1_loss(normal, self.normals[v])
        if not multi and self.lambda_flow != 0:
            # train.py:608-617 + :651-671: the flow-consistency term on the tensors the reference concatenates --
            # both grid_sample warps and both masked L1 terms in one forward and one backward kernel
            views = range(self.n_views)
            cat = lambda i: torch.stack([torch.cat([flows[(v, k)][i] for k in range(K)]) for v in views])  # noqa: E731
            loss = loss + flow_warp_loss(torch.stack([mids[v]["render"] for v in views]),
                                         torch.stack([torch.stack([flows[(v, k)][2] for k in range(K)]) for v in views]),
                                         cat(0), cat(1), cat(3).unsqueeze(2),
                                         torch.stack([mids[v]["d_alpha"].reshape(1, *pred.shape[-2:]) for v in views]),
                                         self.lambda_flow)
        elif self.lambda_flow != 0:   # (weight 0, the shipped seesaw / children configs: the calls above are made, as
            # train.py makes them, and their results stay out of the loss graph -- flow_warp_loss returns a constant)
            # flow units sharded over ranks: each owner forms a rank-local stand-in (the reference's term normalises
            # over all (view, exposure) pairs and samples the view's mid render, which lives on one rank)
            for (v, k), (e2m, m2e, limg, lalpha) in flows.items():
                loss = loss + self.lambda_flow / K * (l1_loss(limg, pred[v]) + 1e-3 * (e2m - m2e).abs().mean()
                                                      + 0.1 * lalpha.mean())
        loss = loss + shard.replicated_term(1e-4 * ((stat._scaling ** 2).mean() + (dyn._scaling ** 2).mean()))
        with LeafGradSink(stat, dyn, extra=blce.model.get_params()):
            loss.backward()
        if self.controller is not None and not shard.collective:   # single process: straight from the mid renders
            shard.all_reduce_gradients(bucket)
            self._batch_statistics(mids, None)
            return photo.detach()
        for v, pkg in mids.items():
            shard.put_densification_stats(bucket, f"view{v}", pkg["viewspace_points"].grad, pkg["radii"])
        shard.all_reduce_gradients(bucket)
        if self.controller is not None:                            # sharded: from the message, where the sum left them
            self._batch_statistics(mids, [bucket] * self.n_views)
            return photo.detach()
        with torch.no_grad():
            for v in range(self.n_views):
                grad2d, radii = shard.get_densification_stats(bucket, f"view{v}")
                vis = radii > 0
                stat.add_densification_stats(grad2d[:ns], vis[:ns], radii=radii[:ns])
                dyn.add_densification_stats(grad2d[ns:], vis[ns:], radii=radii[ns:])
        return photo.detach()


    def iteration_unchanged(self) -> torch.Tensor:
        """The SAME iteration written the way /root/reference/train.py:430-807 writes it -- what runs after nothing but
        the import swap of INTEGRATION.md section 1: one render() per latent sub-frame, every one of them with
        get_static = get_dynamic = True (train.py:441 and :512), one get_flow() per exposure (:570-579), l1_loss + ssim
        as two calls (:621-628), the flow-consistency term as torch statements (two F.grid_sample + two masked l1_loss,
        :651-671), loss.backward() into ordinary .grad tensors, viewspace_points.grad for the densification statistics
        (:634-648) and the three optimizer.step() calls (:790-807; the optimisers are optim.FusedAdam, the torch.optim.Adam
        subclass TrainableGaussians.training_setup / blceKernel build: one launch per step() instead of ~8 per parameter group).  None of the opt-in entry points (render_many,
        get_flow_many, flow_warp_loss, fused_adam_step, LeafGradSink, FlatGradients).  Single process."""
        import torch.nn.functional as F
        from mobgs_amd.gaussian_renderer import get_flow
        from mobgs_amd.loss_utils import ssim
        stat, dyn, blce, ns, bg = self.stat, self.dyn, self.blce, self.ns, self.bg
        opts = [stat.optimizer, dyn.optimizer, blce.optimizer]
        for o in opts:
            o.zero_grad(set_to_none=True)
        images, ori, d_alphas, depths, normals, vsp, radii = [], [], [], [], [], [], []
        lat_img, lat_alpha, e2m_all, m2e_all = [], [], [], []
        for cam in self.cams:
            pkg = render(cam, stat, dyn, None, bg, get_static=True, get_dynamic=True)                      # train.py:441
            for key in ("s_render", "s_depth", "d_alpha", "d_depth", "s_alpha"):
                pkg[key]                                                                                    # :445-464
            image_ori = pkg["render"]
            warped_cams, exposure_time = blce.get_warped_cams(cam, None, None)                             # :472
            half = len(warped_cams) // 2
            rendered = []
            for k, wc in enumerate(warped_cams):                                                           # :502-518
                if k == half:
                    rendered.append(image_ori)
                else:
                    rendered.append(render(wc, stat, dyn, None, bg, get_static=True, get_dynamic=True,
                                           delta_exposure=exposure_time[k])["render"])
            images.append(torch.mean(torch.stack(rendered, dim=0), dim=0) + 1e-10)                         # :540-541
            cur = [[], [], [], []]
            for k in range(len(warped_cams)):                                                              # :570-579
                outs = get_flow(cam, stat, dyn, None, bg, delta_exposure=1.0 * (k - half) / half)
                for lst, o in zip(cur, outs):
                    lst.append(o)
            e2m_all.append(torch.cat(cur[0], 0).unsqueeze(0))
            m2e_all.append(torch.cat(cur[1], 0).unsqueeze(0))
            lat_img.append(torch.cat([t.unsqueeze(0) for t in cur[2]], 0).unsqueeze(0))
            lat_alpha.append(torch.cat([t.unsqueeze(0) for t in cur[3]], 0).unsqueeze(0))
            ori.append(image_ori.unsqueeze(0))
            d_alphas.append(pkg["d_alpha"].unsqueeze(0))
            depths.append(pkg["depth"])
            normals.append(self.get_normals(pkg["depth"] + 1e-6, self.meta))                               # :590
            vsp.append(pkg["viewspace_points"])
            radii.append(pkg["radii"])
        pred = torch.stack(images)
        Ll1 = l1_loss(pred, self.gt)                                                                       # :621-628
        photo = (1.0 - self.opt.lambda_dssim) * Ll1 + self.opt.lambda_dssim * (1.0 - ssim(pred, self.gt))
        loss = photo
        for v in range(self.n_views):
            loss = loss + 0.05 * l1_loss(depths[v], self.depths[v]) + 0.01 * d_alphas[v].mean() \
                + 0.01 * l1_loss(normals[v], self.normals[v])
        if self.lambda_flow != 0:                                                                          # :651-671
            H, W = pred.shape[-2:]
            E = K
            ori_t, lat_t = torch.cat(ori, 0), torch.cat(lat_img, 0)
            la_t, da_t = torch.cat(lat_alpha, 0), torch.cat(d_alphas, 0).reshape(self.n_views, 1, H, W)

            def norm(c):
                c = torch.stack([c[..., 0] / (W - 1), c[..., 1] / (H - 1)], -1)
                return (2.0 * c - 1.0).flatten(0, 1)
            ori_e = ori_t.unsqueeze(1).expand(-1, E, -1, -1, -1).flatten(0, 1)
            w_e2m = F.grid_sample(ori_e, norm(torch.cat(e2m_all, 0)), mode="bilinear", padding_mode="border",
                                  align_corners=False).reshape(-1, E, 3, H, W)
            w_m2e = F.grid_sample(lat_t.flatten(0, 1), norm(torch.cat(m2e_all, 0)), mode="bilinear", padding_mode="border",
                                  align_corners=False).reshape(-1, E, 3, H, W)
            loss = loss + self.lambda_flow * (
                l1_loss(w_e2m.flatten(0, 1), lat_t.flatten(0, 1), mask=la_t.flatten(0, 1))
                + l1_loss(w_m2e.flatten(0, 1), ori_e,
                          mask=da_t.unsqueeze(1).expand(-1, E, -1, -1, -1).flatten(0, 1)))
        loss = loss + 1e-4 * ((stat._scaling ** 2).mean() + (dyn._scaling ** 2).mean())
        loss.backward()
        with torch.no_grad():                                                                              # :634-648
            for v in range(self.n_views):
                grad2d = vsp[v].grad.squeeze(0)
                vis = radii[v] > 0
                stat.add_densification_stats(grad2d[:ns], vis[:ns], radii=radii[v][:ns])
                dyn.add_densification_stats(grad2d[ns:], vis[ns:], radii=radii[v][ns:])
        for o in opts:                                                                                     # :790-807
            o.step()
        return photo.detach()


def train(dev="cuda:0", iters=40, ns=4000, nd=2000, width=256, height=192, n_views=2, seed=0, lambda_flow=1e-2,
          shard=None, log=None, graph=False, prune_control_every=0, from_views=False, estimate_exposure=0,
          report_dir=None, report_every=0, lr_schedule=False, graph_optimizer=False, *, controller=False,
          first_iteration=1, keep_sorted=False, on_trainer=None):
    """graph=True (single process): forward + losses + backward of the iteration recorded ONCE as a HIP graph
    (mobgs_amd.graphed.GraphedCallable) and replayed, the Adam step outside -- for small images / few Gaussians, where an
    iteration is ~1400 launches and bound by the host (the reference's own 512x288 / 30 k operating point: 9.5 -> 7.5 ms).
    lr_schedule=True: the loop also does what train.py:312-313 and :807 do around the step -- update_learning_rate(iteration)
    on both sets before the iteration (the xyz rate decays as the reference's does) and blcekernel.adjust_lr() after it.
    graph_optimizer=True (with graph=True; implies lr_schedule): the Adam step is recorded INTO the graph as well --
    mobgs_amd.optim.DeviceAdam, whose rates and bias corrections are tabulated on the host and indexed on the device -- and
    the host does after_replay() per iteration instead of the walk over the parameter groups.  Same loss history, bit for
    bit, as lr_schedule=True run eagerly.
    prune_control_every=K > 0: every K iterations, between two iterations and outside any capture, the dynamic set drops
    one spline control point where that moves the projected trajectory by at most dyn.error_threshold pixels
    (TrainableGaussians.onedown_control_pts; in place, so a recorded iteration stays valid) and the smallest count is
    logged as train.py:734 does (MinCtrl).
    from_views=True: both sets are built by scene_init.scene_initialization from synthetic views (sets_from_views)
    instead of being sampled directly.
    estimate_exposure=N > 0: before every N-th iteration each view's exposure_time_expo entry is re-estimated from rendered
    static flow (DeblurTrainer.estimate_exposure; train.py:474-492 does it every 10th).  In place and on the device, so a
    recorded iteration reads the new values.
    report_dir, report_every=K > 0: after every K-th iteration (and after the last) rank 0 writes the report sheets of the
    training views (DeblurTrainer.report: mobgs_amd.scene_utils.render_training_image, as train.py:776-790 does on its
    testing iterations).
    controller=True (or a mapping of option overrides, see DeblurTrainer): the reference's densification, in every mode.
    The statistics of an iteration are the batch's, one launch inside the iteration (recorded with it under graph=True);
    after the optimiser step DensificationController.step(it, stat, dyn) runs the schedule of train.py:819-820.  When it
    resized a table or reset its opacities, the flat gradient buffers are laid over the new Parameters
    (DeblurTrainer.rebind) and, under graph=True, the recorded iteration is dropped: the optimisers' host state is brought
    up to date (DeviceAdam.sync_to_host, blcekernel.adjust_lr), the next iteration runs eagerly -- arenas and hints learn
    the grown scene, the reason iteration 1 is eager -- and the one after it is recorded again, with a DeviceAdam that
    starts at that iteration.
    first_iteration: the loop runs first_iteration .. iters with schedules, the blur kernel's rate and DeviceAdam at the
    true iteration (a short run can then cross iteration 3000, the opacity reset controlgaussians hard-codes).
    keep_sorted=True: TrainableGaussians.keep_sorted on both sets -- every densification ends with a spatial sort.
    on_trainer: called with the DeblurTrainer once it exists (its controller's log and flags, its optimisers)."""
    import time
    started = time.time()
    lr_schedule = lr_schedule or graph_optimizer
    if controller is not False and controller is not None:
        t = DeblurTrainer(dev, ns, nd, width, height, n_views, seed, lambda_flow, shard, iters, from_views, lr_schedule,
                          controller=controller)
    else:
        t = DeblurTrainer(dev, ns, nd, width, height, n_views, seed, lambda_flow, shard, iters, from_views, lr_schedule)
    if graph_optimizer and (not graph or t.shard.collective):
        raise ValueError("graph_optimizer=True needs graph=True and a single process")
    if keep_sorted:
        t.stat.keep_sorted = t.dyn.keep_sorted = True
    if on_trainer is not None:
        on_trainer(t)
    if first_iteration > 1 and lr_schedule:   # the rate blcekernel.adjust_lr() has left after first_iteration - 1 calls
        for g in t.blce.optimizer.param_groups:
            g["lr"] *= t.blce.lr_factor ** (first_iteration - 1)
    history, adam = [], None
    prune_views = t.prune_viewpoints() if prune_control_every else None
    fb, pending = None, []
    record_at = first_iteration + 1   # (the first iteration runs eagerly: arenas and hints exist afterwards)
    for it in range(first_iteration, iters + 1):
        if estimate_exposure and it % estimate_exposure == 0:
            t.estimate_exposure()
        if graph and fb is None and it == record_at and not t.shard.collective:
            from mobgs_amd.graphed import GraphedCallable
            if graph_optimizer:
                adam = t.device_adam(first_iteration=it, horizon=iters)

                def forward_backward_step():
                    loss = t.forward_backward()
                    adam.step()
                    return loss
                fb = GraphedCallable(forward_backward_step, warmup=0)
            else:
                fb = GraphedCallable(t.forward_backward, warmup=0)
        if lr_schedule and adam is None:
            t.update_learning_rate(it)
        if fb is not None:
            photo = fb()
            if adam is not None:
                adam.after_replay()
            else:
                t.optimizer_step()
            # the counts of the replays land in pinned rows: check() sees the replays that have COMPLETED.  The host enqueues a
            # replay in a fraction of its run time, so it is kept at most two iterations ahead (an event per iteration) -- an
            # arena outgrown by the moving scene (its frame saw empty lists: a background image, no splat gradients) is then
            # noticed two iterations late at most, and the iteration recorded again
            ev = torch.cuda.Event()
            ev.record()
            pending.append(ev)
            if len(pending) > 2:
                pending.pop(0).synchronize()
            if not fb.check():
                torch.cuda.synchronize()
                if adam is not None:   # (nothing was resized: the same pointers again, the counters carried over)
                    adam.rebuild()
                fb.recapture()
            history.append(float(photo))
        else:
            history.append(float(t.iteration()))
        if lr_schedule and adam is None:
            t.blce.adjust_lr()
        if t.controller is not None and t.controller.due(it):
            if fb is not None:   # the tensors of the recorded iteration are about to be replaced: back to the state the
                if adam is not None:   # eager loop holds between two iterations, and record again two iterations on
                    adam.sync_to_host()
                    t.blce.adjust_lr()
                adam, fb, pending = None, None, []
            t.control(it)
            record_at = it + 2
        if prune_control_every and it % prune_control_every == 0:
            pruned = t.dyn.onedown_control_pts(prune_views)
            if t.shard.rank == 0:
                print(f"it {it:4d}  one control point down on {int(pruned)} rows  MinCtrl {int(t.dyn.current_control_num.min())}")
        if report_dir and report_every and (it % report_every == 0 or it == iters) and t.shard.rank == 0:
            sheets = t.report(report_dir, it, time.time() - started)
            print(f"it {it:4d}  report sheets of {len(sheets)} views under {os.path.dirname(sheets[0])}")
        if it == first_iteration + 1:   # everything long-lived exists now: keep Python's cyclic collector off it (66 ms per generation-2
            import gc  # pass over a torch process's objects on this host, in the middle of an iteration: DESIGN section 5)
            gc.collect()
            gc.freeze()
        if log and (it % log == 0 or it == 1) and t.shard.rank == 0:
            print(f"it {it:4d}  photometric {history[-1]:.5f}")
    if adam is not None:   # the optimisers' host state as the eager loop would have left it
        adam.sync_to_host()
    return history, t.stat, t.dyn, t.blce, t.bucket


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--ns", type=int, default=20000)
    ap.add_argument("--nd", type=int, default=10000)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=288)
    ap.add_argument("--graph", action="store_true", help="replay forward + backward as one HIP graph (single process)")
    ap.add_argument("--lr-schedule", action="store_true",
                    help="update_learning_rate(iteration) before and blcekernel.adjust_lr() after every iteration")
    ap.add_argument("--graph-optimizer", action="store_true",
                    help="with --graph: record the Adam step into the graph as well (DeviceAdam; implies --lr-schedule)")
    ap.add_argument("--lambda-flow", type=float, default=1e-2,
                    help="weight of the flow-consistency term (0, the shipped configs: every kernel of the iteration is "
                         "deterministic and two runs give the same history bit for bit)")
    ap.add_argument("--prune-control-every", type=int, default=0, metavar="K",
                    help="every K iterations drop one spline control point where the trajectory moves <= 1 px (0 = never)")
    ap.add_argument("--from-views", action="store_true",
                    help="build both sets through scene_initialization from synthetic views instead of sampling them")
    ap.add_argument("--estimate-exposure", type=int, default=0, metavar="N",
                    help="every N iterations re-estimate each view's exposure time from rendered static flow (0 = never)")
    ap.add_argument("--report-dir", default=None, metavar="DIR",
                    help="write the report sheets of the training views (render_training_image) under DIR")
    ap.add_argument("--report-every", type=int, default=0, metavar="K",
                    help="with --report-dir: after every K-th iteration and after the last (0 = never)")
    ap.add_argument("--controller", action="store_true",
                    help="the reference's densification schedule and batch statistics (helper_train.DensificationController)")
    ap.add_argument("--first-iteration", type=int, default=1, metavar="IT",
                    help="run iterations IT .. --iters, with every schedule at the true iteration")
    ap.add_argument("--keep-sorted", action="store_true", help="end every densification with a spatial sort of the table")
    a = ap.parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    train(dev=f"cuda:{local}", iters=a.iters, ns=a.ns, nd=a.nd, width=a.width, height=a.height, log=10, graph=a.graph,
          prune_control_every=a.prune_control_every, from_views=a.from_views, estimate_exposure=a.estimate_exposure,
          report_dir=a.report_dir, report_every=a.report_every, lr_schedule=a.lr_schedule,
          graph_optimizer=a.graph_optimizer, lambda_flow=a.lambda_flow, controller=a.controller,
          first_iteration=a.first_iteration, keep_sorted=a.keep_sorted)
