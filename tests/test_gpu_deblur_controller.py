"""The reference's densification schedule inside the deblur loop (examples/train_deblur_synth.py --controller): eager, graphed,
graphed with the Adam step inside, resumed from a checkpoint, and sharded over two ranks.

160 x 112, 2 views, 2500 + 1200 splats, lambda_flow = 0 (every kernel of the iteration is deterministic, as
tests/test_gpu_graphed.py relies on).  The options come from a dry run of three controller-less iterations: the gradient
threshold is a quantile of its accum / denom, opthr a quantile of its sigmoid opacities; interval 4, densify_from_iter 3,
desicnt 2, so that 13 iterations hold two clone + split rounds of both sets (4, 8), an opacity prune of the static set (12)
and a third clone + split of the dynamic set, whose flag never counts.  Every test first asserts from controller.log that
these happened and that each moved between 5 % and 50 % of its set's rows: a run that resized nothing proves nothing.

All comparisons are exact (Python floats equal, torch.equal): the modes differ in WHO launches the kernels, not in what is
launched."""
import gc
import os
import socket
import sys
import types

import pytest
import torch

import test_gpu_checkpoint as CK   # _everything, _assert_same (functions only: nothing runs)

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

SIZE = dict(ns=2500, nd=1200, width=160, height=112, n_views=2, seed=2, lambda_flow=0.0)
ITERS = 13
# The dry run's statistics are the controller-less loop's: per view, and NOT scaled by W / 2, H / 2 as the batch statistics
# are, so most of its distribution lies far below what the controller sees.  Measured once over 0.93 .. 1.0 (rows moved per
# operation, docs/MEASUREMENT_LOG.md K35): only the top of the dry run's distribution keeps every operation under 50 %.
GRAD_QUANTILE, OPACITY_QUANTILE = 1.0, 0.2
_cache = {}


def _options(dev):
    """From three controller-less iterations; computed once."""
    if "options" not in _cache:
        import train_deblur_synth as T
        _, stat, dyn, _, _ = T.train(dev=str(dev), iters=3, **SIZE)
        g = torch.cat([(pc.xyz_gradient_accum / pc.denom).nan_to_num(0.0).reshape(-1) for pc in (stat, dyn)])
        op = torch.cat([torch.sigmoid(pc._opacity.detach()).reshape(-1) for pc in (stat, dyn)])
        _cache["options"] = dict(densify_grad_threshold=float(torch.quantile(g, GRAD_QUANTILE)),
                                 opthr=float(torch.quantile(op, OPACITY_QUANTILE)), densification_interval=4,
                                 densify_from_iter=3, desicnt=2)
        print("controller options from the dry run:", _cache["options"])
        del stat, dyn
        gc.collect()
    return dict(_cache["options"])


def _check_log(log, want_reset=False):
    """A clone + split of both sets and an opacity prune happened, each moving 5 % .. 50 % of its set's rows.  Operations
    AFTER an opacity reset (the run across 3000: those of iteration 3004) cannot stay in that band under any options: the
    reset leaves every opacity at or below 0.01, four Adam steps at opacity_lr move its logit by at most 0.2, and opthr, a
    fifth-quantile of opacities drawn as sigmoid(1.5 z), is about 0.2 -- that prune takes every row, by the reference's own
    rules -- while the nearly empty renders make nearly every row's gradient hot.  They must still have moved rows."""
    reset_at = min([r[0] for r in log if r[2] == "reset_opacity"], default=None)
    moved = {}
    for it, name, op, before, after, flag in log:
        if op == "reset_opacity":
            assert before == after
            continue
        frac = abs(after - before) / before
        print(f"it {it:4d}  {name:4s} {op:13s} {before:5d} -> {after:5d}  ({100 * frac:.1f} %)  flag {flag}")
        assert (after > before) if op == "pruneclone" else (after < before), (it, name, op, before, after)
        if reset_at is None or it <= reset_at:
            assert 0.05 <= frac <= 0.5, (it, name, op, before, after)
        moved.setdefault((name, op), []).append(it)
    assert ("stat", "pruneclone") in moved and ("dyn", "pruneclone") in moved and ("stat", "prune_opacity") in moved, moved
    assert want_reset == any(r[2] == "reset_opacity" for r in log)


def _train(dev, **kw):
    """train() -> (history, everything, controller log, flags, rows); the trainer is let go."""
    import train_deblur_synth as T
    box = {}
    kw.setdefault("iters", ITERS)
    history, *_ = T.train(dev=str(dev), controller=_options(dev), on_trainer=lambda t: box.update(t=t), **SIZE, **kw)
    t = box.pop("t")
    out = (history, CK._everything(t), [list(r) for r in t.controller.log], (t.controller.flag_d, t.controller.flag_s),
           (t.stat._n, t.dyn._n))
    del t
    gc.collect()
    return out


def _eager(dev, **kw):
    key = ("eager",) + tuple(sorted(kw.items()))
    if key not in _cache:
        _cache[key] = _train(dev, **kw)
        _check_log(_cache[key][2], want_reset=kw.get("first_iteration", 1) > 1)
    return _cache[key]


# ---- (f) the keyword exists --------------------------------------------------------------------------------------------------
def test_train_takes_the_controller_and_counts_iterations_not_views(hip_device):
    """train(controller=True): the reference's options, under which nothing is resized in two iterations; the statistics
    are the batch's -- one count per iteration for a row seen in either view, where the controller-less loop counts views."""
    import train_deblur_synth as T
    box = {}
    history, stat, dyn, _, bucket = T.train(dev=str(hip_device), iters=2, controller=True, on_trainer=lambda t: box.update(t=t),
                                            **SIZE)
    t = box["t"]
    assert len(history) == 2 and t.controller.log == [] and (t.controller.flag_d, t.controller.flag_s) == (0, 0)
    assert t.opt.densification_interval == 100 and t.opt.densify_from_iter == 500 and t.opt.desicnt == 6
    assert (stat._n, dyn._n) == (SIZE["ns"], SIZE["nd"]) and bucket.attached()
    assert float(stat.denom.max()) == 2.0 and float(dyn.denom.max()) == 2.0
    _, stat0, dyn0, _, _ = T.train(dev=str(hip_device), iters=2, **SIZE)
    assert float(stat0.denom.max()) == 4.0
    assert torch.equal(stat.max_radii2D, stat0.max_radii2D) and torch.equal(dyn.max_radii2D, dyn0.max_radii2D)
    assert torch.equal(stat.denom > 0, stat0.denom > 0)


# ---- (a) eager against a reconstruction from parts ------------------------------------------------------------------------------
def test_eager_loop_equals_controlgaussians_applied_to_restored_tables(hip_device):
    import train_deblur_synth as T
    from mobgs_amd.densify import TrainableGaussians
    from mobgs_amd.helper_train import controlgaussians
    from mobgs_amd.synth import SynthCamera, dynamic_extras, gaussian_cloud
    dev = str(hip_device)
    t = T.DeblurTrainer(dev, SIZE["ns"], SIZE["nd"], SIZE["width"], SIZE["height"], SIZE["n_views"], SIZE["seed"],
                        SIZE["lambda_flow"], None, ITERS, False, False, controller=_options(hip_device))
    scam = SynthCamera().scaled(SIZE["width"], SIZE["height"])
    small = gaussian_cloud(8, scam, 0)

    def fresh(dynamic, state):
        pc = TrainableGaussians(small, dynamic_extras(small["xyz"], 0) if dynamic else None, t.stat.rgbdecoder, device=dev)
        pc.training_setup(t.opt)
        return pc.load_state_dict(state)

    checked = 0
    for it in range(1, ITERS + 1):
        t.iteration()
        if not t.controller.due(it):
            assert not t.control(it)
            continue
        pre = {"dyn": t.dyn.state_dict(), "stat": t.stat.state_dict()}
        rng = torch.cuda.get_rng_state(hip_device)
        mark = len(t.controller.log)
        assert t.control(it)
        after = torch.cuda.get_rng_state(hip_device)
        assert (t.ns, t.nd) == (t.stat._n, t.dyn._n) and t.bucket.attached()
        assert t.bucket.extra("view1").numel() == 3 * (t.ns + t.nd)
        torch.cuda.set_rng_state(rng, hip_device)
        for name, live in (("dyn", t.dyn), ("stat", t.stat)):        # the reference's order: the split samples are drawn in it
            records = [r for r in t.controller.log[mark:] if r[1] == name]
            assert records and all(r[0] == it for r in records)
            pc = fresh(name == "dyn", pre[name])
            assert pc._n == records[0][3]
            controlgaussians(t.opt, pc, 2, it, types.SimpleNamespace(cameras_extent=t.controller.scene.cameras_extent),
                             None, None, None, records[0][5], is_dynamic=name == "dyn")
            assert pc._n == records[-1][4] == live._n
            a, b = pc.table_state(), live.table_state()
            assert set(a) == set(b)
            bad = [k for k in a if a[k].shape != b[k].shape or not torch.equal(a[k], b[k])]
            assert not bad, (it, name, bad)
            checked += 1
        assert torch.equal(torch.cuda.get_rng_state(hip_device), after)
    _check_log(t.controller.log)
    assert checked == 6 and [r[0] for r in t.controller.log] == [4, 4, 8, 8, 12, 12]
    assert (t.controller.flag_d, t.controller.flag_s) == (0, 2)


# ---- (b) gradient plumbing after a resize, and a resumed run -----------------------------------------------------------------------
def test_flat_gradients_after_a_resize_and_a_resumed_run(hip_device, tmp_path):
    import resume_deblur_synth as R
    dev, path = str(hip_device), str(tmp_path / "run.mobgs")
    settings = dict(iters=ITERS, ns=SIZE["ns"], nd=SIZE["nd"], width=SIZE["width"], height=SIZE["height"], seed=SIZE["seed"],
                    lambda_flow=0.0, controller=_options(hip_device))
    history, t, _, _ = R.run(dev=dev, **settings)
    _check_log(t.controller.log)
    straight = (CK._everything(t), t.controller.state_dict(), (t.stat._n, t.dyn._n))
    del t
    gc.collect()
    first, ta, handles, _ = R.run(dev=dev, path=path, save_at=(4,), stop_at=4, blocking=True, **settings)
    assert first == history[:4] and ta.controller.log and ta.controller.log[-1][0] == 4 and ta.stat._n > SIZE["ns"]
    loaded, tb, _, _ = R.run(dev=dev, resume=path, stop_at=4, **settings)      # nothing left to run: the loaded state
    assert loaded == [] and (tb.stat._n, tb.dyn._n) == (ta.stat._n, ta.dyn._n)
    assert tb.controller.state_dict() == ta.controller.state_dict()
    # one forward + backward on each: a buffer re-laid by rebind() against one built over the loaded tables
    la, lb = ta.forward_backward(), tb.forward_backward()
    assert float(la) == float(lb)
    assert ta.bucket.flat.numel() == tb.bucket.flat.numel() and ta.bucket.param_floats == tb.bucket.param_floats
    assert torch.equal(ta.bucket.flat, tb.bucket.flat) and float(ta.bucket.flat[:ta.bucket.param_floats].abs().sum()) > 0
    assert ta.bucket.attached() and tb.bucket.attached()
    del ta, tb, handles
    gc.collect()
    torch.manual_seed(987654321)
    torch.cuda.manual_seed(123)
    rest, t, _, _ = R.run(dev=dev, resume=path, **settings)
    assert rest == history[4:], (rest, history[4:])
    assert (t.stat._n, t.dyn._n) == straight[2] and t.controller.state_dict() == straight[1]
    CK._assert_same(straight[0], CK._everything(t), "resumed against straight")


# ---- (c) graphed against eager ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["graph", "graph_lr_schedule", "graph_optimizer", "graph_optimizer_keep_sorted"])
def test_graphed_loop_equals_eager(hip_device, mode):
    extra = {} if mode == "graph" else dict(lr_schedule=True)
    if mode.endswith("keep_sorted"):
        extra["keep_sorted"] = True
    history, state, log, flags, rows = _eager(hip_device, **extra)
    got = _train(hip_device, graph=True, graph_optimizer=mode.startswith("graph_optimizer"), **extra)
    assert got[0] == history, (got[0], history)
    assert got[2] == log and got[3] == flags == (0, 2) and got[4] == rows
    CK._assert_same(state, got[1], mode)


def test_keep_sorted_orders_the_rows(hip_device):
    plain, ordered = _eager(hip_device, lr_schedule=True), _eager(hip_device, lr_schedule=True, keep_sorted=True)
    assert plain[4][0] > SIZE["ns"] and not torch.equal(plain[1]["stat.xyz"], ordered[1]["stat.xyz"])


# ---- (d) across iteration 3000 ------------------------------------------------------------------------------------------------------
def test_the_opacity_reset_at_3000_eager_and_graphed(hip_device):
    import train_deblur_synth as T
    moments = {}

    def hook(t):
        control = t.control

        def watched(it):
            changed = control(it)
            if it == 3000:
                moments[len(moments)] = [float(pc.table_state()[k].abs().sum()) for pc in (t.stat, t.dyn)
                                         for k in ("opacity.exp_avg", "opacity.exp_avg_sq")]
                moments[len(moments)] = float(torch.sigmoid(t.stat._opacity.detach()).max())
            return changed
        t.control = watched

    span = dict(first_iteration=2996, iters=3004, lr_schedule=True)
    history, state, log, flags, rows = _eager(hip_device, **span)
    assert len(history) == 9 and [r[0] for r in log if r[2] == "reset_opacity"] == [3000, 3000]
    assert [r[0] for r in log] == [2996, 2996, 3000, 3000, 3000, 3000, 3004, 3004]
    box = {}
    got_history, *_ = T.train(dev=str(hip_device), controller=_options(hip_device), graph=True, graph_optimizer=True,
                              on_trainer=lambda t: (hook(t), box.update(t=t)), **SIZE, **span)
    t = box.pop("t")
    assert moments[0] == [0.0, 0.0, 0.0, 0.0] and moments[1] <= 0.0100001, moments
    assert got_history == history and [list(r) for r in t.controller.log] == log
    CK._assert_same(state, CK._everything(t), "graphed across 3000")


# ---- (e) sharded ---------------------------------------------------------------------------------------------------------------------
def _checksums(t):
    import zlib
    out = {}
    for k, v in CK._everything(t).items():
        out[k] = (tuple(v.shape), zlib.crc32(v.reshape(-1).contiguous().view(torch.uint8).numpy().tobytes()))
    return out


def _rank(rank, world, port, q, options, iters, force):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    if force:
        os.environ["MOBGS_FORCE_COLLECTIVES"] = "1"
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import train_deblur_synth as T
        from mobgs_amd.distributed import SubframeShard
        shard = SubframeShard()
        assert shard.collective
        if force:    # ONE iteration of the sharded path: denom and max_radii2D depend on the forward pass only
            t = T.DeblurTrainer("cuda:0", SIZE["ns"], SIZE["nd"], SIZE["width"], SIZE["height"], SIZE["n_views"], SIZE["seed"],
                                0.0, shard, iters, False, False, controller=options)
            t.iteration()
            q.put((rank, [x.cpu().numpy() for pc in (t.stat, t.dyn) for x in (pc.denom, pc.max_radii2D)]))
            return
        box = {}
        T.train(dev="cuda:0", iters=iters, shard=shard, controller=options, on_trainer=lambda t: box.update(t=t), **SIZE)
        t = box["t"]
        mine = (_checksums(t), [list(r) for r in t.controller.log], (t.controller.flag_d, t.controller.flag_s))
        everyone = [None] * world
        dist.all_gather_object(everyone, mine)
        q.put((rank, everyone[0] == everyone[1], everyone[rank][1], (t.stat._n, t.dyn._n)))
    finally:
        dist.destroy_process_group()


def _spawn(world, args):
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, world, port, q, *args)) for r in range(world)]
    for p in procs:
        p.start()
    results = sorted([q.get(timeout=300) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return results


def test_two_ranks_end_with_identical_tables_and_logs(hip_device):
    results = _spawn(2, (_options(hip_device), ITERS, False))
    for rank, same, log, rows in results:
        assert same, "the ranks' tables, moments, statistics or logs differ"
        _check_log(log)
        assert rows[0] != SIZE["ns"] and rows[1] != SIZE["nd"] and rows == results[0][3]


def test_forced_collectives_give_the_single_process_statistics(hip_device):
    import train_deblur_synth as T
    ((_, got),) = _spawn(1, (_options(hip_device), ITERS, True))
    t = T.DeblurTrainer(str(hip_device), SIZE["ns"], SIZE["nd"], SIZE["width"], SIZE["height"], SIZE["n_views"], SIZE["seed"],
                        0.0, None, ITERS, False, False, controller=_options(hip_device))
    assert not t.shard.collective
    t.iteration()
    want = [x.cpu() for pc in (t.stat, t.dyn) for x in (pc.denom, pc.max_radii2D)]
    assert float(want[0].sum()) > 0 and float(want[2].sum()) > 0
    for g, w in zip(got, want):
        assert torch.equal(torch.from_numpy(g), w)
