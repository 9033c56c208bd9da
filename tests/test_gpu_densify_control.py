"""The densification controller on the GPU: mobgs_densify_plan and mobgs_densify_stats_batch (csrc/densify_ctl.hip) through
the C ABI against tests/control_cases.py, the planned methods of TrainableGaussians against the routes they restate, and
mobgs_amd.helper_train.controlgaussians against the restated schedule on a restated table (tests/densify_restatement.py).
tests/test_control_cases_cpu.py vets the inputs of every case and ties the restatements to the reference's own trace.

The kernels validate neither row indices nor buffer sizes: every buffer passed here has the documented worst-case size.
Lists, counts, grad_sum, radii_max, visible, denom and max_radii2D are compared exactly; xyz_gradient_accum to rtol 3e-7,
the bound of the existing statistics test (one rounded root of a sum of two squares, then one add, no cancellation); split
children's xyz / scaling at the bounds stated in tests/test_gpu_densify_kernels.py's header."""
import ctypes
import os
import sys
import types

import pytest
import torch

import control_cases as C
import densify_restatement as R
import test_gpu_optim as O   # _synthetic_table, _step_against_torch_adam, _clear_of_the_size_threshold, _check_resize

pytestmark = pytest.mark.gpu

SENTINEL = -7777


def _abi():
    from mobgs_amd import _lib
    return _lib.load(), _lib.ptr, _lib.stream, _lib.check, _lib._DEFINES


def _run_plan(dev, op, inp, n, n_split):
    """-> (rc, index, counts, scratch) with the list and the counts pre-filled with SENTINEL."""
    lib, ptr, stream, _, D = _abi()
    d = {k: v.to(dev) for k, v in inp.items()}
    bounds = torch.tensor([*C.MAXB, *C.MINB], dtype=torch.float32, device=dev)
    index = torch.full((max(n * max(2, n_split), 1),), SENTINEL, dtype=torch.int32, device=dev)
    counts = torch.full((4,), SENTINEL, dtype=torch.int32, device=dev)
    scratch = torch.full((3 * ((n + 1023) // 1024) + 1,), SENTINEL, dtype=torch.int32, device=dev)
    p = lambda k: ptr(d[k]) if n else None  # noqa: E731
    rc = lib.mobgs_densify_plan(D["MOBGS_PLAN_" + op], n, n_split, p("accum"), p("denom"), p("scaling"), C.THR, C.SIZE_THR,
                                p("opacity"), C.MIN_OPACITY, p("xyz"), ptr(bounds), p("mask"), ptr(index), ptr(counts),
                                ptr(scratch), stream())
    return rc, index.cpu(), counts.cpu(), scratch.cpu()


@pytest.mark.parametrize("n", C.PLAN_NS)
def test_plan_lists_and_counts_equal_the_restatement(hip_device, n):
    lib, ptr, stream, check, D = _abi()
    inp = C.plan_inputs(n, 9000 + n)
    for op in C.PLAN_OPS:
        for n_split in (C.PLAN_SPLITS if op == "PRUNECLONE" else (1, 3)):
            rc, index, counts, scratch = _run_plan(hip_device, op, inp, n, n_split)
            check(rc, "mobgs_densify_plan")
            want_index, want_counts = C.plan_expected(op, inp, n_split)
            assert torch.equal(counts, want_counts), (op, n, n_split, counts.tolist(), want_counts.tolist())
            n_out = int(want_counts[3])
            assert torch.equal(index[:n_out], want_index), (op, n, n_split)
            assert bool((index[n_out:] == SENTINEL).all()), (op, n, n_split, "the list was written beyond n_out")
            assert int(scratch[-1]) == SENTINEL
    if n == 0:
        return
    # the clone / split sets the list implies are the masks mobgs_densify_select gives on the same buffers
    dev = {k: inp[k].to(hip_device) for k in ("accum", "denom", "scaling")}
    clone = torch.empty(n, dtype=torch.uint8, device=hip_device)
    split = torch.empty(n, dtype=torch.uint8, device=hip_device)
    check(lib.mobgs_densify_select(n, n, ptr(dev["accum"]), ptr(dev["denom"]), ptr(dev["scaling"]), C.THR, C.SIZE_THR,
                                   ptr(clone), ptr(split), stream()), "mobgs_densify_select")
    rc, index, counts, _ = _run_plan(hip_device, "PRUNECLONE", inp, n, 2)
    check(rc, "mobgs_densify_plan")
    kept, clones, parents, n_out = counts.tolist()
    listed = lambda part: torch.zeros(n, dtype=torch.uint8).index_fill_(0, (-(part + 1)).long(), 1)  # noqa: E731
    assert torch.equal(listed(index[kept:kept + clones]), clone.cpu())
    assert torch.equal(listed(index[kept + clones:kept + clones + parents]), split.cpu())
    assert torch.equal(index[kept + clones:kept + clones + parents], index[kept + clones + parents:n_out])


@pytest.mark.parametrize("n_split", [0, 9, -1])
def test_plan_refuses_a_bad_n_split_and_touches_nothing(hip_device, n_split):
    lib, _, _, _, D = _abi()
    inp = C.plan_inputs(1025, 1)
    for op in C.PLAN_OPS:
        rc, index, counts, scratch = _run_plan(hip_device, op, inp, 1025, n_split)
        assert rc == D["MOBGS_E_INVALID"] and b"mobgs_densify_plan" in lib.mobgs_last_error()
        torch.cuda.synchronize()
        assert bool((index == SENTINEL).all()) and bool((counts == SENTINEL).all()) and bool((scratch == SENTINEL).all())


@pytest.mark.parametrize("n,n_views,grad_stride,row0", C.STATS_CASES)
def test_stats_batch_equals_the_restatement(hip_device, n, n_views, grad_stride, row0):
    lib, ptr, stream, check, D = _abi()
    state, steps = C.stats_inputs(n, n_views, grad_stride, row0, 17 * n + n_views)
    dev = {k: v.clone().to(hip_device) for k, v in state.items()}
    W, H = 640, 360
    for step, (grads, radii) in enumerate(steps):
        dg, dr = [g.to(hip_device) for g in grads], [r.to(hip_device) for r in radii]
        g_tab = (ctypes.c_void_p * n_views)(*[t.data_ptr() for t in dg])
        r_tab = (ctypes.c_void_p * n_views)(*[t.data_ptr() for t in dr])
        for outputs in (False, True) if step == 0 else (True,):
            before = {k: v.cpu().clone() for k, v in dev.items()}
            work = {k: v.clone() for k, v in dev.items()} if not outputs else dev   # (the run without outputs is discarded)
            grad_sum = torch.full((n, 2), float("nan"), device=hip_device)
            radii_max = torch.full((n,), SENTINEL, dtype=torch.int32, device=hip_device)
            visible = torch.full((n,), 0xA5, dtype=torch.uint8, device=hip_device)
            opt = [ptr(grad_sum), ptr(radii_max), ptr(visible)] if outputs else [None] * 3
            check(lib.mobgs_densify_stats_batch(n_views, g_tab, grad_stride, r_tab, row0, n, W * 0.5, H * 0.5,
                                                ptr(work["xyz_gradient_accum"]), ptr(work["denom"]),
                                                ptr(work["max_radii2D"]), *opt, stream()), "mobgs_densify_stats_batch")
            want, total, want_radii, vis = C.batch_stats(state, grads, radii, row0, n, W, H)
            got = {k: v.cpu() for k, v in work.items()}
            if outputs:
                assert torch.equal(grad_sum.cpu(), total), (step, "grad_sum")
                assert torch.equal(radii_max.cpu(), want_radii), (step, "radii_max")
                assert torch.equal(visible.cpu(), vis.to(torch.uint8)), (step, "visible")
            else:
                assert bool(torch.isnan(grad_sum).all()) and bool((radii_max == SENTINEL).all())
            for k in want:
                assert torch.equal(got[k][~vis], before[k][~vis]), (step, k, "a row that is not visible changed")
            assert torch.equal(got["denom"], want["denom"]) and torch.equal(got["max_radii2D"], want["max_radii2D"]), step
            ref = want["xyz_gradient_accum"].double()
            err = float(((got["xyz_gradient_accum"].double() - ref).abs() / ref.abs().clamp_min(1e-300)).max())
            print(f"stats_batch n={n} views={n_views} stride={grad_stride} row0={row0} step {step}: accum error {err:.2e}")
            assert torch.allclose(got["xyz_gradient_accum"], want["xyz_gradient_accum"], rtol=3e-7, atol=0), (step, err)
        state = want


def test_stats_batch_refuses_17_views(hip_device):
    lib, ptr, stream, _, D = _abi()
    n = 300
    g = [torch.zeros(n, 2, device=hip_device) for _ in range(17)]
    r = [torch.ones(n, dtype=torch.int32, device=hip_device) for _ in range(17)]
    stats = [torch.full((n,), 3.0, device=hip_device) for _ in range(3)]
    for n_views in (17, 0):
        rc = lib.mobgs_densify_stats_batch(n_views, (ctypes.c_void_p * 17)(*[t.data_ptr() for t in g]), 2,
                                           (ctypes.c_void_p * 17)(*[t.data_ptr() for t in r]), 0, n, 1.0, 1.0,
                                           *[ptr(s) for s in stats], None, None, None, stream())
        assert rc == D["MOBGS_E_INVALID"] and b"mobgs_densify_stats_batch" in lib.mobgs_last_error()
    torch.cuda.synchronize()
    assert all(bool((s == 3.0).all()) for s in stats)


# ---- the planned methods against the routes they restate ------------------------------------------------------------------
def _static_table(n, dev, seed):
    """A STATIC set: TrainableGaussians(params, None), so omega, the control points, their count, zeta, trbf_scale, motion
    and the deformation table are the defaults a set without dynamic extras gets (zeros, 100 xyz repeated, int64 twelves,
    all rows deformable), is_dynamic is False, and the rows straddle the size threshold as test_gpu_optim's table does."""
    import math
    from mobgs_amd.densify import TrainableGaussians
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(n, *s, generator=g)  # noqa: E731
    u = lambda *s: torch.rand(n, *s, generator=g)  # noqa: E731
    top = torch.where(u() < 0.4, math.log(O.SIZE_THR) + 0.2 + 2.0 * u(), math.log(O.SIZE_THR) - 0.2 - 2.0 * u())
    scaling = top[:, None] - 2.0 * u(3)
    scaling[torch.arange(n), torch.randint(0, 3, (n,), generator=g)] = top
    params = {"xyz": 3.0 * r(3), "scaling": scaling, "rotation": r(4), "opacity": r(1), "features_dc": r(6),
              "features_t": r(3)}
    pc = TrainableGaussians(params, None, device=dev)
    assert pc.is_dynamic is False
    pc.training_setup(O._Opt())
    return pc


def _twins(n, dev, dynamic):
    """Two TrainableGaussians from the same tables with two Adam steps behind them, hot statistics, clear of the size and
    the opacity decisions.  dynamic: test_gpu_optim's table with every dynamic extra given; otherwise _static_table."""
    pcs = []
    for _ in range(2):
        pc = O._synthetic_table(n, dev, 40 + n) if dynamic else _static_table(n, dev, 90 + n)
        assert pc.is_dynamic is dynamic
        g = torch.Generator().manual_seed(n + (7 if dynamic else 0))
        for _ in range(2):
            for gr in pc.optimizer.param_groups:
                for p in gr["params"]:
                    if p.requires_grad and p.numel():
                        p.grad = (0.01 * torch.randn(p.shape, generator=g)).to(p.device)
            pc.optimizer.step()
        denom = torch.randint(0, 4, (n, 1), generator=g).float()
        accum = torch.where(torch.rand(n, 1, generator=g) < 0.3, 2.0, 0.5) * 2.0e-4 * denom
        pc.xyz_gradient_accum.copy_(accum.to(dev))
        pc.denom.copy_(denom.to(dev))
        O._clear_of_the_size_threshold(pc)
        op = pc.table_state()["opacity"]
        s = torch.sigmoid(op.double())
        op[((s - 0.3).abs() <= 1e-3 * 0.3)] += 0.01
        pcs.append(pc)
    a, b = (pc.table_state() for pc in pcs)
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a) and "xyz.exp_avg" in a
    if not dynamic:   # the static defaults are in place, with moments of their own after the two steps
        assert a["current_control_num"].dtype == torch.int64 and bool((a["current_control_num"] == 12).all())
        assert bool(a["_deformation_table"].all()) and "omega.exp_avg" in a
    return pcs


def _same_tables(old, new, what):
    a, b = old.table_state(), new.table_state()
    assert set(a) == set(b), what
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (what, k)
    from mobgs_amd.densify import GROUPS
    for pc in (old, new):   # the optimiser's groups are keyed to the new parameters
        for gr in pc.optimizer.param_groups:
            if gr["name"] in dict(GROUPS):
                attr = dict(GROUPS)[gr["name"]]
                assert gr["params"][0] is getattr(pc, attr), (what, gr["name"])
                if gr["name"] != "current_control_num" and gr["params"][0].numel():   # (f_rest has no elements here)
                    assert gr["params"][0] in pc.optimizer.state, (what, gr["name"])


@pytest.mark.parametrize("dynamic", [False, True])
@pytest.mark.parametrize("n", [1500, 2500])
def test_planned_routes_leave_the_tables_of_the_existing_routes(hip_device, n, dynamic):
    old, new = _twins(n, hip_device, dynamic)
    assert C.opacity_margin(old.table_state()["opacity"].cpu(), 0.3) > 1e-4
    torch.manual_seed(123)
    old.densify_pruneclone(2.0e-4, 0.005, O.EXTENT, 20, splitN=2)
    torch.manual_seed(123)
    new.pruneclone_planned(2.0e-4, O.EXTENT, splitN=2)
    assert new.get_xyz.shape[0] > n + 100
    _same_tables(old, new, "pruneclone")            # the random children included: same generator, same draws
    rows = old.get_xyz.shape[0]
    old.prune_points((old.get_opacity < 0.3).squeeze())
    new.prune_opacity_below(0.3)
    assert 0 < new.get_xyz.shape[0] < rows - 100
    _same_tables(old, new, "opacity prune")
    xyz = old.get_xyz.detach()
    lo, hi = xyz.quantile(0.1, dim=0), xyz.quantile(0.9, dim=0)
    rows = old.get_xyz.shape[0]
    mask = ((xyz > hi) | (xyz < lo)).any(dim=1)
    old.prune_points(mask)
    new.prune_outside(list(lo.unbind(0)), list(hi.unbind(0)))     # 0-dim device tensors, as train.py:217-228 makes them
    assert 0 < new.get_xyz.shape[0] == int((~mask).sum()) < rows
    _same_tables(old, new, "bounds prune")


def test_planned_routes_consume_the_generator_alike(hip_device):
    old, new = _twins(1500, hip_device, False)
    torch.manual_seed(5)
    old.densify_pruneclone(2.0e-4, 0.005, O.EXTENT, 20, splitN=3)
    after_old = torch.rand(4, device=hip_device)
    torch.manual_seed(5)
    new.pruneclone_planned(2.0e-4, O.EXTENT, splitN=3)
    after_new = torch.rand(4, device=hip_device)
    assert torch.equal(after_old, after_new)
    _same_tables(old, new, "pruneclone, three children")


# ---- the controller end to end ---------------------------------------------------------------------------------------------
OPTIONS = dict(densify_until_iter=13, densify_from_iter=2, densification_interval=3, opacity_reset_interval=7, desicnt=2,
               opthr=0.3, densify_grad_threshold=2.0e-4)


@pytest.mark.parametrize("dynamic", [False, True])
def test_controlgaussians_follows_the_restated_schedule_on_a_table(hip_device, dynamic):
    """1500 rows, iterations 1 .. 14: two clone + split resizes (both sets: the dynamic set's flag never counts, so it keeps
    densifying), opacity prunes once the static flag reached desicnt, nothing from densify_until_iter on.  Statistics are
    fed before every scheduled iteration, samples are explicit, and after every call the table is the restatement's."""
    from mobgs_amd.helper_train import controlgaussians
    pc = O._synthetic_table(1500, hip_device, 1500)
    g = torch.Generator().manual_seed(8)
    O._step_against_torch_adam(pc, g)
    opt = types.SimpleNamespace(**OPTIONS)
    scene = types.SimpleNamespace(cameras_extent=O.EXTENT)
    want = C.schedule(OPTIONS, 14, dynamic, O.EXTENT)
    by_iteration = {}
    for c in want["calls"]:
        by_iteration.setdefault(c["iteration"], []).append(c)
    assert {c["name"] for c in want["calls"]} == ({"densify_pruneclone"} if dynamic else {"densify_pruneclone", "prune_points"})
    flag, flags, resized = 0, dict(map(tuple, want["flags"])), 0
    for it in range(1, 15):
        n = pc.get_xyz.shape[0]
        calls = by_iteration.get(it, [])
        samples = None
        if calls:
            (call,) = calls
            denom = torch.randint(0, 4, (n, 1), generator=g).float()
            accum = torch.where(torch.rand(n, 1, generator=g) < 0.3, 2.0, 0.5) * 2.0e-4 * denom
            pc.xyz_gradient_accum.copy_(accum.to(hip_device))
            pc.denom.copy_(denom.to(hip_device))
            op = pc.table_state()["opacity"]
            op[((torch.sigmoid(op.double()) - OPTIONS["opthr"]).abs() <= 1e-3 * OPTIONS["opthr"])] += 0.01
            pre = O._clear_of_the_size_threshold(pc)
            assert C.opacity_margin(pre["opacity"], OPTIONS["opthr"]) > 1e-4
            children = None
            if call["name"] == "densify_pruneclone":
                thr = call["args"][0]
                assert thr == (1.0e-4 if dynamic else 2.0e-4)
                _, split = R.select(pre["scaling"], R.mean_grads(pre["xyz_gradient_accum"], pre["denom"]), thr, O.SIZE_THR)
                parents = torch.nonzero(split).reshape(-1).repeat(2)
                samples = torch.randn(parents.shape[0], 3, generator=g) * torch.exp(pre["scaling"][parents])
                lay = {}
                table = C.apply_call(pre, call, O.EXTENT, O._Opt.percent_dense, OPTIONS["opthr"], samples, lay)
                assert lay["clones"] > 50 and lay["children"] == parents.shape[0] > 50
                children = (lay["kept"] + lay["clones"], pre["rotation"][parents], pre["xyz"][parents],
                            pre["scaling"][parents], samples, 2)
                samples = samples.to(hip_device)
            else:
                table = C.apply_call(pre, call, O.EXTENT, O._Opt.percent_dense, OPTIONS["opthr"])
                assert 0 < table["xyz"].shape[0] < n
        flag = controlgaussians(opt, pc, 2, it, scene, None, None, None, flag, is_dynamic=dynamic, samples=samples)
        if calls:
            O._check_resize(pc, table, False, children)
            assert flag == flags[it], (it, flag, flags[it])
            resized += 1
            O._step_against_torch_adam(pc, g)
        else:
            assert pc.get_xyz.shape[0] == n, (it, "a resize on an iteration the schedule does not name")
    assert flag == want["final_flag"] == (0 if dynamic else 2) and resized == len(want["calls"]) == 4


def test_modes_1_and_3_raise_before_touching_the_set(hip_device):
    """On a scheduled iteration of a real set: nothing of the table, the statistics or the optimiser's keys moves."""
    from mobgs_amd.helper_train import controlgaussians
    pc = _static_table(300, hip_device, 3)
    pc.denom.fill_(2.0)
    pc.xyz_gradient_accum.fill_(1.0)    # every row hot: mode 2 would resize here
    before = {k: v.detach().cpu().clone() for k, v in pc.table_state().items()}
    keys = [gr["params"][0] for gr in pc.optimizer.param_groups]
    scene = types.SimpleNamespace(cameras_extent=O.EXTENT)
    for mode in (1, 3):
        with pytest.raises(NotImplementedError):
            controlgaussians(types.SimpleNamespace(**OPTIONS), pc, mode, 3, scene, None, None, None, 0)
        after = pc.table_state()
        assert set(after) == set(before) and all(torch.equal(after[k].cpu(), before[k]) for k in before)
        assert all(gr["params"][0] is k for gr, k in zip(pc.optimizer.param_groups, keys))


def test_batch_densification_stats_validates_what_the_kernel_does_not(hip_device):
    from mobgs_amd.helper_train import batch_densification_stats
    stat, dyn = O._synthetic_table(300, hip_device, 1), O._synthetic_table(200, hip_device, 2)

    def out(n, dtype=torch.int32, gdtype=torch.float32, cols=2):
        vp = torch.zeros(1, n, cols, dtype=gdtype, device=hip_device, requires_grad=True)
        vp.grad = torch.full((1, n, cols), 1e-4, dtype=gdtype, device=hip_device)
        return {"viewspace_points": vp, "radii": torch.ones(n, dtype=dtype, device=hip_device)}

    for bad in ([], [out(500)] * 17, [out(499)], [out(500, dtype=torch.int64)], [out(500, gdtype=torch.float64)],
                [out(500), out(500, cols=3)]):
        with pytest.raises(ValueError):
            batch_densification_stats(stat, dyn, bad, 64, 128)
    no_grad = out(500)
    no_grad["viewspace_points"].grad = None
    with pytest.raises(ValueError):
        batch_densification_stats(stat, dyn, [no_grad], 64, 128)
    assert float(stat.denom.sum()) == 0.0
    (gs, vs, rs), (gd, vd, rd) = batch_densification_stats(stat, dyn, [out(500), out(500)], 64, 128, want_outputs=True)
    assert gs.shape == (300, 2) and gd.shape == (200, 2) and vs.dtype == torch.bool and bool(vd.all()) and rd.dtype == torch.int32
    assert torch.equal(gs.cpu(), torch.tensor([[2e-4 * 32, 2e-4 * 64]], dtype=torch.float32).expand(300, 2))
    assert float(stat.denom.sum()) == 300.0 and float(dyn.denom.sum()) == 200.0 and float(dyn.max_radii2D.min()) == 1.0


def test_train_synth_with_the_controller_resizes_on_scheduled_iterations_only(hip_device):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synth
    iters, every = 40, 12
    history, stat, dyn = train_synth.train(dev=str(hip_device), iters=iters, ns=1500, nd=800, width=128, height=96,
                                           densify_every=every, seed=4, controller=True)
    opt = train_synth.ControlOpt.scaled(iters, every)
    assert all(torch.isfinite(torch.tensor(h[:2])).all() for h in history) and len(history) == iters
    counts = [history[0][2:]] + [(h[2], h[3]) for h in history[1:]] + [(stat.get_xyz.shape[0], dyn.get_xyz.shape[0])]
    # history[it - 1] holds the counts at the START of iteration it, so counts[it] are those after iteration it
    changed = [it for it in range(1, iters + 1) if counts[it] != counts[it - 1]]
    scheduled = [it for it in range(1, iters + 1) if opt.densify_from_iter < it < opt.densify_until_iter
                 and it % opt.densification_interval == 0]
    assert scheduled == [12, 24, 36] and changed and set(changed) <= set(scheduled), (changed, scheduled)
    assert float(stat.denom.sum()) > 0.0   # statistics gathered since the last resize
