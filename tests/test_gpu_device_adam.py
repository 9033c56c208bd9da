"""mobgs_amd.optim.DeviceAdam -- the Adam step with its rates and bias corrections looked up on the device, recordable into a
graph -- against fused_adam_step driven by host-side rates on clones.  The two run the same device arithmetic on the same
factors, so every comparison is exact (torch.equal / bit patterns): no tolerance."""
import math
import struct

import numpy as np
import pytest
import torch

import densify_restatement as R
from mobgs_amd.general_utils import get_expon_lr_func
from mobgs_amd.optim import DeviceAdam, MultiplicativeLR, fused_adam_step

pytestmark = pytest.mark.gpu

CLASSES = [((0.9, 0.999), 1e-15), ((0.8, 0.99), 1e-8)]


def _f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _twin_optimisers(pa, pb, lrs, hyper, split=None):
    """Two lists of torch.optim.Adam over one-tensor groups (device side over pa, yardstick over pb), cut at `split`."""
    def make(ps):
        groups = [{"params": [p], "lr": lrs[i], "betas": hyper(i)[0], "eps": hyper(i)[1], "name": f"g{i}"}
                  for i, p in enumerate(ps)]
        cut = len(groups) if split is None else split
        return [torch.optim.Adam(gs, lr=0.0) for gs in (groups[:cut], groups[cut:]) if gs]
    return make(pa), make(pb)


def _groups(opts):
    return [g for o in opts for g in o.param_groups]


def _set_rates(opts, fns, it):
    """The host side of the yardstick: what update_learning_rate(it) / adjust_lr() leave in group["lr"]."""
    for g, fn in zip(_groups(opts), fns):
        if fn is not None:
            g["lr"] = fn(it)


def _persistent_grads(ps):
    for p in ps:
        p.grad = torch.zeros_like(p)


def _equal_everywhere(oa, ob, what):
    for ga, gb in zip(_groups(oa), _groups(ob)):
        for p, q in zip(ga["params"], gb["params"]):
            assert _same_bits(p, q), (what, ga["name"], "parameter")
            sa, sb = _state(oa, p), _state(ob, q)
            for k in ("exp_avg", "exp_avg_sq"):
                assert _same_bits(sa[k], sb[k]), (what, ga["name"], k)


def _state(opts, p):
    return next(o.state[p] for o in opts if p in o.state)


def _same_bits(a, b):
    """Bit-equal, NaN positions (and payloads) included."""
    a, b = a.detach().contiguous().cpu(), b.detach().contiguous().cpu()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 1. the factors --------------------------------------------------------------------------------------------------------
def test_factors_are_the_host_expressions_bit_for_bit(hip_device):
    """Two (betas, eps) classes x (exponential, constant, multiplicative) rates, horizon 40: after each of the 40 prologue
    launches the factor array holds the bits of lr / (1.0 - b1 ** t) and math.sqrt(1.0 - b2 ** t) passed through a C float --
    i.e. the double quotient on the device is the correctly rounded one, and its conversion rounds to nearest even."""
    dev = hip_device
    ps = [torch.randn(3, device=dev).requires_grad_(True) for _ in range(6)]
    fns = [get_expon_lr_func(8e-4, 8e-6, max_steps=30), None, MultiplicativeLR(1e-4, 0.01 ** (1 / 40)),
           get_expon_lr_func(1.6e-4, 1.6e-6, 10, 0.01, 35), None, MultiplicativeLR(3e-3, 0.1 ** (1 / 7))]
    const = [None, 2.5e-3, None, None, 1.0 / 3.0, None]
    groups = [{"params": [p], "lr": const[i] or 1.0, "betas": CLASSES[i // 3][0], "eps": CLASSES[i // 3][1], "name": f"g{i}"}
              for i, p in enumerate(ps)]
    opt = torch.optim.Adam(groups, lr=0.0)
    _persistent_grads(ps)
    adam = DeviceAdam([opt], {(opt, f"g{i}"): fn for i, fn in enumerate(fns) if fn is not None}, horizon=40)
    assert adam.counters().tolist() == [1] + [0] * 6
    for it in range(1, 41):
        for p in ps:
            p.grad.normal_()
        adam.step()
        got = adam.factors().numpy().view(np.uint32)
        t = float(it)
        for i in range(6):
            b1, b2 = CLASSES[i // 3][0]
            lr = float(fns[i](it)) if fns[i] is not None else const[i]
            want = (_f32_bits(lr / (1.0 - b1 ** t)), _f32_bits(math.sqrt(1.0 - b2 ** t)))
            assert (int(got[i, 0]), int(got[i, 1])) == want, (it, i, got[i].tolist(), want)
    assert adam.counters().tolist() == [41] + [40] * 6


# ---- 2. the update kernel's paths ------------------------------------------------------------------------------------------
def test_vector_body_scalar_tail_misaligned_views_and_an_empty_tensor(hip_device):
    dev = hip_device
    g = torch.Generator().manual_seed(2)
    shapes = [(1,), (3,), (4,), (5,), (1023,), (1024,), (1025,), (4099,), (1025, 3), (7, 0, 3)]
    init = [torch.randn(*s, generator=g) for s in shapes] + [torch.randn(1027, generator=g), torch.randn(1027, generator=g)]
    pa = [t.to(dev).requires_grad_(True) for t in init[:len(shapes)]]
    pbase = torch.full((1029,), 7.0, device=dev)                     # a parameter 4 bytes off a 16-byte boundary
    pbase[1:1028] = init[-2].to(dev)
    pa.append(pbase[1:1028].detach().requires_grad_(True))
    pa.append(init[-1].to(dev).requires_grad_(True))                 # an aligned parameter whose gradient is 4 bytes off
    gbase = torch.full((1029,), 7.0, device=dev)
    pb = [t.to(dev).requires_grad_(True) for t in init]
    _persistent_grads(pa)
    _persistent_grads(pb)
    pa[-1].grad = gbase[1:1028]
    assert pa[-2].is_contiguous() and pa[-2].data_ptr() % 16 == 4 and pa[-1].grad.data_ptr() % 16 == 4
    n = len(pa)
    lrs = [1e-3 * (1 + i % 5) for i in range(n)]
    hyper = lambda i: CLASSES[i % 2]  # noqa: E731
    oa, ob = _twin_optimisers(pa, pb, lrs, hyper)
    fns = [get_expon_lr_func(1e-2, 1e-4, max_steps=12) if i % 3 == 0 else
           (MultiplicativeLR(lrs[i], 0.8) if i % 3 == 1 else None) for i in range(n)]
    adam = DeviceAdam(oa, [(ga, fn) for ga, fn in zip(_groups(oa), fns) if fn is not None], horizon=12)
    for it in range(1, 13):
        for p, q in zip(pa, pb):
            gr = (torch.randn(p.shape, generator=g) * (10.0 ** (it % 3 - 1))).to(dev)
            p.grad.copy_(gr)
            q.grad.copy_(gr)
        adam.step()
        _set_rates(ob, fns, it)
        assert fused_adam_step(ob) == n
        _equal_everywhere(oa, ob, f"step {it}")
        assert pbase[[0, 1028]].tolist() == [7.0, 7.0] and gbase[[0, 1028]].tolist() == [7.0, 7.0]
    adam.sync_to_host()
    for ga, gb in zip(_groups(oa), _groups(ob)):
        assert float(oa[0].state[ga["params"][0]]["step"]) == float(ob[0].state[gb["params"][0]]["step"]) == 12.0
        assert ga["lr"] == gb["lr"], ga["name"]


# ---- 3. more tensors than the old launch took --------------------------------------------------------------------------------
def test_130_tensors_two_optimisers_both_classes(hip_device):
    dev = hip_device
    g = torch.Generator().manual_seed(130)
    lengths = [1 + (i * 1999) % 5000 for i in range(130)]
    hyper = lambda i: CLASSES[1] if i % 13 < 3 else CLASSES[0]  # noqa: E731
    init = [torch.randn(n, generator=g) for n in lengths]
    pa = [t.to(dev).requires_grad_(True) for t in init]
    pb = [t.to(dev).requires_grad_(True) for t in init]
    _persistent_grads(pa)
    _persistent_grads(pb)
    oa, ob = _twin_optimisers(pa, pb, [1e-3 * (1 + i % 7) for i in range(130)], hyper, split=65)
    fns = [get_expon_lr_func(1e-3, 1e-5, max_steps=3) if i % 4 == 0 else None for i in range(130)]
    adam = DeviceAdam(oa, [(ga, fn) for ga, fn in zip(_groups(oa), fns) if fn is not None], horizon=3)
    for it in range(1, 4):
        for p, q in zip(pa, pb):
            gr = torch.randn(p.shape, generator=g).to(dev)
            p.grad.copy_(gr)
            q.grad.copy_(gr)
        adam.step()
        _set_rates(ob, fns, it)
        assert fused_adam_step(ob) == 130
        _equal_everywhere(oa, ob, f"step {it}")
    assert adam.counters().tolist() == [4] + [3] * 130


# ---- 4. non-finite gradients -----------------------------------------------------------------------------------------------
def test_numeric_edges_and_non_finite_gradients(hip_device):
    """The gradients of test_gpu_optim.test_fused_adam_numeric_edges_at_eps_1e_15, in the float4 body and in the tail."""
    dev = hip_device
    n = 1027
    g = torch.Generator().manual_seed(15)
    sign = lambda: torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)  # noqa: E731
    mixed = torch.randn(n, generator=g)
    mixed[[0, 5, 1024]], mixed[[2, 1025]], mixed[[7, 1026]] = float("inf"), float("-inf"), float("nan")
    kinds = {"zero": lambda: torch.zeros(n), "1e-30": lambda: 1e-30 * sign(), "1e20": lambda: 1e20 * sign(),
             "1e21": lambda: 1e21 * sign(), "inf and NaN": lambda: mixed * sign()}
    init = [torch.randn(n, generator=g) for _ in kinds]
    pa = [t.to(dev).requires_grad_(True) for t in init]
    pb = [t.to(dev).requires_grad_(True) for t in init]
    _persistent_grads(pa)
    _persistent_grads(pb)
    oa, ob = _twin_optimisers(pa, pb, [1e-2] * len(kinds), lambda i: CLASSES[0])
    adam = DeviceAdam(oa, None, horizon=3)
    for it in range(1, 4):
        for p, q, make in zip(pa, pb, kinds.values()):
            gr = make().to(dev)
            p.grad.copy_(gr)
            q.grad.copy_(gr)
        adam.step()
        assert fused_adam_step(ob) == len(kinds)
        _equal_everywhere(oa, ob, f"step {it}")
    assert torch.equal(pa[0].detach().cpu(), init[0])
    assert bool(torch.isnan(pa[4]).any()) and bool(torch.isinf(oa[0].state[pa[2]]["exp_avg_sq"]).all())


# ---- 5. inside a graph -----------------------------------------------------------------------------------------------------
def test_step_recorded_into_a_graph_follows_the_eager_loop(hip_device):
    from mobgs_amd.graphed import GraphedCallable
    dev = hip_device
    g = torch.Generator().manual_seed(5)
    shapes = [(257, 3), (1030,), (6, 12), (5,)]
    init = [torch.randn(*s, generator=g) for s in shapes]
    targets = [torch.randn(*s, generator=g).to(dev) for s in shapes]
    pa = [t.to(dev).requires_grad_(True) for t in init]
    pb = [t.to(dev).requires_grad_(True) for t in init]
    _persistent_grads(pa)
    _persistent_grads(pb)
    oa, ob = _twin_optimisers(pa, pb, [1e-2, 2e-2, 5e-3, 1e-2], lambda i: CLASSES[i % 2])
    fns = [get_expon_lr_func(5e-2, 5e-4, max_steps=10), None, MultiplicativeLR(5e-3, 0.7), None]
    adam = DeviceAdam(oa, [(ga, fn) for ga, fn in zip(_groups(oa), fns) if fn is not None], horizon=10)

    def fill(ps):
        with torch.no_grad():
            for p, t in zip(ps, targets):
                p.grad.copy_(2 * (p - t))

    def iteration():
        fill(pa)
        adam.step()

    fb = GraphedCallable(iteration, warmup=0)
    first = None
    for it in range(1, 11):
        fb()
        adam.after_replay()
        if it == 1:
            first = adam.factors()
        fill(pb)
        _set_rates(ob, fns, it)
        assert fused_adam_step(ob) == 4
        _equal_everywhere(oa, ob, f"replay {it}")
    last = adam.factors()
    assert adam.counters().tolist() == [11, 10, 10, 10, 10] and adam.iteration == 11
    assert not torch.equal(first, last)
    # the scheduled rate moved between the replays -- a host scalar frozen at capture time could not
    b1 = CLASSES[0][0][0]
    assert int(last.numpy().view(np.uint32)[0, 0]) == _f32_bits(float(fns[0](10)) / (1.0 - b1 ** 10.0))
    assert fns[0](10) != fns[0](1)


# ---- 6. a tensor that joins late ---------------------------------------------------------------------------------------------
def test_late_joiner_and_missing_gradient(hip_device):
    dev = hip_device
    g = torch.Generator().manual_seed(6)
    init = [torch.randn(n, generator=g) for n in (300, 1025, 40)]
    pa = [t.to(dev).requires_grad_(True) for t in init]
    pb = [t.to(dev).requires_grad_(True) for t in init]
    _persistent_grads(pa[:2])
    _persistent_grads(pb[:2])
    oa, ob = _twin_optimisers(pa, pb, [1e-2, 2e-2, 5e-3], lambda i: CLASSES[0])
    fns = [get_expon_lr_func(1e-2, 1e-4, max_steps=6), None, get_expon_lr_func(5e-3, 5e-5, max_steps=6)]
    adam = DeviceAdam(oa, [(ga, fn) for ga, fn in zip(_groups(oa), fns) if fn is not None], horizon=6)

    def steps(its, live):
        for it in its:
            for p, q in zip(pa[:live], pb[:live]):
                gr = torch.randn(p.shape, generator=g).to(dev)
                p.grad.copy_(gr)
                q.grad.copy_(gr)
            adam.step()
            _set_rates(ob, fns, it)
            assert fused_adam_step(ob) == live

    steps(range(1, 4), 2)
    assert torch.equal(pa[2].detach().cpu(), init[2]) and len(oa[0].state[pa[2]]) == 0      # untouched, no step counted
    assert adam.counters().tolist() == [4, 3, 3]
    _persistent_grads(pa[2:])
    _persistent_grads(pb[2:])
    adam.rebuild()
    assert adam.counters().tolist() == [4, 3, 3, 0]                # the others continue, the joiner starts at t = 1
    steps(range(4, 7), 3)
    adam.sync_to_host()
    for p, q, want in zip(pa, pb, (6.0, 6.0, 3.0)):
        sa, sb = oa[0].state[p], ob[0].state[q]
        assert float(sa["step"]) == float(sb["step"]) == want
        assert _same_bits(p, q) and _same_bits(sa["exp_avg"], sb["exp_avg"]) and _same_bits(sa["exp_avg_sq"], sb["exp_avg_sq"])
    assert [ga["lr"] for ga in _groups(oa)] == [gb["lr"] for gb in _groups(ob)]


def test_a_replaced_gradient_is_refused_with_the_advice_to_rebuild(hip_device):
    p = torch.randn(10, device=hip_device, requires_grad=True)
    p.grad = torch.zeros_like(p)
    opt = torch.optim.Adam([{"params": [p], "lr": 1e-2, "name": "p"}], eps=1e-15)
    adam = DeviceAdam([opt], None, horizon=5)
    adam.step()
    before = p.detach().clone()
    p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="rebuild"):
        adam.step()
    assert torch.equal(p.detach(), before) and adam.counters().tolist() == [2, 1]


def test_what_the_kernel_does_not_cover_raises_at_build(hip_device):
    p = torch.randn(10, device=hip_device).half().requires_grad_(True)
    p.grad = torch.zeros_like(p)
    with pytest.raises(RuntimeError, match="cannot go through the kernel"):
        DeviceAdam([torch.optim.Adam([{"params": [p], "lr": 1e-2, "name": "half"}])], None, horizon=5)
    q = torch.randn(10, device=hip_device, requires_grad=True)
    q.grad = torch.zeros_like(q)
    with pytest.raises(RuntimeError, match="cannot go through the kernel"):
        DeviceAdam([torch.optim.Adam([{"params": [q], "lr": 1e-2, "weight_decay": 0.1, "name": "decayed"}])], None, horizon=5)


# ---- 7. the horizon --------------------------------------------------------------------------------------------------------
def test_stepping_past_the_horizon_raises_before_any_launch(hip_device):
    p = torch.randn(100, device=hip_device, requires_grad=True)
    p.grad = torch.ones_like(p)
    opt = torch.optim.Adam([{"params": [p], "lr": 1e-2, "name": "xyz"}], eps=1e-15)
    adam = DeviceAdam([opt], {(opt, "xyz"): get_expon_lr_func(1e-2, 1e-4, max_steps=3)}, horizon=3)
    for _ in range(3):
        adam.step()
    before, m = p.detach().clone(), opt.state[p]["exp_avg"].clone()
    with pytest.raises(RuntimeError, match="horizon"):
        adam.step()
    assert torch.equal(p.detach(), before) and torch.equal(opt.state[p]["exp_avg"], m)
    assert adam.counters().tolist() == [4, 3]
    with pytest.raises(ValueError):
        DeviceAdam([opt], None, horizon=3, first_iteration=4)


# ---- 8. the per-splat table through resizes ----------------------------------------------------------------------------------
class _Opt:
    percent_dense = 0.01
    position_lr_init, position_lr_final, position_lr_max_steps = 0.00016, 0.0000016, 20
    feature_lr = 0.0025
    featuret_lr = 0.001
    opacity_lr = 0.05
    scaling_lr = 0.005
    rotation_lr = 0.001
    omega_lr = 0.0001
    zeta_lr = 0.0001
    trbfc_lr = 0.0001
    trbfs_lr = 0.03
    movelr = 3.5
    rgb_lr = 0.0001


EXTENT = 4.0
SIZE_THR = _Opt.percent_dense * EXTENT


def _synthetic_table(n, dev, seed):
    from mobgs_amd.densify import TrainableGaussians
    torch.manual_seed(seed)                                  # (the decoder's initial weights: the same on both twins)
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(n, *s, generator=g)  # noqa: E731
    u = lambda *s: torch.rand(n, *s, generator=g)  # noqa: E731
    top = torch.where(u() < 0.4, math.log(SIZE_THR) + 0.2 + 2.0 * u(), math.log(SIZE_THR) - 0.2 - 2.0 * u())
    scaling = top[:, None] - 2.0 * u(3)
    scaling[torch.arange(n), torch.randint(0, 3, (n,), generator=g)] = top     # both sides of the size threshold
    params = {"xyz": 3.0 * r(3), "scaling": scaling, "rotation": r(4), "opacity": r(1), "features_dc": r(6),
              "features_t": r(3)}
    dyn = {"omega": 0.1 * r(4), "trbf_center": u(1), "control_xyz": 100.0 * r(12, 3),
           "current_control_num": torch.randint(4, 13, (n, 1), generator=g), "f_rest": torch.zeros(n, 0, 3),
           "zeta": 0.1 * r(1), "trbf_scale": 0.1 * r(1), "motion": 0.1 * r(9), "_deformation_table": u() > 0.3}
    pc = TrainableGaussians(params, dyn, device=dev)
    pc.training_setup(_Opt())
    pc.setup_schedules(_Opt())
    return pc


def _give_gradients(pcs, g):
    """The same fresh (then persistent) gradient tensors on both tables, for every parameter with elements."""
    for groups in zip(*[pc.optimizer.param_groups for pc in pcs]):
        for ps in zip(*[gr["params"] for gr in groups]):
            if ps[0].requires_grad and ps[0].numel():
                gr = (0.01 * torch.randn(ps[0].shape, generator=g)).to(ps[0].device)
                for p in ps:
                    p.grad = gr.clone()


def _tables_equal(a, b, what):
    sa, sb = a.table_state(), b.table_state()
    assert set(sa) == set(sb) and any(k.endswith(".exp_avg_sq") for k in sa), what
    for k in sa:
        assert sa[k].shape == sb[k].shape and torch.equal(sa[k], sb[k]), (what, k)


def test_real_table_through_densification_and_pruning(hip_device):
    dev = hip_device
    a, b = _synthetic_table(3000, dev, 3000), _synthetic_table(3000, dev, 3000)
    g = torch.Generator().manual_seed(88)
    _give_gradients((a, b), g)
    adam = DeviceAdam([a.optimizer], a.schedules(), horizon=10)
    assert len(a.schedules()) == 1

    def step(it):
        adam.step()
        b.update_learning_rate(it)
        b.optimizer.step()
        _tables_equal(a, b, f"step {it}")

    step(1)
    # densify_pruneclone on statistics that make 30 % of the rows hot, with given samples (as test_gpu_optim._densify)
    n = a.get_xyz.shape[0]
    denom = torch.randint(0, 4, (n, 1), generator=g).float()
    accum = torch.where(torch.rand(n, 1, generator=g) < 0.3, 2.0, 0.5) * 2.0e-4 * denom
    for pc in (a, b):
        pc.xyz_gradient_accum.copy_(accum.to(dev))
        pc.denom.copy_(denom.to(dev))
        s = pc.table_state()["scaling"]
        near = ((torch.exp(s.double()).max(dim=1).values - SIZE_THR).abs() <= 1e-3 * SIZE_THR)
        s[near] += 0.01
    pre = {k: v.detach().cpu().clone() for k, v in a.table_state().items()}
    _, split = R.select(pre["scaling"], R.mean_grads(pre["xyz_gradient_accum"], pre["denom"]), 2.0e-4, SIZE_THR)
    parents = torch.nonzero(split).reshape(-1).repeat(2)
    samples = torch.randn(parents.shape[0], 3, generator=g) * torch.exp(pre["scaling"][parents])
    for pc in (a, b):
        pc.densify_pruneclone(2.0e-4, 0.005, EXTENT, None, 2, samples=samples.to(dev))
    assert a.get_xyz.shape[0] == b.get_xyz.shape[0] > 3000
    _give_gradients((a, b), g)
    adam.rebuild()
    step(2)
    mask = (torch.rand(a.get_xyz.shape[0], generator=g) < 0.2).to(dev)
    for pc in (a, b):
        pc.prune_points(mask)
    assert a.get_xyz.shape[0] == b.get_xyz.shape[0] > 2048
    _give_gradients((a, b), g)
    adam.rebuild()
    step(3)
    adam.sync_to_host()
    for ga, gb in zip(a.optimizer.param_groups, b.optimizer.param_groups):
        assert ga["lr"] == gb["lr"], ga["name"]
        sa, sb = a.optimizer.state.get(ga["params"][0]), b.optimizer.state.get(gb["params"][0])
        assert (sa is None) == (sb is None) and (sa is None or float(sa["step"]) == float(sb["step"])), ga["name"]


# ---- 9. the caches keyed on Tensor._version ----------------------------------------------------------------------------------
class _DeformArgs:
    net_width, timebase_pe, defor_depth, posebase_pe, scale_rotation_pe, opacity_pe = 128, 4, 1, 10, 2, 2
    timenet_width, timenet_output, bounds, grid_pe = 64, 32, 1.6, 0
    kplanes_config = {"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 32,
                      "resolution": [8, 8, 8, 4]}
    multires = [1, 2, 4]
    no_dx = no_grid = no_ds = no_dr = empty_voxel = static_mlp = apply_rotation = False
    no_do = no_dshs = True


def test_deform_network_sees_the_weights_a_replayed_step_wrote(hip_device):
    from mobgs_amd import deformation
    from mobgs_amd.graphed import GraphedCallable
    dev = hip_device
    torch.manual_seed(11)
    net = deformation.deform_network(_DeformArgs()).to(dev)
    g = torch.Generator().manual_seed(12)
    pts = (2.0 * torch.rand(200, 3, generator=g) - 1.0).to(dev)
    scales, rots = torch.randn(200, 3, generator=g).to(dev), torch.randn(200, 4, generator=g).to(dev)
    times = torch.rand(200, 1, generator=g).to(dev)
    opt = torch.optim.Adam([{"params": net.get_mlp_parameters(), "lr": 1e-2, "name": "deformation"}], lr=0.0, eps=1e-15)
    deformation.invalidate_packed_weights()
    first = net(pts, scales, rots, times)
    sum((o * o).sum() for o in first).backward()
    first = [o.detach().clone() for o in first]
    adam = DeviceAdam([opt], {(opt, "deformation"): get_expon_lr_func(1e-2, 1e-3, max_steps=5)}, horizon=5)
    stepped = [p for p in opt.param_groups[0]["params"] if p.grad is not None]
    assert stepped
    fb = GraphedCallable(adam.step, warmup=0)
    before = [p._version for p in stepped]
    fb()
    adam.after_replay()
    assert all(p._version > v for p, v in zip(stepped, before))
    with torch.no_grad():
        second = [o.clone() for o in net(pts, scales, rots, times)]
        deformation.invalidate_packed_weights()
        fresh = [o.clone() for o in net(pts, scales, rots, times)]
    for x, y in zip(second, fresh):
        assert torch.equal(x, y), "deform_network evaluated stale packed weights after a replayed DeviceAdam step"
    assert not torch.equal(second[0], first[0])


# ---- the example's loop ------------------------------------------------------------------------------------------------------
def test_graph_optimizer_loop_gives_the_scheduled_eager_loops_history(hip_device):
    """examples/train_deblur_synth.py: forward, backward AND the step in one graph against the same loop run eagerly with
    update_learning_rate + fused_adam_step + adjust_lr (lambda_flow = 0: every kernel of the iteration is deterministic)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_deblur_synth as T
    kw = dict(dev=str(hip_device), iters=8, ns=3000, nd=1500, width=192, height=144, seed=2, lambda_flow=0.0)
    eager, stat_e, dyn_e, blce_e, _ = T.train(lr_schedule=True, **kw)
    graphed, stat_g, dyn_g, blce_g, _ = T.train(graph=True, graph_optimizer=True, **kw)
    assert eager == graphed, (eager, graphed)
    assert torch.equal(stat_e._xyz, stat_g._xyz) and torch.equal(dyn_e.control_xyz, dyn_g.control_xyz)
    for ge, gg in zip(stat_e.optimizer.param_groups + dyn_e.optimizer.param_groups,
                      stat_g.optimizer.param_groups + dyn_g.optimizer.param_groups):
        assert ge["lr"] == gg["lr"], ge["name"]
    xyz = next(gr for gr in stat_g.optimizer.param_groups if gr["name"] == "xyz")
    assert float(stat_g.optimizer.state[xyz["params"][0]]["step"]) == 8.0 and xyz["lr"] == stat_g.xyz_scheduler_args(8)
