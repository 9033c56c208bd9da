"""mobgs_amd.optim.fused_adam_step against torch.optim.Adam (the reference's optimiser, train.py:790-807)."""
import pytest
import torch

import densify_restatement as R

pytestmark = pytest.mark.gpu


def test_fused_adam_matches_torch_adam(hip_device):
    from mobgs_amd.optim import fused_adam_step
    dev = hip_device
    g = torch.Generator().manual_seed(3)
    shapes = [(1000, 3), (1000, 4), (1000, 1), (777, 12, 3), (6, 12), (5,), (1,), (333, 6)]
    lrs = [1.6e-4, 1e-3, 5e-2, 5.6e-4, 1e-4, 2.5e-3, 1e-3, 3e-2]

    def make():
        ps = [torch.randn(*s, generator=g).to(dev).requires_grad_(True) for s in shapes]
        return ps

    torch.manual_seed(0)
    pa = make()
    pb = [p.detach().clone().requires_grad_(True) for p in pa]
    # two optimisers with one-tensor groups, as the reference builds them; eps = 1e-15 (gaussian_model.py:645)
    oa = [torch.optim.Adam([{"params": [p], "lr": lr, "name": str(i)} for i, (p, lr) in enumerate(zip(ps, lrs[:len(ps)]))],
                           lr=0.0, eps=1e-15) for ps in (pa[:5], pa[5:])]
    ob = [torch.optim.Adam([{"params": [p], "lr": lr, "name": str(i)} for i, (p, lr) in enumerate(zip(ps, lrs[:len(ps)]))],
                           lr=0.0, eps=1e-15) for ps in (pb[:5], pb[5:])]
    for it in range(7):
        grads = [torch.randn(*s, generator=g).to(dev) * (10.0 ** (it % 3 - 1)) for s in shapes]
        for p, q, gr in zip(pa, pb, grads):
            p.grad, q.grad = gr.clone(), gr.clone()
        if it == 3:  # a parameter without a gradient is left alone by both
            pa[2].grad = pb[2].grad = None
        for o in oa:
            o.step()
        assert fused_adam_step(ob) == (len(shapes) - (1 if it == 3 else 0))
        for i, (p, q) in enumerate(zip(pa, pb)):
            # one ulp of the parameter (fp32 contraction of a + alpha * (b / c) may differ between the two kernels)
            assert torch.allclose(q.detach(), p.detach(), rtol=2e-6, atol=2e-7), (it, i, float((p - q).abs().max()))
    for o1, o2 in zip(oa, ob):
        for g1, g2 in zip(o1.param_groups, o2.param_groups):
            s1, s2 = o1.state[g1["params"][0]], o2.state[g2["params"][0]]
            assert float(s1["step"]) == float(s2["step"])
            assert torch.allclose(s2["exp_avg"], s1["exp_avg"], rtol=2e-6, atol=2e-7 * float(s1["exp_avg"].abs().max()))
            assert torch.allclose(s2["exp_avg_sq"], s1["exp_avg_sq"], rtol=2e-6,
                                  atol=2e-7 * float(s1["exp_avg_sq"].abs().max()))


def test_fused_adam_falls_back_for_what_it_does_not_cover(hip_device):
    from mobgs_amd.optim import fused_adam_step
    dev = hip_device
    p32 = torch.randn(50, device=dev, requires_grad=True)
    p16 = torch.randn(50, device=dev).half().requires_grad_(True)
    ref32, ref16 = p32.detach().clone().requires_grad_(True), p16.detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([{"params": [p32], "lr": 1e-2}, {"params": [p16], "lr": 1e-2}], eps=1e-8)
    ref = torch.optim.Adam([{"params": [ref32], "lr": 1e-2}, {"params": [ref16], "lr": 1e-2}], eps=1e-8)
    for _ in range(3):
        g32, g16 = torch.randn(50, device=dev), torch.randn(50, device=dev).half()
        p32.grad, ref32.grad, p16.grad, ref16.grad = g32.clone(), g32.clone(), g16.clone(), g16.clone()
        assert fused_adam_step([opt]) == 1      # the fp32 tensor; the half one goes through torch's own step
        ref.step()
    assert torch.allclose(p32.detach(), ref32.detach(), rtol=2e-6, atol=2e-7)
    assert torch.equal(p16, ref16)


def test_fused_adam_optimizer_class_is_a_drop_in_for_torch_adam(hip_device):
    """optim.FusedAdam -- what TrainableGaussians.training_setup() / blceKernel hand to an unchanged train.py loop
    (`optimizer.step()`, /root/reference/train.py:790-807): torch.optim.Adam's update through ONE launch, torch's own step
    for what the kernel does not cover (a half tensor here), state_dict round trip, zero_grad / param-group edits as usual."""
    from mobgs_amd.optim import FusedAdam
    dev = hip_device
    g = torch.Generator().manual_seed(5)
    shapes = [(500, 3), (500, 12, 3), (6, 12), (40,)]
    pa = [torch.randn(*s, generator=g).to(dev).requires_grad_(True) for s in shapes]
    pa[3] = pa[3].detach().half().requires_grad_(True)
    pb = [p.detach().clone().requires_grad_(True) for p in pa]
    groups = lambda ps: [{"params": [p], "lr": 1e-3 * (i + 1), "name": str(i)} for i, p in enumerate(ps)]  # noqa: E731
    ref, opt = torch.optim.Adam(groups(pa), lr=0.0, eps=1e-15), FusedAdam(groups(pb), lr=0.0, eps=1e-15)
    assert isinstance(opt, torch.optim.Adam)
    for it in range(5):
        for p, q in zip(pa, pb):
            gr = torch.randn(p.shape, generator=g).to(dev).to(p.dtype)
            p.grad, q.grad = gr.clone(), gr.clone()
        ref.step()
        opt.step()
        if it == 2:   # what densification / schedulers do between steps
            for o in (ref, opt):
                o.param_groups[0]["lr"] *= 0.5
            sd = opt.state_dict()
            opt.load_state_dict(sd)
        for i, (p, q) in enumerate(zip(pa, pb)):
            assert torch.allclose(q.detach().float(), p.detach().float(), rtol=2e-6, atol=2e-7 if i < 3 else 1e-3), (it, i)
    opt.zero_grad(set_to_none=True)
    assert all(q.grad is None for q in pb)
    assert float(opt.state[pb[0]]["step"]) == 5.0 and float(opt.state[pb[3]]["step"]) == 5.0


# ---- the kernel's own paths: float4 body, scalar tail, misaligned pointers, chunks of 64, several batches ------------------
def _close_with_same_nonfinite(got, ref, what, atol_scale=None):
    """Same NaN / +inf / -inf pattern; the finite values within the tolerances of this file (moments: atol scaled by their
    largest finite magnitude)."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), (what, "NaN pattern")
    inf = torch.isinf(ref)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], ref[inf]), (what, "inf pattern")
    fin = torch.isfinite(ref)
    scale = 1.0 if atol_scale is None else (float(ref[fin].abs().max()) if bool(fin.any()) else 0.0)
    assert torch.allclose(got[fin], ref[fin], rtol=2e-6, atol=2e-7 * scale), \
        (what, float((got[fin] - ref[fin]).abs().max()) if bool(fin.any()) else 0.0)


def _close_states(ref_opt, p, opt, q, what):
    s1, s2 = ref_opt.state[p], opt.state[q]
    assert float(s1["step"]) == float(s2["step"]), what
    _close_with_same_nonfinite(s2["exp_avg"], s1["exp_avg"], what + " exp_avg", atol_scale=True)
    _close_with_same_nonfinite(s2["exp_avg_sq"], s1["exp_avg_sq"], what + " exp_avg_sq", atol_scale=True)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 1024, 1025, 1027, 4099])
def test_fused_adam_vector_body_scalar_tail_and_misaligned_pointers(hip_device, n):
    """A fresh tensor takes the float4 body and, when n is no multiple of 4, the scalar tail next to it; base[1:1 + n] is
    contiguous with its pointer 4 bytes off a 16-byte boundary, so the whole tensor takes the scalar path -- as parameter,
    and as gradient under an aligned parameter.  The elements around the misaligned view stay what they were."""
    from mobgs_amd.optim import fused_adam_step
    dev = hip_device
    g = torch.Generator().manual_seed(40 + n)
    for variant in ("aligned", "parameter off by 4 bytes", "gradient off by 4 bytes"):
        init = torch.randn(n, generator=g)
        p = init.to(dev).requires_grad_(True)
        base = torch.full((n + 2,), 7.0, device=dev)
        if variant == "parameter off by 4 bytes":
            base[1:1 + n] = init.to(dev)
            q = base[1:1 + n].detach().requires_grad_(True)
            assert q.is_contiguous() and q.data_ptr() % 16 == 4
        else:
            q = init.to(dev).requires_grad_(True)
            assert q.data_ptr() % 16 == 0
        ref = torch.optim.Adam([{"params": [p], "lr": 1e-2}], eps=1e-15)
        opt = torch.optim.Adam([{"params": [q], "lr": 1e-2}], eps=1e-15)
        for it in range(4):
            gr = (torch.randn(n, generator=g) * (10.0 ** (it % 3 - 1))).to(dev)
            p.grad = gr.clone()
            if variant == "gradient off by 4 bytes":
                gbase = torch.full((n + 2,), 7.0, device=dev)
                gbase[1:1 + n] = gr
                q.grad = gbase[1:1 + n]
                assert q.grad.is_contiguous() and q.grad.data_ptr() % 16 == 4
            else:
                q.grad = gr.clone()
            ref.step()
            assert fused_adam_step([opt]) == 1
            assert torch.allclose(q.detach(), p.detach(), rtol=2e-6, atol=2e-7), (n, variant, it,
                                                                                 float((p - q).abs().max()))
            if variant == "gradient off by 4 bytes":
                assert gbase[[0, n + 1]].tolist() == [7.0, 7.0] and torch.equal(gbase[1:1 + n], gr)
        _close_states(ref, p, opt, q, f"n={n} {variant}")
        if variant == "parameter off by 4 bytes":
            assert base.detach()[[0, n + 1]].tolist() == [7.0, 7.0]


def test_fused_adam_130_tensors_in_chunks_and_batches(hip_device):
    """130 one-tensor groups over two optimisers with two (betas, eps) pairs: 100 + 30 tensors, i.e. launches of 64, 36 and
    30 tensors; lengths from 1 to 5000 in no order, because the grid is sized by the longest tensor of a launch."""
    from mobgs_amd.optim import fused_adam_step
    dev = hip_device
    g = torch.Generator().manual_seed(130)
    lengths = [1 + (i * 1999) % 5000 for i in range(130)]
    lengths[17], lengths[70], lengths[99], lengths[129] = 5000, 1, 4099, 5000
    assert min(lengths) == 1 and max(lengths) == 5000 and len(set(lengths)) > 100
    hyper = lambda i: ((0.8, 0.99), 1e-8) if i % 13 < 3 else ((0.9, 0.999), 1e-15)  # noqa: E731
    assert sum(1 for i in range(130) if i % 13 < 3) == 30
    pa = [torch.randn(n, generator=g).to(dev).requires_grad_(True) for n in lengths]
    pb = [p.detach().clone().requires_grad_(True) for p in pa]

    def optimisers(ps):
        groups = [{"params": [p], "lr": 1e-3 * (1 + i % 7), "betas": hyper(i)[0], "eps": hyper(i)[1]}
                  for i, p in enumerate(ps)]
        return [torch.optim.Adam(groups[:65], lr=0.0), torch.optim.Adam(groups[65:], lr=0.0)]

    oa, ob = optimisers(pa), optimisers(pb)
    for it in range(3):
        for p, q in zip(pa, pb):
            gr = torch.randn(p.shape, generator=g).to(dev)
            p.grad, q.grad = gr.clone(), gr.clone()
        for o in oa:
            o.step()
        assert fused_adam_step(ob) == 130
        for i, (p, q) in enumerate(zip(pa, pb)):
            assert torch.allclose(q.detach(), p.detach(), rtol=2e-6, atol=2e-7), (it, i, lengths[i],
                                                                                 float((p - q).abs().max()))
    for i, (p, q) in enumerate(zip(pa, pb)):
        _close_states(oa[i // 65], p, ob[i // 65], q, f"tensor {i}")


def test_fused_adam_numeric_edges_at_eps_1e_15(hip_device):
    """Zero gradients on fresh state (the parameter stays put: 0 / 1e-15), 1e-30 (g * g underflows to zero, exp_avg does
    not), 1e20 and 1e21 (g * g overflows: exp_avg_sq is inf and the parameter stays put, as in torch, whose multi-tensor
    addcmul forms grad * grad before it scales), and inf / -inf / NaN among ordinary values, in the float4 body and in
    the tail: the non-finite pattern is torch's, the finite values are within the tolerance."""
    from mobgs_amd.optim import fused_adam_step
    dev = hip_device
    n = 1027
    g = torch.Generator().manual_seed(15)
    sign = lambda: torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)  # noqa: E731
    mixed = torch.randn(n, generator=g)
    mixed[[0, 5, 1024]], mixed[[2, 1025]], mixed[[7, 1026]] = float("inf"), float("-inf"), float("nan")
    kinds = {"zero": lambda: torch.zeros(n), "1e-30": lambda: 1e-30 * sign(), "1e20": lambda: 1e20 * sign(),
             "1e21": lambda: 1e21 * sign(), "inf and NaN": lambda: mixed * sign()}
    init = {k: torch.randn(n, generator=g) for k in kinds}
    pa = {k: v.to(dev).requires_grad_(True) for k, v in init.items()}
    pb = {k: v.to(dev).requires_grad_(True) for k, v in init.items()}
    ref = torch.optim.Adam([{"params": [p], "lr": 1e-2} for p in pa.values()], lr=0.0, eps=1e-15)
    opt = torch.optim.Adam([{"params": [p], "lr": 1e-2} for p in pb.values()], lr=0.0, eps=1e-15)
    for it in range(3):
        for k, make in kinds.items():
            gr = make().to(dev)
            pa[k].grad, pb[k].grad = gr.clone(), gr.clone()
        ref.step()
        assert fused_adam_step([opt]) == len(kinds)
        for k in kinds:
            _close_with_same_nonfinite(pb[k], pa[k], f"{k} step {it}")
        assert torch.equal(pb["zero"].detach().cpu(), init["zero"])
    for k in kinds:
        _close_states(ref, pa[k], opt, pb[k], k)
    for k in ("1e20", "1e21"):
        assert bool(torch.isinf(opt.state[pb[k]]["exp_avg_sq"]).all()) and torch.equal(pb[k].detach().cpu(), init[k])
    m, v = opt.state[pb["1e-30"]]["exp_avg"], opt.state[pb["1e-30"]]["exp_avg_sq"]
    assert bool((m != 0).all()) and not bool(v.any())


# ---- the version counter (what deformation._packed, _lib.DerivedCache and blce.py key their caches on) --------------------
def test_fused_adam_moves_the_version_counter_of_what_it_wrote(hip_device):
    from mobgs_amd.optim import FusedAdam, fused_adam_step
    dev = hip_device
    for through_class in (True, False):
        ps = [torch.randn(n, device=dev, requires_grad=True) for n in (5, 1024, 3, 40)]
        groups = [{"params": [p], "lr": 1e-2} for p in ps]
        opt = FusedAdam(groups, lr=0.0, eps=1e-15) if through_class else torch.optim.Adam(groups, lr=0.0, eps=1e-15)
        for it in range(2):
            for p in ps[:3]:
                p.grad = torch.randn_like(p)
            before = [p._version for p in ps]
            if through_class:
                opt.step()
            else:
                assert fused_adam_step([opt]) == 3
            assert all(p._version > v for p, v in zip(ps[:3], before[:3])), (through_class, it)
            assert ps[3]._version == before[3]        # no gradient: not written, not moved


class _DeformArgs:
    net_width, timebase_pe, defor_depth, posebase_pe, scale_rotation_pe, opacity_pe = 128, 4, 1, 10, 2, 2
    timenet_width, timenet_output, bounds, grid_pe = 64, 32, 1.6, 0
    kplanes_config = {"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 32,
                      "resolution": [8, 8, 8, 4]}
    multires = [1, 2, 4]
    no_dx = no_grid = no_ds = no_dr = empty_voxel = static_mlp = apply_rotation = False
    no_do = no_dshs = True


def test_deform_network_sees_the_weights_fused_adam_stepped(hip_device):
    """The reference puts the deformation MLP into the optimiser training_setup() creates; deformation._packed keeps a
    re-laid-out copy of the weights keyed on their version counters."""
    from mobgs_amd import deformation
    from mobgs_amd.optim import FusedAdam
    dev = hip_device
    torch.manual_seed(11)
    net = deformation.deform_network(_DeformArgs()).to(dev)
    g = torch.Generator().manual_seed(12)
    pts = (2.0 * torch.rand(200, 3, generator=g) - 1.0).to(dev)
    scales, rots = torch.randn(200, 3, generator=g).to(dev), torch.randn(200, 4, generator=g).to(dev)
    times = torch.rand(200, 1, generator=g).to(dev)
    opt = FusedAdam([{"params": net.get_mlp_parameters(), "lr": 1e-2, "name": "deformation"}], lr=0.0, eps=1e-15)
    deformation.invalidate_packed_weights()
    first = net(pts, scales, rots, times)
    sum((o * o).sum() for o in first).backward()
    first = [o.detach().clone() for o in first]
    opt.step()
    with torch.no_grad():
        second = [o.clone() for o in net(pts, scales, rots, times)]
        deformation.invalidate_packed_weights()
        fresh = [o.clone() for o in net(pts, scales, rots, times)]
    for a, b in zip(second, fresh):
        assert torch.equal(a, b), "deform_network evaluated stale packed weights after FusedAdam.step()"
    assert not torch.equal(second[0], first[0])


def test_derived_cache_sees_a_tensor_fused_adam_stepped(hip_device):
    from mobgs_amd import _lib
    from mobgs_amd.optim import fused_adam_step
    dev = hip_device
    p = torch.randn(64, device=dev)            # (a source that requires grad is never cached)
    opt = torch.optim.Adam([{"params": [p], "lr": 1e-1}], eps=1e-15)
    cache = _lib.DerivedCache()
    build = lambda: p * 2.0  # noqa: E731
    first = cache.get((p,), build)
    assert cache.get((p,), build) is first
    p.grad = torch.randn(64, device=dev)
    assert fused_adam_step([opt]) == 1
    second = cache.get((p,), build)
    assert torch.equal(second, p * 2.0), "DerivedCache returned the value derived before fused_adam_step()"
    assert not torch.equal(second, first)


# ---- parameters and moments through resizes of a 3000-row table, against tests/densify_restatement.py ---------------------
class _Opt:
    percent_dense = 0.01
    position_lr_init = 0.00016
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
ID_ROW = 11   # the final control point carries the row's id in its three columns


def _synthetic_table(n, dev, seed):
    import math
    from mobgs_amd.densify import TrainableGaussians
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(n, *s, generator=g)  # noqa: E731
    u = lambda *s: torch.rand(n, *s, generator=g)  # noqa: E731
    control = 100.0 * r(12, 3)
    control[:, ID_ROW, :] = torch.arange(n, dtype=torch.float32)[:, None]
    top = torch.where(u() < 0.4, math.log(SIZE_THR) + 0.2 + 2.0 * u(), math.log(SIZE_THR) - 0.2 - 2.0 * u())
    scaling = top[:, None] - 2.0 * u(3)
    scaling[torch.arange(n), torch.randint(0, 3, (n,), generator=g)] = top     # both sides of the size threshold
    params = {"xyz": 3.0 * r(3), "scaling": scaling, "rotation": r(4), "opacity": r(1), "features_dc": r(6),
              "features_t": r(3)}
    dyn = {"omega": 0.1 * r(4), "trbf_center": u(1), "control_xyz": control,
           "current_control_num": torch.randint(4, 13, (n, 1), generator=g), "f_rest": torch.zeros(n, 0, 3),
           "zeta": 0.1 * r(1), "trbf_scale": 0.1 * r(1), "motion": 0.1 * r(9), "_deformation_table": u() > 0.3}
    pc = TrainableGaussians(params, dyn, device=dev)
    pc.training_setup(_Opt())
    return pc


def _step_against_torch_adam(pc, g):
    """One optimizer.step() with random gradients; every stepped parameter and its moments against a torch.optim.Adam
    stepping clones of the pre-step tensors and moments."""
    opt = pc.optimizer
    groups, pairs = [], []
    for gr in opt.param_groups:
        for p in gr["params"]:
            if not (p.requires_grad and p.numel()):
                continue
            p.grad = (0.01 * torch.randn(p.shape, generator=g)).to(p.device)
            q = p.detach().clone().requires_grad_(True)
            q.grad = p.grad.clone()
            groups.append({"params": [q], "lr": gr["lr"], "betas": gr["betas"], "eps": gr["eps"]})
            pairs.append((gr["name"], p, q))
    ref = torch.optim.Adam(groups, lr=0.0)
    for _, p, q in pairs:
        st = opt.state.get(p)
        if st is not None and "exp_avg" in st:
            ref.state[q] = {"step": torch.tensor(float(st["step"])), "exp_avg": st["exp_avg"].detach().clone(),
                            "exp_avg_sq": st["exp_avg_sq"].detach().clone()}
    versions = [p._version for _, p, _ in pairs]
    opt.step()
    ref.step()
    assert len(pairs) >= 13
    for (name, p, q), v in zip(pairs, versions):
        assert p._version > v, name
        assert torch.allclose(p.detach(), q.detach(), rtol=2e-6, atol=2e-7), (name, float((p - q).abs().max()))
        _close_states(ref, q, opt, p, name)


def _clear_of_the_size_threshold(pc):
    """Rows whose largest exp(scaling) lies within 1e-3 of the size threshold are moved off it (device expf against host
    exp must not decide a row); -> the table on the host, with the margin asserted on it."""
    s = pc.table_state()["scaling"]
    near = ((torch.exp(s.double()).max(dim=1).values - SIZE_THR).abs() <= 1e-3 * SIZE_THR)
    s[near] += 0.01
    state = {k: v.detach().cpu().clone() for k, v in pc.table_state().items()}
    assert R.size_margin(state["scaling"], SIZE_THR) > 1e-4
    return state


def _ordered_by_id(state, extra):
    """Rows of `state` (and of the per-row arrays `extra`) ordered by id, then by the first xyz moment (an original before
    its clone; bit-equal on both sides), then by x (the children of one parent)."""
    import numpy as np
    order = torch.from_numpy(np.lexsort((state["xyz"][:, 0].numpy(), state["xyz.exp_avg"][:, 0].numpy(),
                                         state["control_xyz"][:, ID_ROW, 0].numpy())))
    return {k: v[order] for k, v in state.items()}, [e[order] for e in extra]


def _check_resize(pc, want, as_multiset, children=None):
    """Every field of the table against the restatement's: bit-equal, except xyz / scaling of split children, which are
    held to densify_restatement.SPLIT_ALLOWED against the float64 children.  children: (first row, parents' rotation,
    xyz, scaling [n_children, .], samples, N)."""
    got = {k: v.detach().cpu().clone() for k, v in pc.table_state().items()}
    assert set(got) == set(want), set(got) ^ set(want)
    n = want["xyz"].shape[0]
    assert all(v.shape[0] == n for v in got.values())
    child = torch.zeros(n, dtype=torch.bool)
    ref_xyz, ref_scl = want["xyz"].double(), want["scaling"].double()
    den_xyz = torch.ones(n, 3, dtype=torch.float64)
    if children is not None:
        first, rot, xyz, scl, samples, N = children
        child[first:] = True
        ref_xyz[first:], ref_scl[first:] = R.split_children(rot, xyz, scl, samples, N)
        den_xyz[first:] = xyz.double().abs() + samples.double().abs().sum(1, keepdim=True)
    if as_multiset:
        got, _ = _ordered_by_id(got, [])
        want, (child, ref_xyz, ref_scl, den_xyz) = _ordered_by_id(want, [child, ref_xyz, ref_scl, den_xyz])
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        rows = ~child if k in ("xyz", "scaling") else slice(None)
        assert torch.equal(got[k][rows], want[k][rows]), k
        if k.endswith(".exp_avg") or k.endswith(".exp_avg_sq"):
            assert not bool(got[k][child].any()), (k, "a new row's moments are not zero")
    if children is not None:
        ex = float(((got["xyz"].double() - ref_xyz).abs() / den_xyz)[child].max())
        es = float(((got["scaling"].double() - ref_scl).abs() / (1.0 + ref_scl.abs()))[child].max())
        print(f"split children in the table: xyz {ex:.3e}, scaling {es:.3e} (allowed {R.SPLIT_ALLOWED})")
        assert ex <= R.SPLIT_ALLOWED[0] and es <= R.SPLIT_ALLOWED[1], (ex, es)


def _densify(pc, hot_fraction, N, g, as_multiset):
    """densify_pruneclone with given samples on statistics that make `hot_fraction` of the rows hot."""
    n = pc.get_xyz.shape[0]
    denom = torch.randint(0, 4, (n, 1), generator=g).float()
    accum = torch.where(torch.rand(n, 1, generator=g) < hot_fraction, 2.0, 0.5) * 2.0e-4 * denom
    pc.xyz_gradient_accum.copy_(accum.to(pc.xyz_gradient_accum.device))
    pc.denom.copy_(denom.to(pc.denom.device))
    pre = _clear_of_the_size_threshold(pc)
    _, split = R.select(pre["scaling"], R.mean_grads(pre["xyz_gradient_accum"], pre["denom"]), 2.0e-4, SIZE_THR)
    parents = torch.nonzero(split).reshape(-1).repeat(N)
    samples = torch.randn(parents.shape[0], 3, generator=g) * torch.exp(pre["scaling"][parents])
    lay = {}
    want = R.densify_pruneclone(pre, 2.0e-4, EXTENT, N, samples, percent_dense=_Opt.percent_dense, layout=lay)
    assert lay["clones"] > 100 and lay["children"] == parents.shape[0] > 100 and torch.equal(lay["parents"], parents)
    pc.densify_pruneclone(2.0e-4, 0.005, EXTENT, None, N, samples=samples.to(pc.get_xyz.device))
    _check_resize(pc, want, as_multiset, (lay["kept"] + lay["clones"], pre["rotation"][parents], pre["xyz"][parents],
                                          pre["scaling"][parents], samples, N))


@pytest.mark.parametrize("keep_sorted", [False, True])
def test_parameters_and_moments_through_resizes(hip_device, keep_sorted):
    """3000 rows: mask_indices crosses two of its 1024-row strides; the first densification stays inside the table's
    capacity, the last one outgrows it.  keep_sorted = True ends every densification with a spatial sort: the table is
    then compared as a multiset of rows, ordered by the id the final control point carries (zero learning rate on that
    group, so that the ids survive the steps)."""
    pc = _synthetic_table(3000, hip_device, 3000)
    pc.keep_sorted = keep_sorted
    if keep_sorted:
        next(gr for gr in pc.optimizer.param_groups if gr["name"] == "control_xyz")["lr"] = 0.0
    g = torch.Generator().manual_seed(77)
    capacity = pc._capacity
    _step_against_torch_adam(pc, g)
    _densify(pc, 0.3, 2, g, keep_sorted)
    assert 3000 < pc.get_xyz.shape[0] <= capacity == pc._capacity
    _step_against_torch_adam(pc, g)
    pre = {k: v.detach().cpu().clone() for k, v in pc.table_state().items()}
    mask = torch.rand(pc.get_xyz.shape[0], generator=g) < 0.2
    pc.prune_points(mask.to(hip_device))
    _check_resize(pc, R.prune_points(pre, mask), keep_sorted)
    assert pc.get_xyz.shape[0] == int((~mask).sum()) > 2048
    _step_against_torch_adam(pc, g)
    _densify(pc, 1.0, 3, g, keep_sorted)
    assert pc.get_xyz.shape[0] > capacity and pc._capacity > capacity
    _step_against_torch_adam(pc, g)
    if keep_sorted:
        ids = pc.control_xyz.detach()[:, ID_ROW, :].cpu()
        assert bool((ids == ids.round()).all()) and bool((ids[:, 0] == ids[:, 2]).all()) and 0 <= float(ids.min())
        assert float(ids.max()) <= 2999.0 and ids[:, 0].unique().shape[0] > 2000
