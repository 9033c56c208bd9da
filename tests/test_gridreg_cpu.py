"""CPU checks of the grid regularisers: the float64 restatement (tests/gridreg_restatement.py) against the fixture of the
reference's own outputs (tests/golden/gridreg.npz), its closed-form gradients against float64 autograd, the CPU path of
mobgs_amd.regulation against both, and the analytic cases."""
import numpy as np
import pytest
import torch

import gridreg_restatement as GR
from helpers import load

FX = load("gridreg")
GRIDS = [[FX[f"plane_{li}_{pi}"] for pi in range(n)] for li, n in ((0, 6), (1, 3))]
WEIGHTS = tuple(float(x) for x in FX["weights"])      # (plane_tv, time_smoothness, l1_time_planes)


def tgrids(requires_grad=False, dtype=torch.float32):
    return [[torch.tensor(p, dtype=dtype, requires_grad=requires_grad) for p in level] for level in GRIDS]


def within_gap(got, name, what=""):
    """3 x the recorded distance between the reference's fp32 result and the float64 restatement."""
    ref, gap = FX[name], float(FX["gap_" + name])
    if ref.ndim == 0:
        err = abs(float(got) - float(ref)) / abs(float(ref)) if float(got) != float(ref) else 0.0
    else:
        top = np.abs(FX[name + "_f64"]).max()
        err = np.abs(np.asarray(got, dtype=np.float64) - ref).max() / top if top > 0 else np.abs(got).max()
    assert err <= 3.0 * gap, (what or name, err, gap)


def within_f64(got, name):
    """An fp32 evaluation against the fixture's float64 restatement: 3 x the gap the reference's own fp32 result keeps."""
    f64, gap = FX[name + "_f64"], float(FX["gap_" + name])
    if f64.ndim == 0:
        err = abs(float(got) - float(f64)) / abs(float(f64))
    else:
        err = np.abs(np.asarray(got, dtype=np.float64) - f64).max() / np.abs(f64).max()
    assert err <= 3.0 * gap, (name, err, gap)


def test_restatement_against_the_reference_fixture():
    for pi, p in enumerate(GRIDS[0]):
        within_gap(GR.smoothness(p), f"smooth_{pi}")
        within_gap(GR.tv(p), f"tv_{pi}")
        within_gap(GR.smoothness_grad(p)[0], f"g_smooth_{pi}")
        within_gap(GR.tv_grad(p)[0], f"g_tv_{pi}")
    plane, time, l1 = GR.terms(GRIDS)
    within_gap(plane, "reg_plane")
    within_gap(time, "reg_time")
    within_gap(l1, "reg_l1")
    within_gap(WEIGHTS[0] * plane + WEIGHTS[1] * time + WEIGHTS[2] * l1, "reg_total")
    within_gap(GR.weighted((plane, time, l1), WEIGHTS), "reg_total", "fp32 statement of the total")
    for name, scales in (("plane", (1, 0, 0)), ("time", (0, 1, 0)), ("l1", (0, 0, 1)), ("total", WEIGHTS)):
        grads = GR.regulation_grads(GRIDS, scales)
        assert grads[1] == [None] * 3
        for pi in range(6):
            within_gap(grads[0][pi][0], f"g_reg_{name}_{pi}")


def exact_planes(seed, shape):
    """Values on a 2^-10 lattice in [0, 2): every fp32 difference the statements form is exact, so their float64
    evaluation is the restatement's up to float64 rounding."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 2048, shape, generator=g).float() / 1024.0)


@pytest.mark.parametrize("shape", [(1, 3, 3, 4), (2, 5, 4, 1), (1, 4, 7, 6), (1, 1, 5, 5)])
def test_closed_form_gradients_against_float64_autograd(shape):
    from mobgs_amd import regulation as R
    p = exact_planes(sum(shape), shape)
    p[0, 0, 1, 0] = 1.0                                    # one element on the kink of |1 - t|
    for fn, val, grad in ((R._smoothness_torch, GR.smoothness, GR.smoothness_grad), (R._tv_torch, GR.tv, GR.tv_grad),
                          (R._l1_torch, GR.l1, GR.l1_grad)):
        t = p.double().requires_grad_(True)
        v = fn(t)
        v.backward()
        g, mag = grad(p.numpy(), 1.0)
        assert abs(v.item() - val(p.numpy())) <= 1e-14 * abs(v.item())
        assert np.all(np.abs(t.grad.numpy() - g) <= 1e-14 * mag + 1e-300), fn.__name__
        assert np.all(np.abs(g) <= mag * (1 + 1e-15))


def test_cpu_path_against_the_reference_fixture():
    """The CPU path is an fp32 evaluation of the same terms: within 3 x the gap the reference's own fp32 results keep to
    the restatement (no bit equality: the order of a CPU reduction depends on the build and the vector ISA)."""
    from mobgs_amd import regulation as R
    for pi, p in enumerate(GRIDS[0]):
        for name, fn in (("smooth", R.compute_plane_smoothness), ("tv", R.compute_plane_tv)):
            t = torch.tensor(p, requires_grad=True)
            v = fn(t)
            v.backward()
            assert v.dim() == 0
            within_f64(v.item(), f"{name}_{pi}")
            within_f64(t.grad.numpy(), f"g_{name}_{pi}")
    terms = R.regulation_terms(tgrids())
    assert terms.shape == (3,)
    for k, name in enumerate(("plane", "time", "l1")):
        within_f64(terms[k].item(), "reg_" + name)
    g = tgrids(requires_grad=True)
    total = R.grid_regulation(g, time_smoothness_weight=WEIGHTS[1], l1_time_planes_weight=WEIGHTS[2],
                              plane_tv_weight=WEIGHTS[0])
    total.backward()
    assert total.dim() == 0
    within_f64(total.item(), "reg_total")
    for pi in range(6):
        within_f64(g[0][pi].grad.numpy(), f"g_reg_total_{pi}")
    assert all(p.grad is None for p in g[1]), "a level of exactly 3 planes contributes nothing"
    empty = [[torch.rand(1, 4, 5, 5) for _ in range(3)]]
    assert R.regulation_terms(empty).tolist() == [0.0, 0.0, 0.0] and float(R.grid_regulation(empty, 1.0, 1.0, 1.0)) == 0.0


def test_deform_network_methods_delegate():
    from mobgs_amd import regulation as R
    from mobgs_amd.deformation import SeesawArgs, deform_network

    class Small(SeesawArgs):
        kplanes_config = dict(SeesawArgs.kplanes_config, resolution=[6, 5, 4, 3])
        multires = [1, 2, 3]

    torch.manual_seed(3)
    net = deform_network(Small())
    grids = net.deformation_net.grid.grids
    with torch.no_grad():
        for level in grids:
            for i in R.TIME_PLANES:
                level[i].add_(torch.randn_like(level[i]) * 0.1)
    want = R.regulation_terms(grids)
    assert torch.equal(net._plane_regulation(), want[0]) and torch.equal(net._time_regulation(), want[1])
    assert torch.equal(net._l1_regulation(), want[2])
    v = net.compute_regulation(0.001, 0.0001, 0.0002)
    assert torch.equal(v, 0.0002 * want[0] + 0.001 * want[1] + 0.0001 * want[2])
    v.backward()
    planes = [[p.detach().numpy() for p in level] for level in grids]
    ref = GR.regulation_grads(planes, (0.0002, 0.001, 0.0001))
    for li, level in enumerate(grids):
        for pi, p in enumerate(level):
            g64, mag = ref[li][pi]
            assert p.grad.shape == p.shape
            assert np.all(np.abs(p.grad.numpy() - g64) <= 8 * 2.0 ** -24 * mag), (li, pi)   # a handful of fp32 roundings


def test_quadratic_ramp_gives_the_analytic_value():
    """t = a h^2 + b h + c on integers with a = 1/4: every value and difference is exact, sd = 2 a everywhere."""
    from mobgs_amd import regulation as R
    a, b, c = 0.25, -1.5, 3.0
    hh = torch.arange(9, dtype=torch.float32).view(1, 1, 9, 1)
    t = (a * hh * hh + b * hh + c).expand(1, 3, 9, 4).contiguous()
    assert float(R.compute_plane_smoothness(t)) == (2 * a) ** 2 == GR.smoothness(t.numpy())
    g, _ = GR.smoothness_grad(t.numpy())
    assert np.all(g[:, :, 2:-2] == 0)                      # interior: 2a - 2 (2a) + 2a


def test_constant_along_h_is_exactly_zero():
    from mobgs_amd import regulation as R
    t = torch.rand(1, 5, 1, 7, generator=torch.Generator().manual_seed(1)).expand(1, 5, 6, 7).contiguous()
    assert float(R.compute_plane_smoothness(t)) == 0.0 == GR.smoothness(t.numpy())
    assert not np.any(GR.smoothness_grad(t.numpy())[0])


def test_fresh_time_planes_sit_on_the_kink():
    """Time planes are initialised to exactly 1: l1 = 0, and with sign(0) = 0 the gradient is zero too."""
    from mobgs_amd import regulation as R
    grids = [[torch.ones(1, 4, 3, 5, requires_grad=True) if i in R.TIME_PLANES else
              torch.rand(1, 4, 5, 5, requires_grad=True) for i in range(6)]]
    terms = R.regulation_terms(grids)
    assert terms.tolist()[1:] == [0.0, 0.0]
    (terms[1] + terms[2]).backward()
    for i in R.TIME_PLANES:
        assert not grids[0][i].grad.any()
        p = grids[0][i].detach().numpy()
        assert GR.l1(p) == 0.0 and not np.any(GR.l1_grad(p)[0]) and not np.any(GR.smoothness_grad(p)[0])


def test_h_below_3_raises():
    from mobgs_amd import regulation as R
    t = torch.rand(1, 4, 2, 5)
    with pytest.raises(ValueError, match="NaN"):
        R.compute_plane_smoothness(t)
    grids = [[torch.rand(1, 4, 5, 5)] * 2 + [t] + [torch.rand(1, 4, 5, 5)] + [t, t]]
    with pytest.raises(ValueError, match="NaN"):
        R.grid_regulation(grids, 0.001, 0.0001, 0.0002)
    with pytest.raises(ValueError, match="NaN"):
        R.regulation_terms(grids)
    assert float(R.compute_plane_tv(t)) >= 0.0              # TV has no such limit


def test_table_records_and_bad_tables_are_refused_before_any_launch():
    """The C ABI refuses a bad table with MOBGS_E_INVALID under its own name, without touching a device."""
    import ctypes
    from mobgs_amd import _lib
    h = _lib.load()
    D = _lib._DEFINES
    none = ctypes.c_void_p(None)
    fake = 4096                                              # never dereferenced: every call below is refused or host-only

    def rec(**kw):
        r = _lib.MobgsGridPlane(t=fake, grad=None, C=32, h=64, w=64, kind=D["MOBGS_GRIDREG_SMOOTH"], slot=0,
                                sc=1, sh=64 * 32, sw=32, inv0=1.0, inv1=1.0)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    def table(*recs):
        return (_lib.MobgsGridPlane * len(recs))(*recs)

    # 64 x 32 / 4 = 512 units -> 2 workgroups along the run, 64 / 8 = 8 along h
    assert h.mobgs_gridreg_blocks(1, table(rec()), 1) == 16
    assert h.mobgs_gridreg_blocks(2, table(rec(), rec(C=5, h=3, w=6, sc=18, sh=6, sw=1)), 1) == 16 + 1
    bad = [rec(t=None), rec(C=0), rec(h=0), rec(w=-1), rec(kind=4), rec(kind=-1), rec(slot=1), rec(slot=-1), rec(h=2),
           rec(sc=2, sw=2), rec(sh=-1), rec(inv0=-1.0), rec(inv1=float("nan")), rec(t=fake + 2),
           rec(kind=D["MOBGS_GRIDREG_SMOOTH_L1"], slot=0), rec(sh=1 << 40)]
    for r in bad:
        assert h.mobgs_gridreg_blocks(1, table(r), 1) == 0
        h.mobgs_raster_bwd_reduce(0, 5, 3, 0, *[none] * 12)  # leaves another entry point's message behind
        assert h.mobgs_gridreg_fwd(1, table(r), 1, none, fake, fake, none, none) == D["MOBGS_E_INVALID"] == -1
        assert b"mobgs_gridreg_fwd" in h.mobgs_last_error()
    ok = table(rec())
    too_many = table(*[rec() for _ in range(D["MOBGS_GRIDREG_MAX_PLANES"] + 1)])
    for args in ((0, ok, 1, none, fake, fake, none), (1, none, 1, none, fake, fake, none), (1, ok, 0, none, fake, fake, none),
                 (1, ok, D["MOBGS_GRIDREG_MAX_SLOTS"] + 1, none, fake, fake, none), (1, ok, 1, none, none, fake, none),
                 (1, ok, 1, none, fake, none, none), (1, ok, 1, none, fake + 4, fake, none),
                 (1, ok, 1, fake, fake, fake, none), (1, ok, 1, none, fake, fake, fake),      # weights without total, total without
                 (len(too_many), too_many, 1, none, fake, fake, none)):
        assert h.mobgs_gridreg_fwd(*args, none) == -1 and b"mobgs_gridreg_fwd" in h.mobgs_last_error(), args
    # backward: the gradient pointer and the cotangent are needed
    assert h.mobgs_gridreg_bwd(1, ok, 1, none, fake, none) == -1 and b"mobgs_gridreg_bwd" in h.mobgs_last_error()
    assert h.mobgs_gridreg_bwd(1, table(rec(grad=fake)), 1, none, none, none) == -1
    with pytest.raises(RuntimeError, match="mobgs_gridreg_bwd"):
        _lib.check(-1, "mobgs_gridreg_bwd")
    assert ctypes.sizeof(_lib.MobgsGridPlane) == 80


def test_remembered_table_follows_address_shape_and_strides():
    """A table is reused for the same plane object only while its address, shape and strides are what was described."""
    from mobgs_amd import _lib
    from mobgs_amd import regulation as R
    kinds, slots = (_lib._DEFINES["MOBGS_GRIDREG_SMOOTH"],), (0,)
    p = torch.rand(1, 4, 6, 8)

    def plan():
        return R._plan([p], [R._kernel_view(p)], kinds, slots, 1)

    n, tab, blocks = plan()
    assert plan()[1] is tab and (tab[0].h, tab[0].w, n, blocks) == (6, 8, 1, 1)
    p.data = p.data.view(1, 4, 8, 6)                         # same object, same address, another shape
    tab2 = plan()[1]
    assert tab2 is not tab and (tab2[0].h, tab2[0].w, tab2[0].sh) == (8, 6, 6)
    p.data = torch.as_strided(p.data, (1, 4, 8, 6), (192, 1, 24, 4))   # ... that shape, channels-last strides
    tab3 = plan()[1]
    assert tab3 is not tab2 and (tab3[0].h, tab3[0].w, tab3[0].sc, tab3[0].sh, tab3[0].sw) == (8, 6, 1, 24, 4)
    assert plan()[1] is tab3
    # an entry holds no tensor: weak references, integers, the ctypes table
    (refs, sig, _), = [v for k, v in R._plan_memo.items() if k[3] == (id(p),)]
    assert not any(torch.is_tensor(x) for x in refs) and not any(torch.is_tensor(y) for x in sig for y in x)
