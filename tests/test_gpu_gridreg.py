"""GPU checks of the grid regularisers (csrc/gridreg.hip through mobgs_amd/regulation.py) against the float64 restatement
(tests/gridreg_restatement.py), at the smallest shapes at which the kernels can still go wrong, and once at the real size.

VALUES: within 1 fp32 ulp of the restatement's float64 result rounded to fp32.  Derivation: kernel and restatement form
the same fp32 differences (bit for bit: one subtraction per written statement, no contraction), whose squares are exact in
float64 (24 x 24 bits).  A float64 sum of n <= 2^23 non-negative terms is off by at most (n - 1) 2^-53 <= 2^-30 relative in
ANY order, and the reciprocal count and the sum over planes add a few 2^-53 more; so the two float64 results differ by
less than 2^-29 relative, far inside half an fp32 ulp (2^-24): after the one rounding to fp32 they are equal, or
neighbours where the float64 values straddle a rounding boundary.

GRADIENTS: element by element, no allowance of elements: |got - g64| <= K 2^-24 mag, with mag = scale (|sd[j-2]| +
2 |sd[j-1]| + |sd[j]|) (+ the |1 - t| coefficient; TV: 4 scale (inv_h (|dh[j-1]| + |dh[j]|) + inv_w (|dw[i-1]| +
|dw[i]|))) as the restatement returns it.  K from the operation count: the kernel forms the combination in float64 and
rounds it to fp32 ONCE -- 2^-24 |g| <= 2^-24 mag -- and ahead of that it and the restatement each do at most 8 float64
operations (coefficient, combination, product, the l1 part), 2^-53 mag apiece: K = 1 + 16 x 2^-29.
"""
import numpy as np
import pytest
import torch

import gridreg_restatement as GR
from helpers import load, same_bits

pytestmark = pytest.mark.gpu

K = 1.0 + 16 * 2.0 ** -29
EPS = 2.0 ** -24
WEIGHTS = (0.0002, 0.001, 0.0001)            # (plane_tv, time_smoothness, l1_time_planes): the reference's stereo config


def one_ulp(got, want64, what):
    want = np.float32(want64)
    got = np.float32(got.detach().cpu().numpy() if torch.is_tensor(got) else got)
    assert abs(np.float64(got) - np.float64(want)) <= np.spacing(np.abs(want)), (what, got, want, want64)


def grad_close(got, g64, mag, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == g64.shape, (what, got.shape, g64.shape)
    bad = np.abs(got - g64) > K * EPS * mag
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(np.abs(got - g64).max()))


def place(a, layout, device, offset=0):
    """A leaf on the device holding the fp32 array a [B,C,h,w] in the given layout; offset: elements (4 bytes each) the
    base pointer is moved off its 16-byte boundary."""
    B, C, h, w = a.shape
    src = torch.from_numpy(np.ascontiguousarray(a))
    if layout == "nchw":
        strides = (C * h * w, h * w, w, 1)
    elif layout == "cl":
        strides = (C * h * w, 1, w * C, C)
    else:                                    # "cl_of8": the first C channels of a channels-last buffer of 8
        assert layout == "cl_of8" and C <= 8
        strides = (8 * h * w, 1, w * 8, 8)
    span = 1 + sum((n - 1) * s for n, s in zip(a.shape, strides))
    flat = torch.zeros(span + offset, dtype=torch.float32, device=device)
    t = torch.as_strided(flat, a.shape, strides, offset)
    t.copy_(src)
    assert t.data_ptr() % 16 == (4 * offset) % 16
    return t.requires_grad_(True)


def spatial(rng, shape):
    return rng.uniform(0.1, 0.5, shape).astype(np.float32)


def timeplane(rng, shape):
    """Exact ones mixed with values on both sides of 1."""
    p = np.ones(shape, dtype=np.float32)
    off = rng.uniform(-0.1, 0.1, shape).astype(np.float32)
    return np.where(rng.uniform(size=shape) < 0.4, p, p + off).astype(np.float32)


# (B, C, h, w, layout, offset)
PLANE_CASES = [
    (1, 4, 3, 6, "cl", 0), (1, 4, 4, 6, "nchw", 0), (1, 4, 5, 6, "cl", 0),     # the window is cut at both ends at once
    (1, 3, 5, 1, "cl", 0), (1, 3, 5, 1, "nchw", 0),                            # w = 1
    (1, 1, 6, 7, "nchw", 0), (1, 1, 6, 7, "cl", 0),                            # C = 1
    (1, 3, 7, 5, "cl", 0),                                                     # scalar only (run of 15)
    (1, 4, 7, 5, "cl", 0),                                                     # exact float4
    (1, 5, 6, 8, "cl", 0),                                                     # run of 40: float4 across the channel ends
    (1, 5, 6, 7, "cl", 0),                                                     # run of 35: rows not 16-byte aligned
    (1, 5, 6, 7, "cl_of8", 0), (1, 3, 4, 3, "cl_of8", 0),                      # float4 then a scalar tail; tail only
    (1, 4, 5, 6, "cl", 1), (1, 8, 19, 36, "nchw", 1), (1, 5, 6, 7, "cl_of8", 3),  # base off its boundary: unaligned arm
    (1, 32, 37, 40, "cl", 0),                                                  # 2 workgroups along the run x 5 along h
    (1, 8, 19, 36, "nchw", 0), (2, 6, 20, 33, "nchw", 0),                      # NCHW float4; odd rows; a batch of 2
    (1, 32, 17, 9, "cl", 0), (1, 4, 9, 6, "nchw", 0),                          # h one past two segments, past one
]


@pytest.mark.parametrize("case", PLANE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_plane_functions(hip_device, case):
    from mobgs_amd import regulation as R
    B, C, h, w, layout, offset = case
    rng = np.random.default_rng(hash(case[:4]) % 2 ** 31)
    a = timeplane(rng, (B, C, h, w)) if C % 2 else spatial(rng, (B, C, h, w))
    for name, fn, val, grad in (("smooth", R.compute_plane_smoothness, GR.smoothness, GR.smoothness_grad),
                                ("tv", R.compute_plane_tv, GR.tv, GR.tv_grad)):
        t = place(a, layout, hip_device, offset)
        v = fn(t)
        assert v.dim() == 0 and v.dtype == torch.float32
        print(name, case, v.item(), val(a))
        one_ulp(v, val(a), (name, case))
        v.backward(torch.tensor(0.75, device=hip_device))
        g64, mag = grad(a, 0.75)
        grad_close(t.grad, g64, mag, (name, case))


def test_gradient_buffer_has_the_parameters_strides(hip_device):
    from mobgs_amd import regulation as R
    p = torch.rand(1, 32, 6, 5, device=hip_device).contiguous(memory_format=torch.channels_last)
    q = torch.rand(1, 8, 6, 5, device=hip_device)
    gp, gq = R._alloc_grads([R._kernel_view(p), R._kernel_view(q)])
    assert gp.stride() == p.stride() and gq.stride() == q.stride() and gq.data_ptr() % 16 == 0


def make_grids(rng, C, levels, time_h, three_plane_level=True):
    """levels: [(h, w) of the spatial planes]; time planes [1, C, time_h, w]."""
    grids = []
    for (h, w) in levels:
        grids.append([timeplane(rng, (1, C, time_h, w)) if i in GR.TIME else spatial(rng, (1, C, h, w)) for i in range(6)])
    if three_plane_level:
        grids.insert(1, [spatial(rng, (1, C, 4, 4)) for _ in range(3)])
    return grids


def check_grids(grids, layout, device, what, cot=1.0):
    from mobgs_amd import regulation as R
    leaves = [[place(p, layout, device) for p in level] for level in grids]
    want = GR.terms(grids)
    terms = R.regulation_terms(leaves)
    assert terms.shape == (3,) and terms.dtype == torch.float32
    print(what, terms.tolist(), want)
    for k in range(3):
        one_ulp(terms[k], want[k], (what, k))
    total = R.grid_regulation(leaves, time_smoothness_weight=WEIGHTS[1], l1_time_planes_weight=WEIGHTS[2],
                              plane_tv_weight=WEIGHTS[0])
    assert total.dim() == 0
    # the fp32 statement on the kernel's own three terms: the same three products and two sums, bit for bit
    assert np.float32(total.item()) == GR.weighted(terms.detach().cpu().numpy(), WEIGHTS), what
    total.backward(torch.tensor(cot, device=device))
    scales = [cot * float(np.float32(x)) for x in WEIGHTS]
    ref = GR.regulation_grads(grids, scales)
    for li, level in enumerate(leaves):
        for pi, leaf in enumerate(level):
            if ref[li][pi] is None:
                assert leaf.grad is None, "a level of exactly 3 planes contributes nothing"
            else:
                grad_close(leaf.grad, *ref[li][pi], (what, li, pi))
    return leaves, terms, total


@pytest.mark.parametrize("time_h", (3, 4, 5))
@pytest.mark.parametrize("layout", ("cl", "nchw"))
def test_small_grids(hip_device, layout, time_h):
    rng = np.random.default_rng(100 + time_h)
    check_grids(make_grids(rng, 4, [(5, 6)], time_h), layout, hip_device, f"small {layout} h={time_h}", cot=0.5)


def test_analytic_cases(hip_device):
    """A quadratic ramp along h gives (2 a)^2, a plane constant along h exactly 0, fresh time planes (exact ones) l1 = 0 and
    a zero gradient: sign(0) = 0."""
    from mobgs_amd import regulation as R
    a = 0.25
    hh = torch.arange(21, dtype=torch.float32, device=hip_device).view(1, 1, 21, 1)
    ramp = (a * hh * hh - 1.5 * hh + 3.0).expand(1, 6, 21, 5).contiguous()
    assert float(R.compute_plane_smoothness(ramp)) == (2 * a) ** 2
    flat = torch.rand(1, 5, 1, 7, device=hip_device).expand(1, 5, 19, 7).contiguous().requires_grad_(True)
    v = R.compute_plane_smoothness(flat)
    v.backward()
    assert v.item() == 0.0 and not flat.grad.any()
    grids = [[torch.ones(1, 4, 3, 5, device=hip_device, requires_grad=True) if i in GR.TIME else
              torch.rand(1, 4, 5, 5, device=hip_device, requires_grad=True) for i in range(6)]]
    terms = R.regulation_terms(grids)
    assert terms.tolist()[1:] == [0.0, 0.0] and terms[0].item() > 0.0
    (terms[1] + terms[2]).backward()
    for i in range(6):
        assert not grids[0][i].grad.any(), i


def test_l1_only_kind_and_a_non_finite_value(hip_device):
    """The |1 - t| kind alone (the C ABI; the Python functions use it only together with the smoothness): value and
    gradient against the restatement, and where a plane holds +inf the gradient is the finite +inv torch gives -- the
    smoothness part the kind does not have is left out, not multiplied by zero."""
    from mobgs_amd import _lib
    from mobgs_amd import regulation as R
    h = _lib.load()
    a = timeplane(np.random.default_rng(3), (1, 5, 11, 7))
    for poke in (False, True):
        t = torch.from_numpy(a).to(hip_device)
        if poke:
            t[0, 2, 4, 3] = float("inf")
        grad = torch.full_like(t, -7.0)
        n, tab = R._table([t], (_lib._DEFINES["MOBGS_GRIDREG_L1"],), (0,), [grad])
        out = torch.empty(1, device=hip_device)
        partial = torch.empty(h.mobgs_gridreg_blocks(n, tab, 1), 2, dtype=torch.float64, device=hip_device)
        cot = torch.tensor([0.75], device=hip_device)
        _lib.check(h.mobgs_gridreg_fwd(n, tab, 1, None, _lib.ptr(partial), _lib.ptr(out), None, _lib.stream()), "fwd")
        _lib.check(h.mobgs_gridreg_bwd(n, tab, 1, None, _lib.ptr(cot), _lib.stream()), "bwd")
        g64, mag = GR.l1_grad(a, 0.75)
        if poke:
            assert out.item() == float("inf")
            g64 = g64.copy()
            g64[0, 2, 4, 3] = 0.75 / a.size                  # -inv sign(1 - inf)
        else:
            one_ulp(out[0], GR.l1(a), "l1 alone")
        grad_close(grad, g64, mag, ("l1 alone", poke))


def test_no_contributing_level_gives_zeros_on_the_planes_device(hip_device):
    from mobgs_amd import regulation as R
    grids = [[torch.rand(1, 4, 5, 5, device=hip_device) for _ in range(3)]]
    terms, total = R.regulation_terms(grids), R.grid_regulation(grids, 0.001, 0.0001, 0.0002)
    assert terms.device == grids[0][0].device == total.device and terms.tolist() == [0.0] * 3 and total.item() == 0.0


def test_reference_fixture(hip_device):
    """The reference's own fp32 results (tests/golden/gridreg.npz) within 3 x their recorded distance to the restatement
    plus the kernel's own distance: 1 ulp (2 x 2^-24 relative) per term; for the total that and the five fp32 roundings of
    its statement (three products, two sums of positive numbers), 2^-24 each: 7, taken as 8."""
    fx = load("gridreg")
    grids = [[fx[f"plane_{li}_{pi}"] for pi in range(n)] for li, n in ((0, 6), (1, 3))]
    _, terms, total = check_grids(grids, "nchw", hip_device, "fixture")
    for k, name in enumerate(("plane", "time", "l1")):
        ref = float(fx["reg_" + name])
        assert abs(float(terms[k]) - ref) <= (3 * float(fx["gap_reg_" + name]) + 2 * EPS) * abs(ref), name
    ref = float(fx["reg_total"])
    assert abs(float(total) - ref) <= (3 * float(fx["gap_reg_total"]) + 8 * EPS) * abs(ref)


def test_table_of_18_planes_over_several_partial_rows(hip_device):
    """Three 6-plane levels of C = 32: the largest spatial plane takes 2 x 7 workgroups, every plane of the last level more
    than one."""
    rng = np.random.default_rng(18)
    grids = make_grids(rng, 32, [(18, 20), (36, 40), (54, 60)], 5, three_plane_level=False)
    check_grids(grids, "cl", hip_device, "18 planes")


@pytest.fixture(scope="module")
def seesaw(hip_device):
    from mobgs_amd.deformation import SeesawArgs, deform_network
    torch.manual_seed(11)
    net = deform_network(SeesawArgs()).to(hip_device)
    net.deformation_net.set_aabb([1.5, 1.4, 1.3], [-1.5, -1.4, -1.3])
    with torch.no_grad():
        for level in net.deformation_net.grid.grids:
            for i in GR.TIME:
                keep = torch.rand_like(level[i]) < 0.4
                level[i].add_(torch.where(keep, torch.zeros_like(level[i]), (torch.rand_like(level[i]) - 0.5) * 0.2))
    return net


def plane_grads(net):
    return [p.grad.clone() for level in net.deformation_net.grid.grids for p in level]


def test_seesaw_network_at_its_real_size(hip_device, seesaw):
    """18 planes, the largest 256 x 256 x 32: value, gradient, and the same bits from a second run."""
    net = seesaw
    grids_np = [[p.detach().cpu().numpy() for p in level] for level in net.deformation_net.grid.grids]
    want = GR.terms(grids_np)
    runs = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        v = net.compute_regulation(WEIGHTS[1], WEIGHTS[2], WEIGHTS[0])
        v.backward()
        runs.append((v.detach().clone(), plane_grads(net)))
    assert same_bits(runs[0][0], runs[1][0]) and all(same_bits(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    terms = torch.stack([net._plane_regulation(), net._time_regulation(), net._l1_regulation()])
    print("seesaw", terms.tolist(), want)
    for k in range(3):
        one_ulp(terms[k], want[k], ("seesaw", k))
    assert np.float32(runs[0][0].item()) == GR.weighted(terms.detach().cpu().numpy(), WEIGHTS)
    ref = GR.regulation_grads(grids_np, [float(np.float32(x)) for x in WEIGHTS])
    flat = [pair for level in ref for pair in level]
    params = [p for level in net.deformation_net.grid.grids for p in level]
    for k, (g, (g64, mag)) in enumerate(zip(runs[0][1], flat)):
        assert g.stride() == params[k].stride()          # channels-last, as the parameter
        grad_close(g, g64, mag, ("seesaw", k))


def test_regulation_and_deformation_in_one_loss(hip_device, seesaw):
    """compute_regulation + the deformation output in one loss: each plane's .grad is the sum of the two gradients
    computed separately (one fp32 addition, by autograd).  The HexPlane backward adds with float atomics, so its result
    has fixed bits only where no two contributions meet: five points at least ten cells of the coarsest level apart in
    every coordinate share no bilinear tap on any plane of any level."""
    net = seesaw
    N = 5
    line = torch.linspace(-1.2, 1.2, N)
    pts = torch.stack([line, line.flip(0) * 0.9, line * 0.8], dim=1).to(hip_device)
    g = torch.Generator(device="cpu").manual_seed(5)
    scales = torch.rand(N, 3, generator=g).to(hip_device)
    rots = torch.randn(N, 4, generator=g).to(hip_device)
    times = torch.linspace(0.1, 0.9, N).view(N, 1).to(hip_device)

    def deform_loss():
        p, s, r = net(pts, scales, rots, times)
        return p.square().sum() + s.sum() + r.square().sum()

    def reg_loss():
        return 50.0 * net.compute_regulation(WEIGHTS[1], WEIGHTS[2], WEIGHTS[0])

    grads = {}
    for name, loss in (("deform", deform_loss), ("reg", reg_loss), ("both", lambda: deform_loss() + reg_loss())):
        net.zero_grad(set_to_none=True)
        loss().backward()
        grads[name] = plane_grads(net)
    for k, (d, r, b) in enumerate(zip(grads["deform"], grads["reg"], grads["both"])):
        assert r.abs().max() > 0
        assert same_bits(b, d + r) or same_bits(b, r + d), k


def test_forward_and_backward_in_one_graph(hip_device):
    """Forward and backward recorded once, replayed twice with the planes changed in between: the eager bits each time."""
    from mobgs_amd import regulation as R
    rng = np.random.default_rng(7)
    grids = make_grids(rng, 32, [(18, 20), (36, 40)], 4)
    leaves = [[place(p, "cl", hip_device) for p in level] for level in grids]
    planes = [p for level in leaves if len(level) == 6 for p in level]

    def step():
        v = R.grid_regulation(leaves, WEIGHTS[1], WEIGHTS[2], WEIGHTS[0])
        return (v, *torch.autograd.grad(v, planes))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                      # (uploads the weights once)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for round_ in range(2):
        with torch.no_grad():
            for k, p in enumerate(planes):
                p.mul_(1.0 + 0.01 * (k + round_)).add_(0.003 * round_)
        eager = [o.clone() for o in step()]
        for o in outs:
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(same_bits(a, b) for a, b in zip(outs, eager)), round_
    assert np.isfinite(float(eager[0]))


def test_bad_tables_are_refused_and_nothing_is_launched(hip_device):
    from mobgs_amd import _lib
    from mobgs_amd import regulation as R
    h = _lib.load()
    D = _lib._DEFINES
    t = torch.rand(1, 4, 5, 6, device=hip_device)
    out = torch.full((2,), -7.0, device=hip_device)
    partial = torch.full((4, 2), -7.0, dtype=torch.float64, device=hip_device)
    grad = torch.full_like(t, -7.0)
    n, tab = R._table([t], (D["MOBGS_GRIDREG_SMOOTH"],), (0,), [grad])
    stream = _lib.stream()
    for field, value in (("kind", 9), ("h", 2), ("slot", 1), ("sw", 2), ("C", 0), ("t", None), ("inv0", -1.0)):
        keep = getattr(tab[0], field)
        setattr(tab[0], field, value)
        assert h.mobgs_gridreg_blocks(n, tab, 1) == 0
        assert h.mobgs_gridreg_fwd(n, tab, 1, None, _lib.ptr(partial), _lib.ptr(out), None, stream) == D["MOBGS_E_INVALID"]
        assert b"mobgs_gridreg_fwd" in h.mobgs_last_error()
        assert h.mobgs_gridreg_bwd(n, tab, 1, None, _lib.ptr(out), stream) == D["MOBGS_E_INVALID"]
        assert b"mobgs_gridreg_bwd" in h.mobgs_last_error()
        setattr(tab[0], field, keep)
    assert h.mobgs_gridreg_fwd(D["MOBGS_GRIDREG_MAX_PLANES"] + 1, tab, 1, None, _lib.ptr(partial), _lib.ptr(out),
                               None, stream) == D["MOBGS_E_INVALID"]
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((partial == -7).all()) and bool((grad == -7).all())
    with pytest.raises(ValueError, match="table holds"):
        R.compute_plane_tv(torch.rand(D["MOBGS_GRIDREG_MAX_PLANES"] + 1, 1, 3, 3, device=hip_device))
    with pytest.raises(ValueError, match="NaN"):
        R.compute_plane_smoothness(torch.rand(1, 4, 2, 6, device=hip_device))
    # the table itself is good: the same call goes through
    assert h.mobgs_gridreg_fwd(n, tab, 1, None, _lib.ptr(partial), _lib.ptr(out), None, stream) == 0
    torch.cuda.synchronize()
    one_ulp(out[0], GR.smoothness(t.cpu().numpy()), "after the refusals")
