"""mobgs_densify_stats_sets (csrc/densify_ctl.hip) through the C ABI: the batch statistics of both sets in ONE launch, from
int32 radii or from the fp32-coded radii of a gradient message, against tests/stats_sets_cases.py (vetted on the CPU by
tests/test_stats_sets_cases_cpu.py).

Every comparison is torch.equal.  On the `exact` family the restatement (control_cases.batch_stats per set) owes the same
bits as any correct chain of fp32 operations; on the `random` family, whose roundings show, the yardstick is the EXISTING
kernel, mobgs_densify_stats_batch called once per set on copies -- for the fp32-coded cases on the int32 form of the same
numbers (the owner's value plus other ranks' zeros is exact; integers below 2^24 are exact in fp32).  Every statistics
buffer carries a sentinel tail beyond its end, and every view's arrays PAD rows beyond both sets."""
import ctypes

import pytest
import torch

import stats_sets_cases as S

pytestmark = pytest.mark.gpu

TAIL = 8
SENTINEL = -7777.0
KEYS = ("xyz_gradient_accum", "denom", "max_radii2D")


def _abi():
    from mobgs_amd import _lib
    return _lib.load(), _lib.ptr, _lib.stream, _lib.check, _lib._DEFINES


def _padded(state, dev):
    """Each statistics array flat on the device with TAIL sentinels behind it."""
    out = {}
    for k in KEYS:
        flat = state[k].reshape(-1)
        out[k] = torch.cat([flat, torch.full((TAIL,), SENTINEL)]).to(dev)
    return out


def _check_tail(bufs, n, what):
    for k in KEYS:
        assert bool((bufs[k][n:] == SENTINEL).all()), (what, k, "written beyond the end")


def _tables(grads, radii, encoding, stride, dev):
    """-> (gradient table, radii table, the device tensors they point into).  FP32 at stride 2: one message slot per view,
    gradients first, radii behind them, as SubframeShard.put_densification_stats lays them."""
    if encoding == "FP32":
        fp = S.coded(radii)
        if stride == 2:
            keep = [S.slot(g, r).to(dev) for g, r in zip(grads, fp)]
            n = grads[0].shape[0]
            g_ptrs, r_ptrs = [t.data_ptr() for t in keep], [t.data_ptr() + 8 * n for t in keep]
        else:
            keep = [g.to(dev) for g in grads] + [r.to(dev) for r in fp]
            g_ptrs = [t.data_ptr() for t in keep[:len(grads)]]
            r_ptrs = [t.data_ptr() for t in keep[len(grads):]]
    else:
        keep = [g.to(dev) for g in grads] + [r.to(dev) for r in radii]
        g_ptrs = [t.data_ptr() for t in keep[:len(grads)]]
        r_ptrs = [t.data_ptr() for t in keep[len(grads):]]
    K = len(grads)
    return (ctypes.c_void_p * K)(*g_ptrs), (ctypes.c_void_p * K)(*r_ptrs), keep


def _call_sets(tabs, n_views, stride, encoding, ns, nd, a, b):
    lib, ptr, stream, _, D = _abi()
    return lib.mobgs_densify_stats_sets(n_views, tabs[0], stride, tabs[1], D["MOBGS_RADII_" + encoding] if isinstance(encoding, str)
                                        else encoding, S.WIDTH * 0.5, S.HEIGHT * 0.5,
                                        0, ns, ptr(a[KEYS[0]]), ptr(a[KEYS[1]]), ptr(a[KEYS[2]]),
                                        ns, nd, ptr(b[KEYS[0]]), ptr(b[KEYS[1]]), ptr(b[KEYS[2]]), stream())


def _call_batch(grads, radii, stride, dev, row0, n, bufs):
    """The existing kernel on one set, int32 radii."""
    lib, ptr, stream, check, _ = _abi()
    dg, dr = [g.to(dev) for g in grads], [r.to(dev) for r in radii]
    K = len(grads)
    check(lib.mobgs_densify_stats_batch(K, (ctypes.c_void_p * K)(*[t.data_ptr() for t in dg]), stride,
                                        (ctypes.c_void_p * K)(*[t.data_ptr() for t in dr]), row0, n, S.WIDTH * 0.5,
                                        S.HEIGHT * 0.5, ptr(bufs[KEYS[0]]), ptr(bufs[KEYS[1]]), ptr(bufs[KEYS[2]]), None, None,
                                        None, stream()), "mobgs_densify_stats_batch")
    torch.cuda.synchronize()


@pytest.mark.parametrize("encoding", S.ENCODINGS)
@pytest.mark.parametrize("stride", S.STRIDES)
@pytest.mark.parametrize("n_views", S.VIEWS)
@pytest.mark.parametrize("ns,nd", S.SETS_ROWS)
def test_stats_sets_equals_the_restatement_and_the_existing_kernel(hip_device, ns, nd, n_views, stride, encoding):
    _, _, _, check, _ = _abi()
    for family in ("exact", "random"):
        states, grads, radii, planted = S.inputs(ns, nd, n_views, stride, family, 1000 * ns + 10 * nd + n_views + stride)
        want, vis = S.expected(states, grads, radii, ns, nd)
        a, b = _padded(states[0], hip_device), _padded(states[1], hip_device)
        tabs = _tables(grads, radii, encoding, stride, hip_device)
        check(_call_sets(tabs, n_views, stride, encoding, ns, nd, a, b), "mobgs_densify_stats_sets")
        torch.cuda.synchronize()
        for which, (bufs, n, row0) in enumerate(((a, ns, 0), (b, nd, ns))):
            what = (family, "static" if which == 0 else "dynamic")
            _check_tail(bufs, n, what)
            got = {k: bufs[k][:n].cpu().reshape(states[which][k].shape) for k in KEYS}
            seen = vis[which]
            for k in KEYS:   # rows that are not visible are unchanged
                assert torch.equal(got[k][~seen], states[which][k][~seen]), (what, k, "a row that is not visible changed")
            for row in planted.get(1, []):
                if row0 <= row < row0 + n:
                    assert not bool(seen[row - row0])
            for row in planted.get(0, []):   # visible only in the last view: counted, with the largest radius
                if row0 <= row < row0 + n:
                    assert bool(seen[row - row0]) and float(got["max_radii2D"][row - row0]) == float(S.BIG)
            assert torch.equal(got["denom"], want[which]["denom"]), what
            assert torch.equal(got["max_radii2D"], want[which]["max_radii2D"]), what
            if family == "exact":
                assert torch.equal(got["xyz_gradient_accum"], want[which]["xyz_gradient_accum"]), what
            else:
                assert torch.allclose(got["xyz_gradient_accum"], want[which]["xyz_gradient_accum"], rtol=3e-7, atol=0), what
            # the existing kernel, one call for this set, on copies of the same start
            ref = _padded(states[which], hip_device)
            _call_batch(grads, radii, stride, hip_device, row0, n, ref)
            for k in KEYS:
                assert torch.equal(bufs[k], ref[k]), (what, k, "differs from mobgs_densify_stats_batch")


def test_refused_calls_return_invalid_and_write_nothing(hip_device):
    lib, ptr, stream, _, D = _abi()
    ns, nd, stride = 257, 255, 2
    states, grads, radii, _ = S.inputs(ns, nd, 16, stride, "random", 3)
    grads, radii = grads + [grads[0]], radii + [radii[0]]            # 17 views' worth of arrays
    a, b = _padded(states[0], hip_device), _padded(states[1], hip_device)
    before = {(i, k): t[k].clone() for i, t in enumerate((a, b)) for k in KEYS}
    tabs = _tables(grads, radii, "INT32", stride, hip_device)
    holed_g = (ctypes.c_void_p * 17)(*[None if v == 1 else tabs[0][v] for v in range(17)])
    holed_r = (ctypes.c_void_p * 17)(*[None if v == 1 else tabs[1][v] for v in range(17)])
    refused = [(0, tabs, "INT32"), (17, tabs, "INT32"), (-1, tabs, "INT32"), (2, (holed_g, tabs[1]), "INT32"),
               (2, (tabs[0], holed_r), "FP32"), (2, (None, tabs[1]), "INT32"), (2, (tabs[0], None), "INT32"),
               (2, tabs, 2), (2, tabs, -1)]
    for n_views, t, enc in refused:
        rc = _call_sets(t, n_views, stride, enc, ns, nd, a, b)
        assert rc == D["MOBGS_E_INVALID"] and b"mobgs_densify_stats_sets" in lib.mobgs_last_error(), (n_views, enc)
    assert _call_sets(tabs, 2, stride, "INT32", -1, nd, a, b) == D["MOBGS_E_INVALID"]
    assert _call_sets(tabs, 2, 1, "INT32", ns, nd, a, b) == D["MOBGS_E_INVALID"]
    null = {k: None for k in KEYS}
    assert _call_sets(tabs, 2, stride, "INT32", ns, nd, a, null) == D["MOBGS_E_INVALID"]
    torch.cuda.synchronize()
    for i, t in enumerate((a, b)):
        for k in KEYS:
            assert torch.equal(t[k], before[(i, k)]), (i, k, "a refused call wrote")
    # a set without rows needs no arrays; two empty sets launch nothing
    assert _call_sets(tabs, 2, stride, "INT32", ns, 0, a, null) == D["MOBGS_OK"]
    assert _call_sets(tabs, 2, stride, "INT32", 0, 0, null, null) == D["MOBGS_OK"]
    torch.cuda.synchronize()
    assert torch.equal(b["denom"], before[(1, "denom")]) and not torch.equal(a["denom"], before[(0, "denom")])


@pytest.mark.parametrize("encoding", S.ENCODINGS)
def test_a_recorded_call_replayed_twice_equals_two_eager_calls(hip_device, encoding):
    _, _, _, check, _ = _abi()
    ns, nd, n_views, stride = 1025, 63, 2, 2
    states, grads, radii, _ = S.inputs(ns, nd, n_views, stride, "random", 9)
    tabs = _tables(grads, radii, encoding, stride, hip_device)
    eager = [_padded(states[0], hip_device), _padded(states[1], hip_device)]
    for _ in range(2):
        check(_call_sets(tabs, n_views, stride, encoding, ns, nd, *eager), "mobgs_densify_stats_sets")
    torch.cuda.synchronize()
    replayed = [_padded(states[0], hip_device), _padded(states[1], hip_device)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # the tables are copied into the kernel's arguments: nothing of the host is read later
        check(_call_sets(tabs, n_views, stride, encoding, ns, nd, *replayed), "mobgs_densify_stats_sets")
    for v in range(n_views):
        tabs[0][v] = tabs[1][v] = None
    torch.cuda.synchronize()
    for k in KEYS:   # recording runs nothing
        assert torch.equal(replayed[0][k][:ns].cpu(), states[0][k].reshape(-1))
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(replayed, eager):
        for k in KEYS:
            assert torch.equal(got[k], want[k]), k
    assert not torch.equal(eager[0]["denom"][:ns].cpu(), states[0]["denom"].reshape(-1))
