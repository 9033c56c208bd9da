"""FlatGradients.rebind (mobgs_amd/distributed.py) on CPU tensors: the layout after a resize -- fp32 parameters in order,
then the named slots, fp16 parameters in the half buffer --, storage kept while the layout fits and grown by a factor when
it does not, every .grad the new view, buffers zero, no old view left on a parameter."""
import torch

from mobgs_amd.distributed import FlatGradients


def _params(n, half=False):
    g = torch.Generator().manual_seed(n)
    ps = [torch.nn.Parameter(torch.randn(n, 3, generator=g)), torch.nn.Parameter(torch.randn(n, 1, generator=g)),
          torch.nn.Parameter(torch.randn(7, generator=g)), torch.nn.Parameter(torch.randn(n, 0, 3, generator=g))]
    frozen = torch.nn.Parameter(torch.randn(n, 2, generator=g), requires_grad=False)
    if half:
        ps.insert(1, torch.nn.Parameter(torch.randn(n, 4, generator=g).half()))
    return ps + [frozen]


def _storage(t):
    return t.untyped_storage().data_ptr()


def _check_layout(b, params, extra):
    live = [p for p in params if p.requires_grad]
    assert len(b.params) == len(live) and all(x is y for x, y in zip(b.params, live))
    off = {torch.float32: 0, torch.float16: 0}
    for p, v in zip(live, b.views):
        buf = b.flat if p.dtype == torch.float32 else b.flat_half
        assert v.shape == p.shape and v.dtype == p.dtype
        assert v.data_ptr() == buf.data_ptr() + off[p.dtype] * buf.element_size() or p.numel() == 0
        assert p.grad is v or (p.grad.data_ptr() == v.data_ptr() and p.grad.shape == v.shape)
        off[p.dtype] += p.numel()
    assert b.param_floats == off[torch.float32] and b.flat_half.numel() == off[torch.float16]
    at = b.param_floats
    for name, k in extra.items():
        s = b.extra(name)
        assert s.numel() == k and s.data_ptr() == b.flat.data_ptr() + 4 * at
        at += k
    assert b.flat.numel() == at and b.attached()
    assert sorted(x.numel() for x in b.buffers()) == sorted(n for n in (at, off[torch.float16]) if n)
    assert all(float(x.abs().sum()) == 0.0 for x in b.buffers())
    # the views ALIAS the flat storage: a write through a parameter's .grad shows in the buffer
    for p in live:
        if p.numel():
            p.grad.fill_(1.0)
    assert float(b.flat[:b.param_floats].sum()) == b.param_floats and float(b.flat[b.param_floats:].sum()) == 0.0
    assert float(b.flat_half.float().sum()) == b.flat_half.numel()
    b.zero()


def test_rebind_keeps_the_storage_when_the_layout_fits_and_grows_it_by_a_factor_when_not():
    old = _params(100)
    extra = {"view0": 300, "view1": 300}
    b = FlatGradients(old, extra=extra)
    b.zero()
    _check_layout(b, old, extra)
    first, first_size = _storage(b.flat), b.flat.numel()
    old_views = list(b.views)
    b.flat.fill_(3.0)

    same = _params(100)                                  # new objects of the same sizes (an opacity reset, a load)
    assert b.rebind(same, extra=extra) is b
    _check_layout(b, same, extra)
    assert _storage(b.flat) == first and b.flat.numel() == first_size
    assert all(p.grad is None for p in old if p.requires_grad), "an old parameter still holds a view"
    assert not any(p.grad is v for p in same if p.requires_grad for v in old_views)

    grown = _params(160)                                 # a clone + split: more rows, larger slots
    extra2 = {"view0": 480, "view1": 480}
    b.rebind(grown, extra=extra2)
    _check_layout(b, grown, extra2)
    need = b.flat.numel()
    assert need > first_size and _storage(b.flat) != first
    room = b.flat.untyped_storage().nbytes() // 4
    assert room == int(need * FlatGradients.GROWTH) + 1024, (room, need)
    second = _storage(b.flat)

    more = _params(200)                                  # fits in the headroom: no allocation
    extra3 = {"view0": 600, "view1": 600}
    assert sum(p.numel() for p in more if p.requires_grad) + 1200 <= room
    b.rebind(more, extra=extra3)
    _check_layout(b, more, extra3)
    assert _storage(b.flat) == second

    small = _params(40)                                  # a prune: a smaller layout keeps the storage
    b.rebind(small, extra={"view0": 120})
    _check_layout(b, small, {"view0": 120})
    assert _storage(b.flat) == second and b.flat.untyped_storage().nbytes() // 4 == room
    assert "view1" not in b.extra_slices

    b.rebind(small)                                      # extra=None: no slots
    _check_layout(b, small, {})


def test_fp16_parameters_land_in_the_half_buffer():
    ps = _params(50, half=True)
    b = FlatGradients(_params(10, half=True), extra={"s": 5})
    half_before = _storage(b.flat_half)
    b.rebind(ps, extra={"s": 9})
    _check_layout(b, ps, {"s": 9})
    assert b.flat_half.dtype == torch.float16 and b.flat_half.numel() == 200 and _storage(b.flat_half) != half_before
    assert ps[1].grad.dtype == torch.float16 and ps[1].grad.data_ptr() == b.flat_half.data_ptr()
    kept = _storage(b.flat_half)
    smaller = _params(20, half=True)
    b.rebind(smaller, extra={"s": 9})
    _check_layout(b, smaller, {"s": 9})
    assert _storage(b.flat_half) == kept


def test_the_constructor_allocates_exactly_the_layout():
    ps = _params(30)
    b = FlatGradients(ps, extra={"a": 11})
    assert b.flat.untyped_storage().nbytes() == 4 * b.flat.numel() == 4 * (30 * 3 + 30 + 7 + 11)
    assert all(p.grad is None for p in ps)               # (zero() attaches, as before)
