"""The five densification kernels of csrc/densify.hip through the C ABI, on buffers the tests allocate, against
tests/densify_restatement.py (tied to the reference's recorded states by tests/test_densify_restatement_cpu.py), at the
smallest shapes that cross each kernel's boundaries: the 1024-row strides of mask_indices, the 4096 x 256-thread grid
cap and the byte / word paths of rows_gather, the 256-thread blocks of the other three.

The kernels validate neither row indices nor buffer sizes: every index passed here is in range and every output buffer
has the worst-case size.

split_children is held to 3 x what torch's fp32 evaluation of the same formulas misses against float64 on these inputs
(densify_restatement.split_fp32_gap: observed 2.73e-7 of |xyz_parent| + |sample|_1 and 1.16e-7 of 1 + |scaling|, so
8.19e-7 and 3.48e-7 are allowed)."""
import ctypes

import pytest
import torch

import densify_restatement as R

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _abi():
    from mobgs_amd import _lib
    return _lib.load(), _lib.ptr, _lib.stream, _lib.check


# ---- mobgs_mask_indices -----------------------------------------------------------------------------------------------
def _masks(n, g):
    """name -> uint8 [n] whose non-zero bytes are 1, 2 or 255 (the kernel's rule is "non-zero")."""
    on = {"zeros": torch.zeros(n, dtype=torch.bool), "ones": torch.ones(n, dtype=torch.bool),
          "alternating": torch.arange(n) % 2 == 1, "last": torch.arange(n) == n - 1}
    for d in (0.01, 0.5, 0.99):
        on[f"random {d}"] = torch.rand(n, generator=g) < d
    values = torch.tensor([1, 2, 255], dtype=torch.uint8)
    return {k: torch.where(m, values[torch.randint(0, 3, (n,), generator=g)], torch.zeros(n, dtype=torch.uint8))
            for k, m in on.items()}


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3001])
def test_mask_indices_lists_the_rows_in_order_across_strides(hip_device, n):
    lib, ptr, stream, check = _abi()
    g = torch.Generator().manual_seed(1000 + n)
    for name, mask in _masks(n, g).items():
        dmask = mask.to(hip_device)
        for want in (0, 1):
            idx = torch.full((max(n, 1),), -1, dtype=torch.int32, device=hip_device)
            cnt = torch.full((1,), -1, dtype=torch.int32, device=hip_device)
            check(lib.mobgs_mask_indices(n, ptr(dmask) if n else None, want, ptr(idx), ptr(cnt), stream()),
                  "mobgs_mask_indices")
            expect = torch.nonzero((mask != 0) == bool(want)).reshape(-1).to(torch.int32)
            assert int(cnt.item()) == expect.shape[0], (n, name, want, int(cnt.item()), expect.shape[0])
            assert torch.equal(idx[:expect.shape[0]].cpu(), expect), (n, name, want)


# ---- mobgs_rows_gather ------------------------------------------------------------------------------------------------
# (row bytes, dtype, zero_new): the empty row, the byte path with and without zeroing, the word path likewise
FIELDS = [(0, torch.float32, 0), (1, torch.uint8, 1), (2, torch.uint8, 0), (4, torch.int32, 0), (12, torch.float32, 1),
          (16, torch.int32, 0), (144, torch.float32, 1)]


def _index_list(n_out, n_src, negative_single, g):
    """A permutation of source rows in which about a third of the entries were replaced by repeats of other rows and
    about a third of all entries are "new" copies (-(row + 1)); every decoded row lies in [0, n_src)."""
    rows = torch.randperm(n_src, generator=g)[:n_out]
    repeat = torch.rand(n_out, generator=g) < 1 / 3
    rows = torch.where(repeat, rows[torch.randint(0, n_out, (n_out,), generator=g)], rows)
    new = torch.rand(n_out, generator=g) < 1 / 3
    if n_out == 1:
        new[0] = negative_single
    assert 0 <= int(rows.min()) and int(rows.max()) < n_src
    return rows, new, torch.where(new, -(rows + 1), rows).to(torch.int32)


def _typed(rows_of_bytes, dtype):
    """uint8 [n, row bytes] as a field of `dtype` (an empty row has nothing to reinterpret)."""
    if rows_of_bytes.shape[1] == 0:
        return torch.empty(rows_of_bytes.shape, dtype=dtype, device=rows_of_bytes.device)
    return rows_of_bytes.view(dtype)


@pytest.mark.parametrize("n_out,dst_offset", [(1, 0), (1, 7), (255, 0), (255, 7), (256, 0), (256, 7), (257, 0), (257, 7),
                                              (30000, 7)])
def test_rows_gather_moves_every_field_bit_for_bit(hip_device, n_out, dst_offset):
    """30 000 rows of the 144-byte field are 1 080 000 words: more than the 4096 x 256 threads of the capped grid, so
    the grid-stride loop takes its second trip there."""
    lib, ptr, stream, check = _abi()
    g = torch.Generator().manual_seed(7 * n_out + dst_offset)
    n_src, n_dst = n_out + 3, dst_offset + n_out + 5
    rows, new, index = _index_list(n_out, n_src, dst_offset != 0, g)
    if n_out > 1:
        assert bool(new.any()) and not bool(new.all()) and rows.unique().shape[0] < n_out
    src_bytes = [torch.randint(0, 256, (n_src, rb), dtype=torch.uint8, generator=g) for rb, _, _ in FIELDS]
    src = [_typed(b.to(hip_device), dt) for b, (_, dt, _) in zip(src_bytes, FIELDS)]
    dst = [_typed(torch.full((n_dst, rb), SENTINEL, dtype=torch.uint8, device=hip_device), dt) for rb, dt, _ in FIELDS]
    assert all(t.is_contiguous() and t.shape[0] == n for ts, n in ((src, n_src), (dst, n_dst)) for t in ts)
    nf = len(FIELDS)
    args = ((ctypes.c_void_p * nf)(*[t.data_ptr() for t in src]), (ctypes.c_void_p * nf)(*[t.data_ptr() for t in dst]),
            (ctypes.c_int32 * nf)(*[rb for rb, _, _ in FIELDS]), (ctypes.c_int32 * nf)(*[zn for _, _, zn in FIELDS]))
    dindex = index.to(hip_device)
    check(lib.mobgs_rows_gather(nf, *args, ptr(dindex), n_out, dst_offset, stream()), "mobgs_rows_gather")
    for (rb, dt, zn), sb, d in zip(FIELDS, src_bytes, dst):
        expect = torch.full((n_dst, rb), SENTINEL, dtype=torch.uint8)
        moved = sb.index_select(0, rows)
        if zn:
            moved[new] = 0
        expect[dst_offset:dst_offset + n_out] = moved
        got = d.view(torch.uint8).reshape(n_dst, rb).cpu()
        assert torch.equal(got[dst_offset:dst_offset + n_out], expect[dst_offset:dst_offset + n_out]), (rb, "rows")
        assert torch.equal(got, expect), (rb, "rows outside [dst_offset, dst_offset + n_out) were touched")


# ---- mobgs_densify_stats ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grad_stride", [2, 3, 4])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1500])
def test_densify_stats_accumulates_like_the_restatement(hip_device, n, grad_stride):
    lib, ptr, stream, check = _abi()
    for form in ("mask+radii", "mask", "radii"):
        g = torch.Generator().manual_seed(31 * n + grad_stride)
        state = {"xyz_gradient_accum": 1e-3 * torch.rand(n, 1, generator=g),
                 "denom": torch.randint(0, 5, (n, 1), generator=g).float(),
                 "max_radii2D": torch.randint(0, 30, (n,), generator=g).float()}
        dev = {k: v.clone().to(hip_device) for k, v in state.items()}
        for step in range(3):
            vgrad = 3e-4 * torch.randn(n, grad_stride, generator=g)
            vgrad[torch.rand(n, generator=g) < 0.05] = 0.0
            visible = (torch.rand(n, generator=g) > 0.4).to(torch.uint8) * (1 + 253 * (step % 2)) if "mask" in form else None
            radii = torch.randint(-2, 40, (n,), generator=g).to(torch.int32) if "radii" in form else None
            before = {k: v.cpu().clone() for k, v in dev.items()}
            dg = vgrad.to(hip_device)
            dvis = visible.to(hip_device) if visible is not None else None
            drad = radii.to(hip_device) if radii is not None else None
            check(lib.mobgs_densify_stats(n, ptr(dg), grad_stride, ptr(dvis), ptr(drad), ptr(dev["xyz_gradient_accum"]),
                                          ptr(dev["denom"]), ptr(dev["max_radii2D"]) if radii is not None else None,
                                          stream()), "mobgs_densify_stats")
            state = R.add_densification_stats(state, vgrad, visible, radii)   # (three steps on its own: never re-seeded)
            got = {k: v.cpu() for k, v in dev.items()}
            vis = (visible != 0) if visible is not None else (radii > 0)
            assert 0 < int(vis.sum()) < n or n == 1
            for k in state:
                assert torch.equal(got[k][~vis], before[k][~vis]), (form, step, k, "a row that is not visible changed")
            assert torch.equal(got["denom"], state["denom"]), (form, step)
            assert torch.equal(got["max_radii2D"], state["max_radii2D"]), (form, step)
            if radii is None:
                assert torch.equal(got["max_radii2D"], before["max_radii2D"]), (form, step)
            ref = state["xyz_gradient_accum"].double()
            err = float(((got["xyz_gradient_accum"].double() - ref).abs() / ref.abs().clamp_min(1e-300)).max())
            print(f"stats n={n} stride={grad_stride} {form} step {step}: accum relative error {err:.2e}")
            assert torch.allclose(got["xyz_gradient_accum"], state["xyz_gradient_accum"], rtol=3e-7, atol=0), \
                (form, step, err)


# ---- mobgs_densify_select -----------------------------------------------------------------------------------------------
THR, SIZE_THR = 2.0e-4, 0.04
_thr32 = torch.tensor(THR, dtype=torch.float32)
_below = torch.nextafter(_thr32, torch.tensor(0.0))
# planted (accum, denom): 0 / 0 -> 0; x / 0 -> inf; -x / 0 -> -inf; g == thr; one ulp below; the negative ones through
# the explicit-grads route (denom = 1): |g| counts for a clone, the signed g for a split
PLANTED = [(0.0, 0.0), (3e-4, 0.0), (-3e-4, 0.0), (float(_thr32), 1.0), (float(_below), 1.0), (-float(_thr32), 1.0),
           (-float(_below), 1.0), (-1.0e-3, 1.0), (2.0 * float(_thr32), 2.0)]


def _select_inputs(n, first_kind, g):
    denom = torch.randint(0, 4, (n,), generator=g).float()
    accum = 4e-4 * torch.rand(n, generator=g) * denom
    big = torch.rand(n, generator=g) < 0.5
    k = torch.arange(n)
    planted = k < 2 * len(PLANTED)
    kind = (k + first_kind) % len(PLANTED)
    table = torch.tensor(PLANTED, dtype=torch.float32)
    accum = torch.where(planted, table[kind, 0], accum)
    denom = torch.where(planted, table[kind, 1], denom)
    big = torch.where(planted, ((k + first_kind) // len(PLANTED)) % 2 == 1, big)   # every planted kind at both sizes
    log_size = float(torch.log(torch.tensor(SIZE_THR, dtype=torch.float64)))
    top = torch.where(big, log_size + 0.05 + 3.0 * torch.rand(n, generator=g),
                      log_size - 0.05 - 3.0 * torch.rand(n, generator=g))
    scaling = top[:, None] - 2.0 * torch.rand(n, 3, generator=g)
    scaling[k, torch.randint(0, 3, (n,), generator=g)] = top
    return accum, denom, scaling.float().contiguous()


@pytest.mark.parametrize("n_grads_of", ["0", "n // 2", "n"])
@pytest.mark.parametrize("n", [1, 257, 1500])
def test_densify_select_masks_equal_the_restatement(hip_device, n, n_grads_of):
    lib, ptr, stream, check = _abi()
    n_grads = {"0": 0, "n // 2": n // 2, "n": n}[n_grads_of]
    for first_kind in (range(2 * len(PLANTED)) if n == 1 else (0,)):
        g = torch.Generator().manual_seed(5 * n + n_grads + first_kind)
        accum, denom, scaling = _select_inputs(n, first_kind, g)
        # device expf against host exp cannot flip a size decision
        assert R.size_margin(scaling, SIZE_THR) > 1e-4
        want_clone, want_split = R.select(scaling, R.mean_grads(accum, denom)[:n_grads], THR, SIZE_THR)
        if n > 1 and n_grads == n:
            assert bool(want_clone.any()) and bool(want_split.any()) and not bool((want_clone | want_split).all())
        da, dd, ds = accum.to(hip_device), denom.to(hip_device), scaling.to(hip_device)
        clone = torch.full((n,), SENTINEL, dtype=torch.uint8, device=hip_device)
        split = torch.full((n,), SENTINEL, dtype=torch.uint8, device=hip_device)
        check(lib.mobgs_densify_select(n, n_grads, ptr(da), ptr(dd), ptr(ds), THR, SIZE_THR, ptr(clone), ptr(split),
                                       stream()), "mobgs_densify_select")
        assert torch.equal(clone.cpu(), want_clone.to(torch.uint8)), (n, n_grads, first_kind, "clone")
        assert torch.equal(split.cpu(), want_split.to(torch.uint8)), (n, n_grads, first_kind, "split")


# ---- mobgs_split_children -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_row", [0, 777])
@pytest.mark.parametrize("n_split,N", R.SPLIT_CASES)
def test_split_children_against_float64(hip_device, n_split, N, first_row):
    lib, ptr, stream, check = _abi()
    rotation, xyz, scaling, samples = R.split_inputs(n_split, N, 100 * N + n_split)
    n_children = n_split * N
    n_rows = first_row + n_children + 9
    g = torch.Generator().manual_seed(n_children)

    def table(rows, width):   # the children's rows hold copies of their parents, as after the gather
        t = torch.randn(n_rows, width, generator=g)
        t[first_row:first_row + n_children] = rows
        return t

    t_rot, t_xyz, t_scl = table(rotation, 4), table(xyz, 3), table(scaling, 3)
    d_rot, d_xyz, d_scl = t_rot.to(hip_device), t_xyz.to(hip_device), t_scl.to(hip_device)
    d_smp = samples.to(hip_device)
    check(lib.mobgs_split_children(n_children, first_row, N, ptr(d_smp), ptr(d_rot), ptr(d_xyz), ptr(d_scl), stream()),
          "mobgs_split_children")
    got_xyz, got_scl = d_xyz.cpu(), d_scl.cpu()
    mine = slice(first_row, first_row + n_children)
    ex, es = R.split_errors(got_xyz[mine], got_scl[mine], rotation, xyz, scaling, samples, N)
    print(f"split n_split={n_split} N={N} first={first_row}: xyz {ex:.3e} (allowed {R.SPLIT_ALLOWED[0]:.3e}), "
          f"scaling {es:.3e} (allowed {R.SPLIT_ALLOWED[1]:.3e})")
    assert ex <= R.SPLIT_ALLOWED[0] and es <= R.SPLIT_ALLOWED[1], (ex, es)
    outside = torch.ones(n_rows, dtype=torch.bool)
    outside[mine] = False
    assert torch.equal(got_xyz[outside], t_xyz[outside]) and torch.equal(got_scl[outside], t_scl[outside])
    assert torch.equal(d_rot.cpu(), t_rot)
