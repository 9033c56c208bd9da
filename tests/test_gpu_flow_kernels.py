"""The flow-warp loss kernels (csrc/flowloss.hip through mobgs_amd.loss_utils.flow_warp_loss and the C ABI) against the float64
reference on the kink-free cases of tests/flow_cases.py, in all three builds of the backward kernel.

Cases (tests/test_flow_cases_cpu.py shows from the references alone that each reaches its edge): images of 2 x 2, 2 x 70 and
70 x 2 (size - 1 = 1); widths 64, 65 and 129 (lane 63's right-hand column, one live lane in the last strip); 37 rows in the
4-row build (a last workgroup with dead waves); 500 x 70 x 32 and 33 x 65 x 256, exactly 1024 workgroups of 32 rows -- the
8-row build that training runs, with strips cut after 4 rows, a dead wave, a workgroup of ONE live row and a strip of ONE
live lane --, and 33 x 65 x 255 right under that threshold; white-noise coordinates in both builds (every contribution is a
stray, the queue drains in the middle of a row); all pixels sampling one cell; a constant sub-pixel translation (the ideal
give / take / carry pattern across every strip end); a band of samples outside each border and a corner; masks that are zero
over 8 x 8 blocks across a strip end and over a whole batch entry; the smooth generator of tests/test_gpu_flow_loss.py made
kink-free.  Every case runs with combine_taps on and off (off: always the <false, 4> build) and its own cotangent from
{1, 0.37, -2.5}; before comparing, the build that the library reports (mobgs_flow_warp_loss_bwd_rows, the function the
launcher itself dispatches by) must be the one tests/flow_cases.expected_rows restates.

Compared (tests/flow_cases.py): the loss as a scalar, the six gradients per tensor and per stratum -- the last live row of a
strip, the first row of the next, columns 63 / 64, clamped, zero mask, interior, in the case's own build -- with
deform_cases.close_to_f64 at k = 3 and exact zeros where float64 has them; the two scatter targets get
the term allowance 2^-24 sqrt(n) T.  No flip allowance, no share of elements left out.  The plain-store outputs (loss, both
coordinate gradients, both mask gradients) are bit-reproducible, equal between combine_taps on and off, equal for every
subset of requested gradients, exactly linear in the cotangent and independent of alignment and layout of the inputs; the
two image gradients are atomic sums and are held to the bound each time.

Worst k needed on an MI355X per family and build (docs/MEASUREMENT_LOG.md, "Flow-warp loss kernels against float64"):

    family                  <true, 8>                    <true, 4>                  <false, 4>                  k
    loss                    0     (below the floor)      0                          0                           3
    scatter targets         0.996 (white_noise_8)        1.31  (pile_up)            1.31  (pile_up)             3
    coordinate gradients    1.000 (white_noise_8)        1.035 (w65)                1.035 (w65)                 3
    mask gradients          1.028 (tall8_b)              1.378 (min_2x2)            1.378 (min_2x2)             3

The term allowance was used by one stratum: g_ori of pile_up in the row below the pile, where the plain rule would need
k = 8.5 / 9.5 and the error is a third of the allowance.  With Scatter::flush or the last StrayQueue::drain skipped 20 / 21 of
the 22 cases fail, with the 8-row build walking 4-row strips the three 8-row cases do (scratch builds, same log)."""
import pytest
import torch

import flow_cases as C
from helpers import same_bits

pytestmark = pytest.mark.gpu


def _lib():
    from mobgs_amd import _lib
    return _lib.load()


def _build(c, combine):
    """The library's own report of the build for the case's sizes, held to the restated rule, and printed."""
    rows = _lib().mobgs_flow_warp_loss_bwd_rows(c.B, c.H, c.W, int(combine))
    print(f"BUILD {c.name} combine_taps={int(combine)}: flow_warp_l1_bwd_kernel<{str(bool(combine)).lower()}, {rows}>")
    assert rows == C.expected_rows(c.B, c.H, c.W, combine), (c.name, combine, rows)
    return rows


def _run(c, dev, combine=True, v=None, inputs=None):
    """-> {loss, ori, latent, e2m, m2e, la, da} on the CPU: value and gradients through mobgs_amd.loss_utils."""
    from mobgs_amd.loss_utils import flow_warp_loss
    t = inputs or {k: x.to(dev).requires_grad_(True) for k, x in c.inputs.items()}
    loss = flow_warp_loss(*(t[k] for k in C.NAMES), combine_taps=combine)
    loss.backward(torch.tensor(c.v if v is None else v, device=dev))
    out = {k: t[k].grad.detach().cpu() for k in C.NAMES}
    out["loss"] = loss.detach().cpu()
    return out


def _report(name, build, needs):
    """One WORST line per family: the largest k the run needed, and the largest k of the plain rule where the term
    allowance was used (a failed comparison shows as nan)."""
    worst = {}
    for family, stratum, _, k, plain in needs:
        if not k <= worst.get(family, (-1.0, "", 0.0))[0]:
            worst[family] = (k, stratum, worst.get(family, (0.0, "", 0.0))[2])
        if plain > C.K and plain > worst[family][2]:
            worst[family] = worst[family][:2] + (plain,)
    for family, (k, stratum, plain) in worst.items():
        note = f"; plain rule up to k {plain:.2f}, inside the term allowance" if plain else ""
        print(f"WORST {build} {family}: k {k:.3f} ({name}, {stratum}){note}")


@pytest.mark.parametrize("name", C.CASES)
def test_flow_warp_loss_matches_float64(hip_device, name):
    c = C.case(name)
    plain = {}
    for combine in (True, False):
        rows = _build(c, combine)
        assert combine or rows == 4
        got = _run(c, hip_device, combine)
        build = f"<{str(combine).lower()}, {rows}>"
        sink = []
        try:
            C.compare(name, rows, got, f"{name} {build}", sink=sink)
        finally:
            _report(name, build, sink)
        plain[combine] = got
    for k in C.PLAIN + ("loss",):  # one value per element, no atomics: the same bits with and without merged taps
        assert same_bits(plain[True][k], plain[False][k]), k


def test_build_query():
    """mobgs_flow_warp_loss_bwd_rows is a size query: the rule on both sides of its threshold, and the flow entry points'
    error for sizes they do not take."""
    lib = _lib()
    for B, H, W, want in ((2, 1014, 1352, 8), (1, 1014, 1352, 4), (256, 33, 65, 8), (255, 33, 65, 4), (1024, 2, 2, 8),
                          (1023, 2, 2, 4), (1, 32 * 1024, 64, 8), (1, 32 * 1023, 64, 4), (1, 32 * 1023 + 1, 64, 8),
                          (1, 2, 64 * 1023 + 1, 8), (1, 2, 64 * 1023, 4)):
        assert lib.mobgs_flow_warp_loss_bwd_rows(B, H, W, 1) == want == C.expected_rows(B, H, W, True), (B, H, W)
        assert lib.mobgs_flow_warp_loss_bwd_rows(B, H, W, 0) == 4
    for B, H, W in ((0, 8, 8), (1, 1, 8), (1, 8, 1), (-3, 8, 8)):
        assert lib.mobgs_flow_warp_loss_bwd_rows(B, H, W, 1) == -1
        assert b"mobgs_flow_warp_loss_bwd_rows" in lib.mobgs_last_error() and b"bad sizes" in lib.mobgs_last_error()


@pytest.mark.parametrize("name", ["rows_tail4", "tall8_b", "white_noise_4"])
def test_plain_stores_are_bit_reproducible_and_atomic_sums_stay_in_bound(hip_device, name):
    c = C.case(name)
    rows = _build(c, True)
    first = _run(c, hip_device, True)
    for run in ("second", "third"):
        again = _run(c, hip_device, True)
        for k in C.PLAIN + ("loss",):
            assert same_bits(first[k], again[k]), (run, k)
        C.compare(name, rows, again, f"{name} {run} run", keys=C.SCATTER, loss=False)  # atomic sums: the bound, each time


def _abi_call(c, dev, want, combine=1, scratch=True):
    """mobgs_flow_warp_loss_fwd + _bwd through ctypes with the gradient pointers `want` non-NULL and the others NULL.
    -> (rc of bwd, {loss, requested gradients} on the CPU).  Plain-store outputs start as NaN, scatter targets as zeros."""
    from mobgs_amd import _lib as L
    lib = L.load()
    B, Kx, H, W = c.B, c.K, c.H, c.W
    t = {k: x.to(dev) for k, x in c.inputs.items()}
    partial = torch.empty(lib.mobgs_flow_warp_loss_blocks(B, H, W), 4, device=dev)
    out = torch.empty(5, device=dev)
    L.check(lib.mobgs_flow_warp_loss_fwd(B, Kx, H, W, *(L.ptr(t[k]) for k in C.NAMES), L.ptr(partial), L.ptr(out),
                                         L.ptr(out[4:]), L.stream()), "mobgs_flow_warp_loss_fwd")
    v = torch.tensor([c.v], device=dev)
    g = {k: None for k in C.NAMES}
    for k in want:
        g[k] = torch.zeros_like(t[k]) if k in C.SCATTER else torch.full_like(t[k], float("nan"))
    buf = None
    if scratch:
        buf = torch.empty(lib.mobgs_flow_warp_loss_bwd_scratch_floats(B, Kx, H, W), device=dev)
    rc = lib.mobgs_flow_warp_loss_bwd(B, Kx, H, W, *(L.ptr(t[k]) for k in C.NAMES), L.ptr(out), L.ptr(v),
                                      *(L.ptr(g[k]) for k in C.NAMES), L.ptr(buf), combine, L.stream())
    torch.cuda.synchronize()
    res = {k: g[k].cpu() for k in want}
    res["loss"] = out[4].cpu()
    return rc, res


@pytest.mark.parametrize("name", ["rows_tail4", "tall8_b"])
def test_gradient_subsets_at_the_c_abi(hip_device, name):
    """Any gradient pointer may be NULL: each single one alone (the two image gradients separately, too -- the launcher
    handles each on its own), the four plain stores without a scratch buffer."""
    c = C.case(name)
    rows = _build(c, True)
    rc, full = _abi_call(c, hip_device, C.NAMES)
    assert rc == 0
    C.compare(name, rows, full, f"{name} C ABI, all six")
    for key in C.NAMES:
        rc, one = _abi_call(c, hip_device, (key,), scratch=key in C.SCATTER)
        assert rc == 0 and same_bits(one["loss"], full["loss"]), key
        if key in C.SCATTER:
            C.compare(name, rows, one, f"{name} C ABI, g_{key} alone", keys=(key,), loss=False)
        else:
            assert same_bits(one[key], full[key]), key
    rc, four = _abi_call(c, hip_device, C.PLAIN, scratch=False)
    assert rc == 0 and all(same_bits(four[k], full[k]) for k in C.PLAIN)


def test_image_gradient_without_scratch_is_refused(hip_device):
    from mobgs_amd import _lib as L
    c = C.case("w65")
    for want in (("ori",), ("latent",), C.NAMES):
        rc, _ = _abi_call(c, hip_device, want, scratch=False)
        assert rc == L._DEFINES["MOBGS_E_INVALID"] == -1
        msg = L.load().mobgs_last_error()
        assert b"mobgs_flow_warp_loss_bwd: image gradients need the scratch buffer" in msg
        assert b"mobgs_flow_warp_loss_bwd_scratch_floats" in msg


@pytest.mark.parametrize("name", ["rows_tail4", "tall8_b"])
def test_gradients_are_linear_in_the_cotangent(hip_device, name):
    """v and 2 v: a power of two, so the plain-store gradients double exactly; the loss does not move."""
    c = C.case(name)
    one, two = _run(c, hip_device, True, v=c.v), _run(c, hip_device, True, v=2 * c.v)
    assert same_bits(one["loss"], two["loss"])
    for k in C.PLAIN:
        assert one[k].abs().max() > 0 and same_bits(2 * one[k], two[k]), k
    rows = _build(c, True)
    half = {k: 0.5 * two[k] for k in C.SCATTER}  # exact halves: the atomic sums of 2 v, held to the bound of v
    C.compare(name, rows, half, f"{name} at 2 v, halved", keys=C.SCATTER, loss=False)


def test_other_layouts_and_alignments(hip_device):
    """The same data 4, 8 and 12 bytes past a 16-byte boundary (the coordinate pairs are read as float2, the image gradients
    are summed as float4 where they can be) and as non-contiguous views: plain-store outputs and loss keep their bits."""
    dev = hip_device
    c = C.case("smooth_a")  # B = 2: a channel slice is not contiguous
    rows = _build(c, True)
    plain = _run(c, dev, True)

    def shifted(x, k):
        buf = torch.zeros(x.numel() + 4, device=dev)
        view = buf[k:k + x.numel()]
        view.copy_(x.reshape(-1))
        view = view.view(x.shape)
        assert view.data_ptr() % 16 == 4 * k and view.is_contiguous()
        return view.requires_grad_(True)

    for shifts in ((1, 1, 1, 1, 1, 1), (3, 2, 1, 3, 2, 1), (0, 1, 3, 2, 0, 3)):
        got = _run(c, dev, True, inputs={k: shifted(c.inputs[k], s) for k, s in zip(C.NAMES, shifts)})
        for k in C.PLAIN + ("loss",):
            assert same_bits(got[k], plain[k]), (shifts, k)
        C.compare(c.name, rows, got, f"smooth_a shifted by {shifts}", keys=C.SCATTER, loss=False)
    # channel / component slices of wider tensors, and a permuted coordinate map
    wide = {"ori": torch.rand(c.B, 5, c.H, c.W), "latent": torch.rand(c.B, c.K, 4, c.H, c.W),
            "e2m": torch.rand(c.B, c.K, c.H, c.W, 3), "la": torch.rand(c.B, c.K, 2, c.H, c.W),
            "da": torch.rand(c.B, 3, c.H, c.W)}
    cut = {"ori": lambda w: w[:, 1:4], "latent": lambda w: w[:, :, 1:4], "e2m": lambda w: w[..., 1:3],
           "la": lambda w: w[:, :, 1:2], "da": lambda w: w[:, 2:3]}
    for k in wide:
        cut[k](wide[k]).copy_(c.inputs[k])
        wide[k] = wide[k].to(dev).requires_grad_(True)
    m2e = c.inputs["m2e"].permute(0, 1, 4, 2, 3).contiguous().to(dev).requires_grad_(True)  # [B,K,2,H,W]
    inputs = {k: cut[k](wide[k]) for k in wide}
    inputs["m2e"] = m2e.permute(0, 1, 3, 4, 2)
    assert not any(t.is_contiguous() for t in inputs.values())
    from mobgs_amd.loss_utils import flow_warp_loss
    loss = flow_warp_loss(*(inputs[k] for k in C.NAMES))
    loss.backward(torch.tensor(c.v, device=dev))
    got = {k: cut[k](wide[k].grad).cpu() for k in wide}
    got["m2e"] = m2e.grad.permute(0, 1, 3, 4, 2).cpu()
    got["loss"] = loss.detach().cpu()
    for k in C.PLAIN + ("loss",):
        assert same_bits(got[k], plain[k]), k
    C.compare(c.name, rows, got, "smooth_a as views", keys=C.SCATTER, loss=False)
    assert float(wide["ori"].grad[:, 0].abs().max()) == 0.0 and float(wide["e2m"].grad[..., 0].abs().max()) == 0.0
