"""The per-splat state build by itself (ops.PrepSplats: csrc/prep.hip + csrc/prep_shared.h, forward and backward with
cotangents for all five outputs) against the float64 restatement of tests/splat_cases.py, row by row.

Cases (tests/test_splat_cases_cpu.py shows from the oracle alone that each reaches its edge): one row of either kind, dynamic
rows that start inside a wave / at a wave / run into a second workgroup (prep_bwd_clear_rows), every knot count 4 .. 12 in
every case with nine dynamic rows, times at the curve's ends, exactly on knots (not filtered: the spline and its control-point
gradient are continuous there) and outside [0, 1], three instants in one launch, two backward passes into one
ops.LeafGradSink, and half attribute storage.  Compared in full, no flip allowance:
  * per tensor, `close_to_f64`: max |got - ref64| <= k max |ref32 - ref64| + 2^-23 max |ref64|, and exact zeros where the
    reference has them (knots beyond a row's count, the static f_t);
  * per row within each stratum (static / dynamic, and per knot count for positions and control-point gradients),
    `rows_close_to_f64`: with e_i = |got_i - ref64_i|_inf / (|ref64_i|_inf + 1e-3 median row norm), max_i e_i and
    median_i e_i are each at most k x the same statistic of the fp32 restatement;
  * `accumulate`: the first pass alone equals the non-accumulating run bit for bit, the sum obeys the same rules;
  * `half`: the references are evaluated on the half-rounded values, and a gradient stored as half gets the one rounding
    to half on top: 2^-11 |ref| per element (2^-25 below the normal range).
  * the two host bodies (csrc/fastpath.cpp and the Python one in ops.py fill MobgsPrepInputs / MobgsLeafGrads each on its
    own): `k3`, `half` and `accumulate` -- a second workgroup, K > 1, the binary16 flag on both records, accumulate = 1 --
    run with the fast path on and off; every output and leaf gradient is bit-identical, and obeys the rules above.
k = 3 (three times the fp32 reference's own gap, a rule that needs no run of the code under test).

Worst k needed on an MI355X per family (docs/MEASUREMENT_LOG.md, "Per-splat kernels against float64"):

    family                               worst k needed (case, tensor / stratum)                   k
    outputs, per tensor                  0.18  (k3, means)                                          3
    outputs, per row                     1.79  (outside_hi, opac / static, 40 rows)                 3
    leaf gradients, per tensor           0.69  (accumulate sum, s_opacity)                          3
    leaf gradients, per row              1.68  (outside_lo, s_opacity / static, 40 rows)            3
"""
from types import SimpleNamespace

import pytest
import torch

import splat_cases as S

pytestmark = pytest.mark.gpu

K = {"outputs": 3, "leaves": 3}


def _leaves(case, dev):
    """The 13 leaves on the device (attributes as halves in `half`) and the 16 arguments of PrepSplats.apply."""
    L = {k: (v.half() if case.half and k in S.HALF_LEAVES else v).to(dev).requires_grad_(True) for k, v in case.leaves.items()}
    return L, lambda times: (times.to(dev), L["s_xyz"], L["s_scaling"], L["s_rotation"], L["s_opacity"], L["s_fdc"], L["s_ft"],
                             L["d_control"], case.d_ncp.to(dev), L["d_scaling"], L["d_rotation"], L["d_omega"],
                             L["d_opacity"], L["d_fdc"], L["d_ft"], case.d_trbf.to(dev))


def _compare(case, got, ref64, ref32, keys, family, tag):
    for key in keys:
        g, r64, r32 = got[key], ref64[key], ref32[key]
        assert g is not None and tuple(g.shape) == tuple(r64.shape), (key, None if g is None else tuple(g.shape))
        if g.dtype == torch.float16:  # one rounding to half, derived, taken off before either comparator looks
            g = S.shrink(g, r64, S.half_allowance(r64))
        S.close_to_f64(g, r64, r32, K[family], f"{tag} [{family}] {key}")
        S.rows_close_to_f64(g, r64, r32, S.prep_row_strata(case, key), S.COLS[key], K[family], f"{tag} [{family}] {key}")


def _single_run(case, dev):
    """One forward + backward pass -> (the five outputs, the 13 leaf gradients)."""
    from mobgs_amd import ops
    L, args = _leaves(case, dev)
    outs = ops.PrepSplats.apply(*args(case.times))
    torch.autograd.backward(outs, [c.to(dev) for c in case.cots])
    torch.cuda.synchronize()
    return dict(zip(S.PREP_OUTPUTS, outs)), {k: L[k].grad for k in S.LEAVES}


def _sink_run(case, dev):
    """`accumulate`: the first pass alone, then both passes into one ops.LeafGradSink -> (outputs of the first pass, its
    gradients from the non-accumulating run, the sink's buffers after the first pass, the leaves' .grad after both)."""
    from mobgs_amd import ops
    L, args = _leaves(case, dev)
    cots1, cots2 = ([c.to(dev) for c in cs] for cs in (case.cots, case.cots2))
    # the non-accumulating run of the first pass
    torch.autograd.backward(ops.PrepSplats.apply(*args(case.times)), cots1)
    plain = {k: L[k].grad.clone() for k in S.LEAVES}
    for t in L.values():
        t.grad = None
    stat = SimpleNamespace(_xyz=L["s_xyz"], _scaling=L["s_scaling"], _rotation=L["s_rotation"], _opacity=L["s_opacity"],
                           _features_dc=L["s_fdc"], _features_t=L["s_ft"])
    dyn = SimpleNamespace(get_control_xyz=L["d_control"], _scaling=L["d_scaling"], _rotation=L["d_rotation"],
                          _omega=L["d_omega"], _opacity=L["d_opacity"], _features_dc=L["d_fdc"], _features_t=L["d_ft"])
    outs1 = ops.PrepSplats.apply(*args(case.times))
    outs2 = ops.PrepSplats.apply(*args(torch.tensor(S.T_SECOND)))
    with ops.LeafGradSink(stat, dyn) as sink:
        torch.autograd.backward(outs1, cots1)
        assert sink.buffers is not None and all(L[k].grad is None for k in S.LEAVES)  # the kernel wrote the sink's buffers
        first = {k: sink.buffers[k].clone() for k in S.LEAVES}
        torch.autograd.backward(outs2, cots2)
    torch.cuda.synchronize()
    return dict(zip(S.PREP_OUTPUTS, outs1)), plain, first, {k: L[k].grad for k in S.LEAVES}


def _check_single(case, outs, got, ref64, ref32, tag):
    assert all(o.dtype == torch.float32 for o in outs.values())
    _compare(case, outs, ref64, ref32, S.PREP_OUTPUTS, "outputs", tag)
    if case.half:
        assert all(got[k].dtype == torch.float16 for k in S.HALF_LEAVES) and got["d_control"].dtype == torch.float32
    _compare(case, got, ref64, ref32, S.LEAVES, "leaves", tag)
    if case.K == 1:  # the static positions pass their cotangent on untouched
        assert torch.equal(got["s_xyz"].cpu(), case.cots[0][:case.Ns])


def _check_sink(case, outs1, plain, first, total, ref64, ref32, tag):
    for k in S.LEAVES:  # the first pass alone: the non-accumulating run, bit for bit
        assert torch.equal(first[k].view_as(plain[k]), plain[k]), k
    _compare(case, outs1, ref64, ref32, S.PREP_OUTPUTS, "outputs", tag)
    _compare(case, first, ref64["first"], ref32["first"], S.LEAVES, "leaves", tag + " first pass")
    _compare(case, total, ref64, ref32, S.LEAVES, "leaves", tag + " sum")


@pytest.mark.parametrize("name", [n for n in S.PREP_CASES if n != "accumulate"])
def test_prep_matches_float64(hip_device, name):
    from mobgs_amd import ops
    assert tuple(ops._LEAF_NAMES) == S.LEAVES
    case = S.prep_case(name)
    outs, got = _single_run(case, hip_device)
    _check_single(case, outs, got, *S.prep_reference(name), f"prep {name}")


def test_prep_accumulates_two_passes_in_a_sink(hip_device):
    case = S.prep_case("accumulate")
    _check_sink(case, *_sink_run(case, hip_device), *S.prep_reference("accumulate"), "prep accumulate")


@pytest.mark.parametrize("name", ["k3", "half", "accumulate"])
def test_prep_host_bodies_agree_bit_for_bit(hip_device, name):
    """csrc/fastpath.cpp and the Python body of ops.py each fill MobgsPrepInputs / MobgsLeafGrads themselves: a swapped
    member in one of them shows here as a difference between the two, not only inside a full render."""
    from mobgs_amd import _fast
    case = S.prep_case(name)
    run, check = (_sink_run, _check_sink) if name == "accumulate" else (_single_run, _check_single)
    was = _fast.enabled
    results = {}
    try:
        for on in (True, False):
            _fast.reset(on)
            assert (_fast.get() is not None) == on, _fast.load_error
            results[on] = run(case, hip_device)
    finally:
        _fast.reset(was)
    for on in (True, False):
        check(case, *results[on], *S.prep_reference(name), f"prep {name} [fast path {'on' if on else 'off'}]")
    for i, (a, b) in enumerate(zip(results[True], results[False])):
        assert a.keys() == b.keys()
        for k in a:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (i, k)
