"""The two BLCE kernels (csrc/blce.hip through mobgs_amd.blce._FusedView, FUSED on, graph capture off) against the torch
module of mobgs_amd/blce.py evaluated in float64 on the CPU, on the cases of tests/blce_cases.py.

Cases (tests/test_blce_cases_cpu.py shows from the float64 module alone that each reaches its regime and that none of its 320
ReLU units is near a kink): the state of tests/golden/blce.npz; the module exactly as its constructor leaves it -- decoder
gain 1e-5, rot and theta ~1e-6, 1 - cosf(theta) == 0, the state training starts in --; |rot| == 0 (coef = 0, gradient
Vu x 1e10); |theta| > pi and |trans| >= 1; dead units in both hidden layers and negative trajectory units; the camera 100
units from the origin (the cofactor inverse in fp32); (view, table size) = (0, 1), (2, 3), (0, 200), (199, 200): the zeroing
loop of the embedding-table gradient shorter than one trip, with a tail and with 100 trips.  Each with cotangents on both
outputs, on c2w only and on w2c only.

Compared per tensor -- the 9 c2w poses, the 9 w2c poses, each of the 22 parameter gradients -- with
deform_cases.close_to_f64 at k = 3 (a rule that needs no run of the code under test), exact zeros
where float64 has them (the last time-embedding row, every other row of the embedding table).  The gap of a tensor is
the largest of nine draws of the fp32 module's own error -- the case and eight inputs within half an ulp of it
(tests/blce_cases.py, neighbour allowance) --; a RATIO line shows the k of the plain rule unless it says `with extra`.  One case runs twice: the
kernels are single-wave and bit-reproducible.

Worst k needed on an MI355X per family (docs/MEASUREMENT_LOG.md, "Loss, normals and BLCE kernels against float64"):

    family                   worst k needed (case [cotangent], tensor)                                       k
    poses                    2.77  (large, w2c); c2w of `large` needs 4.39 alone, 1.22 against nine draws     3
    parameter gradients      2.93  (large [w2c], theta_decoder.bias); 22 of 660 tensors need more than 3      3
                             alone -- worst 13.9 (init [both], theta_decoder.bias, one entry), 12.2
                             (view_199_of_200 [c2w], v_linear.bias), 11.4 (fixture [both], theta_decoder.bias)
                             -- and at most 1.89 against nine draws (on the inputs of those tensors the fp32
                             module's gap on a neighbouring input is 4 to 65 times its gap on the case itself)"""
import copy

import pytest
import torch

import blce_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture()
def fused(monkeypatch):
    from mobgs_amd import blce as B
    monkeypatch.setattr(B, "FUSED", True)
    monkeypatch.setattr(B, "GRAPH_CAPTURE", False)
    return B


_on_device = {}


def _model(name, dev):
    if name not in _on_device:
        _on_device[name] = copy.deepcopy(C.case(name).model).to(dev)
    return _on_device[name]


def _run(B, name, cot, dev):
    c = C.case(name)
    params = B._view_param_list(_model(name, dev), c.idx)
    for p in params:
        p.grad = None
    c2w, w2c = B._FusedView.apply(c.Rt.to(dev), c.bf.to(dev), c.idx, c.num_views, *params)
    C.backward((c2w, w2c), [None if v is None else v.to(dev) for v in c.cots[cot]])
    assert all(p.grad is not None and p.grad.shape == p.shape for p in params)
    return {"c2w": c2w.detach(), "w2c": w2c.detach(), "grads": [p.grad.clone() for p in params]}


@pytest.mark.parametrize("cot", C.COTS)
@pytest.mark.parametrize("name", C.CASES)
def test_blce_matches_float64(hip_device, fused, name, cot):
    got = _run(fused, name, cot, hip_device)
    C.compare(name, cot, got, f"blce {name} [{cot}]")
    assert not got["grads"][11][8].any()  # the last time-embedding row is never used


def test_blce_is_bit_reproducible(hip_device, fused):
    a, b = _run(fused, "fixture", "both", hip_device), _run(fused, "fixture", "both", hip_device)
    assert torch.equal(a["c2w"], b["c2w"]) and torch.equal(a["w2c"], b["w2c"])
    assert all(torch.equal(x, y) for x, y in zip(a["grads"], b["grads"]))
