"""tests/blce_cases.py checked from the float64 module alone (no GPU): every case reaches the regime it is named after, no
ReLU unit of any case is near a kink, the restated forward is the module's, and the comparator at k = 3 accepts the fp32
module and rejects both planted errors."""
import math

import pytest
import torch

import blce_cases as C


def _parts(name, dtype=torch.float64):
    c = C.case(name)
    with torch.no_grad():
        return C.forward_parts(C.typed_model(name, dtype), c.Rt.to(dtype), c.bf.to(dtype), c.idx)


@pytest.mark.parametrize("name", C.CASES)
def test_no_unit_is_near_a_kink(name):
    c = C.case(name)
    print(f"BLCE {name}: seed {c.seed}, {c.near} of {c.units} ReLU units near a kink ({c.near / c.units:.2%})")
    assert c.units == 320 and c.near / c.units <= C.MAX_NEAR
    assert c.near == 0  # fp32 and float64 take the same branch everywhere: no flip allowance exists
    P64, P32 = _parts(name), _parts(name, torch.float32)
    for key in ("z1", "z2"):
        assert torch.equal(getattr(P64, key) > 0, getattr(P32, key) > 0)
    assert torch.equal(P64.xs[:8] > 0, P32.xs[:8] > 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_restated_forward_is_the_modules(dtype):
    for name in ("fixture", "init", "zero_rot", "view_199_of_200"):
        c = C.case(name)
        m = C.typed_model(name, dtype)
        with torch.no_grad():
            want = m(c.Rt.to(dtype), c.bf.to(dtype), c.idx)[0]
            assert torch.equal(C.forward_parts(m, c.Rt.to(dtype), c.bf.to(dtype), c.idx).c2w, want), name


def test_fixture_case_is_the_fixtures_state():
    c, fx = C.case("fixture"), C._fixture()
    assert c.idx == 1 and c.num_views == 3 and float(c.bf) == float(fx["out_blur"])
    with torch.no_grad():
        out = c.model(c.Rt, c.bf, c.idx)[0]
    assert float((out - torch.from_numpy(fx["out_Rt_new"])).abs().max()) <= 1e-5


def test_init_is_the_state_training_starts_in():
    c = C.case("init")
    fresh = C._seeded_model(3, c.seed)
    assert all(torch.equal(a, b) for a, b in zip(fresh.state_dict().values(), c.model.state_dict().values()))
    assert not c.model.view_embedder.any() and not c.model.rot_decoder[c.idx].bias.any()
    P, P32 = _parts("init"), _parts("init", torch.float32)
    n = P.w_rigid.norm(dim=-1)
    print(f"init: |rot| {float(n.min()):.2e} .. {float(n.max()):.2e}, |theta| up to {float(P.theta.abs().max()):.2e}")
    assert 1e-10 < float(n.min()) and float(n.max()) < 1e-4 and 0 < float(P.theta.abs().max()) < 1e-4
    assert not (1 - torch.cos(P32.theta)).any() and (1 - torch.cos(P.theta)).all()  # 1 - cosf(theta) == 0 in fp32 only


def test_zero_rot_has_the_finite_gradient_vu_times_1e10():
    c = C.case("zero_rot")
    m = C.typed_model("zero_rot", torch.float64)
    P = C.forward_parts(m, c.Rt.double(), c.bf.double(), c.idx)
    assert not P.w_rigid.any() and not P.w_unit.any() and P.theta.abs().min() > 1e-3
    P.w_rigid.retain_grad()
    P.w_unit.retain_grad()
    C.backward((P.c2w, torch.inverse(P.c2w)), c.cots["both"])
    assert torch.isfinite(P.w_rigid.grad).all() and P.w_unit.grad.abs().min() > 0
    assert torch.allclose(P.w_rigid.grad, P.w_unit.grad * 1e10, rtol=1e-12, atol=0)  # Vu / (0 + 1e-10), and coef = 0
    r64, r32 = C.reference("zero_rot", "both")
    g = r64["grads"][C.PARAM_NAMES.index("rot_decoder.bias")]
    assert torch.allclose(g, P.w_rigid.grad.sum(0), rtol=1e-9) and float(g.abs().max()) > 1e6
    assert all(torch.isfinite(t).all() for t in r32["grads"])


def test_large_dead_relu_and_far_camera_reach_their_regimes():
    P = _parts("large")
    assert int((P.theta.abs() > math.pi).sum()) >= 2 and float(P.v_rigid.abs().max()) >= 1.0
    P = _parts("dead_relu")
    assert (P.z1[:16] < -1).all() and (P.z2[:16] < -1).all()  # half of both hidden layers: dead, and far from the kink
    assert int((P.z1 > 0).sum()) >= 4 and int((P.z2 > 0).sum()) >= 4
    negative = (P.xs[:8] < 0).any(dim=0)
    print(f"dead_relu: {int((P.z1 <= 0).sum())} / {int((P.z2 <= 0).sum())} dead hidden units, {int(negative.sum())} of 32 "
          f"trajectory units negative at some step")
    assert int(negative.sum()) >= 8
    c = C.case("far_camera")
    assert abs(float(c.Rt[:3, 3].norm()) - 100.0) < 1e-3
    assert torch.equal(c.Rt[:3, :3], C.case("fixture").Rt[:3, :3])


def test_view_cases_cover_the_three_shapes_of_the_zeroing_loop():
    got = {(C.case(n).idx, C.case(n).num_views) for n in C.CASES if n.startswith("view_")}
    assert got == set(C.VIEWS)
    assert 1 * 32 < 64 and 3 * 32 == 64 + 32 and 200 * 32 == 100 * 64  # shorter than one trip, a tail, 100 trips
    for name in ("view_0_of_200", "view_199_of_200"):
        c = C.case(name)
        table = C.reference(name, "both")[0]["grads"][0]
        assert tuple(table.shape) == (200, 32) and table[c.idx].abs().min() > 0
        assert int(table.any(dim=1).sum()) == 1


@pytest.mark.parametrize("name", C.CASES)
def test_comparator_accepts_the_fp32_module(name):
    for cot in C.COTS:
        r64, r32 = C.reference(name, cot)
        assert len(r64["grads"]) == 22 and not r64["grads"][11][8].any()  # the last time-embedding row is never used
        C.compare(name, cot, r32, f"fp32 module {name} [{cot}]")


def test_planted_error_unguarded_division_is_nan_and_rejected():
    bad = C.evaluate("zero_rot", "both", torch.float32, unit=C.UnitNoGuard.apply)
    assert torch.isnan(bad["grads"][C.PARAM_NAMES.index("rot_decoder.weight")]).all()  # 0 / 0 at |rot| == 0
    with pytest.raises(AssertionError):
        C.compare("zero_rot", "both", bad, "planted (a) zero_rot")
    ok = C.evaluate("fixture", "both", torch.float32, unit=C.UnitNoGuard.apply)  # away from 0 it is the same function
    C.compare("fixture", "both", ok, "unguarded division, |rot| > 0")


def test_planted_error_last_time_embedding_row_is_rejected():
    for name in ("fixture", "init"):
        r32 = C.reference(name, "both")[1]
        bad = dict(r32, grads=[g.clone() for g in r32["grads"]])
        bad["grads"][11][8] = bad["grads"][11][7]
        assert bad["grads"][11][8].any()
        with pytest.raises(AssertionError):
            C.compare(name, "both", bad, f"planted (b) {name}")
