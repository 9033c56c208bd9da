"""CPU checks of the densification controller's restatements and cases (tests/control_cases.py): the restated schedule and
bounds mask reproduce what the reference's own controlgaussians / removeminmax did (tests/golden/controlgaussians_trace.json,
written by tests/golden/make_golden_control.py), mobgs_amd.helper_train.controlgaussians gives the same trace on a
recording stand-in, and the inputs of every GPU case of tests/test_gpu_densify_control.py are what the cases need."""
import json
import os
import types

import pytest
import torch

import control_cases as C
import densify_restatement as R

TRACE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "controlgaussians_trace.json")


@pytest.fixture(scope="module")
def trace():
    with open(TRACE) as f:
        return json.load(f)


def test_the_fixture_covers_what_it_is_meant_to(trace):
    runs = trace["runs"]
    assert len({r["name"] for r in runs}) >= 3 and {r["is_dynamic"] for r in runs} == {False, True}
    static = [r for r in runs if not r["is_dynamic"]]
    assert any(0 < r["options"]["desicnt"] == r["final_flag"] and r["flags"][10][1] == r["final_flag"] for r in static)
    assert any(r["final_flag"] == r["options"]["desicnt"] > 30 for r in static)                # reached late
    assert any(r["final_flag"] < r["options"]["desicnt"] for r in static)                      # never reached
    assert any(r["options"]["densify_from_iter"] % r["options"]["densification_interval"] for r in runs)
    assert any(r["options"]["densify_until_iter"] < r["last_iteration"] for r in runs)
    assert all(r["last_iteration"] > 6000 for r in runs)
    names = {c["name"] for r in runs for c in r["calls"]}
    assert names == {"densify_pruneclone", "prune_points", "reset_opacity"}
    assert all(r["final_flag"] == 0 for r in runs if r["is_dynamic"])


def test_restated_schedule_reproduces_the_reference_call_for_call(trace):
    for r in trace["runs"]:
        mine = C.schedule(r["options"], r["last_iteration"], r["is_dynamic"], r["extent"], trace["opacity"])
        assert mine["calls"] == r["calls"], (r["name"], r["is_dynamic"])
        assert mine["flags"] == r["flags"] and mine["final_flag"] == r["final_flag"], (r["name"], r["is_dynamic"])


def test_controlgaussians_of_the_package_gives_the_same_trace(trace):
    from mobgs_amd.helper_train import controlgaussians
    for r in trace["runs"]:
        opt = types.SimpleNamespace(**r["options"])
        scene = types.SimpleNamespace(cameras_extent=r["extent"])
        rec, flag, every = C.Recorder(trace["opacity"]), 0, []
        for it in range(1, r["last_iteration"] + 1):
            rec.iteration = it
            flag = controlgaussians(opt, rec, 2, it, scene, None, None, None, flag, is_dynamic=r["is_dynamic"])
            every.append(flag)
        assert rec.calls == C.reduced(r["calls"]), (r["name"], r["is_dynamic"])
        # the fixture lists flag at the iterations with a call; it cannot change anywhere else
        want, at = [], dict(map(tuple, r["flags"]))
        for it in range(1, r["last_iteration"] + 1):
            want.append(at.get(it, want[-1] if want else 0))
        assert every == want and flag == r["final_flag"], (r["name"], r["is_dynamic"])


def test_modes_1_and_3_raise_and_name_the_reason():
    from mobgs_amd.helper_train import controlgaussians
    opt = types.SimpleNamespace(densify_until_iter=10)
    with pytest.raises(NotImplementedError, match="omega freeze"):
        controlgaussians(opt, None, 1, 1, None, None, None, None, 0)
    with pytest.raises(NotImplementedError, match="breakpoint"):
        controlgaussians(opt, None, 3, 1, None, None, None, None, 0)


def test_restated_bounds_mask_equals_the_reference(trace):
    b = trace["bounds"]
    xyz = torch.tensor([[float("nan") if v is None else v for v in row] for row in b["xyz"]], dtype=torch.float32)
    want = torch.tensor(b["mask"])
    assert torch.equal(C.bounds_mask(xyz, b["maxbounds"], b["minbounds"]), want)
    assert bool(torch.isnan(xyz).any()) and 6 <= int(want.sum()) < want.shape[0]
    hi, lo = torch.tensor(b["maxbounds"]), torch.tensor(b["minbounds"])
    assert int(((xyz == hi) | (xyz == lo)).any(dim=1).sum()) >= 6        # rows exactly on a bound: kept
    assert not bool(want[((xyz == hi) | (xyz == lo)).any(dim=1)].any())
    index, counts = C.plan_prune(want)
    assert counts.tolist() == [int((~want).sum()), 0, 0, int((~want).sum())] and bool((index[1:] > index[:-1]).all())


@pytest.mark.parametrize("n", C.PLAN_NS)
def test_plan_inputs_exercise_every_section_and_stay_clear_of_the_decisions(n):
    inp = C.plan_inputs(n, 9000 + n)
    assert all(v.shape[0] == n for v in inp.values())
    if n == 0:
        for op in C.PLAN_OPS:
            index, counts = C.plan_expected(op, inp, 2)
            assert index.numel() == 0 and counts.tolist() == [0, 0, 0, 0]
        return
    # device expf against host exp can flip neither a size decision nor an opacity decision
    assert R.size_margin(inp["scaling"], C.SIZE_THR) > 1e-4
    assert C.opacity_margin(inp["opacity"], C.MIN_OPACITY) > 1e-4
    for n_split in C.PLAN_SPLITS:
        index, counts = C.plan_expected("PRUNECLONE", inp, n_split)
        kept, clones, parents, n_out = counts.tolist()
        assert n_out == kept + clones + n_split * parents == index.shape[0] <= n * max(2, n_split)
        assert kept + parents == n
        if n > 1:
            assert kept > 0 and clones > 0 and parents > 0
    for op in C.PLAN_OPS[1:]:
        index, counts = C.plan_expected(op, inp, 1)
        if n > 1:
            assert 0 < counts[0] < n, op
        assert bool((index >= 0).all()) and bool((index[1:] > index[:-1]).all())
    if n > 12:
        drop = C.bounds_mask(inp["xyz"], C.MAXB, C.MINB)
        assert drop[:12].tolist() == [False, True] * 6 and not bool(drop[12])   # on a bound, one ulp outside; NaN


@pytest.mark.parametrize("n,n_views,grad_stride,row0", C.STATS_CASES)
def test_stats_inputs_leave_rows_visible_and_rows_unseen(n, n_views, grad_stride, row0):
    state, steps = C.stats_inputs(n, n_views, grad_stride, row0, 17 * n + n_views)
    assert len(steps) == 3
    seen_some = False
    for grads, radii in steps:
        assert len(grads) == len(radii) == n_views and grads[0].shape == (row0 + n + 5, grad_stride)
        new, total, radii_max, visible = C.batch_stats(state, grads, radii, row0, n, 640, 360)
        assert n == 1 or 0 < int(visible.sum()) < n
        seen_some |= bool(visible.any())
        assert torch.equal(new["denom"][~visible], state["denom"][~visible])
        assert torch.equal(visible, radii_max > 0)
        if n_views > 1 and n >= 255:   # the norm of the sum is not the sum of the norms
            norms = sum(torch.sqrt((g[row0:row0 + n, :2].double() * torch.tensor([320.0, 180.0])).pow(2).sum(1)) for g in grads)
            assert float((norms - total.double().norm(dim=1)).abs().max()) > 1e-3
        state = new
    assert seen_some or n == 1


def test_batch_stats_with_one_view_is_the_per_view_update():
    state, steps = C.stats_inputs(300, 1, 2, 0, 5)
    grads, radii = steps[0]
    new, total, radii_max, visible = C.batch_stats(state, grads, radii, 0, 300, 2, 2)   # W / 2 = H / 2 = 1
    want = R.add_densification_stats(state, grads[0][:300], None, radii[0][:300])
    assert all(torch.equal(new[k], want[k]) for k in want)


def test_header_enums_join_the_constants_and_fail_loudly():
    """include/mobgs_hip.h selects the plan's op by an enum: mobgs_amd/_lib.py reads the enumerators with the defines."""
    from mobgs_amd import _lib
    good = "typedef enum MobgsOp { MOBGS_A = 0, MOBGS_B = 3 } MobgsOp;\nint mobgs_f(int op);\n"
    defines, _, sigs = _lib._parse_header(good)
    assert defines == {"MOBGS_A": 0, "MOBGS_B": 3} and list(sigs) == ["mobgs_f"]
    for bad, what in (("typedef enum E { MOBGS_C } E;", "MOBGS_C"),             # an enumerator without a value
                      ("typedef enum E { MOBGS_C = 1 } F;", "typedef'd as F")):
        with pytest.raises(ValueError, match=what):
            _lib._parse_header(good + bad)
    D = _lib._DEFINES
    assert [D["MOBGS_PLAN_" + op] for op in C.PLAN_OPS] == [0, 1, 2, 3]
    assert "mobgs_densify_plan" in _lib._SIGS and "mobgs_densify_stats_batch" in _lib._SIGS
