"""Learning-rate schedules and the host tables of mobgs_amd.optim.DeviceAdam, without a GPU.

tests/golden/lr_schedule.npz holds the rates of the reference's own get_expon_lr_func (tests/golden/make_golden_lr.py
imports it in place).  The restatement is the same float64 statements, so it can differ from the fixture only where numpy's
exp / log differ in the last place between two machines (vector or scalar loops, another libm): one ulp in each of the two
logarithms, whose magnitudes are at most 16, is 16 * 2^-52 = 3.6e-15 absolute in the exponent each, i.e. 7.1e-15 relative
in the result, plus the exp's own ulp (2.2e-16) and the roundings of the three products and the sum (a few 1e-16 of an
exponent of magnitude <= 16: < 2e-15): below 1e-14 relative.  The bound is that sum, not a measurement.
"""
import math
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lr_schedule.npz")
ITERATIONS = [-1, 0, 1, 2, 99, 100, 101, 4999, 9999, 10000, 10001, 30000]
REL = 1e-14


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_fixture_holds_the_cases_it_should(golden):
    assert golden["iterations"].tolist() == ITERATIONS
    assert set(golden["names"].tolist()) == {"xyz", "grid", "deformation", "delayed", "both_zero"}
    a = golden["delayed.args"]
    assert a[2] == 100 and a[3] == 0.01
    assert golden["both_zero.args"][0] == 0.0 and golden["both_zero.args"][1] == 0.0


@pytest.mark.parametrize("name", ["xyz", "grid", "deformation", "delayed", "both_zero"])
def test_get_expon_lr_func_matches_the_reference(golden, name):
    from mobgs_amd.general_utils import get_expon_lr_func
    a, b, steps, mult, max_steps = golden[name + ".args"].tolist()
    fn = get_expon_lr_func(lr_init=a, lr_final=b, lr_delay_steps=int(steps), lr_delay_mult=mult, max_steps=int(max_steps))
    want = golden[name + ".rates"]
    for it, w in zip(ITERATIONS, want.tolist()):
        got = float(fn(it))
        if w == 0.0:
            assert got == 0.0 and math.copysign(1.0, got) == 1.0, (name, it, got)    # exact zeros are exactly zero
        else:
            assert abs(got - w) <= REL * abs(w), (name, it, got, w, abs(got - w) / abs(w))
    assert float(fn(-1)) == 0.0                                                     # the step < 0 arm
    if name == "both_zero":
        assert all(fn(it) == 0.0 for it in ITERATIONS)
    else:
        assert float(fn(0)) == pytest.approx(a * (mult if steps else 1.0), rel=1e-13)
        assert abs(float(fn(int(max_steps))) - b) <= REL * b and abs(float(fn(30000)) - b) <= REL * b   # clipped at the end


def test_default_arguments_are_the_references():
    import inspect

    from mobgs_amd.general_utils import get_expon_lr_func
    sig = inspect.signature(get_expon_lr_func)
    assert list(sig.parameters) == ["lr_init", "lr_final", "lr_delay_steps", "lr_delay_mult", "max_steps"]
    assert [p.default for p in sig.parameters.values()][2:] == [0, 1.0, 1000000]


# ---- TrainableGaussians.update_learning_rate on a stand-in for the group list ---------------------------------------------
class _Args:
    position_lr_init, position_lr_final, position_lr_max_steps = 0.00016, 0.0000016, 20000
    deformation_lr_init, deformation_lr_final = 0.00016, 0.000016
    grid_lr_init, grid_lr_final = 0.0016, 0.00016
    pose_lr_init, pose_lr_final = 0.0005, 0.00005


class _Groups:
    """What update_learning_rate reads of an optimiser."""

    def __init__(self, names):
        self.param_groups = [{"params": [], "lr": -1.0, "name": n} for n in names]


def _stand_in(names, scale=5.0):
    """A TrainableGaussians without tensors: update_learning_rate reads the optimiser's group list and the schedules only."""
    from mobgs_amd.densify import TrainableGaussians
    pc = object.__new__(TrainableGaussians)
    pc.spatial_lr_scale = scale
    pc.optimizer = _Groups(names)
    return pc


def test_update_learning_rate_sets_the_groups_the_reference_selects():
    from mobgs_amd.general_utils import get_expon_lr_func
    names = ["xyz", "control_xyz", "xyz_extra", "deformation", "deformation_2", "grid", "hexgrid_planes", "f_dc", "posenet",
             "posenet_cvdscale", "focal", "decoder"]
    pc = _stand_in(names).setup_schedules(_Args())
    kinds = {"xyz": "xyz", "deformation": "deformation", "grid": "grid", "hexgrid_planes": "grid", "posenet": "pose"}
    want = {"xyz": get_expon_lr_func(0.00016 * 5.0, 0.0000016 * 5.0, max_steps=20000),
            "deformation": get_expon_lr_func(0.00016 * 5.0, 0.000016 * 5.0, max_steps=20000),
            "grid": get_expon_lr_func(0.0016 * 5.0, 0.00016 * 5.0, max_steps=20000),
            "pose": get_expon_lr_func(0.0005, 0.00005, max_steps=20000)}
    for it in (0, 1, 777, 20000, 25000):
        for g in pc.optimizer.param_groups:
            g["lr"] = -1.0
        pc.update_learning_rate(it)
        for g in pc.optimizer.param_groups:
            if g["name"] in kinds:
                assert g["lr"] == want[kinds[g["name"]]](it), (it, g["name"])        # the same statements: the same bits
            else:
                assert g["lr"] == -1.0, (it, g["name"])
    sched = pc.schedules()
    assert {k[1] for k in sched} == set(kinds) and all(k[0] is pc.optimizer for k in sched)
    assert sched[(pc.optimizer, "grid")] is sched[(pc.optimizer, "hexgrid_planes")] is pc.grid_scheduler_args
    fine = _stand_in(["posenet"]).setup_schedules(_Args(), stage="fine")
    assert fine.pose_scheduler_args(0) == get_expon_lr_func(0.0005 / 10, 0.00005, max_steps=20000)(0)


def test_schedules_the_arguments_do_not_carry_are_left_out():
    class OnlyPosition:
        position_lr_init, position_lr_final, position_lr_max_steps = 0.00016, 0.0000016, 20000

    pc = _stand_in(["xyz", "f_dc"]).setup_schedules(OnlyPosition())
    assert hasattr(pc, "xyz_scheduler_args") and not hasattr(pc, "grid_scheduler_args")
    pc.update_learning_rate(10)
    assert pc.optimizer.param_groups[0]["lr"] == pc.xyz_scheduler_args(10) and pc.optimizer.param_groups[1]["lr"] == -1.0
    with pytest.raises(AttributeError, match="grid_scheduler_args"):
        _stand_in(["grid"]).setup_schedules(OnlyPosition()).update_learning_rate(1)


# ---- the host tables of DeviceAdam -----------------------------------------------------------------------------------------
def _bits(x):
    import struct
    return struct.pack("<d", float(x))


def test_lr_table_rows_are_the_callables_values_bit_for_bit():
    from mobgs_amd.general_utils import get_expon_lr_func
    from mobgs_amd.optim import MultiplicativeLR, lr_table
    from mobgs_amd.tto import tto_learning_rates
    cosine = tto_learning_rates(60, 10, 1e-3, 1e-5)
    fns = [get_expon_lr_func(8e-4, 8e-6, max_steps=50), get_expon_lr_func(1.6e-4, 1.6e-6, 10, 0.01, 40),
           MultiplicativeLR(1e-4, 0.01 ** (1 / 40), first_iteration=1), lambda it: cosine[min(it, 59)]]
    table = lr_table(fns, 60)
    assert table.dtype == torch.float64 and tuple(table.shape) == (61, 4) and not table.is_cuda
    for it in range(61):
        for c, fn in enumerate(fns):
            assert _bits(table[it, c]) == _bits(fn(it)), (it, c)
    assert tuple(lr_table([], 7).shape) == (8, 0)


def test_constant_groups_take_one_value_with_stride_zero():
    from mobgs_amd.optim import rate_layout
    ga, gb, gc = {"lr": 1e-3, "name": "a"}, {"lr": 2.5e-3, "name": "b"}, {"lr": 5e-2, "name": "c"}
    consts, layout = rate_layout([1, None, None, 0, None], [ga, gb, gb, gc, ga], n_columns=2, horizon=40)
    assert layout == [(True, 1, 2, 41), (False, 0, 0, 1), (False, 0, 0, 1), (True, 0, 2, 41), (False, 1, 0, 1)]
    assert consts.dtype == torch.float64 and consts.tolist() == [2.5e-3, 1e-3]


def test_multiplicative_schedule_is_a_loop_of_multiplications():
    from mobgs_amd.optim import MultiplicativeLR
    lr, factor = 1e-4, 0.01 ** (1 / 30)
    fn = MultiplicativeLR(lr, factor, first_iteration=3)
    assert fn(0) == fn(3) == lr
    group = {"lr": lr}
    for it in range(3, 200):
        assert _bits(fn(it)) == _bits(group["lr"]), it
        group["lr"] *= factor                                # blceKernel.adjust_lr after the step
    assert _bits(fn(57)) != _bits(lr * factor ** 54) or _bits(fn(91)) != _bits(lr * factor ** 88)   # (not a power)


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.8, 0.99)])
def test_bias_tables_are_the_python_expressions_bit_for_bit(betas):
    from mobgs_amd.optim import bias_tables
    b1, b2 = betas
    bc1, bc2s = bias_tables(b1, b2, 3000)
    assert bc1.dtype == bc2s.dtype == torch.float64 and bc1.shape == bc2s.shape == (3001,)
    for t in range(3001):
        step = float(torch.tensor(float(t), dtype=torch.float32))          # fused_adam_step: float(state["step"])
        assert _bits(bc1[t]) == _bits(1.0 - b1 ** step) and _bits(bc2s[t]) == _bits(math.sqrt(1.0 - b2 ** step)), t
    assert float(bc1[0]) == 0.0 and float(bc2s[0]) == 0.0


def test_header_declares_the_device_adam_entry_points():
    from mobgs_amd import _lib
    assert {"mobgs_adam_dev_factors", "mobgs_adam_dev_step"} <= set(_lib._SIGS)
    assert [n for n, _ in _lib._STRUCTS["MobgsAdamDevSchedule"]] == ["lr", "bc1", "bc2s", "lr_stride", "lr_rows", "bc_rows",
                                                                    "reserved"]
    assert [n for n, _ in _lib._STRUCTS["MobgsAdamDevTensor"]] == ["param", "grad", "exp_avg", "exp_avg_sq", "n", "w1",
                                                                  "beta2", "w2", "eps"]
    from mobgs_amd.optim import _DevSchedule, _DevTensor
    import ctypes
    assert ctypes.sizeof(_DevSchedule) == 40 and ctypes.sizeof(_DevTensor) == 56
