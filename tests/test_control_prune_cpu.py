"""Host side of the control-point pruning (mobgs_amd.scene_init.one_down_tables / onedown_control_pts, csrc/
control_prune.hip) against tests/golden/prune.npz: what the reference's own inverse_cubic_hermite_for_prune and
compute_prune_error gave for a seeded set (make_golden_prune.py), next to the float64 restatement
tests/prune_restatement.py.

Tolerances: 3 x the reference's own fp32 / float64 gap on this fixture, which the generator printed and
stored in `ref_gaps`: control points 5.12e-4 absolute at a coordinate scale of 1.05e3, 6.31e-7 of a row's own largest
coordinate; pixel error 6.49e-5 px.  Rows whose count is 4 are outside these comparisons: the reference refits them
against a dummy equation that halves the fourth point (up to 517 units and 62 px here), the product leaves them alone.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from helpers import GOLDEN, load

import prune_restatement as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mobgs_hip.h")
SYMBOL = "mobgs_control_onedown"


def _fixture():
    fx = load("prune")
    T = torch.from_numpy
    focal, W, H, thr = (float(v) for v in fx["intrinsics"])
    return fx, T(fx["control_xyz"]), T(fx["control_num"]), T(fx["w2c"]), T(fx["times"]), focal, W, H, thr


def _row_gaps(a, b64, rows):
    err = (a.double() - b64)[rows].abs().reshape(int(rows.sum()), -1).max(1).values
    own = b64[rows].abs().reshape(int(rows.sum()), -1).max(1).values
    return float(err.max()), float((err / own).max())


def test_restatement_agrees_with_the_reference_fixture():
    fx, control, num, w2c, times, focal, W, H, thr = _fixture()
    gap_new, gap_rel, gap_err = (float(v) for v in fx["ref_gaps"])
    cand = num.reshape(-1) >= 5
    new64, m = PR.one_down_f64(control, num)
    err64 = PR.prune_error_f64(control, num, new64, m, w2c, times, focal, W / 2, H / 2)
    # the stored float64 values are this function's (the fixture and the helper have not drifted apart)
    assert float((new64 - torch.from_numpy(fx["f64_new"])).abs().max()) <= 1e-9
    assert float((err64 - torch.from_numpy(fx["f64_err"])).abs().max()) <= 1e-9
    ref_new, ref_err = torch.from_numpy(fx["ref_new"]), torch.from_numpy(fx["ref_err"])
    d_abs, d_rel = _row_gaps(ref_new, new64, cand)
    d_err = float((ref_err.double() - err64)[cand].abs().max())
    print(f"reference fp32 vs restatement, count >= 5: control points {d_abs:.3e} abs / {d_rel:.3e} of the row "
          f"(stored {gap_new:.3e} / {gap_rel:.3e}); pixel error {d_err:.3e} px (stored {gap_err:.3e})")
    assert 0 < gap_new < 2e-3 and 0 < gap_err < 3e-4   # the floor itself is fp32 noise at this scale, not a blunder
    assert d_abs <= 3 * gap_new and d_rel <= 3 * gap_rel and d_err <= 3 * gap_err
    # decisions: none flips outside the margin, and the margin holds almost no rows
    near = (err64 - thr).abs() <= 3 * gap_err
    ref_prune = torch.from_numpy(fx["ref_prune"])
    assert not bool((((err64 <= thr) != ref_prune) & cand & ~near).any())
    assert float((near & cand).double().sum() / cand.double().sum()) <= 0.02
    # the reference's commit is its decision applied to its counts
    n = num.reshape(-1)
    after = torch.where(ref_prune, torch.clamp(n - 1, min=4), n)
    assert torch.equal(torch.from_numpy(fx["ref_num_after"]).reshape(-1), after)


def test_fixture_covers_what_it_should():
    fx, control, num, w2c, times, focal, W, H, thr = _fixture()
    assert os.path.getsize(os.path.join(GOLDEN, "prune.npz")) <= os.path.getsize(os.path.join(GOLDEN, "init.npz"))
    n = num.reshape(-1)
    assert sorted(set(n.tolist())) == list(range(4, 13)) and 900 <= n.numel() <= 1100 and times.numel() == 24
    err64 = torch.from_numpy(fx["f64_err"])
    cand = n >= 5
    within = float((err64[cand] <= thr).double().mean())
    assert 0.30 <= within <= 0.70 and int((err64 > 5.0).sum()) >= 10
    eyes = torch.linalg.inv(w2c.double())[:, :3, 3]
    assert float(eyes.norm(dim=1).max()) > 3.0
    # count 4: the reference moved those rows (the upstream defect this project does not reproduce)
    four = n == 4
    ref_new = torch.from_numpy(fx["ref_new"])
    assert float((ref_new[four, :4] - control[four, :4]).abs().max()) > 1.0
    assert float(torch.from_numpy(fx["ref_err"])[four].max()) > 0.1 and bool((err64[four] == 0).all())


def test_tables_full_rank_shape_and_padding():
    from mobgs_amd.scene_init import hermite_design, one_down_design, one_down_tables
    t = one_down_tables()
    assert t.dtype == torch.float32 and tuple(t.shape) == (8, 11, 12) and t.is_contiguous()
    assert one_down_tables() is t   # cached
    for n in range(5, 13):
        A = one_down_design(n)
        assert tuple(A.shape) == (n, n - 1) and int(torch.linalg.matrix_rank(A)) == n - 1
        assert torch.equal(A, hermite_design(torch.arange(n, dtype=torch.float64) / (n - 1), n - 1))
        cond = float(torch.linalg.cond(A))
        assert 1.0 < cond < 2.0, (n, cond)   # 1.29 (n = 5) .. 1.75 (n = 12)
        blk = t[n - 5]
        assert bool((blk[n - 1:] == 0).all()) and bool((blk[:, n:] == 0).all())
        assert float((blk[:n - 1, :n].double() - torch.linalg.pinv(A)).abs().max()) < 1e-7
        assert float((blk[:n - 1, :n].double() @ A - torch.eye(n - 1, dtype=torch.float64)).abs().max()) < 1e-6
    with pytest.raises(ValueError):
        one_down_design(4)
    with pytest.raises(ValueError):
        one_down_design(13)


def test_table_formulation_equals_the_full_system():
    """The fit depends on the count only: table[n - 5] applied to a row's (masked) points is the least-squares solution
    of the reference's full [12, 11] system, dummy equations included -- in float64 to rounding."""
    from mobgs_amd.scene_init import one_down_design
    fx, control, num, *_ = _fixture()
    new64 = torch.from_numpy(fx["f64_new"])
    n = num.reshape(-1)
    worst = 0.0
    for k in range(5, 13):
        rows = n == k
        P = torch.linalg.pinv(one_down_design(k))
        got = torch.zeros(int(rows.sum()), 11, 3, dtype=torch.float64)
        got[:, :k - 1] = torch.einsum("jk,bkc->bjc", P, control[rows, :k].double())
        worst = max(worst, float((got - new64[rows]).abs().max()))
    print(f"pseudo-inverse per count vs batched least squares over the full system (float64): {worst:.3e}")
    assert worst < 1e-8


def test_header_binding_and_library_agree_on_the_entry_point():
    from mobgs_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+" + SYMBOL + r"\s*\(", text), "not declared in include/mobgs_hip.h"
    assert SYMBOL in _lib._SIGS and len(_lib._SIGS[SYMBOL][1]) == 16
    assert "control_prune.hip" in build.SOURCES
    lib = ctypes.CDLL(str(build.build_extension()))
    assert hasattr(lib, SYMBOL), "declared in the header but not exported by the library"


def test_bad_arguments_are_refused_before_any_launch():
    """V < 3, n_rows < 0, a NULL table and NULL buffers return MOBGS_E_INVALID with a message; no device is touched
    (this runs without one).  The Python layer refuses CPU tensors and short camera lists."""
    import types
    from mobgs_amd import _lib
    from mobgs_amd.scene_init import one_down_fit, onedown_control_pts
    h = _lib.load()
    none = ctypes.c_void_p(None)
    fake = ctypes.c_void_p(256)   # never dereferenced: every call below is refused before the launch

    def call(n_rows, n_views, table=fake, bufs=fake):
        return h.mobgs_control_onedown(n_rows, n_views, bufs, bufs, 500.0, 320.0, 240.0, table, 1.0, bufs, bufs, bufs,
                                       none, bufs, 0, none)
    for args, word in (((10, 2), b"n_views"), ((10, 0), b"n_views"), ((-1, 5), b"n_rows"),
                       ((10, 5, none), b"pinv_table"), ((10, 5, fake, none), b"NULL buffer")):
        assert call(*args) == -1
        assert SYMBOL.encode() in h.mobgs_last_error() and word in h.mobgs_last_error(), h.mobgs_last_error()
    with pytest.raises(RuntimeError, match="HIP device"):
        one_down_fit(torch.zeros(4, 12, 3), torch.full((4, 1), 12), torch.eye(4).repeat(3, 1, 1), torch.rand(3), 500.0,
                     640, 480)
    md = types.SimpleNamespace(focal_length=500.0)
    cams = [types.SimpleNamespace(metadata=md, image_width=640, image_height=480, time=0.5,
                                  world_view_transform=torch.eye(4)) for _ in range(2)]
    pc = types.SimpleNamespace(control_xyz=torch.zeros(4, 12, 3), current_control_num=torch.full((4, 1), 12))
    with pytest.raises(ValueError, match="at least 3 viewpoints"):
        onedown_control_pts(pc, cams)


def test_gaussian_params_carry_the_threshold():
    from mobgs_amd.densify import TrainableGaussians
    from mobgs_amd.gaussian_model import GaussianParams
    assert GaussianParams.error_threshold == 1.0 and TrainableGaussians.error_threshold == 1.0
    assert callable(TrainableGaussians.onedown_control_pts)
