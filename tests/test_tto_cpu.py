"""The test-time pose refinement without a GPU: the restatement (tests/tto_restatement.py) against independent statements
-- rotation by quaternion products, autograd in float64, the edge case of equal images --, matrix_to_quaternion's round
trip, the learning rates against a real torch.optim pair, the restated loop against torch.optim.Adam on a toy function, and
the C ABI: source list, entries, the size query, refusals before any launch, the public names."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

import tto_restatement as TR
from helpers import GOLDEN

F64 = torch.float64


def rand_quats(n, seed, dtype=F64):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(n, 4, generator=g, dtype=F64)
    return (q / q.norm(dim=-1, keepdim=True)).to(dtype)


# ---- the head ----------------------------------------------------------------------------------------------------------

def test_rotation_is_the_quaternion_sandwich_for_any_norm():
    g = torch.Generator().manual_seed(1)
    for n, q in enumerate(rand_quats(8, 0)):
        for scale in (1.0, 1e-3, 0.5, 2.0, -1.0):
            R = TR.rotation(q * scale)
            x = torch.randn(3, generator=g, dtype=F64)
            assert (R @ x - TR.rotate_by_products(q * scale, x)).abs().max() <= 1e-14, (n, scale)
            assert (R @ R.T - torch.eye(3, dtype=F64)).abs().max() <= 1e-14 and abs(float(torch.det(R)) - 1) <= 1e-14
            assert (R - TR.rotation(q)).abs().max() <= 1e-14            # the norm and the sign do not matter
    assert torch.equal(TR.rotation(torch.tensor([1.0, 0, 0, 0], dtype=F64)), torch.eye(3, dtype=F64))
    w = TR.head(rand_quats(1, 3)[0], torch.tensor([1.0, -2.0, 3.0], dtype=F64))
    assert w.shape == (4, 4) and w[3].tolist() == [0, 0, 0, 1] and w[:3, 3].tolist() == [1, -2, 3]


def test_public_quaternion_functions_agree_with_the_restatement():
    from mobgs_amd.tto import quaternion_to_matrix
    q = rand_quats(6, 4) * torch.tensor([1.0, 0.5, 2.0, 1e-3, -1.0, 3.0], dtype=F64)[:, None]
    R = quaternion_to_matrix(q)
    assert R.shape == (6, 3, 3) and R.dtype == F64
    for n in range(6):
        assert torch.equal(R[n], TR.rotation(q[n]))
    assert quaternion_to_matrix(q.reshape(2, 3, 4)).shape == (2, 3, 3, 3)


def test_head_vjp_is_the_jacobian():
    g = torch.Generator().manual_seed(5)
    t = torch.tensor([0.3, -1.2, 4.0], dtype=F64)
    for n, q in enumerate(rand_quats(6, 6) * torch.tensor([1.0, 1e-3, 0.5, 2.0, -1.0, 1.0], dtype=F64)[:, None]):
        qa, ta = q.clone().requires_grad_(True), t.clone().requires_grad_(True)
        assert torch.autograd.gradcheck(TR.head, (qa, ta), eps=1e-6 * float(q.norm()), atol=1e-6 * float(1 / q.norm()),
                                        rtol=1e-6)
        cot = torch.randn(4, 4, generator=g, dtype=F64)
        v_q, v_t = torch.autograd.grad(TR.head(qa, ta), (qa, ta), cot)
        w_q, w_t = TR.head_vjp(q, cot)
        scale = float(v_q.abs().max())
        assert (w_q - v_q).abs().max() <= 1e-13 * scale and torch.equal(w_t, v_t), n
        # R does not depend on |q|: the gradient has no component along q
        assert abs(float((w_q * q).sum())) <= 1e-13 * scale * float(q.norm())


# ---- the loss ----------------------------------------------------------------------------------------------------------

def test_loss_and_gradient_against_autograd():
    g = torch.Generator().manual_seed(7)
    for shape in ((3, 1, 1), (3, 7, 5), (3, 17, 33)):
        gt = torch.rand(shape, generator=g, dtype=F64)
        pred = (gt + 0.1 * torch.randn(shape, generator=g, dtype=F64)).requires_grad_(True)
        loss = TR.neg_psnr(pred, gt)
        mse = float(((pred.detach() - gt) ** 2).mean())
        assert abs(float(loss.detach()) - 10 * math.log10(mse)) <= 1e-12 * abs(float(loss.detach()))     # -PSNR = 10 log10(mse)
        (want,) = torch.autograd.grad(loss, pred, torch.tensor(0.7, dtype=F64))
        got = TR.neg_psnr_grad(pred.detach(), gt, 0.7)
        assert (got - want).abs().max() <= 1e-13 * float(want.abs().max())


def test_equal_images_give_minus_inf_and_nan():
    """What the reference's statements give (eval.py:137-139 under autograd), in both dtypes."""
    for dtype in (torch.float32, F64):
        gt = torch.rand(3, 4, 4, dtype=dtype)
        pred = gt.clone().requires_grad_(True)
        loss = TR.neg_psnr(pred, gt)
        loss.backward()
        assert float(loss) == -math.inf and bool(torch.isnan(pred.grad).all())
        assert bool(torch.isnan(TR.neg_psnr_grad(gt, gt)).all())


# ---- matrix_to_quaternion ------------------------------------------------------------------------------------------------

def fp32_ulps(got, want):
    return float(((got.double() - want.double()).abs() / (2.0 ** -24)).max())      # entries of a rotation are <= 1


def test_matrix_to_quaternion_round_trip():
    from mobgs_amd.tto import matrix_to_quaternion, quaternion_to_matrix
    cases = [q for q in rand_quats(32, 8)]
    for axis in range(3):                                            # 180 degrees about each axis: the real part is 0
        q = torch.zeros(4, dtype=F64)
        q[1 + axis] = 1.0
        cases.append(q)
    for eps in (1e-3, 1e-5, 1e-7):                                   # a trace close to -1
        for q in rand_quats(4, 9):
            q = q.clone()
            q[0] = eps
            cases.append(q / q.norm())
    cases.append(torch.tensor([1.0, 0, 0, 0], dtype=F64))
    for n, q in enumerate(cases):
        R64 = TR.rotation(q)
        back = matrix_to_quaternion(R64)
        assert back.dtype == F64 and abs(float(back.norm()) - 1) <= 1e-15
        assert min(float((back - q).abs().max()), float((back + q).abs().max())) <= 1e-12, n       # the sign is free
        # from an fp32 matrix, as refine_pose calls it: the matrix comes back to a few fp32 ulps
        R32 = R64.float()
        q32 = matrix_to_quaternion(R32)
        assert q32.dtype == torch.float32 and q32.shape == (4,)
        assert fp32_ulps(quaternion_to_matrix(q32.double()), R32) <= 4, (n, fp32_ulps(quaternion_to_matrix(q32.double()), R32))
    stack = torch.stack([TR.rotation(q) for q in cases[:6]]).reshape(2, 3, 3, 3)
    assert matrix_to_quaternion(stack).shape == (2, 3, 4)
    with pytest.raises(ValueError):
        matrix_to_quaternion(torch.eye(4))


# ---- the schedule ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps, decay_start", [(25, 15), (100, 30), (250, 15), (25, 25), (25, 40)])
def test_learning_rates_against_torch(steps, decay_start):
    from mobgs_amd.tto import tto_learning_rates
    for lr, lr_final in ((3e-3, 1e-4), (3e-4, 1e-6), (3e-4, 1e-5)):
        want = TR.torch_learning_rates(steps, decay_start, lr, lr_final)
        for got in (tto_learning_rates(steps, decay_start, lr, lr_final), TR.learning_rates(steps, decay_start, lr, lr_final)):
            assert len(got) == steps
            assert max(abs(a - b) / b for a, b in zip(got, want)) <= 1e-14
            assert got[:min(steps, decay_start + 1)] == [lr] * min(steps, decay_start + 1)
        if decay_start >= steps:
            assert want == [lr] * steps                               # the reference never steps the scheduler
        else:
            assert want[-1] > lr_final and all(a > b for a, b in zip(want[decay_start:], want[decay_start + 1:]))


def test_adam_scalars_are_formed_as_fused_adam_step_forms_them():
    from mobgs_amd.tto import BETAS, EPS, adam_step_scalars
    assert (BETAS, EPS) == ((0.9, 0.999), 1e-8) == (TR.BETAS, TR.EPS)
    for step, lr in ((1, 3e-3), (7, 1.2e-4), (250, 1e-6)):
        assert adam_step_scalars(step, lr) == (lr / (1.0 - 0.9 ** float(step)), math.sqrt(1.0 - 0.999 ** float(step)))


# ---- the loop ----------------------------------------------------------------------------------------------------------

def toy(target):
    """A smooth function of w2c with its minimum at `target`: points moved by both poses should land together."""
    g = torch.Generator().manual_seed(10)
    pts = torch.cat([torch.randn(40, 3, generator=g, dtype=F64), torch.ones(40, 1, dtype=F64)], 1)

    def loss_of_w2c(w2c):
        return ((pts @ w2c.T - pts @ target.T) ** 2).mean()
    return loss_of_w2c


@pytest.mark.parametrize("settings", [TR.DEFAULTS, TR.MAIN, dict(TR.DEFAULTS, tto_steps=250), dict(TR.DEFAULTS, decay_start=40)])
def test_restated_loop_against_torch_optim(settings):
    q_true, t_true = rand_quats(1, 11)[0], torch.tensor([0.2, -0.1, 1.5], dtype=F64)
    f = toy(TR.head(q_true, t_true))
    # a start so far away that no setting arrives (a step moves a value by about its rate): near the minimum Adam's
    # m / sqrt(v) turns a difference in the last place into a different path, and two correct loops part company
    q0 = q_true + 0.5 * rand_quats(1, 12)[0]
    t0 = t_true + torch.tensor([2.0, -3.0, 2.5], dtype=F64)

    def loss_and_grad(w2c):
        w = w2c.detach().requires_grad_(True)
        loss = f(w)
        return loss.detach(), torch.autograd.grad(loss, w)[0]

    q_a, t_a, l_a = TR.restated_loop(loss_and_grad, q0, t0, **settings)
    q_b, t_b, l_b = TR.composed_loop(f, q0, t0, **settings)
    assert len(l_a) == len(l_b) == settings["tto_steps"]
    # float64 on both sides; what differs is the order of a few operations and the recursive schedule
    assert (q_a - q_b).abs().max() <= 1e-11 and (t_a - t_b).abs().max() <= 1e-11
    assert max(abs(a - b) for a, b in zip(l_a, l_b)) <= 1e-11
    assert l_a[-1] < l_a[0] and TR.pose_gap(q_a, t_a, q_true, t_true) < TR.pose_gap(q0, t0, q_true, t_true)


# ---- the C ABI and the public names ----------------------------------------------------------------------------------------

ENTRIES = ("mobgs_pose_head_fwd", "mobgs_pose_head_bwd", "mobgs_pose_step", "mobgs_neg_psnr_scratch_doubles",
           "mobgs_neg_psnr_fwd", "mobgs_neg_psnr_bwd")


def test_abi_entries_size_query_and_refusals():
    from mobgs_amd import _lib, build
    assert "pose.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["pose.hip"]
    assert (build.CSRC / "adam_shared.h") in build.headers()
    for unit in ("densify.hip", "pose.hip"):                         # one statement of the Adam arithmetic, used by both
        text = (build.CSRC / unit).read_text()
        assert '#include "adam_shared.h"' in text and "adam_update(" in text and "sqrtf(v)" not in text, unit
    h = _lib.load()
    assert _lib.ABI_VERSION == 16 == h.mobgs_abi_version()
    for name in ENTRIES:
        assert name in _lib._SIGS and hasattr(h, name), name
    assert _lib._SIGS["mobgs_neg_psnr_scratch_doubles"] == (ctypes.c_size_t, [ctypes.c_int64])
    assert _lib._SIGS["mobgs_pose_step"][1][5:11] == [ctypes.c_float] * 3 + [ctypes.c_double] * 3
    # the size query: a host computation; one double per workgroup of 256 quads, 1024 workgroups at most, 0 outside [1, 2^40]
    q = h.mobgs_neg_psnr_scratch_doubles
    assert [q(1), q(3), q(1024), q(1025), q(3 * 16 * 16), q(3 * 288 * 512), q(3 * 1014 * 1352), q(1 << 40)] == \
        [1, 1, 1, 2, 1, 432, 1024, 1024]
    assert [q(0), q(-5), q((1 << 40) + 1)] == [0, 0, 0]
    none = ctypes.c_void_p(None)
    buf = (ctypes.c_double * 64)()                     # host memory: every call below is refused before any launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd, four = ctypes.c_void_p(p.value + 2), ctypes.c_void_p(p.value + 4)
    E = _lib._DEFINES["MOBGS_E_INVALID"]

    def refused(rc, who):
        assert rc == E == -1 and who.encode() + b":" in h.mobgs_last_error(), (who, rc, h.mobgs_last_error())

    def fwd(n=48, pred=p, gt=p, partial=p, mse=p, loss=p):
        return h.mobgs_neg_psnr_fwd(n, pred, gt, partial, mse, loss, none)

    def bwd(n=48, pred=p, gt=p, mse=p, v_loss=none, v_pred=p):
        return h.mobgs_neg_psnr_bwd(n, pred, gt, mse, v_loss, v_pred, none)

    for kw in (dict(n=0), dict(n=-1), dict(n=(1 << 40) + 1), dict(pred=none), dict(gt=none), dict(partial=none),
               dict(mse=none), dict(loss=none), dict(pred=odd), dict(gt=odd), dict(loss=odd), dict(partial=four),
               dict(mse=four)):
        refused(fwd(**kw), "mobgs_neg_psnr_fwd")
    for kw in (dict(n=0), dict(n=-1), dict(pred=none), dict(gt=none), dict(mse=none), dict(v_pred=none), dict(pred=odd),
               dict(gt=odd), dict(mse=four), dict(v_loss=odd), dict(v_pred=odd)):
        refused(bwd(**kw), "mobgs_neg_psnr_bwd")
    for bad in (none, odd):
        for at in range(3):
            args = [p, p, p]
            args[at] = bad
            refused(h.mobgs_pose_head_fwd(*args, none), "mobgs_pose_head_fwd")
        for at in range(4):
            args = [p, p, p, p]
            args[at] = bad
            refused(h.mobgs_pose_head_bwd(*args, none), "mobgs_pose_head_bwd")
        for at in (0, 1, 2, 3, 4, 11):
            args = [p, p, p, p, p, 1e-3, 1e-3, 1.0, 0.9, 0.999, 1e-8, p]
            args[at] = bad
            refused(h.mobgs_pose_step(*args, none), "mobgs_pose_step")


def test_public_names_and_refusal_of_host_tensors(tmp_path):
    from mobgs_amd import tto as T
    a = torch.rand(3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        T.neg_psnr_loss(a, a.clone())
    with pytest.raises(RuntimeError, match="no CPU path"):
        T.pose_matrix(torch.tensor([1.0, 0, 0, 0]), torch.zeros(3))
    par = inspect.signature(T.render_test_tto).parameters                  # the reference's keyword names and defaults
    want = dict(tto_steps=25, decay_start=15, lr_p=0.003, lr_q=0.003, lr_final=0.0001, use_sgd=False, loss_type="psnr",
                initialize_from_previous_camera=True, initialize_from_previous_step_factor=10,
                initialize_from_previous_lr_factor=0.1, fg_mask_th=0.1, local_viewdirs=None, batch_shape=None, renderArgs=None)
    assert {k: par[k].default for k in want} == want
    assert list(par)[:6] == ["H", "W", "scene", "test_cams", "save_dir", "gt_images"]
    for kw in (dict(use_sgd=True), dict(loss_type="abs")):
        with pytest.raises(NotImplementedError):
            T.render_test_tto(8, 8, None, [object()], str(tmp_path), [a], **kw)
    par = inspect.signature(T.refine_pose).parameters
    for k in ("steps", "decay_start", "lr_p", "lr_q", "lr_final"):
        assert par[k].kind is par[k].KEYWORD_ONLY and par[k].default is par[k].empty, k
    assert T.RefinedPose._fields == ("w2c", "q", "t", "loss_history")


def test_restatement_against_pytorch3d_vectors():
    """Present only after scripts/dump_pose_vectors.py ran where pytorch3d is installed: pins the quaternion convention to
    the package itself; skipped otherwise (README, "UNPINNED")."""
    path = os.path.join(GOLDEN, "pose_external", "pytorch3d.npz")
    if not os.path.exists(path):
        pytest.skip("no tests/golden/pose_external/pytorch3d.npz (run scripts/dump_pose_vectors.py where pytorch3d is "
                    "installed): the quaternion convention stays UNPINNED")
    from mobgs_amd.tto import matrix_to_quaternion, quaternion_to_matrix
    ex = dict(np.load(path))
    q = torch.from_numpy(ex["q"])
    assert q.dtype == F64
    R = torch.from_numpy(ex["quaternion_to_matrix"])
    assert (quaternion_to_matrix(q) - R).abs().max() <= 1e-14
    theirs = torch.from_numpy(ex["matrix_to_quaternion"])
    ours = matrix_to_quaternion(R)
    gap = torch.minimum((ours - theirs).abs().amax(-1), (ours + theirs).abs().amax(-1))
    assert float(gap.max()) <= 1e-12
