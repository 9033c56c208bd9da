"""The test-time pose refinement (include/mobgs_hip.h K23, mobgs_amd/tto.py) restated with torch on the CPU, in our own
words and parameterised by dtype, for the tests to compare against: the pose head of /root/reference/eval.py:122-123
(pytorch3d's quaternion_to_matrix, real part first, not normalised), its Jacobian written out, the loss of eval.py:137-139
and its gradient, Adam's update, the learning rates of eval.py:111-115 / :147-148, and the loop of eval.py:120-150 twice:

    restated_loop   the statements above, nothing from torch.optim
    composed_loop   the same algorithm from torch's parts: autograd through head(), torch.optim.Adam and
                    CosineAnnealingLR around any function of w2c -- with this project's render() as that function it is
                    what a caller could do before mobgs_amd.tto existed, and the yardstick of the GPU tests

dtype=torch.float64 is the truth the GPU tests measure against; dtype=torch.float32 with the torch composition stands for
"the reference as it can be run here"."""
from __future__ import annotations

import math

import torch

from regterms_restatement import FLOOR, FLOOR_DB, allowed  # noqa: F401  (the rule of DESIGN 3a)

BETAS, EPS = (0.9, 0.999), 1e-8
MAIN = dict(tto_steps=100, decay_start=30, lr_p=3e-4, lr_q=3e-4, lr_final=1e-6)        # eval.py:257-264, __main__
DEFAULTS = dict(tto_steps=25, decay_start=15, lr_p=3e-3, lr_q=3e-3, lr_final=1e-4)     # eval.py:51-55


# ---- the head ----------------------------------------------------------------------------------------------------------

def rotation(q):
    """pytorch3d.transforms.quaternion_to_matrix for one quaternion [4]."""
    r, i, j, k = q.unbind(-1)
    two_s = 2.0 / (q * q).sum()
    return torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                        two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                        two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j))).reshape(3, 3)


def head(q, t):
    """eval.py:122-123: cat([cat([R, t[:, None]], 1), [0 0 0 1]], 0), in the dtype of q."""
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=q.dtype, device=q.device)
    return torch.cat([torch.cat([rotation(q), t[:, None]], 1), bottom[None]], 0)


def quat_mul(a, b):
    """Hamilton product, real part first."""
    ar, ai, aj, ak = a.unbind(-1)
    br, bi, bj, bk = b.unbind(-1)
    return torch.stack((ar * br - ai * bi - aj * bj - ak * bk, ar * bi + ai * br + aj * bk - ak * bj,
                        ar * bj - ai * bk + aj * br + ak * bi, ar * bk + ai * bj - aj * bi + ak * br), -1)


def rotate_by_products(q, x):
    """q x q^-1 for a point x [3]: an independent statement of what rotation(q) @ x must be, for any non-zero q."""
    conj = q * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=q.dtype)
    p = torch.cat([torch.zeros(1, dtype=q.dtype), x])
    return quat_mul(quat_mul(q, p), conj / (q * q).sum())[1:]


def head_vjp(q, g):
    """(v_q [4], v_t [3]) for a cotangent g [4,4] of head(q, t), written out: with R = I + s M(q), s = 2 / (q . q),
    v_q = s (dM/dq)^T g - s^2 <g, M> q."""
    r, i, j, k = q.unbind(-1)
    s = 2.0 / (q * q).sum()
    M = torch.stack((-(j * j + k * k), i * j - k * r, i * k + j * r, i * j + k * r, -(i * i + k * k), j * k - i * r,
                     i * k - j * r, j * k + i * r, -(i * i + j * j))).reshape(3, 3)
    G = g[:3, :3]
    vs = (G * M).sum()
    sym, anti = G + G.T, G - G.T
    v_r = k * anti[1, 0] + j * anti[0, 2] + i * anti[2, 1]
    v_i = j * sym[0, 1] + k * sym[0, 2] - 2 * i * (G[1, 1] + G[2, 2]) + r * anti[2, 1]
    v_j = i * sym[0, 1] + k * sym[1, 2] - 2 * j * (G[0, 0] + G[2, 2]) + r * anti[0, 2]
    v_k = i * sym[0, 2] + j * sym[1, 2] - 2 * k * (G[0, 0] + G[1, 1]) + r * anti[1, 0]
    return s * torch.stack((v_r, v_i, v_j, v_k)) - s * s * vs * q, g[:3, 3].clone()


# ---- the loss ----------------------------------------------------------------------------------------------------------

def neg_psnr(pred, gt):
    """eval.py:137-139 as written, in the dtype of pred."""
    mse = ((pred - gt) ** 2).mean()
    return -(20 * torch.log10(1.0 / torch.sqrt(mse)))


def neg_psnr_grad(pred, gt, v_loss=1.0):
    """d neg_psnr / d pred, written out: v_loss 20 / (ln 10 n mse) (pred - gt)."""
    d = pred - gt
    mse = (d ** 2).mean()
    return v_loss * 20.0 / (math.log(10.0) * d.numel() * mse) * d


# ---- Adam and the schedule -----------------------------------------------------------------------------------------------

def learning_rates(steps, decay_start, lr, lr_final):
    """The rate of each optimiser step: CosineAnnealingLR(T_max = steps - decay_start, eta_min = lr_final) evaluated in
    closed form after max(0, s - decay_start) scheduler steps."""
    rates = []
    for s in range(steps):
        k = max(0, s - decay_start)
        rates.append(lr if k == 0 else lr_final + (lr - lr_final) * (1 + math.cos(math.pi * k / (steps - decay_start))) / 2)
    return rates


def torch_learning_rates(steps, decay_start, lr, lr_final):
    """The rates a real torch.optim.Adam + CosineAnnealingLR pair goes through when driven as eval.py:111-148 drives it."""
    p = torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))
    opt = torch.optim.Adam([{"params": p, "lr": lr}])
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=steps - decay_start, eta_min=lr_final)
    rates = []
    for s in range(steps):
        rates.append(opt.param_groups[0]["lr"])
        p.grad = torch.ones_like(p)
        opt.step()
        if s >= decay_start:
            sched.step()
    return rates


def adam_update(p, g, m, v, step, lr):
    """torch.optim.Adam's update (amsgrad = False, no weight decay) of step `step` (1-based) -> (p, m, v), in p's dtype."""
    b1, b2 = BETAS
    m = m + (1 - b1) * (g - m)
    v = v * b2 + (1 - b2) * (g * g)
    step_size = lr / (1 - b1 ** step)
    denom = v.sqrt() / math.sqrt(1 - b2 ** step) + EPS
    return p - step_size * (m / denom), m, v


# ---- the loop ----------------------------------------------------------------------------------------------------------

def restated_loop(loss_and_grad, q0, t0, *, tto_steps, decay_start, lr_p, lr_q, lr_final):
    """eval.py:120-150 from the statements of this file.  loss_and_grad(w2c) -> (loss, d loss / d w2c [4,4]).
    -> (q, t, [loss per step])."""
    q, t = q0.clone(), t0.clone()
    mq, vq, mt, vt = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(t), torch.zeros_like(t)
    rp, rq = learning_rates(tto_steps, decay_start, lr_p, lr_final), learning_rates(tto_steps, decay_start, lr_q, lr_final)
    losses = []
    for s in range(tto_steps):
        loss, g = loss_and_grad(head(q, t))
        v_q, v_t = head_vjp(q, g)
        t, mt, vt = adam_update(t, v_t, mt, vt, s + 1, rp[s])
        q, mq, vq = adam_update(q, v_q, mq, vq, s + 1, rq[s])
        losses.append(float(loss))
    return q, t, losses


def composed_loop(loss_of_w2c, q0, t0, *, tto_steps, decay_start, lr_p, lr_q, lr_final, read_back=True):
    """The refinement put together from torch's own parts, as a caller without mobgs_amd.tto would: autograd through
    head(), ONE torch.optim.Adam with a group per pose part (lr_q for the quaternion, lr_p for the translation, torch's
    default betas and eps), and torch's CosineAnnealingLR over the tto_steps - decay_start last steps down to lr_final, advanced
    only once step decay_start has been taken.  loss_of_w2c(w2c) -> the loss tensor.  -> (q, t, losses): the losses as
    Python floats, read back every step as the reference does, or with read_back=False as detached tensors."""
    quat = q0.detach().clone().requires_grad_(True)
    trans = t0.detach().clone().requires_grad_(True)
    adam = torch.optim.Adam([dict(params=[quat], lr=lr_q), dict(params=[trans], lr=lr_p)])
    cosine = torch.optim.lr_scheduler.CosineAnnealingLR(adam, T_max=tto_steps - decay_start, eta_min=lr_final)
    history = []
    for s in range(tto_steps):
        adam.zero_grad(set_to_none=True)
        loss = loss_of_w2c(head(quat, trans))
        loss.backward()
        adam.step()
        if s >= decay_start:
            cosine.step()
        history.append(float(loss.detach()) if read_back else loss.detach())
    return quat.detach(), trans.detach(), history


def render_loss(render, cam, stat, dyn, pipe, bg, gt):
    """The loss of eval.py:125-139 as a function of w2c, around this project's render (gt [3,H,W]; the mean does not care
    about the reference's permute to [H,W,3])."""
    def loss_of_w2c(w2c):
        pred = render(cam, stat, dyn, pipe, bg, stage="fine", get_static=False, get_dynamic=False, w2c=w2c)["render"]
        return neg_psnr(pred, gt)
    return loss_of_w2c


# ---- distances -----------------------------------------------------------------------------------------------------------

def max_gap(a, b):
    """Largest element-wise distance of a from the truth b, relative to the truth's largest magnitude."""
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    scale = float(b.abs().max())
    return float((a - b).abs().max()) / (scale if scale > 0 else 1.0)


def pose_gap(q_a, t_a, q_b, t_b):
    """Distance of two poses: the largest entry of the difference of their 3x4 matrices, in float64 (a quaternion's norm
    and sign do not matter)."""
    a = head(q_a.double().cpu(), t_a.double().cpu())
    b = head(q_b.double().cpu(), t_b.double().cpu())
    return float((a - b).abs().max())
