"""Deterministic cases for the two BLCE kernels (csrc/blce.hip through mobgs_amd.blce._FusedView), with float64 and fp32
references from the torch BLCE module of mobgs_amd/blce.py on the CPU (pinned by the reference's fixture in
tests/test_blce_cpu.py) followed by torch.inverse, as blceKernel.get_warped_cams states it.  Torch on the CPU only: nothing
here loads the HIP library; tests/test_blce_cases_cpu.py checks from the float64 module alone that every case reaches the
regime it is named after.

Cases: `fixture` (the state of tests/golden/blce.npz), `init` (the module as its constructor leaves it: decoder gain 1e-5,
rot and theta ~1e-6, 1 - cos(theta) == 0 in fp32), `zero_rot` (|rot| == 0: the gradient of the axis is Vu x 1e10), `large`
(|theta| > pi, |trans| >= 1), `dead_relu`, `far_camera` (c2w translation of length 100: the cofactor inverse in fp32) and
four (view index, table size) pairs for the zeroing loop of the embedding-table gradient.  Cotangents on both outputs, on
c2w only and on w2c only.

Near-kink rule.  A ReLU pre-activation z is near a kink when |z| <= 64 x 2^-24 x (sum |w x| + |b|), the fp32 dot-product
error bound of that unit; for the trajectory x_{i+1} = x_i + W in_i + b the sum runs over every term since x_0.  320 units
per case: 2 x 32 of the blur-feature encoder, 8 x 32 of the trajectory.  The seeded cases redraw their seed until no unit is
near a kink, the fixture's state has none: fp32 and float64 take the same branch everywhere, nothing is compared with a
flip allowance.

Compared per tensor with deform_cases.close_to_f64 at k = 3, with one derived allowance.
Neighbour allowance.  One view is ONE vector through one small network: every entry of an output tensor is driven by the
same few roundings (of the trajectory, of theta - sin(theta) and 1 - cos(theta)), so max |ref32 - ref64| over a tensor is
one draw of the fp32 module's error, not a maximum over many, and a bias of one or three entries can draw 0.1 of what the
next input draws.  The gap of a tensor is therefore the largest of 1 + NEIGHBOURS draws: the case itself and 8 neighbouring
inputs (every parameter, the pose and the blur feature moved by at most half an fp32 ulp), each neighbour's fp32 result
against the float64 result on the same neighbour.  References alone; k stays 3; the RATIO line shows the addition as
`extra` = 3 (largest gap - the case's own gap)."""
import copy
import functools
import math
import os
from types import SimpleNamespace

import numpy as np
import torch

from loss_cases import close_map, gather
from mobgs_amd.blce import BLCE, _view_param_list

K = 3
KINK = 64 * 2.0 ** -24
MAX_NEAR = 0.05
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARAM_NAMES = ("view_embedder", "Rt_encoder.weight", "Rt_encoder.bias", "view_encoder.weight", "view_encoder.bias",
               "blur_feature_encoder.0.weight", "blur_feature_encoder.0.bias", "blur_feature_encoder.2.weight",
               "blur_feature_encoder.2.bias", "blur_feature_encoder.4.weight", "blur_feature_encoder.4.bias",
               "time_embedder", "w_linear.weight", "w_linear.bias", "v_linear.weight", "v_linear.bias", "rot_decoder.weight",
               "rot_decoder.bias", "trans_decoder.weight", "trans_decoder.bias", "theta_decoder.weight", "theta_decoder.bias")
COTS = ("both", "c2w", "w2c")
VIEWS = ((0, 1), (2, 3), (0, 200), (199, 200))
CASES = ("fixture", "init", "zero_rot", "large", "dead_relu", "far_camera") + tuple(f"view_{i}_of_{n}" for i, n in VIEWS)


# ---- the module's forward, restated with its parts in reach ------------------------------------------------------------
def forward_parts(m, Rt, bf, idx, unit=None):
    """BLCE.forward(Rt, bf, idx) of mobgs_amd/blce.py statement by statement -> namespace(c2w, z1, z2 (pre-activations of
    the blur-feature encoder), xs [9,32] (the trajectory), w_rigid, w_unit, theta, v_rigid).  `unit`: what to use for
    w_rigid / (|w_rigid| + 1e-10) (a planted error); tests/test_blce_cases_cpu.py holds c2w to the module bit for bit."""
    freqs = (2 ** torch.arange(m.num_freqs)).to(torch.float32)
    angles = bf * freqs * np.pi
    embed = torch.cat([bf.unsqueeze(0), torch.sin(angles), torch.cos(angles)], dim=-1)
    enc = m.blur_feature_encoder[idx]
    z1 = enc[0](embed)
    z2 = enc[2](torch.relu(z1))
    e = enc[4](torch.relu(z2))
    view = torch.cat([m.view_embedder[idx], m.Rt_encoder[idx](Rt[:3, :].reshape(-1))], dim=-1)
    x = m.view_encoder[idx](view)
    wv = m.wv_derivative[idx]
    xs = [x]
    for i in range(m.num_warp - 1):
        w, v = torch.chunk(torch.relu(x), 2, dim=-1)
        t_embed = wv.time_embedder[i]
        x = x + torch.cat([wv.w_linear(torch.cat([w, t_embed, e], dim=-1)), wv.v_linear(torch.cat([v, t_embed, e], dim=-1))],
                          dim=-1)
        xs.append(x)
    latent = torch.stack(xs, 0)
    latent_w, latent_v = torch.chunk(latent, 2, dim=-1)
    w_rigid = m.rot_decoder[idx](latent_w)
    theta = m.theta_decoder[idx](latent_w)[..., None]
    v_rigid = m.trans_decoder[idx](latent_v)
    w_unit = unit(w_rigid) if unit is not None else w_rigid / (torch.norm(w_rigid, dim=-1)[..., None] + 1e-10)
    w1, w2, w3 = torch.chunk(w_unit, 3, dim=-1)
    z = torch.zeros_like(w1)
    Km = torch.cat([z, -w3, w2, w3, z, -w1, -w2, w1, z], dim=-1).reshape(-1, 3, 3)
    K2 = torch.matmul(Km, Km)
    eye = torch.eye(3, dtype=Rt.dtype)
    R_exp = eye + torch.sin(theta) * Km + (1 - torch.cos(theta)) * K2
    G = eye[None] * theta + (1 - torch.cos(theta)) * Km + (theta - torch.sin(theta)) * K2
    p = torch.matmul(G, v_rigid[..., None])
    top = torch.cat([R_exp, p], dim=-1)
    fill = eye.new_zeros(top.size(0), 1, 4)
    fill[..., 3] = 1.0
    c2w = torch.einsum("ij,tjk->tik", Rt, torch.cat([top, fill], dim=1))
    return SimpleNamespace(c2w=c2w, z1=z1, z2=z2, xs=latent, w_rigid=w_rigid, w_unit=w_unit, theta=theta[..., 0, 0],
                           v_rigid=v_rigid, embed=embed, e=e, view=view)


def near_kink(m, Rt, bf, idx):
    """-> (units near a kink, units): the rule of the module docstring on the float64 copy `m`."""
    with torch.no_grad():
        P = forward_parts(m, Rt, bf, idx)
        enc, wv = m.blur_feature_encoder[idx], m.wv_derivative[idx]
        lim1 = enc[0].weight.abs() @ P.embed.abs() + enc[0].bias.abs()
        lim2 = enc[2].weight.abs() @ torch.relu(P.z1) + enc[2].bias.abs()
        ve = m.view_encoder[idx]
        mag = ve.weight.abs() @ P.view.abs() + ve.bias.abs()
        near = int((P.z1.abs() <= KINK * lim1).sum()) + int((P.z2.abs() <= KINK * lim2).sum())
        for i in range(m.num_warp - 1):
            near += int((P.xs[i].abs() <= KINK * mag).sum())
            w, v = torch.chunk(torch.relu(P.xs[i]), 2, dim=-1)
            t = wv.time_embedder[i].abs()
            mag = mag + torch.cat([wv.w_linear.weight.abs() @ torch.cat([w, t, P.e.abs()]) + wv.w_linear.bias.abs(),
                                   wv.v_linear.weight.abs() @ torch.cat([v, t, P.e.abs()]) + wv.v_linear.bias.abs()])
    return near, 2 * 32 + (m.num_warp - 1) * 32


# ---- cases -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture():
    return dict(np.load(os.path.join(GOLDEN, "blce.npz")))


def _fixture_model():
    fx = _fixture()
    m = BLCE(num_views=3, view_dim=32, num_warp=9)
    m.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("sd_")}, strict=True)
    return m


def _seeded_model(num_views, seed):
    """The module as its constructor leaves it."""
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        return BLCE(num_views=num_views, view_dim=32, num_warp=9)


def _spread(m, seed):
    """Decoders, time embeddings and the embedding table away from their initial near-zero (as the fixture's generator
    does)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for i in range(m.num_views):
            for dec, sc in ((m.rot_decoder[i], 0.3), (m.trans_decoder[i], 0.05), (m.theta_decoder[i], 0.1)):
                dec.weight.copy_(sc * torch.randn(dec.weight.shape, generator=g))
                dec.bias.copy_(0.1 * sc * torch.randn(dec.bias.shape, generator=g))
            m.wv_derivative[i].time_embedder.copy_(0.5 * torch.randn(9, 8, generator=g))
        m.view_embedder.copy_(torch.randn(m.num_views, 32, generator=g))
    return m


def _build(name, seed):
    """-> (model, idx, Rt, bf) for one draw of a case."""
    fx = _fixture()
    Rt, bf, idx = torch.from_numpy(fx["in_c2w"]).clone(), torch.from_numpy(fx["out_blur"]).reshape(()).clone(), int(fx["in_idx"][0])
    g = torch.Generator().manual_seed(seed)
    if name == "init":
        m, idx, bf = _seeded_model(3, seed), 1, 0.2 + 0.7 * torch.rand((), generator=g)
    elif name.startswith("view_"):
        idx, n = (int(v) for v in name[5:].split("_of_"))
        if n == 3:
            m = _fixture_model()
        else:
            m, bf = _spread(_seeded_model(n, seed), seed + 1), 0.2 + 0.7 * torch.rand((), generator=g)
    else:
        m = _fixture_model()
    with torch.no_grad():
        if name == "zero_rot":
            m.rot_decoder[idx].weight.zero_()
            m.rot_decoder[idx].bias.zero_()
        elif name == "large":
            P = forward_parts(copy.deepcopy(m).double(), Rt.double(), bf.double(), idx)
            s_th = 1.25 * math.pi / float(P.theta.abs().sort().values[-2])   # the second largest |theta| to 1.25 pi
            s_tr = 1.5 / float(P.v_rigid.abs().max())
            for dec, s in ((m.theta_decoder[idx], s_th), (m.trans_decoder[idx], s_tr)):
                dec.weight.mul_(s)
                dec.bias.mul_(s)
        elif name == "dead_relu":
            enc = m.blur_feature_encoder[idx]
            enc[0].bias[:16] -= 10.0
            enc[2].bias[:16] -= 10.0
            m.view_encoder[idx].bias[:8] -= 3.0
        elif name == "far_camera":
            Rt[:3, 3] *= 100.0 / float(Rt[:3, 3].norm())
    return m, idx, Rt, bf


@functools.lru_cache(maxsize=None)
def case(name):
    """-> namespace(name, model (fp32, CPU), idx, num_views, Rt [4,4], bf (0-d), cots {name: (v_c2w | None, v_w2c | None)},
    seed, near, units): the first seed from 5000 + 100 x (index of the case) on whose draw no unit is near a kink."""
    base = 5000 + 100 * CASES.index(name)
    for seed in range(base, base + 20):
        m, idx, Rt, bf = _build(name, seed)
        near, units = near_kink(copy.deepcopy(m).double(), Rt.double(), bf.double(), idx)
        if near == 0 or not (name == "init" or (name.startswith("view_") and m.num_views != 3)):
            break  # (a state taken from the fixture has no seed to redraw)
    g = torch.Generator().manual_seed(base + 50)
    v_c2w, v_w2c = torch.randn(9, 4, 4, generator=g), torch.randn(9, 4, 4, generator=g)
    cots = {"both": (v_c2w, v_w2c), "c2w": (v_c2w, None), "w2c": (None, v_w2c)}
    return SimpleNamespace(name=name, model=m, idx=idx, num_views=m.num_views, Rt=Rt, bf=bf, cots=cots, seed=seed, near=near,
                           units=units)


@functools.lru_cache(maxsize=None)
def typed_model(name, dtype):
    return copy.deepcopy(case(name).model).to(dtype)


def backward(outs, cots):
    pairs = [(o, c.to(o)) for o, c in zip(outs, cots) if c is not None]
    torch.autograd.backward([o for o, _ in pairs], [c for _, c in pairs])


def _neighbour(t, g):
    """An fp32 tensor with every element moved by at most half an ulp and rounded again: itself or an adjacent value."""
    return (t.double() * (1 + 2.0 ** -24 * (2 * torch.rand(t.shape, generator=g, dtype=torch.float64) - 1))).float()


def evaluate(name, cot, dtype, unit=None, neighbour=None):
    """-> {c2w, w2c [9,4,4], grads: the 22 parameter gradients in the order of csrc/blce.hip} in `dtype`: the module (its
    restatement with `unit`), torch.inverse, autograd.  neighbour = i: on the i-th neighbouring input of the case (the 22
    parameters, the pose and the blur feature through `_neighbour`; the pose's last row stays 0 0 0 1)."""
    c = case(name)
    m = typed_model(name, dtype)
    params = _view_param_list(m, c.idx)
    own = [p.detach().clone() for p in params]
    Rt, bf = c.Rt, c.bf
    if neighbour is not None:
        g = torch.Generator().manual_seed(9000 + 97 * CASES.index(name) + neighbour)
        with torch.no_grad():
            for p, src in zip(params, _view_param_list(c.model, c.idx)):
                p.copy_(_neighbour(src.detach(), g))
        Rt, bf = torch.cat([_neighbour(Rt[:3], g), Rt[3:]]), _neighbour(bf, g)
    try:
        for p in params:
            p.grad = None
        Rt, bf = Rt.to(dtype), bf.to(dtype)
        c2w = forward_parts(m, Rt, bf, c.idx, unit).c2w if unit is not None else m(Rt, bf, c.idx)[0]
        w2c = torch.inverse(c2w)
        backward((c2w, w2c), c.cots[cot])
        grads = [torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in params]
    finally:
        with torch.no_grad():
            for p, v in zip(params, own):
                p.copy_(v)
    return {"c2w": c2w.detach(), "w2c": w2c.detach(), "grads": grads}


@functools.lru_cache(maxsize=None)
def reference(name, cot):
    """(float64, fp32) references of a case and cotangent, computed once and shared: leave them unchanged."""
    return evaluate(name, cot, torch.float64), evaluate(name, cot, torch.float32)


NEIGHBOURS = 8


def _flat(out):
    return [out["c2w"], out["w2c"]] + out["grads"]


@functools.lru_cache(maxsize=None)
def neighbour_gaps(name, cot):
    """24 floats (c2w, w2c, the 22 gradients): max |ref32 - ref64| per tensor, the largest over the case itself and
    NEIGHBOURS neighbouring inputs, each neighbour's fp32 result against the float64 result on the SAME neighbour."""
    gaps = [float((a.double() - b).abs().max()) for a, b in zip(_flat(reference(name, cot)[1]), _flat(reference(name, cot)[0]))]
    for i in range(NEIGHBOURS):
        r64, r32 = evaluate(name, cot, torch.float64, neighbour=i), evaluate(name, cot, torch.float32, neighbour=i)
        gaps = [max(g, float((a.double() - b).abs().max())) for g, a, b in zip(gaps, _flat(r32), _flat(r64))]
    return gaps


def compare(name, cot, got, what, refs=None, sink=None):
    """close_to_f64 at k = 3 on the 9 c2w and the 9 w2c poses and on each of the 22 parameter gradients, with the neighbour
    allowance of the module docstring; the rows of the embedding-table gradient other than the view's own must be exactly
    0.  Every RATIO line is printed, then all failures are raised together.  -> [(family, what, k needed)]."""
    ref64, ref32 = refs or reference(name, cot)
    c = case(name)
    wide = neighbour_gaps(name, cot)
    assert len(got["grads"]) == 22
    needs, failures = [], []
    names = ("c2w", "w2c") + tuple("grad " + n for n in PARAM_NAMES)
    for i, (tag, g, r64, r32) in enumerate(zip(names, _flat(got), _flat(ref64), _flat(ref32))):
        own = float((r32.double() - r64).abs().max())
        needs.append(("poses" if i < 2 else "gradients", f"{what} {tag}",
                      gather(failures, close_map, g, r64, r32, K, f"{what} {tag}", K * (wide[i] - own))))
    table = got["grads"][0].detach().cpu()
    assert tuple(table.shape) == (c.num_views, 32)
    others = torch.ones(c.num_views, dtype=torch.bool)
    others[c.idx] = False
    assert not table[others].any(), f"{what}: rows of the embedding-table gradient other than {c.idx} are not 0"
    if sink is not None:
        sink.extend(needs)
    assert not failures, "\n".join(failures)
    return needs


# ---- planted error (a): the axis normalisation differentiated without the guard at |rot| == 0 ---------------------------
class UnitNoGuard(torch.autograd.Function):
    """w / (|w| + 1e-10) whose backward divides by |w| alone: g / d - w (g . w) / (d d |w|), d = |w| + 1e-10."""

    @staticmethod
    def forward(ctx, w):
        n = w.norm(dim=-1, keepdim=True)
        ctx.save_for_backward(w, n)
        return w / (n + 1e-10)

    @staticmethod
    def backward(ctx, g):
        w, n = ctx.saved_tensors
        d = n + 1e-10
        return g / d - w * ((g * w).sum(-1, keepdim=True) / (d * d * n))
