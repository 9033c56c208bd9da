"""mobgs_amd.loss_utils.flow_warp_loss (csrc/flowloss.hip) against the restated reference block train.py:651-671
(oracle.render_torch.flow_warp_loss = the reference's own torch calls, on the CPU): value and all six gradients."""
import pytest
import torch

from oracle import render_torch as RT

pytestmark = pytest.mark.gpu


def _case(B, K, H, W, seed, flow=2.5, zero_frac=0.3, far=0.02):
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    pix = torch.stack([xs, ys], dim=-1)

    def coords():
        # a smooth flow (what get_flow renders) + per-pixel noise + a few far-away samples that hit the border clamp
        low = torch.randn(B, K, max(H // 8, 2), max(W // 8, 2), 2, generator=g) * flow
        smooth = torch.nn.functional.interpolate(low.flatten(0, 1).permute(0, 3, 1, 2), size=(H, W), mode="bilinear",
                                                 align_corners=True).permute(0, 2, 3, 1).reshape(B, K, H, W, 2)
        c = pix + smooth + 0.3 * torch.randn(B, K, H, W, 2, generator=g)
        out = torch.rand(B, K, H, W, generator=g) < far
        c[out] += 3.0 * max(H, W) * torch.randn(int(out.sum()), 2, generator=g)
        return c.contiguous()

    def mask(*shape):
        m = torch.rand(*shape, generator=g)
        blocks = torch.rand(*shape[:-2], max(H // 6, 1), max(W // 6, 1), generator=g) < zero_frac
        z = torch.nn.functional.interpolate(blocks.float().reshape(-1, 1, *blocks.shape[-2:]), size=(H, W)).reshape(shape)
        return (m * (1 - z)).contiguous()   # exactly zero over whole regions, like a dynamic-object alpha

    return dict(ori=torch.rand(B, 3, H, W, generator=g), latent=torch.rand(B, K, 3, H, W, generator=g),
                e2m=coords(), m2e=coords(), la=mask(B, K, 1, H, W), da=mask(B, 1, H, W))


NAMES = ("ori", "latent", "e2m", "m2e", "la", "da")


def _run(fn, case, dev, dtype=torch.float32, **kw):
    t = {k: v.clone().to(dev, dtype).requires_grad_(True) for k, v in case.items()}
    loss = fn(*(t[k] for k in NAMES), **kw)
    loss.backward()
    return float(loss), {k: t[k].grad.detach().cpu() for k in NAMES}


def _check(got, ggot, ref, gref, what, ref32=None, gref32=None, tight32=True):
    """The reference is evaluated in float64 on the CPU, so the comparison does not depend on the order in which some
    torch version / thread count happens to add fp32 terms.  Against float64 the bounds are those of the fp32
    FORMULATION (which the kernel shares with the reference's torch calls), measured as fp32-CPU against fp64-CPU at
    1352x1014: the loss (a mean over 12 M terms) 3e-8 relative; gradient elements up to 1.3e-4 of the tensor's maximum
    (coordinate gradients are differences of neighbouring image values, the mask gradients carry the fp32 sum of 4 M mask
    values in their denominator).  Both grow with the number of summed terms, so the allowance does too (a flat
    3e-4 let a regression 100x the observed error pass on the small cases): 1e-5 of the maximum on the small cases, rising
    linearly to 3e-4 at the benchmark size = ~2.3x what is observed there.
    The L1 terms have sgn() in their derivative: where |difference * mask| is within rounding of zero fp32 and fp64 may pick
    different signs.  Such an element is accepted only if (a) at most 1e-4 of the tensor's elements are concerned, and (b)
    the element looks like a flipped term: the fp32 evaluation of the reference's own torch statements on the CPU misses
    float64 there as well (same formulation, same near-zero difference), or the value is the reference mirrored
    (|err| <= 2 |ref| + bound: what flipping the one term of an image-gradient element does).
    ref32 / gref32 (small cases): a second, TIGHT comparison against that fp32 CPU evaluation -- observed <= 5e-7 of the
    maximum (scripts/observed_flow_loss_errors.py), allowed 5e-6 and 3e-6 relative on the loss."""
    n_terms = max(int(gref["latent"].numel()), 1)
    rel = min(3e-4, max(1e-5, 3e-4 * n_terms / 12.3e6))
    assert abs(got - ref) <= max(1e-6, 1e-5 * n_terms / 12.3e6) * abs(ref), (what, got, ref)
    for k in NAMES:
        a, b = ggot[k].double(), gref[k].double()
        assert a.shape == b.shape
        m = float(b.abs().max())
        bound = rel * m + 1e-5 * b.abs() + 1e-14
        err = (a - b).abs()
        bad = err > bound
        nbad = int(bad.sum())
        assert nbad <= 1e-4 * bad.numel(), (what, k, nbad, float(err.max()), m)
        if nbad:
            mirrored = err <= 2.0 * b.abs() + bound
            cpu_too = torch.zeros_like(bad)
            if gref32 is not None:
                cpu_too = (gref32[k].double() - b).abs() > bound
            unexplained = bad & ~mirrored & ~cpu_too
            assert int(unexplained.sum()) == 0, (what, k, nbad, int(unexplained.sum()), float(err[bad].max()), m)
            assert float(err[bad].max()) <= 2.0 * m, (what, k, nbad, float(err[bad].max()), m)
    if gref32 is not None and tight32:
        assert abs(got - ref32) <= 3e-6 * abs(ref32), (what, got, ref32)
        for k in NAMES:
            a, b = ggot[k].double(), gref32[k].double()
            m = float(b.abs().max())
            err = (a - b).abs()
            bad = err > 5e-6 * m + 1e-14
            # (fp32 against fp32: a sign may still flip where the difference is within rounding of zero)
            assert int((bad & ~(err <= 2.0 * b.abs() + 5e-6 * m)).sum()) == 0 and int(bad.sum()) <= 1e-4 * bad.numel() + 1, \
                (what, k, "fp32 reference", int(bad.sum()), float(err.max()), m)


@pytest.mark.parametrize("B,K,H,W,seed", [(1, 1, 5, 7, 0), (2, 3, 37, 70, 1), (1, 9, 67, 129, 2), (2, 2, 130, 64, 3)])
def test_flow_warp_loss_matches_reference_block(hip_device, B, K, H, W, seed):
    from mobgs_amd.loss_utils import flow_warp_loss
    case = _case(B, K, H, W, seed)
    ref, gref = _run(RT.flow_warp_loss, case, "cpu", torch.float64)
    ref32, gref32 = _run(RT.flow_warp_loss, case, "cpu", torch.float32)
    for combine in (True, False):
        got, ggot = _run(flow_warp_loss, case, hip_device, combine_taps=combine)
        # observed (scripts/observed_flow_loss_errors.py, against the fp32 CPU evaluation): loss 1e-7 relative; gradients
        # <= 5e-7 of the tensor's maximum (2.3e-6 on the atomically summed image gradients at the benchmark size)
        _check(got, ggot, ref, gref, f"combine_taps={combine}", ref32, gref32)


def test_zero_weight_is_a_constant_and_inputs_are_untouched(hip_device):
    from mobgs_amd.loss_utils import flow_warp_loss
    case = {k: v.to(hip_device) for k, v in _case(1, 2, 16, 24, 5).items()}
    before = {k: v.clone() for k, v in case.items()}
    z = flow_warp_loss(*(case[k].requires_grad_(True) for k in NAMES), lambda_flow_loss=0)
    assert float(z) == 0.0 and not z.requires_grad
    v = flow_warp_loss(*(case[k] for k in NAMES), lambda_flow_loss=1e-2)
    v.backward()
    for k in NAMES:  # (the reference normalises its coordinate tensors in place; this entry point must not)
        assert torch.equal(case[k].detach(), before[k])
    assert float(v) > 0 and all(case[k].grad is not None for k in NAMES)


def test_needs_input_grad_subsets_and_shapes(hip_device):
    from mobgs_amd.loss_utils import flow_warp_loss
    case = {k: v.to(hip_device) for k, v in _case(2, 2, 12, 20, 6).items()}
    full, gfull = _run(flow_warp_loss, {k: v.cpu() for k, v in case.items()}, hip_device)
    # only the coordinate maps differentiable (a caller that detaches the images)
    t = dict(case)
    t["e2m"] = case["e2m"].clone().requires_grad_(True)
    t["la"] = case["la"].reshape(2, 2, 12, 20)           # [B,K,H,W] accepted like [B,K,1,H,W]
    loss = flow_warp_loss(*(t[k] for k in NAMES))
    loss.backward()
    assert abs(float(loss) - full) <= 1e-6 * full
    assert torch.allclose(t["e2m"].grad.cpu(), gfull["e2m"], rtol=1e-5, atol=1e-9)
    with pytest.raises(ValueError):
        flow_warp_loss(case["ori"], case["latent"], case["e2m"][..., :1], case["m2e"], case["la"], case["da"])


def test_flow_warp_loss_at_benchmark_size(hip_device):
    """One view x K = 3 exposures at 1352x1014 against the reference block on the CPU.  One view is 22 x 32 = 704 workgroups
    of 32 rows, under the 1024 from which the backward pass walks 8-row strips: this runs the 4-ROW build at many
    workgroups.  The 8-row build (what training launches for two views of this size) is tested on the cases tall8_a,
    tall8_b and white_noise_8 of tests/test_gpu_flow_kernels.py."""
    from mobgs_amd import _lib
    from mobgs_amd.loss_utils import flow_warp_loss
    assert _lib.load().mobgs_flow_warp_loss_bwd_rows(1, 1014, 1352, 1) == 4
    assert _lib.load().mobgs_flow_warp_loss_bwd_rows(2, 1014, 1352, 1) == 8
    case = _case(1, 3, 1014, 1352, 9, flow=3.0)
    ref, gref = _run(RT.flow_warp_loss, case, "cpu", torch.float64)
    _, gref32 = _run(RT.flow_warp_loss, case, "cpu", torch.float32)  # only to tell flipped sgn() terms (see _check)
    got, ggot = _run(flow_warp_loss, case, hip_device)
    _check(got, ggot, ref, gref, "benchmark size", None, gref32, tight32=False)
