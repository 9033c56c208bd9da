"""The regularisation terms on the MI355X (csrc/regterms.hip through loss_utils.regularisation_terms, entropy_loss and
sparsity_loss) against float64 on the fixture of tests/golden/regterms.npz and on maps large enough for the grid-stride
loop, under the rule of DESIGN.md 3a: 3 x the reference's own distance from float64, not less than 8 x 2^-24; the depth
gradient bit for bit; run-to-run identity, other layouts and alignments, one-sided gradients, and a captured graph."""
import pytest
import torch

import regterms_restatement as RR
from helpers import load, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return load("regterms")


def run(c, dev, images=True, need=(True, True), cotangent=None):
    """regularisation_terms on the device -> the restatement's dictionary, on the host."""
    from mobgs_amd.loss_utils import regularisation_terms
    depth = c["depth"].to(dev).requires_grad_(need[0])
    alpha = c["alpha"].to(dev).requires_grad_(need[1])
    kw = {"image": c["image"].to(dev), "gt_image": c["gt_image"].to(dev)} if images else {}
    t = regularisation_terms(depth, c["gt_depth"].to(dev), alpha, **kw)
    assert t.reg_loss.requires_grad and not t.depth_loss.requires_grad and not t.mask_loss.requires_grad
    assert t.reg_loss.shape == t.depth_loss.shape == t.mask_loss.shape == ()
    (t.reg_loss if cotangent is None else t.reg_loss * cotangent).backward()
    out = {"reg_loss": t.reg_loss, "depth_loss": t.depth_loss, "mask_loss": t.mask_loss, "g_depth": depth.grad,
           "g_alpha": alpha.grad}
    if images:
        assert t.psnr.shape == (c["image"].shape[0], 1) and not t.psnr.requires_grad
        out["psnr"] = t.psnr
    else:
        assert t.psnr is None
    return {k: (None if v is None else v.detach().cpu()) for k, v in out.items()}


def run_alone(alpha, dev):
    from mobgs_amd.loss_utils import entropy_loss, sparsity_loss
    out = {}
    for name, fn in (("entropy", entropy_loss), ("sparsity", sparsity_loss)):
        a = alpha.to(dev).requires_grad_(True)
        v = fn(a)
        assert v.shape == () and v.requires_grad
        v.backward()
        out[name], out["g_" + name] = v.detach().cpu(), a.grad.cpu()
    return out


def check_scalar(what, got, truth, ref_gap):
    err, tol = RR.rel_gap(got, truth), RR.allowed(ref_gap)
    print(f"{what}: {float(got)!r}, float64 {float(truth)!r}, relative error {err:.2e} (allowed {tol:.2e}, ref_gap "
          f"{float(ref_gap):.1e})")
    assert err <= tol, what


def check_map(what, got, truth, ref_gap):
    truth = torch.as_tensor(truth)
    assert got.shape == truth.shape and got.dtype == torch.float32, what
    err, tol = RR.map_gap(got, truth), RR.allowed(ref_gap)
    print(f"{what}: largest error {err:.2e} of the largest magnitude (allowed {tol:.2e}, ref_gap {float(ref_gap):.1e})")
    assert err <= tol, what            # the LARGEST error: no element lies outside


def check_psnr(what, got, truth, ref_gap):
    err, tol = RR.db_gap(got, truth), RR.allowed(ref_gap, RR.FLOOR_DB)
    print(f"{what}: {got.reshape(-1).tolist()} dB, error {err:.2e} dB (allowed {tol:.2e}, ref_gap {float(ref_gap):.1e})")
    assert err <= tol, what


@pytest.mark.parametrize("i", range(len(RR.CASES)))
def test_fixture_parity(fx, i, hip_device):
    c, want = RR.fixture_case(fx, i)
    restated = RR.block(c["depth"], c["gt_depth"], c["alpha"], dtype=torch.float32)
    for images in (True, False):
        got = run(c, hip_device, images=images)
        tag = f"case {RR.CASES[i]} {'with' if images else 'without'} images"
        for k in ("reg_loss", "depth_loss", "mask_loss"):
            check_scalar(f"{tag} {k}", got[k], want["f64_" + k][0], want["ref_gap_" + k][0])
        check_map(f"{tag} g_alpha", got["g_alpha"], want["f64_g_alpha"], want["ref_gap_g_alpha"][0])
        # v_depth takes the values +-(0.2 / n) and 0 only: bit for bit what autograd gives in fp32
        assert same_bits(got["g_depth"], restated["g_depth"]), tag
        assert same_bits(got["g_depth"], torch.from_numpy(want["ref_g_depth"])), tag
        if images:
            check_psnr(f"{tag} psnr", got["psnr"], want["f64_psnr"], want["ref_gap_psnr"][0])
    alone = run_alone(c["alpha"], hip_device)
    for k in ("entropy", "sparsity"):
        tag = f"case {RR.CASES[i]} {k}_loss"
        check_scalar(tag, alone[k], want["f64_" + k][0], want["ref_gap_" + k][0])
        check_map(tag + " gradient", alone["g_" + k], want["f64_g_" + k], want["ref_gap_g_" + k][0])


def test_nan_is_not_clamped(fx, hip_device):
    from mobgs_amd.loss_utils import regularisation_terms
    alpha = torch.from_numpy(fx["nan_in_alpha"])
    assert alpha.tolist().count(1.5) == 1
    alone = run_alone(alpha, hip_device)
    assert bool(torch.isnan(alone["entropy"])) and float(alone["sparsity"]) == float((alpha ** 2).sum())
    assert torch.isnan(alone["g_entropy"]).tolist() == [False, True, False, False]
    finite = [0, 2, 3]
    want = torch.from_numpy(fx["nan_ref_g_entropy"])
    assert float((alone["g_entropy"][finite] - want[finite]).abs().max()) <= RR.FLOOR * float(want[finite].abs().max())
    assert torch.equal(alone["g_sparsity"], 2 * alpha)             # the switched-off entropy term leaves no NaN behind
    d = torch.tensor([0.25, 0.5, 1.0, 2.0])
    got = run({"depth": d, "gt_depth": d + 0.5, "alpha": alpha}, hip_device, images=False)
    assert bool(torch.isnan(got["reg_loss"])) and bool(torch.isnan(got["mask_loss"]))
    assert float(got["depth_loss"]) == 0.5 and torch.isnan(got["g_alpha"]).tolist() == [False, True, False, False]
    with pytest.raises(ValueError, match="differ in shape"):
        regularisation_terms(d.to(hip_device), d[:2].to(hip_device), alpha.to(hip_device))
    with pytest.raises(ValueError, match="go together"):
        regularisation_terms(d.to(hip_device), d.to(hip_device), alpha.to(hip_device), image=torch.rand(1, 3, 2, 2))
    with pytest.raises(NotImplementedError, match="gt_depth"):
        regularisation_terms(d.to(hip_device), d.to(hip_device).requires_grad_(True), alpha.to(hip_device))


def grid_stride_size():
    """From the size query alone: the elements one workgroup takes per trip, the cap on the workgroups, and a size at
    which every workgroup makes two full trips and the first few a third, ragged one."""
    from mobgs_amd import _lib
    h = _lib.load()
    per = next(n for n in range(1, 1 << 16) if h.mobgs_reg_terms_blocks(n + 1) == 2)
    cap = h.mobgs_reg_terms_blocks(1 << 40)
    n = 2 * cap * per + 5 * per + 3
    assert h.mobgs_reg_terms_blocks(n) == cap and n > (2 * cap - 1) * per and n % 4 == 3 and n <= 4 * 1000 * 1000
    return n


def test_grid_stride(hip_device):
    n = grid_stride_size()
    depth, gt_depth, alpha = RR.random_maps(n, seed=7)
    c = {"depth": depth, "gt_depth": gt_depth, "alpha": alpha}
    f32 = RR.block(depth, gt_depth, alpha, dtype=torch.float32)
    f64 = RR.block(depth, gt_depth, alpha, dtype=torch.float64)
    got = run(c, hip_device, images=False)
    for k in ("reg_loss", "depth_loss", "mask_loss"):
        check_scalar(f"n = {n} {k}", got[k], f64[k], RR.rel_gap(f32[k], f64[k]))
    check_map(f"n = {n} g_alpha", got["g_alpha"], f64["g_alpha"], RR.map_gap(f32["g_alpha"], f64["g_alpha"]))
    assert same_bits(got["g_depth"], f32["g_depth"])
    alone, a32, a64 = run_alone(alpha, hip_device), RR.alone(alpha, torch.float32), RR.alone(alpha, torch.float64)
    for k in ("entropy", "sparsity"):
        check_scalar(f"n = {n} {k}_loss", alone[k], a64[k], RR.rel_gap(a32[k], a64[k]))


def test_run_to_run(fx, hip_device):
    c, _ = RR.fixture_case(fx, 2)
    a, b = run(c, hip_device), run(c, hip_device)
    assert set(a) == set(b) and all(same_bits(a[k], b[k]) for k in a)
    x, y = run_alone(c["alpha"], hip_device), run_alone(c["alpha"], hip_device)
    assert all(same_bits(x[k], y[k]) for k in x)


def test_other_layouts_and_alignments(fx, hip_device):
    from mobgs_amd.loss_utils import regularisation_terms
    dev = hip_device
    c, want = RR.fixture_case(fx, 1)                                # (2, 37, 53): nothing is a multiple of 4
    B, H, W = RR.CASES[1]
    plain = run(c, dev)
    # a channel slice of a wider map (non-contiguous) and the [B,1,H,W] depth: the same call on a contiguous copy
    wide = torch.rand(B, 3, H, W)
    wide[:, 1:2] = c["alpha"]
    wide = wide.to(dev).requires_grad_(True)
    depth = c["depth"].to(dev).requires_grad_(True)
    d_alpha = wide[:, 1:2]
    assert not d_alpha.is_contiguous() and depth.shape == (B, 1, H, W)
    t = regularisation_terms(depth, c["gt_depth"].to(dev), d_alpha, image=c["image"].to(dev), gt_image=c["gt_image"].to(dev))
    t.reg_loss.backward()
    for k, v in (("reg_loss", t.reg_loss), ("depth_loss", t.depth_loss), ("mask_loss", t.mask_loss), ("psnr", t.psnr),
                 ("g_depth", depth.grad), ("g_alpha", wide.grad[:, 1:2])):
        assert same_bits(v, plain[k]), k
    assert depth.grad.shape == (B, 1, H, W) and wide.grad.shape == (B, 3, H, W)
    assert float(wide.grad[:, 0].abs().max()) == 0.0 and float(wide.grad[:, 2].abs().max()) == 0.0
    # flat maps that start 4, 8 and 12 bytes past a 16-byte boundary (gt_depth elsewhere than depth): the gradients are
    # element-wise and stay bit-equal, the sums are added in another order and stay inside the tolerance
    def shifted(t, k):
        buf = torch.zeros(t.numel() + 4, device=dev)
        buf[k:k + t.numel()] = t.reshape(-1).to(dev)
        view = buf[k:k + t.numel()]
        assert view.data_ptr() % 16 == 4 * k and view.is_contiguous()
        return view
    for kd, kg, ka in ((1, 1, 2), (1, 3, 3), (2, 0, 1)):
        depth = shifted(c["depth"], kd).requires_grad_(True)
        alpha = shifted(c["alpha"], ka).requires_grad_(True)
        t = regularisation_terms(depth, shifted(c["gt_depth"], kg), alpha)
        t.reg_loss.backward()
        assert same_bits(depth.grad, plain["g_depth"].reshape(-1)) and same_bits(alpha.grad, plain["g_alpha"].reshape(-1))
        for k, v in (("reg_loss", t.reg_loss), ("depth_loss", t.depth_loss), ("mask_loss", t.mask_loss)):
            check_scalar(f"shifted by {(kd, kg, ka)} {k}", v.detach().cpu(), want["f64_" + k][0], want["ref_gap_" + k][0])


def test_one_sided_gradients(fx, hip_device):
    c, _ = RR.fixture_case(fx, 1)
    both = run(c, hip_device, images=False, cotangent=3.0)
    only_depth = run(c, hip_device, images=False, need=(True, False), cotangent=3.0)
    only_alpha = run(c, hip_device, images=False, need=(False, True), cotangent=3.0)
    assert only_depth["g_alpha"] is None and only_alpha["g_depth"] is None
    assert same_bits(only_depth["g_depth"], both["g_depth"]) and same_bits(only_alpha["g_alpha"], both["g_alpha"])
    for k in ("reg_loss", "depth_loss", "mask_loss"):
        assert same_bits(only_depth[k], both[k]) and same_bits(only_alpha[k], both[k])
    restated = RR.block(c["depth"], c["gt_depth"], c["alpha"], dtype=torch.float32, cotangent=3.0)
    assert same_bits(both["g_depth"], restated["g_depth"])          # the cotangent is read from the device


def test_graph_capture(fx, hip_device):
    from mobgs_amd.graphed import GraphedCallable
    from mobgs_amd.loss_utils import regularisation_terms
    dev = hip_device
    c, _ = RR.fixture_case(fx, 1)
    other = RR.make_case(*RR.CASES[1], seed=5)
    static = {k: v.to(dev).clone() for k, v in c.items()}
    static["depth"].requires_grad_(True)
    static["alpha"].requires_grad_(True)

    def step():     # forward + backward on one stream, no parallel branches
        t = regularisation_terms(static["depth"], static["gt_depth"], static["alpha"], image=static["image"],
                                 gt_image=static["gt_image"])
        g_depth, g_alpha = torch.autograd.grad(t.reg_loss, [static["depth"], static["alpha"]])
        return t.reg_loss.detach(), t.depth_loss, t.mask_loss, t.psnr, g_depth, g_alpha

    graphed = GraphedCallable(step, warmup=1)
    names = ("reg_loss", "depth_loss", "mask_loss", "psnr", "g_depth", "g_alpha")
    for inputs in (c, other, c):
        with torch.no_grad():
            for k, v in inputs.items():
                static[k].copy_(v)
        replay = [v.detach().cpu().clone() for v in graphed()]
        eager = run(inputs, dev)
        for k, v in zip(names, replay):
            assert same_bits(v, eager[k]), k
    assert not same_bits(run(other, dev)["reg_loss"], run(c, dev)["reg_loss"])
