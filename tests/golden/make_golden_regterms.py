"""Generate tests/golden/regterms.npz by RUNNING THE REFERENCE'S OWN l1_loss, entropy_loss, sparsity_loss
(utils/loss_utils.py) and psnr (utils/image_utils.py) on the CPU, in the container that holds the reference.

    python tests/golden/make_golden_regterms.py

For each case of regterms_restatement.CASES the block of train.py:651-655 and :622 is evaluated with the reference's
functions in fp32 and differentiated by autograd; the same block is evaluated in float64 by the restatement.  The fixture
holds data only: the inputs (depths and images as the float16 / uint8 values they were drawn as, alpha as float32), the
reference's fp32 values and gradients, the float64 values and gradients, and the `ref_gap_*` quantities -- the distance
between the two, of which the GPU tests allow 3 x: relative for a scalar, relative to the map's largest
magnitude for a gradient, in dB for the PSNR.  One more tiny case holds a single alpha = 1.5: every value is NaN.
`log_probe` records torch.log of case 1's arguments as this machine's math library rounds them."""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ref_harness as RH  # noqa: E402
import regterms_restatement as RR  # noqa: E402
from helpers import save_npz  # noqa: E402


def reference_block(L, I, c):
    """train.py:651-655 and :622 with the reference's functions, fp32 -> values and autograd gradients."""
    depth = c["depth"].clone().requires_grad_(True)
    alpha = c["alpha"].clone().requires_grad_(True)
    reg_loss = 0
    depth_loss = L.l1_loss(depth, c["gt_depth"])
    reg_loss += 0.2 * depth_loss
    e, s = L.entropy_loss(alpha), L.sparsity_loss(alpha)
    mask_loss = 1e-7 * e + 1e-7 * s
    reg_loss += mask_loss
    reg_loss.backward()
    out = {"reg_loss": reg_loss, "depth_loss": depth_loss, "mask_loss": mask_loss, "entropy": e, "sparsity": s}
    out = {k: v.detach() for k, v in out.items()}
    out["g_depth"], out["g_alpha"] = depth.grad, alpha.grad
    out["psnr"] = I.psnr(c["image"], c["gt_image"])
    for name, fn in (("entropy", L.entropy_loss), ("sparsity", L.sparsity_loss)):
        a = c["alpha"].clone().requires_grad_(True)
        v = fn(a)
        v.backward()
        assert torch.equal(v.detach(), out[name])
        out["g_" + name] = a.grad
    return out


def np_(t):
    return t.detach().cpu().numpy()


def main():
    for name in ("sklearn", "sklearn.neighbors"):             # imported by utils/loss_utils.py, used by neither function
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["sklearn.neighbors"].NearestNeighbors = None
    L = RH.ref_import("utils.loss_utils")
    I = RH.ref_import("utils.image_utils")
    arrays = {"shapes": np.array(RR.CASES, dtype=np.int64)}
    for i, (B, H, W) in enumerate(RR.CASES):
        c = RR.make_case(B, H, W)
        for k in ("depth", "gt_depth", "image"):
            assert torch.equal(c[k].half().float(), c[k])
        u8 = (c["gt_image"] * 255.0).round().to(torch.uint8)
        assert torch.equal(u8.float() / 255.0, c["gt_image"])
        ref = reference_block(L, I, c)
        f64 = RR.block(c["depth"], c["gt_depth"], c["alpha"], c["image"], c["gt_image"], torch.float64)
        f64.update({k: v for k, v in RR.alone(c["alpha"], torch.float64).items() if k.startswith("g_")})
        assert all(bool(torch.isfinite(v).all()) for v in list(ref.values()) + list(f64.values())), (B, H, W)
        p = f"c{i}_"
        arrays.update({p + "in_depth": np_(c["depth"].half()), p + "in_gt_depth": np_(c["gt_depth"].half()),
                       p + "in_alpha": np_(c["alpha"]), p + "in_image": np_(c["image"].half()),
                       p + "in_gt_image": np_(u8)})
        line = [f"({B},{H},{W})"]
        for k in RR.SCALARS:
            assert ref[k].dtype == torch.float32 and f64[k].dtype == torch.float64
            arrays[p + "ref_" + k], arrays[p + "f64_" + k] = np_(ref[k]).reshape(1), np_(f64[k]).reshape(1)
            arrays[p + "ref_gap_" + k] = np.array([RR.rel_gap(ref[k], f64[k])])
            line.append(f"{k} {arrays[p + 'ref_gap_' + k][0]:.1e}")
        for k in ("g_depth", "g_alpha", "g_entropy", "g_sparsity"):
            arrays[p + "ref_" + k], arrays[p + "f64_" + k] = np_(ref[k]), np_(f64[k])
            arrays[p + "ref_gap_" + k] = np.array([RR.map_gap(ref[k], f64[k])])
            line.append(f"{k} {arrays[p + 'ref_gap_' + k][0]:.1e}")
        arrays[p + "ref_psnr"], arrays[p + "f64_psnr"] = np_(ref["psnr"]), np_(f64["psnr"])
        arrays[p + "ref_gap_psnr"] = np.array([RR.db_gap(ref["psnr"], f64["psnr"])])
        line.append(f"psnr {arrays[p + 'ref_gap_psnr'][0]:.1e} dB")
        print("ref_gap " + "  ".join(line))
    nan_alpha = torch.tensor([0.25, 1.5, 0.0, 0.75])
    a = nan_alpha.clone().requires_grad_(True)
    v = L.entropy_loss(a)
    v.backward()
    assert bool(torch.isnan(v)) and bool(torch.isnan(a.grad[1])) and bool(torch.isfinite(a.grad[[0, 2, 3]]).all())
    arrays.update({"nan_in_alpha": np_(nan_alpha), "nan_ref_entropy": np_(v).reshape(1), "nan_ref_g_entropy": np_(a.grad)})
    # what torch.log gives on this machine for the arguments of case 1: the CPU math library behind it depends on the
    # processor, and so do the last bits of every fp32 value that passes through a logarithm (test_regterms_cpu.py)
    arrays["log_probe"] = np_(torch.log(RR.make_case(*RR.CASES[1])["alpha"].reshape(-1) + RR.EPS))
    files = save_npz(os.path.join(HERE, "regterms.npz"), arrays)
    print(f"wrote {', '.join(files)}  ({sum(os.path.getsize(f) for f in files) / 1024:.0f} KiB, {len(arrays)} arrays)")


if __name__ == "__main__":
    main()
