"""The list-free float64 restatement (oracle/gsplat_bruteforce.py) against the two restatements that build tile lists
(oracle/gsplat_torch.py: torch fp32 + autograd; oracle/gsplat_cpu.c: plain C with a hand-written backward).  VERDICT r3
item 7: nothing pins the rasterizer core to real gsplat, but a mistake in the tile-list picture the other restatements
(and the HIP kernels) share -- binning rectangle, key order, offsets, batch walk -- would show here, where no lists exist.

Bounds: projection outputs 1e-5 relative (fp32 vs fp64 arithmetic); radii equal except splats whose 3 sqrt(lambda) lies
within fp32 rounding of an integer; images within 3e-5 of the channel range except the elements a flipped skip / stop
decision touches (helpers.close_image_with_blend_flips: derived one-blend-step bound); gradients rtol 1e-3 + 1e-4 of the
tensor's maximum with the 1e-5 flip tail of the full-size tests."""
import os

import numpy as np
import pytest
import torch

from helpers import close, close_image_with_blend_flips, load_npz, save_npz
from mobgs_amd.synth import SynthCamera, splat_inputs

NAMES = ["means", "quats", "scales", "opacities", "colors"]


def _scene(n=2000, w=160, h=128, seed=3, channels=9):
    cam = SynthCamera().scaled(w, h)
    s = splat_inputs(n, cam, seed, channels)
    g = torch.Generator().manual_seed(seed + 50)
    bg = torch.rand(1, channels, generator=g)
    v_img = torch.randn(1, h, w, channels + 1, generator=g)
    v_a = torch.randn(1, h, w, 1, generator=g)
    return s, bg, v_img, v_a, w, h


def _run(fn, s, bg, v_img, v_a, w, h, dtype):
    t = {k: v.clone().to(dtype).requires_grad_(k in NAMES) for k, v in s.items()}
    img, a, meta = fn(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], t["viewmats"], t["Ks"], w, h,
                      backgrounds=bg.to(dtype), render_mode="RGB+ED", packed=False)
    torch.autograd.backward([img, a], [v_img.to(dtype), v_a.to(dtype)])
    return img.detach(), a.detach(), meta, {k: t[k].grad.detach() for k in NAMES}


# The float64 evaluation of _scene() takes ~45 s of CPU time.  The CPU suite computes it (fixture below) and checks the
# stored copy tests/golden/bruteforce_ref.npz against it; the GPU suite, which has 300 s for everything, loads the copy
# (`python tests/test_bruteforce_oracle_cpu.py` rewrites it: the oracle's own output on _scene(), nothing else).
REF_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bruteforce_ref.npz")
_META = ("radii", "means2d", "conics", "depths")


def save_reference(ref, path=REF_FILE):
    img, a, meta, g = ref
    save_npz(path, dict(img=img.numpy(), alpha=a.numpy(), **{"meta_" + k: meta[k].detach().numpy() for k in _META},
                        **{"grad_" + k: v.numpy() for k, v in g.items()}))


def load_reference(path=REF_FILE):
    z = load_npz(path)
    meta = {k: torch.from_numpy(z["meta_" + k]) for k in _META}
    return (torch.from_numpy(z["img"]), torch.from_numpy(z["alpha"]), meta,
            {k: torch.from_numpy(z["grad_" + k]) for k in NAMES})


@pytest.fixture(scope="module")
def brute():
    from oracle import gsplat_bruteforce as BF
    s, bg, v_img, v_a, w, h = _scene()
    return (s, bg, v_img, v_a, w, h), _run(BF.rasterization, s, bg, v_img, v_a, w, h, torch.float64)


def test_stored_reference_is_the_oracles_output(brute):
    """tests/golden/bruteforce_ref.npz (what tests/test_gpu_bruteforce.py compares the HIP path with) IS what
    oracle/gsplat_bruteforce.py computes on _scene() -- to float64 rounding of another host's summation order."""
    _, ref = brute
    img, a, meta, g = ref
    simg, sa, smeta, sg = load_reference()
    assert torch.equal(smeta["radii"], meta["radii"])
    for name, x, y in [("img", simg, img), ("alpha", sa, a)] + [(k, smeta[k], meta[k].detach()) for k in _META[1:]] + \
            [("grad " + k, sg[k], g[k]) for k in NAMES]:
        assert x.dtype == torch.float64 and x.shape == y.shape, name
        assert float((x - y).abs().max()) <= 1e-10 * max(1.0, float(y.abs().max())), name


def check_against_bruteforce(img, alpha, radii, means2d, conics, grads, scene, ref, what):
    """Shared with tests/test_gpu_bruteforce.py (the HIP path against the same reference)."""
    s = scene[0]
    rimg, ra, rmeta, rg = ref
    rr = rmeta["radii"][0].numpy()
    rad = np.asarray(radii).reshape(-1)
    differ = rad != rr
    # fp32 vs fp64: ceil(3 sqrt(lambda)) may land on the other side of an integer for a handful of splats
    assert int(differ.sum()) <= 2e-3 * rad.size and int(np.abs(rad - rr).max()) <= 1, (what, int(differ.sum()))
    vis = (rad > 0) & (rr > 0)
    close(torch.as_tensor(means2d).reshape(-1, 2)[vis], rmeta["means2d"][0][vis], 1e-5, 1e-4, f"{what}: means2d")
    close(torch.as_tensor(conics).reshape(-1, 3)[vis], rmeta["conics"][0][vis], 2e-4, 1e-6, f"{what}: conics")
    if int(differ.sum()):
        return  # a different radius changes a tile rectangle: lists differ by construction, nothing more to compare
    depth = rmeta["depths"][0][vis]
    spread = float((depth.max() - depth.min()).detach())
    scale = max(1.0, float(rimg[..., :9].abs().max()))
    close_image_with_blend_flips(img[0], rimg[0], ra[0], float(s["colors"].abs().max()), spread, 3e-5 * max(scale, spread),
                                 f"{what}: image", flip_frac=2e-3, n_colour_channels=9,
                                 alphas_img=torch.as_tensor(alpha).reshape(ra.shape)[0])
    close(torch.as_tensor(alpha).reshape(ra.shape), ra, 0, 3e-5, f"{what}: alpha", flip_frac=2e-3, flip_atol=2.0 * 1.001 / 255.0)
    for k in NAMES:
        sc = float(rg[k].abs().max())
        close(grads[k], rg[k], 1e-3, 1e-4 * sc + 1e-9, f"{what}: grad[{k}]", flip_frac=2e-3, flip_atol=2e-2 * sc)


def test_torch_oracle_agrees_with_the_list_free_restatement(brute):
    from oracle import gsplat_torch as G
    scene, ref = brute
    img, a, meta, g = _run(G.rasterization, *scene, torch.float32)
    check_against_bruteforce(img, a, meta["radii"].numpy(), meta["means2d"], meta["conics"], g, scene, ref, "torch oracle")


def test_c_oracle_agrees_with_the_list_free_restatement(brute):
    from oracle import gsplat_cpu as Cc
    scene, ref = brute
    s, bg, v_img, v_a, w, h = scene
    r = Cc.rasterization_fwd_bwd(s["means"].numpy(), s["quats"].numpy(), s["scales"].numpy(), s["opacities"].numpy(),
                                 s["colors"].numpy(), s["viewmats"].numpy(), s["Ks"].numpy(), w, h,
                                 backgrounds=bg.numpy(), render_mode="RGB+ED", v_render=v_img.numpy(),
                                 v_alphas=v_a[..., 0].numpy())
    grads = {k: torch.from_numpy(r["v_" + k]) for k in NAMES}
    check_against_bruteforce(torch.from_numpy(r["render"]), torch.from_numpy(r["alphas"]), r["radii"], r["means2d"],
                             r["conics"], grads, scene, ref, "C oracle")


def test_membership_rule_matters():
    """The list-free walk still applies A.2's tile rectangle, which is semantics and not an optimisation: an opaque
    isotropic splat (variance 7.06 px^2 -> radius ceil(3 x 2.657) = 8) centred in tile (1, 1) has the box [16, 32]^2,
    i.e. exactly that tile, yet reaches alpha = exp(-8.5^2 / 14.12) = 0.006 > 1/255 at the nearest pixel centres of the
    neighbouring tiles.  gsplat never evaluates it there; a restatement without the rule would."""
    from oracle import gsplat_bruteforce as BF
    m2d = torch.tensor([[24.0, 24.0]])
    conics = torch.tensor([[1 / 7.06, 0.0, 1 / 7.06]])
    col, op, depth = torch.ones(1, 1), torch.ones(1), torch.ones(1)
    img, a, last = BF.composite(m2d, conics, col, op, depth, torch.tensor([8]), 48, 48)
    assert float(a[24, 16]) > 1.0 / 255.0 and float(a[24, 24]) > 0.9
    outside = a.clone()
    outside[16:32, 16:32] = 0.0
    assert float(outside.abs().max()) == 0.0, "the splat must not be evaluated outside its tile rectangle"
    _, a2, _ = BF.composite(m2d, conics, col, op, depth, torch.tensor([1000]), 48, 48)  # rectangle = whole image
    assert 0.0055 < float(a2[24, 15]) < 0.0065 and float(a2[24, 15]) > 1.0 / 255.0


if __name__ == "__main__":
    from oracle import gsplat_bruteforce as BF
    sc = _scene()
    save_reference(_run(BF.rasterization, *sc, torch.float64))
    print("wrote", REF_FILE, os.path.getsize(REF_FILE), "bytes")
