"""The cases of the LPIPS gradient tests (include/mobgs_hip.h K24, backward; mobgs_amd.lpips.LpipsAlex.loss), their float64
truth and their vetting.  Built on lpips_restatement: its seeded trunk, the reference's heads, its constants and its model,
restated here once more (`model`) only to expose the pre-activations and to stay in ONE dtype from the leaf on -- `lpips`
rounds its inputs to fp32, which would round the gradient on its way back; test_lpips_grad_cases_cpu.py holds the two
together bit for bit.

THE TRUTH is torch autograd in float64 through `model` (about 0.1 s per case, 1 s for `flat`, whose convolutions are
conv_sequential -- see truth_conv: recomputed, not stored): the gradient of
sum_b v_b total_b with respect to both images and to the five pre-activations of both images (the ReLU mask applied: what
tap_grads= of the C call stores).

VETTING.  ReLU and max-pool are kinks: a unit that lands on the other side in fp32 changes the gradient by a whole term.  So
the images are searched (`python tests/lpips_grad_cases.py --search`) until the float64 run shows, for BOTH images of every
pair,
  1. every pre-activation of tap l at least margin_l from 0,
  2. in every pool window with a positive maximum the top two at least margin_l apart,
  3. no feature vector that is all zero (there the reference's autograd gives NaN, the kernel 0: DESIGN 15b),
with margin_l = 4 x tolerance(tap_l) x max(tap_l): tolerance(tap_l) is the forward's own bound (lpips_restatement.tolerance
over tests/golden/lpips.npz), within which test_gpu_lpips.py already holds the kernel's maps, so a unit that clears the margin
has the float64 sign and order on the device as well.  The conditions are per image, so the search is per image: a seed for
each pair's ground truth, then one for its noise (SEEDS).  `flat` (two constants, FLAT, vetted like the seeds) has exact
float64 ties in its pool windows: condition 2 lets two positions tie exactly where both meet the image border in the same
way (border_signatures: the same taps of every convolution below them fall into the padding; the positions whose receptive
fields lie inside the image are one such class) -- the kernel's arithmetic is then the same chain on the same values at both,
a padded tap adding fma(0, w, acc) = acc, so they tie in fp32 too, and the first in row-major order takes the gradient in
torch and in the kernel; any other pair needs the margin.  (A rule for the interior alone would refuse every constant image:
along a border row neighbouring positions tie in just this way.)

THE TOLERANCE follows DESIGN 3a: per quantity (the image gradient and the five tap gradients) 3 x the reference's own fp32
distance from float64 -- the larger of torch's fp32 autograd through F.conv2d and through conv_sequential, largest over all
cases, pairs and sides --, not below 8 x 2^-24; an error is the largest absolute error over a pair's gradient array relative
to that array's largest float64 magnitude.  `python tests/lpips_grad_cases.py` measures the gaps and writes them with the
probes and margins to tests/golden/lpips_grad.npz."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

import lpips_restatement as LR
from regterms_restatement import FLOOR, allowed

QUANTITIES = ("image", "tap1", "tap2", "tap3", "tap4", "tap5")
SIZES = ((31, 31, 1), (31, 48, 2), (35, 33, 1), (38, 34, 1), (64, 97, 2), (130, 67, 2))           # (H, W, B)
EXTRA_SIZE = (64, 97, 2)
EXTRAS = ("identical", "clamp", "flat")
CASES = tuple(s + ("noisy",) for s in SIZES) + tuple(EXTRA_SIZE + (e,) for e in EXTRAS)
NOISE = 0.1
FLAT = (0.61, 0.37)                                  # ground truth, prediction: vetted like the seeds (0.5, 0.25 have units inside the margins)
MARGIN_FACTOR = 4.0
# per case and pair (ground-truth seed, noise seed), found by --search; flat has none
SEEDS = {
    "31x31-B1-noisy": [(100004, 105000)],
    "31x48-B2-noisy": [(200002, 205000), (210000, 215000)],
    "35x33-B1-noisy": [(300000, 305000)],
    "38x34-B1-noisy": [(400000, 405001)],
    "64x97-B2-noisy": [(500054, 505005), (510063, 515042)],
    "130x67-B2-noisy": [(600312, 605132), (610123, 615095)],
    "64x97-B2-identical": [(700033, 0), (710002, 0)],
    "64x97-B2-clamp": [(800049, 805009), (810002, 815034)],
}


def case_name(i):
    H, W, B, what = CASES[i]
    return f"{H}x{W}-B{B}-{what}"


def draw_gt(H, W, what, seed):
    """One ground-truth image [3,H,W] fp32."""
    gt = np.random.Generator(np.random.PCG64(seed)).random((3, H, W)).astype(np.float32)
    if what == "clamp":                                  # values outside [0, 1] on both sides, some exactly 0 and 1
        gt = (gt * 2 - 0.5).astype(np.float32)
        gt.reshape(-1)[3::53] = 0.0
        gt.reshape(-1)[17::59] = 1.0
    return gt


def draw_pred(gt, what, seed):
    """The prediction of a ground-truth image."""
    if what == "identical":
        return gt.copy()
    rng = np.random.Generator(np.random.PCG64(seed))
    noise = (NOISE * rng.standard_normal(gt.shape)).astype(np.float32)
    if what == "clamp":
        pred = (gt + 2 * noise).astype(np.float32)
        pred.reshape(-1)[5::61] = 0.0
        pred.reshape(-1)[29::67] = 1.0
        return pred
    return np.clip(gt + noise, 0, 1).astype(np.float32)


def make_case(i, seeds=None):
    """-> dict(gt, pred [B,3,H,W] fp32 arrays, clamp)."""
    H, W, B, what = CASES[i]
    if what == "flat":
        gt = np.full((B, 3, H, W), FLAT[0], np.float32)
        return dict(gt=gt, pred=np.full_like(gt, FLAT[1]), clamp=False)
    seeds = SEEDS[case_name(i)] if seeds is None else seeds
    assert len(seeds) == B
    gt = np.stack([draw_gt(H, W, what, s[0]) for s in seeds])
    pred = np.stack([draw_pred(g, what, s[1]) for g, s in zip(gt, seeds)])
    return dict(gt=gt, pred=pred, clamp=what == "clamp")


def probe(c):
    """A checksum of a case's inputs: what the fixture stores instead of the images."""
    flat = c["pred"].reshape(-1).astype(np.float64)[::7]
    return np.array([c["pred"].sum(dtype=np.float64), c["gt"].sum(dtype=np.float64), float(flat @ np.arange(flat.size)),
                     float(c["clamp"])])


# ---- the model, in one dtype from the leaf on ---------------------------------------------------------------------------

def trunk(x, net, conv=LR.conv_torch):
    """x [N,3,H,W] in [-1, 1], any dtype -> (the five pre-activations, the five ReLU maps)."""
    dtype = x.dtype
    shift = torch.tensor(LR.SHIFT, dtype=dtype).reshape(1, 3, 1, 1)
    scale = torch.tensor(LR.SCALE, dtype=dtype).reshape(1, 3, 1, 1)
    h = (x - shift) / scale
    pre, taps = [], []
    for l, idx in enumerate(LR.TRUNK_INDEX):
        if l in (1, 2):
            h = F.max_pool2d(h, 3, 2)
        w, b = net[f"features.{idx}.weight"].to(dtype), net[f"features.{idx}.bias"].to(dtype)
        z = conv(h, w, b, LR.STRIDE[l], LR.PAD[l])
        h = torch.relu(z)
        pre.append(z)
        taps.append(h)
    return pre, taps


def model(img0, img1, net, heads, clamp=False, unit_range=True, conv=LR.conv_torch):
    """lpips_restatement.lpips in the dtype of img0 / img1 (tensors; leaves keep their graph) -> (totals [B], pre-activations
    and taps of both images).  The clamp acts on the values as given: exact in any dtype, and torch.clamp passes the gradient
    where 0 <= v <= 1, bounds included."""
    dtype = img0.dtype
    a, b = (img0.clamp(0, 1), img1.clamp(0, 1)) if clamp else (img0, img1)
    if unit_range:
        a, b = 2 * a - 1, 2 * b - 1
    (z0, t0), (z1, t1) = trunk(a, net, conv), trunk(b, net, conv)
    layers = []
    for l in range(5):
        n0 = t0[l] / (torch.sqrt(torch.sum(t0[l] ** 2, dim=1, keepdim=True)) + 1e-10)
        n1 = t1[l] / (torch.sqrt(torch.sum(t1[l] ** 2, dim=1, keepdim=True)) + 1e-10)
        lin = heads[f"lin{l}.model.1.weight"].to(dtype)
        layers.append(F.conv2d((n0 - n1) ** 2, lin).mean([2, 3]).reshape(-1))
    total = layers[0]
    for l in range(1, 5):
        total = total + layers[l]
    return total, (z0, z1), (t0, t1)


def gradients(c, net, heads, dtype=torch.float64, conv=LR.conv_torch, v_total=None, unit_range=True):
    """-> dict(total [B], image = (g_gt, g_pred) [B,3,H,W], tap1 .. tap5 = (of gt, of pred) [B,C,h,w]) in dtype: the
    gradient of sum_b v_b total_b (v = 1 without v_total), the tap gradients with respect to the pre-activations."""
    gt = torch.from_numpy(c["gt"]).to(dtype).requires_grad_(True)
    pred = torch.from_numpy(c["pred"]).to(dtype).requires_grad_(True)
    total, (z0, z1), _ = model(gt, pred, net, heads, clamp=c["clamp"], unit_range=unit_range, conv=conv)
    for z in z0 + z1:
        z.retain_grad()
    v = torch.ones_like(total) if v_total is None else torch.as_tensor(v_total).to(dtype)
    (total * v).sum().backward()
    out = dict(total=total.detach(), image=(gt.grad, pred.grad))
    for l in range(5):
        out[f"tap{l + 1}"] = (z0[l].grad, z1[l].grad)
    return out


def pair_gap(got, truth):
    """[B]: per pair the largest absolute error over the array, relative to the array's largest float64 magnitude."""
    got, truth = torch.as_tensor(got).double(), torch.as_tensor(truth).double()
    B = truth.shape[0]
    err = (got - truth).abs().reshape(B, -1).max(1).values
    scale = truth.abs().reshape(B, -1).max(1).values
    return (err / torch.where(scale > 0, scale, torch.ones_like(scale))).numpy()


# ---- vetting ------------------------------------------------------------------------------------------------------------

_FORWARD_TOL = None


def forward_tolerances():
    """[5]: the forward's own bound per tap (lpips_restatement.tolerance over tests/golden/lpips.npz)."""
    global _FORWARD_TOL
    if _FORWARD_TOL is None:
        gaps = LR.reference_gaps(dict(np.load(os.path.join(LR.GOLDEN, "lpips.npz"))))
        _FORWARD_TOL = np.array([LR.tolerance(name, gaps) for name in LR.TAPS])
    return _FORWARD_TOL


def border_signatures(H, W):
    """Per tap an integer map [h,w] (float64 storage): two positions carry the same number where their receptive fields
    meet the image border in the same way -- the same taps of every convolution below them fall into the padding --, so that
    on a constant image both are the same chain of operations on the same values, in float64 and in the kernel's fp32
    alike.  A position whose receptive field lies inside the image carries the interior's number.  Computed by pushing an
    inside indicator through the trunk's geometry with random integer weights (exact in float64: every sum stays below
    2^53), so different patterns get different numbers but for a hash collision (p ~ 1e-6 per pair)."""
    rng = np.random.Generator(np.random.PCG64(4242))
    prime = 999983.0

    def mix(s, k, stride, pad):
        w = torch.from_numpy(rng.integers(1, 1000, (1, 1, k, k)).astype(np.float64))
        return torch.remainder(F.conv2d((s + 1.0)[None, None], w, stride=stride, padding=pad)[0, 0], prime)
    s = torch.zeros(H, W, dtype=torch.float64)
    out = []
    for l in range(5):
        if l in (1, 2):
            s = mix(s, 3, 2, 0)
        s = mix(s, LR.KS[l], LR.STRIDE[l], LR.PAD[l])
        out.append(s)
    return out


def truth_conv(what):
    """The convolution of the float64 truth and of the vetting.  F.conv2d, except for `flat`: there the truth hangs on EXACT
    ties, and whether a library's blocked convolution rounds two same-chain positions alike depends on the machine (its
    vector width, its tails); conv_sequential is element-wise arithmetic, the same operations at every position anywhere."""
    return LR.conv_sequential if what == "flat" else LR.conv_torch


def vet_image(x, net, flat=False):
    """x [1,3,H,W] float64, the image as the model sees it before 2 x - 1 (clamped already) -> dict(ok, margin [5],
    min_abs_z [5], min_pool_gap [2], zero_vectors): the three conditions of the module docstring for one image."""
    tol = forward_tolerances()
    with torch.no_grad():
        pre, taps = trunk(2 * x - 1, net, truth_conv("flat" if flat else ""))
    sigs = border_signatures(x.shape[2], x.shape[3]) if flat else None
    margin, min_z, gaps, zero = np.zeros(5), np.zeros(5), np.full(2, np.inf), 0
    ok = True
    for l in range(5):
        margin[l] = MARGIN_FACTOR * tol[l] * float(taps[l].max())
        min_z[l] = float(pre[l].abs().min())
        ok &= min_z[l] >= margin[l]
        zero += int((taps[l].sum(1) == 0).sum())
        if l < 2:
            t = taps[l][0]                                                   # [C,h,w]
            win = F.unfold(t[:, None], 3, stride=2)                          # [C, 9, L]
            top, at = win.max(1, keepdim=True)                               # (the first maximum)
            gap = top - win                                                  # of every position from the maximum
            need = (top > 0).expand_as(win).clone()
            need.scatter_(1, at, False)
            if flat:                                                         # exact ties of same-chain positions are fine
                sg = F.unfold(sigs[l][None, None], 3, stride=2).expand_as(win)
                need &= ~((gap == 0) & (sg == torch.gather(sg, 1, at)))
            if bool(need.any()):
                gaps[l] = float(gap[need].min())
                ok &= gaps[l] >= margin[l]
    ok &= zero == 0
    return dict(ok=bool(ok), margin=margin, min_abs_z=min_z, min_pool_gap=gaps, zero_vectors=zero)


def prepared(c, key, b):
    x = torch.from_numpy(c[key][b:b + 1])
    return (x.clamp(0, 1) if c["clamp"] else x).double()


def vet_case(c, net, flat=False):
    """-> (ok, [per pair (report of gt, report of pred)])."""
    reports = [(vet_image(prepared(c, "gt", b), net, flat), vet_image(prepared(c, "pred", b), net, flat))
               for b in range(c["gt"].shape[0])]
    return all(r[0]["ok"] and r[1]["ok"] for r in reports), reports


def search(i, net, tries=4000, log=print):
    """Seeds for case i: per pair a ground truth that passes, then a noise that passes with it."""
    H, W, B, what = CASES[i]
    seeds, base = [], 100000 * (i + 1)
    for b in range(B):
        found = None
        for k in range(tries):
            sg = base + 10000 * b + k
            gt = draw_gt(H, W, what, sg)
            x = torch.from_numpy(gt[None])
            if not vet_image((x.clamp(0, 1) if what == "clamp" else x).double(), net)["ok"]:
                continue
            if what == "identical":
                found = (sg, 0)
                break
            for j in range(tries):
                sn = base + 10000 * b + 5000 + j
                p = torch.from_numpy(draw_pred(gt, what, sn)[None])
                if vet_image((p.clamp(0, 1) if what == "clamp" else p).double(), net)["ok"]:
                    found = (sg, sn)
                    break
            if found:
                break
        if not found:
            raise RuntimeError(f"{case_name(i)}: no seeds for pair {b} in {tries} tries")
        log(f"{case_name(i)} pair {b}: {found}")
        seeds.append(found)
    return seeds


# ---- the fixture --------------------------------------------------------------------------------------------------------

def reference_gaps(fx):
    """Per quantity the LARGEST fp32 distance from float64 over the fixture's cases, pairs, sides and both fp32 runs."""
    return {name: float(max(fx["gap_f32"][:, j].max(), fx["gap_seq"][:, j].max())) for j, name in enumerate(QUANTITIES)}


def tolerance(name, ref_gaps):
    return allowed(ref_gaps[name], FLOOR)


def build_fixture(log=print):
    net, heads = LR.seeded_trunk(), LR.reference_heads()
    g32, gseq, probes, margins, min_z, min_gap = [], [], [], [], [], []
    for i in range(len(CASES)):
        c = make_case(i)
        ok, reports = vet_case(c, net, flat=CASES[i][3] == "flat")
        assert ok, case_name(i)
        truth = gradients(c, net, heads, conv=truth_conv(CASES[i][3]))
        rows = []
        for conv in (LR.conv_torch, LR.conv_sequential):
            got = gradients(c, net, heads, torch.float32, conv)
            rows.append([max(float(pair_gap(got[q][s], truth[q][s]).max()) for s in (0, 1)) for q in QUANTITIES])
        if CASES[i][3] == "identical":                                       # every gradient is 0: no distance to measure
            assert all(float(truth[q][s].abs().max()) == 0 for q in QUANTITIES for s in (0, 1))
        g32.append(rows[0])
        gseq.append(rows[1])
        probes.append(probe(c))
        margins.append(np.max([r[s]["margin"] for r in reports for s in (0, 1)], 0))
        min_z.append(np.min([r[s]["min_abs_z"] for r in reports for s in (0, 1)], 0))
        min_gap.append(np.min([r[s]["min_pool_gap"] for r in reports for s in (0, 1)], 0))
        log(case_name(i), "f32", rows[0], "seq", rows[1])
    return dict(gap_f32=np.array(g32), gap_seq=np.array(gseq), probe=np.stack(probes), margin=np.stack(margins),
                min_abs_z=np.stack(min_z), min_pool_gap=np.stack(min_gap))


if __name__ == "__main__":
    if "--search" in sys.argv:
        only = [int(a) for a in sys.argv[1:] if a.isdigit()] or range(len(CASES))
        net = LR.seeded_trunk()
        for i in only:
            if CASES[i][3] != "flat":
                print(f'    "{case_name(i)}": {search(i, net)},', flush=True)
    else:
        np.savez_compressed(os.path.join(LR.GOLDEN, "lpips_grad.npz"), **build_fixture())
