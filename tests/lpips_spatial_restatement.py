"""The spatial and masked forms of LPIPS (include/mobgs_hip.h K24, mobgs_lpips_alex_spatial) restated with torch on the CPU,
on top of lpips_restatement: what /root/reference/models/networks_basic.py:16-28 and :79-82 (spatial_average with a mask,
upsample under spatial=True) and dycheck_metrics.py:203-244 (compute_lpips, masked_mean) define, in our own words, in
either dtype.  float64 of these statements is the truth the GPU tests measure against; float32, once with F.conv2d and once
with conv_sequential, stands for "the reference as it can be run here".

    ds = dist_maps(img0, img1, trunk, heads, dtype, conv)     five maps d_l [B,1,h_l,w_l]
    spatial_map(ds, H, W)                                     up(d_1) + ... + up(d_5) in that order: F.interpolate(size=(H, W),
                                                              mode="bilinear", align_corners=False)
    dycheck_mean(map, m)                                      per pair sum(map m) / max(sum(m), 1e-6)
    masked_layers(ds, m)                                      per pair and layer sum(d_l m_l) / (sum(m_l) + 1e-8), the
                                                              numerators and denominators; m_l = F.interpolate(m, size=(h_l,
                                                              w_l)) (nearest)
    nearest_index(n_out, n_in)                                the rule the kernel uses for m_l: min(floor(fl32(i fl32(n_in /
                                                              n_out))), n_in - 1) (tests/test_lpips_spatial_cpu.py holds it
                                                              against F.interpolate)

THE SIZE.  The reference's upsample passes scale_factor = H / h, for which torch sizes the output floor(h scale_factor): H - 1
for some (H, h) (quirk_sizes), where the reference raises at val += res[l].  The map here is defined at H x W for every
size (size=).  Where the reference's form works the two agree to rounding (tested).

The cases: lpips_restatement.SIZES plus (49, 61, 1), which has the quirk on both axes, with gt = rand and pred = clamp(gt +
0.1 randn), plus one identical pair; per case seven masks (MASKS).  compute_lpips (both images times the mask first) is
recorded for the B = 1 sizes on the ones, rectangle, soft and Bernoulli masks: premultiplied by a one-pixel mask both images
are almost equal and the value would test nothing.

tests/golden/lpips_spatial.npz is written by `python tests/lpips_spatial_restatement.py` (a few minutes on one core): per
case, mask and pair the eight VALUES in float64 and in both fp32 runs, per case the map's distance of both fp32 runs from
float64 (largest error over the map relative to its largest value), the compute_lpips values, and a probe per case; no images,
no masks, no maps."""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn.functional as F

import lpips_restatement as LR
from lpips_restatement import FLOOR, allowed, map_gap, rel_gap  # noqa: F401

GOLDEN = LR.GOLDEN
SIZES = LR.SIZES + ((49, 61, 1),)                                          # (H, W, B)
IDENTICAL_SIZE = (64, 97, 3)
CASES = tuple(s + ("noisy",) for s in SIZES) + (IDENTICAL_SIZE + ("identical",),)
MASKS = ("ones", "bernoulli", "rect", "soft", "empty", "first", "last")
VALUES = ("mean", "masked_mean", "masked_total", "mlayer1", "mlayer2", "mlayer3", "mlayer4", "mlayer5")
CL_MASKS = ("ones", "rect", "soft", "bernoulli")                           # compute_lpips: on the B = 1 noisy cases
CL_CASES = tuple(i for i, c in enumerate(CASES) if c[2] == 1 and c[3] == "noisy")
QUANTITIES = ("map",) + VALUES + ("compute_lpips",)


def case_name(i):
    H, W, B, what = CASES[i]
    return f"{H}x{W}-B{B}-{what}"


def make_case(i):
    """-> dict(gt, pred): [B,3,H,W] fp32 arrays in [0, 1]."""
    H, W, B, what = CASES[i]
    rng = np.random.Generator(np.random.PCG64(3000 + i))
    gt = rng.random((B, 3, H, W)).astype(np.float32)
    pred = np.clip(gt + (LR.NOISE * rng.standard_normal((B, 3, H, W))).astype(np.float32), 0, 1).astype(np.float32)
    if what == "identical":
        pred = gt.copy()
    return dict(gt=gt, pred=pred)


def make_mask(i, name):
    """-> [B,H,W] fp32 in [0, 1]."""
    H, W, B, _ = CASES[i]
    rng = np.random.Generator(np.random.PCG64(4000 + 16 * i + MASKS.index(name)))
    m = np.zeros((B, H, W), np.float32)
    if name == "ones":
        m[:] = 1
    elif name == "bernoulli":
        m[:] = rng.random((B, H, W)) < 0.5
    elif name == "rect":                         # leaves a border out, unequal on the four sides
        m[:, H // 5:H - H // 4, W // 4:W - W // 6] = 1
    elif name == "soft":
        m[:] = rng.random((B, H, W))
    elif name == "first":
        m[:, 0, 0] = 1
    elif name == "last":
        m[:, H - 1, W - 1] = 1
    elif name != "empty":
        raise ValueError(name)
    return m


def probe(c, masks):
    flat = c["pred"].reshape(-1).astype(np.float64)[::7]
    return np.array([c["pred"].sum(dtype=np.float64), c["gt"].sum(dtype=np.float64), float(flat @ np.arange(flat.size))] +
                    [float(m.sum(dtype=np.float64)) for m in masks])


# ---- the three arms -----------------------------------------------------------------------------------------------------

def dist_maps(img0, img1, trunk, heads, dtype=torch.float64, conv=LR.conv_torch):
    """img0, img1 [B,3,H,W] in [0, 1] -> five maps d_l [B,1,h_l,w_l]: the head-weighted squared difference of the
    channel-normalised taps."""
    a, b = (2 * torch.as_tensor(x, dtype=torch.float32).to(dtype) - 1 for x in (img0, img1))
    t0, t1 = LR.trunk_taps(a, trunk, dtype, conv), LR.trunk_taps(b, trunk, dtype, conv)
    ds = []
    for l in range(5):
        n0 = t0[l] / (torch.sqrt(torch.sum(t0[l] ** 2, dim=1, keepdim=True)) + 1e-10)
        n1 = t1[l] / (torch.sqrt(torch.sum(t1[l] ** 2, dim=1, keepdim=True)) + 1e-10)
        ds.append(F.conv2d((n0 - n1) ** 2, heads[f"lin{l}.model.1.weight"].to(dtype)))
    return ds


def spatial_map(ds, H, W):
    """[B,1,H,W]: val = res[0]; val += res[l] over the upsampled maps."""
    val = None
    for d in ds:
        up = F.interpolate(d, size=(H, W), mode="bilinear", align_corners=False)
        val = up if val is None else val + up
    return val


def reference_upsample(d, H, W):
    """networks_basic.py:24-28 as written: scale_factor = 1. * H / h.  Its output is not always H x W."""
    sh, sw = 1. * H / d.shape[2], 1. * W / d.shape[3]
    return torch.nn.Upsample(scale_factor=(sh, sw), mode="bilinear", align_corners=False)(d)


def quirk(n_out, n_in):
    """True where torch sizes the reference's upsample of n_in to something else than n_out: floor(n_in (n_out / n_in))."""
    return int(np.floor(n_in * (1. * n_out / n_in))) != n_out


def tap_edges(n):
    """The three distinct tap edges of an image edge n (>= 31)."""
    a = (n - 7) // 4 + 1
    b = (a - 3) // 2 + 1
    return a, b, (b - 3) // 2 + 1


def dycheck_mean(val, m):
    """dycheck's masked_mean per pair: val [B,1,H,W], m [B,H,W] -> [B]."""
    m = m.to(val.dtype)
    return (val[:, 0] * m).sum((1, 2)) / m.sum((1, 2)).clamp(min=1e-6)


def nearest_index(n_out, n_in):
    """Source index of every output index of a nearest-neighbour resize n_in -> n_out, as the kernel forms it in fp32."""
    s = np.float32(n_in) / np.float32(n_out)
    i = np.floor(np.arange(n_out, dtype=np.float32) * s).astype(np.int64)
    return np.minimum(i, n_in - 1)


def masked_layers(ds, m):
    """-> (values [B,5], numerators [B,5], denominators [B,5]) in ds' dtype: spatial_average with a mask, per pair."""
    num, den = [], []
    for d in ds:
        ml = F.interpolate(m.to(d.dtype)[:, None], size=d.shape[2:])
        num.append((d * ml).sum((1, 2, 3)))
        den.append(ml.sum((1, 2, 3)))
    num, den = torch.stack(num, 1), torch.stack(den, 1)
    return num / (den + 1e-8), num, den


def values(ds, val, m):
    """[B, len(VALUES)] in ds' dtype."""
    layers, _, _ = masked_layers(ds, m)
    total = layers[:, 0]
    for l in range(1, 5):
        total = total + layers[:, l]
    return torch.cat([torch.stack([val.mean((1, 2, 3)), dycheck_mean(val, m), total], 1), layers], 1)


def evaluate(c, masks, trunk, heads, dtype, conv=LR.conv_torch):
    """-> (map [B,1,H,W], [len(masks), B, len(VALUES)]): the ground truth goes first, as metrics.py:130 passes it."""
    with torch.no_grad():
        ds = dist_maps(c["gt"], c["pred"], trunk, heads, dtype, conv)
        val = spatial_map(ds, *c["gt"].shape[2:])
        return val, torch.stack([values(ds, val, torch.from_numpy(m)) for m in masks])


def compute_lpips(c, m, trunk, heads, dtype, conv=LR.conv_torch):
    """dycheck's compute_lpips per pair: both images times the mask, the map, its masked mean -> [B]."""
    with torch.no_grad():
        mm = torch.from_numpy(m)[:, None]
        gt, pred = torch.from_numpy(c["gt"]) * mm, torch.from_numpy(c["pred"]) * mm            # (fp32, as numpy forms it)
        ds = dist_maps(gt, pred, trunk, heads, dtype, conv)
        return dycheck_mean(spatial_map(ds, *gt.shape[2:]), torch.from_numpy(m))


# ---- the fixture --------------------------------------------------------------------------------------------------------

def rows(fx, i, key="f64"):
    """[len(MASKS), B, len(VALUES)] of case i."""
    B = CASES[i][2]
    return fx[key][int(fx["first"][i]):int(fx["first"][i + 1])].reshape(len(MASKS), B, len(VALUES))


def reference_gaps(fx):
    """Per quantity the LARGEST distance of the fixture's two fp32 runs from its float64 values, over all cases, masks and
    pairs (entries whose float64 value is exactly 0 have no relative distance: the tests assert exact zeros there)."""
    out = {"map": float(max(fx["map_gap_f32"].max(), fx["map_gap_seq"].max()))}
    t = fx["f64"]
    for j, name in enumerate(VALUES):
        nz = t[:, j] != 0
        out[name] = float(max((np.abs(fx[k][nz, j] - t[nz, j]) / np.abs(t[nz, j])).max() for k in ("f32", "seq")))
    t = fx["cl_f64"]
    out["compute_lpips"] = float(max((np.abs(fx[k] - t) / np.abs(t)).max() for k in ("cl_f32", "cl_seq")))
    return out


def tolerance(name, ref_gaps):
    return allowed(ref_gaps[name], FLOOR)


def build_fixture():
    trunk, heads = LR.seeded_trunk(), LR.reference_heads()
    runs = (("f64", torch.float64, LR.conv_torch), ("f32", torch.float32, LR.conv_torch),
            ("seq", torch.float32, LR.conv_sequential))
    fx = {k: [] for k, _, _ in runs}
    fx.update({"cl_" + k: [] for k, _, _ in runs})
    first, probes, g32, gseq = [0], [], [], []
    for i in range(len(CASES)):
        c = make_case(i)
        masks = [make_mask(i, n) for n in MASKS]
        maps = {}
        for k, dtype, conv in runs:
            maps[k], v = evaluate(c, masks, trunk, heads, dtype, conv)
            fx[k].append(v.double().numpy().reshape(-1, len(VALUES)))
            if i in CL_CASES:
                fx["cl_" + k].append(np.stack([compute_lpips(c, make_mask(i, n), trunk, heads, dtype, conv).double().numpy()[0]
                                               for n in CL_MASKS]))
        g32.append(map_gap(maps["f32"], maps["f64"]))
        gseq.append(map_gap(maps["seq"], maps["f64"]))
        first.append(first[-1] + fx["f64"][-1].shape[0])
        probes.append(probe(c, masks))
        print(case_name(i), fx["f64"][-1][:CASES[i][2], :3].tolist(), g32[-1], gseq[-1], flush=True)
    out = {k: np.concatenate(v) if not k.startswith("cl_") else np.stack(v) for k, v in fx.items()}
    out.update(first=np.array(first), probe=np.stack(probes), map_gap_f32=np.array(g32), map_gap_seq=np.array(gseq))
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(GOLDEN, "lpips_spatial.npz"), **build_fixture())
