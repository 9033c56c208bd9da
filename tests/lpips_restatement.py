"""LPIPS (include/mobgs_hip.h K24) restated with torch on the CPU, for the tests to compare against: the net-lin model with
the AlexNet trunk, version 0.1, spatial average, no mask, as /root/reference/models/networks_basic.py:68-105,
models/pretrained_networks.py:57-95, models/__init__.py:42-44 and metrics.py:49-51 define it, in our own words, in either
dtype.

    lpips(img0, img1, trunk, heads, dtype=..., unit_range=..., clamp=..., quantize=..., conv=...) -> (values [B,6], taps)

dtype=torch.float32 stands for "the reference as it can be run here", dtype=torch.float64 is the truth the GPU tests measure
against: the fp32 inputs and weights widened exactly.  The clamp and the 8-bit truncation are fp32 operations in both (they
produce the fp32 inputs).  conv: `conv_torch` (F.conv2d) or `conv_sequential` -- unfold, then a strictly sequential sum
over (ci, ky, kx) with a rounded product and a rounded addition per term: the least favourable order a K-loop may use.

THE TRUNK of the tests is seeded (seeded_trunk): torchvision's file is not here.  Weights are normal x sqrt(2 / (Cin k k)),
generated in float64 from a PCG64 stream and rounded to fp32; biases are uniform in +-0.1.  The heads are the reference's own
(tests/golden/lpips_heads_v0.1.npz: the five vectors of models/weights/v0.1/alex.pth, 1152 floats).  With gt = rand and
pred = clamp(gt + 0.1 randn) this gives layer values of 1e-3 .. 3e-3 and totals around 1e-2.

Also here: the fixture's cases (CASES, make_case: seeded streams, nothing stored but a checksum probe) and the tolerance rule
of the GPU tests (regterms_restatement.allowed over the fixture's largest reference gap).

tests/golden/lpips.npz is written by `python tests/lpips_restatement.py` (about a minute on one core): per case the [B,6]
values (total, five layer values) in float64, in fp32 with F.conv2d and in fp32 with conv_sequential, the per-tap distance
of both fp32 runs from float64 (largest error over the map relative to the map's largest value) and the probe; no images."""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn.functional as F

from regterms_restatement import FLOOR, allowed, rel_gap  # noqa: F401  (the rule of DESIGN 3a)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CIN, COUT = (3, 64, 192, 384, 256), (64, 192, 384, 256, 256)
KS, STRIDE, PAD = (11, 5, 3, 3, 3), (4, 1, 1, 1, 1), (2, 2, 1, 1, 1)
TRUNK_INDEX = (0, 3, 6, 8, 10)
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
QUANTITIES = ("total", "layer1", "layer2", "layer3", "layer4", "layer5")
TAPS = ("tap1", "tap2", "tap3", "tap4", "tap5")
SIZES = ((31, 31, 1), (31, 48, 2), (35, 33, 1), (64, 97, 3), (130, 67, 2))          # (H, W, B)
EXTRAS = ("identical", "flat", "clamp", "quantize")
EXTRA_SIZE = (64, 97, 3)
NOISE = 0.1
CASES = tuple(s + ("noisy",) for s in SIZES) + tuple(EXTRA_SIZE + (e,) for e in EXTRAS)


def case_name(i):
    H, W, B, what = CASES[i]
    return f"{H}x{W}-B{B}-{what}"


def seeded_trunk(seed=0):
    """A state dict with torchvision's keys: features.{0,3,6,8,10}.{weight,bias}, fp32."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = {}
    for l, idx in enumerate(TRUNK_INDEX):
        fan = CIN[l] * KS[l] * KS[l]
        w = rng.standard_normal((COUT[l], CIN[l], KS[l], KS[l])) * np.sqrt(2.0 / fan)
        b = rng.uniform(-0.1, 0.1, COUT[l])
        sd[f"features.{idx}.weight"] = torch.from_numpy(w.astype(np.float32))
        sd[f"features.{idx}.bias"] = torch.from_numpy(b.astype(np.float32))
    return sd


def reference_heads():
    """A state dict with the reference's keys lin{0..4}.model.1.weight [1,C,1,1], from tests/golden/lpips_heads_v0.1.npz."""
    z = np.load(os.path.join(GOLDEN, "lpips_heads_v0.1.npz"))
    return {f"lin{l}.model.1.weight": torch.from_numpy(z[f"lin{l}"]).reshape(1, -1, 1, 1) for l in range(5)}


def quantize8(x):
    """eval.py:162 then metrics.py:99-100: the 8-bit image and back, in fp32."""
    x = torch.as_tensor(x, dtype=torch.float32)
    return (x.clamp(0, 1) * 255).to(torch.uint8).to(torch.float32) / 255


def conv_torch(x, w, b, stride, pad):
    return F.conv2d(x, w, b, stride=stride, padding=pad)


def conv_sequential(x, w, b, stride, pad):
    """The same convolution with one rounded product and one rounded addition per (ci, ky, kx), in that order, the bias
    last.  In x's dtype."""
    B, _, H, W = x.shape
    cout, _, k, _ = w.shape
    ho, wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    cols = F.unfold(x, k, padding=pad, stride=stride)            # [B, Cin k k, L], rows in (ci, ky, kx) order
    wk = w.reshape(cout, -1)
    acc = torch.zeros(B, cout, cols.shape[-1], dtype=x.dtype)
    for i in range(wk.shape[1]):
        acc = acc + wk[None, :, i, None] * cols[:, None, i, :]
    return (acc + b[None, :, None]).reshape(B, cout, ho, wo)


def prepare(img0, img1, clamp, quantize):
    """The fp32 operations in front of the model: clamp both, then truncate img1 (the prediction) to 8 bits."""
    a, b = torch.as_tensor(img0, dtype=torch.float32), torch.as_tensor(img1, dtype=torch.float32)
    if clamp:
        a, b = a.clamp(0, 1), b.clamp(0, 1)
    if quantize:
        b = quantize8(b)
    return a, b


def trunk_taps(x, trunk, dtype, conv=conv_torch):
    """x [N,3,H,W] in [-1, 1] -> the five ReLU maps [N,C,h,w]."""
    shift = torch.tensor(SHIFT, dtype=dtype).reshape(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=dtype).reshape(1, 3, 1, 1)
    h = (x.to(dtype) - shift) / scale
    taps = []
    for l, idx in enumerate(TRUNK_INDEX):
        if l in (1, 2):
            h = F.max_pool2d(h, 3, 2)
        w, b = trunk[f"features.{idx}.weight"].to(dtype), trunk[f"features.{idx}.bias"].to(dtype)
        h = torch.relu(conv(h, w, b, STRIDE[l], PAD[l]))
        taps.append(h)
    return taps


def lpips(img0, img1, trunk, heads, dtype=torch.float64, unit_range=True, clamp=False, quantize=False, conv=conv_torch):
    """-> (values [B,6] in dtype: the total and the five layer values; the taps of both images, 2 lists of 5 maps)."""
    a, b = prepare(img0, img1, clamp, quantize)
    a, b = a.to(dtype), b.to(dtype)
    if unit_range:
        a, b = 2 * a - 1, 2 * b - 1
    t0, t1 = trunk_taps(a, trunk, dtype, conv), trunk_taps(b, trunk, dtype, conv)
    layers = []
    for l in range(5):
        n0 = t0[l] / (torch.sqrt(torch.sum(t0[l] ** 2, dim=1, keepdim=True)) + 1e-10)
        n1 = t1[l] / (torch.sqrt(torch.sum(t1[l] ** 2, dim=1, keepdim=True)) + 1e-10)
        d = (n0 - n1) ** 2
        lin = heads[f"lin{l}.model.1.weight"].to(dtype)
        layers.append(F.conv2d(d, lin).mean([2, 3]).reshape(-1))
    total = layers[0]
    for l in range(1, 5):
        total = total + layers[l]
    return torch.stack([total] + layers, 1), (t0, t1)


# ---- the fixture's cases ------------------------------------------------------------------------------------------------

def make_case(i):
    """-> dict(gt, pred [B,3,H,W] fp32 arrays in [0, 1] unless the case says otherwise, clamp, quantize)."""
    H, W, B, what = CASES[i]
    rng = np.random.Generator(np.random.PCG64(2000 + i))
    gt = rng.random((B, 3, H, W)).astype(np.float32)
    noisy = gt + (NOISE * rng.standard_normal((B, 3, H, W))).astype(np.float32)
    pred = np.clip(noisy, 0, 1).astype(np.float32)
    c = dict(clamp=False, quantize=False)
    if what == "identical":
        pred = gt.copy()
    elif what == "flat":                       # two different constants: only the bias and the padded border speak
        gt = np.full_like(gt, 0.5)
        pred = np.full_like(gt, 0.25)
    elif what == "clamp":                      # values outside [0, 1] on both sides
        gt = (gt * 2 - 0.5).astype(np.float32)
        pred = (noisy * 2 - 0.5).astype(np.float32)
        c["clamp"] = True
    elif what == "quantize":
        gt = quantize8(gt).numpy()
        pred = (noisy * 1.2 - 0.1).astype(np.float32)
        c["quantize"] = True
    elif what != "noisy":
        raise ValueError(what)
    c.update(pred=pred, gt=gt)
    return c


def probe(c):
    """A checksum of a case's inputs: what the fixture stores instead of the images."""
    flat = c["pred"].reshape(-1).astype(np.float64)[::7]
    return np.array([c["pred"].sum(dtype=np.float64), c["gt"].sum(dtype=np.float64), float(flat @ np.arange(flat.size)),
                     float(c["clamp"]) + 2.0 * float(c["quantize"])])


def evaluate(c, trunk, heads, dtype, conv=conv_torch):
    """-> (values [B,6], taps of (gt, pred)): the ground truth goes first, as metrics.py:130 passes it."""
    with torch.no_grad():
        return lpips(c["gt"], c["pred"], trunk, heads, dtype=dtype, clamp=c["clamp"], quantize=c["quantize"], conv=conv)


def map_gap(got, truth):
    """Largest error over a map relative to the map's largest value."""
    got, truth = torch.as_tensor(got).double(), torch.as_tensor(truth).double()
    scale = float(truth.abs().max())
    return float((got - truth).abs().max()) / scale if scale > 0 else float((got - truth).abs().max())


def taps_gap(taps, truth):
    """[5]: per tap, map_gap over the maps of both images."""
    return np.array([max(map_gap(taps[s][l], truth[s][l]) for s in (0, 1)) for l in range(5)])


def reference_gaps(fx):
    """Per quantity and per tap, the LARGEST distance of the fixture's two fp32 runs (F.conv2d, conv_sequential) from its
    float64 values over all cases and images: where a case happens to land closer that is luck, not a bound."""
    out = {}
    for j, name in enumerate(QUANTITIES):
        out[name] = max(max(rel_gap(a, t), rel_gap(s, t))
                        for a, s, t in zip(fx["f32"][:, j], fx["seq"][:, j], fx["f64"][:, j]))
    for l, name in enumerate(TAPS):
        out[name] = float(max(fx["tap_gap_f32"][:, l].max(), fx["tap_gap_seq"][:, l].max()))
    return out


def tolerance(name, ref_gaps):
    return allowed(ref_gaps[name], FLOOR)


def build_fixture():
    trunk, heads = seeded_trunk(), reference_heads()
    f64, f32, seq, first, probes, g32, gseq = [], [], [], [0], [], [], []
    for i in range(len(CASES)):
        c = make_case(i)
        v64, t64 = evaluate(c, trunk, heads, torch.float64)
        v32, t32 = evaluate(c, trunk, heads, torch.float32)
        vsq, tsq = evaluate(c, trunk, heads, torch.float32, conv_sequential)
        f64.append(v64.numpy())
        f32.append(v32.double().numpy())
        seq.append(vsq.double().numpy())
        g32.append(taps_gap(t32, t64))
        gseq.append(taps_gap(tsq, t64))
        first.append(first[-1] + v64.shape[0])
        probes.append(probe(c))
        print(case_name(i), v64[:, 0].tolist(), g32[-1], gseq[-1])
    return dict(f64=np.concatenate(f64), f32=np.concatenate(f32), seq=np.concatenate(seq), first=np.array(first),
                probe=np.stack(probes), tap_gap_f32=np.stack(g32), tap_gap_seq=np.stack(gseq))


if __name__ == "__main__":
    np.savez_compressed(os.path.join(GOLDEN, "lpips.npz"), **build_fixture())
