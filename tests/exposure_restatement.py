"""The exposure-time estimate (include/mobgs_hip.h K20) restated in torch on the CPU, for the tests to compare against.

    estimate(cam_flow, latent_flow, q, scale, dtype)   the semantics as the header states them, sort-based
    reference_chain(cam_flow, latent_flow, q, edge)    the statements of /root/reference/train.py:482-491 themselves:
                                                       torch.norm, torch.quantile, the boolean mask, torch.median

estimate(dtype=torch.float32) evaluates every operation as written in fp32 (magnitude sqrt(x x + y y), position
q * float32(n - 1), the two-branch interpolation of ATen's lerp, lower median) -- tests/test_exposure_cpu.py holds it
bit-equal to torch.quantile / torch.median on the same magnitudes.  dtype=torch.float64 is the same in double
precision (the noise floor of the fp32 chain is measured against it).  Both carry the library's one deliberate difference
from the reference: with no valid pixel or a non-finite magnitude nothing is updated (value None) where the reference
would store NaN."""
from __future__ import annotations

import math

import torch


def magnitudes(flow: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """[n,2] (or [...,2]) -> sqrt(x x + y y) per row, flattened; every operation rounded once to `dtype`.
    The fp32 root is taken in float64 and rounded (exact: 53 >= 2 x 24 + 2 bits): torch.sqrt on an fp32 CPU tensor goes
    through a vector library whose root is off by one ulp for about 0.7 % of arguments, the kernel's is correctly
    rounded."""
    f = flow.reshape(-1, 2).to(dtype)
    x, y = f[:, 0], f[:, 1]
    s = x * x + y * y
    return torch.sqrt(s.double()).to(dtype) if dtype == torch.float32 else torch.sqrt(s)


def quantile_sorted(mag: torch.Tensor, q: float) -> torch.Tensor:
    """torch.quantile(mag, q) (linear) by a sort: the position is formed in mag's dtype."""
    n = mag.numel()
    s = torch.sort(mag).values
    pos = torch.tensor(q, dtype=mag.dtype) * torch.tensor(n - 1, dtype=mag.dtype)
    lo, hi = torch.floor(pos), torch.ceil(pos)
    w = pos - lo
    a, b = s[int(lo)], s[int(hi)]
    return a + w * (b - a) if float(w) < 0.5 else b - (b - a) * (1 - w)


def estimate(cam_flow, latent_flow, q=0.01, scale=1.0, dtype=torch.float32):
    """-> {"threshold", "n_valid", "n_nonfinite", "updated", "value"}; value is None when nothing would be stored."""
    cam, lat = magnitudes(cam_flow, dtype), magnitudes(latent_flow, dtype)
    n_nonfinite = int((~torch.isfinite(cam)).sum() + (~torch.isfinite(lat)).sum())
    thr = quantile_sorted(cam, q)
    valid = cam > thr
    n_valid = int(valid.sum())
    out = {"threshold": thr, "n_valid": n_valid, "n_nonfinite": n_nonfinite, "updated": 0, "value": None}
    if n_valid == 0 or n_nonfinite:
        return out
    ratio = torch.sort(lat[valid] / cam[valid]).values
    out["value"] = ratio[(n_valid - 1) // 2] * torch.tensor(scale, dtype=dtype)
    out["updated"] = 1
    return out


def torch_judge(cam_flow, latent_flow, q=0.01, scale=1.0):
    """torch.quantile / torch.median themselves on the fp32 magnitudes as written -> (threshold, n_valid, value)."""
    cam, lat = magnitudes(cam_flow), magnitudes(latent_flow)
    thr = torch.quantile(cam, q)
    valid = cam > thr
    n_valid = int(valid.sum())
    value = torch.median(lat[valid] / cam[valid]) * scale if n_valid else None
    return thr, n_valid, value


def reference_chain(rendered_cam_flow, rendered_latent_flow, q=0.01, edge=False):
    """train.py:482-491 on two rendered flow images [1,H,W,2] -> new_exposure_time (0-d tensor of their dtype)."""
    cam_flow_mag = torch.norm(rendered_cam_flow, dim=-1)
    latent_flow_mag = torch.norm(rendered_latent_flow, dim=-1)
    valid_id = cam_flow_mag > torch.quantile(cam_flow_mag, q)
    cam_flow_mag = cam_flow_mag[valid_id]
    latent_flow_mag = latent_flow_mag[valid_id]
    new_exposure_time = torch.median(latent_flow_mag / cam_flow_mag)
    if edge:
        new_exposure_time = new_exposure_time * 0.5
    return new_exposure_time


def ulp(value: float) -> float:
    """Spacing of fp32 numbers at |value|."""
    v = abs(float(value))
    if v == 0.0:
        return 2.0 ** -149
    return 2.0 ** (max(math.floor(math.log2(v)), -126) - 23)


def fixture_bound(ref_gap: float, value: float) -> float:
    """Allowed |kernel - float64 result| on the fixture: 3 x the reference's own fp32 noise, but at least
    4 ulp of the result -- two magnitudes at 1 ulp each (torch.norm against sqrt(x x + y y)), the division, the
    interpolation."""
    return max(3.0 * float(ref_gap), 4.0 * ulp(value))


def exact_case(n: int, seed: int = 0, ties: bool = True, tail=None):
    """Inputs whose arithmetic is exact in fp32: camera flow (3k, 4k) with small integer k (magnitude 5k), latent flow =
    camera flow * j / 64 (magnitude 5 k j / 64, ratio j / 64).  25 (k j)^2 < 2^24, so every square, sum, root and
    quotient is representable.  ties: k in 1..8 with about one pixel in 40 at k = 1 (heavy ties, a populated 1 % tail),
    j in 1..100; otherwise k in 1..25, j in 1..32.  tail = t (with ties): exactly t pixels at k = 1 instead, so that the
    order statistics of rank t - 1 and t differ (5 and 10).  The order is shuffled.  -> (cam_flow [n,2], latent_flow [n,2])."""
    g = torch.Generator().manual_seed(1000 * seed + n)
    if ties:
        k = torch.randint(2, 9, (n,), generator=g)
        if tail is None:
            k[torch.rand(n, generator=g) < 0.025] = 1
        else:
            k[:tail] = 1
        j = torch.randint(1, 101, (n,), generator=g)
    else:
        k = torch.randint(1, 26, (n,), generator=g)
        j = torch.randint(1, 33, (n,), generator=g)
    perm = torch.randperm(n, generator=g)
    k, j = k[perm].float(), j[perm].float()
    cam = torch.stack([3 * k, 4 * k], 1)
    lat = cam * (j / 64)[:, None]
    return cam.contiguous(), lat.contiguous()
