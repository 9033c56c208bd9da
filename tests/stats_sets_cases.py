"""Case tables and inputs for mobgs_densify_stats_sets (csrc/densify_ctl.hip): the batch statistics of both sets in one
launch, from int32 radii or from the fp32-coded radii of a gradient message.  The restatement is control_cases.batch_stats,
once per set; nothing here shares code with the kernel.  tests/test_stats_sets_cases_cpu.py vets what is here,
tests/test_gpu_densify_stats_sets.py runs it on the GPU.

Two families of inputs per case:

  exact    every operation of the statistics is EXACT in fp32, so the kernel's chain of rounded fp32 operations and the
           restatement's float64 norm, rounded once, are the same numbers and torch.equal is the right comparison for
           xyz_gradient_accum too.  Gradients are integers times 2^-20 below 2^12, so every partial sum over the views is
           exact in any order; the sum over the views is planted as (a u, 2 b u) for a Pythagorean triple (a, b, c) --
           (0, 1, 1) and (1, 0, 1) among them -- and with sx = 64, sy = 32 (W = 128, H = 64) the scaled gradient is
           64 u (a, b): both squares, their sum and the root 64 u c are exact.  The accumulators start at integers times
           2^-14, the unit of 64 u, so the final addition is exact as well.
  random   normal gradients, as control_cases.stats_inputs draws them.  The sum over the views then depends on the order
           and the norm on every rounding: these inputs are compared bit for bit with the EXISTING kernel
           (mobgs_densify_stats_batch, one call per set), and with the restatement at the existing test's rtol 3e-7.

Planted rows, per set, as far as the set has rows: row 0 is visible only in the LAST view, with radius 16 777 215 (the
largest odd integer fp32 holds: 2^24 - 1); row 1 is visible in NO view (radii 0 and negative); row 2 has radius 1 in view 0
alone.  With one row per set, the first set gets the first plant and the second set the second."""
import torch

import control_cases as C

SETS_ROWS = [(257, 255), (0, 300), (300, 0), (1, 1), (1025, 63)]   # block edges at 255 / 256 / 257, a seam inside a workgroup
VIEWS = [1, 2, 16]
STRIDES = [2, 3]
ENCODINGS = ["INT32", "FP32"]
CASES = [(ns, nd, v, s, e) for (ns, nd) in SETS_ROWS for v in VIEWS for s in STRIDES for e in ENCODINGS]
PAD = 5                      # rows of every view's arrays past both sets: never read
WIDTH, HEIGHT = 128, 64      # sx = 64, sy = 32
BIG = 16777215
TRIPLES = [(3, 4, 5), (4, 3, 5), (5, 12, 13), (8, 15, 17), (0, 1, 1), (1, 0, 1), (0, 0, 0), (12, 5, 13)]
UNIT = 2.0 ** -20


def _plant(radii, row, kind):
    last = len(radii) - 1
    for v, r in enumerate(radii):
        if kind == 0:
            r[row] = BIG if v == last else -(v % 2)
        elif kind == 1:
            r[row] = -(v % 3 == 1)          # 0 and -1
        else:
            r[row] = 1 if v == 0 else 0


def _radii(ns, nd, n_views, g):
    total = ns + nd + PAD
    p_seen = 1.0 - 0.5 ** (1.0 / n_views)   # a row is visible in some view with probability 1/2
    radii = []
    for _ in range(n_views):
        r = torch.randint(1, 40, (total,), generator=g)
        r = torch.where(torch.rand(total, generator=g) < p_seen, r, torch.randint(-2, 1, (total,), generator=g))
        radii.append(r.to(torch.int32))
    planted = {}
    kind = 0
    for row0, n in ((0, ns), (ns, nd)):
        for j in range(min(n, 3)):
            k = (kind + j) % 3
            _plant(radii, row0 + j, k)
            planted.setdefault(k, []).append(row0 + j)
        kind += 1 if n == 1 else 0
    return radii, planted


def _state(n, g, exact):
    accum = torch.randint(0, 1000, (n, 1), generator=g).float() * 2.0 ** -14 if exact else 1e-3 * torch.rand(n, 1, generator=g)
    return {"xyz_gradient_accum": accum, "denom": torch.randint(0, 5, (n, 1), generator=g).float(),
            "max_radii2D": torch.randint(0, 30, (n,), generator=g).float()}


def inputs(ns, nd, n_views, grad_stride, family, seed):
    """-> (states [static, dynamic], grads per view [N_total, grad_stride] fp32, radii per view [N_total] int32, planted rows
    {kind: [rows]}) over N_total = ns + nd + PAD rows.  Columns past the second hold 1e30: nothing may read them."""
    g = torch.Generator().manual_seed(seed)
    total = ns + nd + PAD
    radii, planted = _radii(ns, nd, n_views, g)
    states = [_state(ns, g, family == "exact"), _state(nd, g, family == "exact")]
    if family == "random":
        grads = []
        for _ in range(n_views):
            vg = 3e-4 * torch.randn(total, grad_stride, generator=g)
            vg[torch.rand(total, generator=g) < 0.05] = 0.0
            grads.append(vg)
    else:
        assert family == "exact"
        tri = torch.tensor(TRIPLES)[torch.randint(0, len(TRIPLES), (total,), generator=g)]
        sign = 1 - 2 * torch.randint(0, 2, (total, 2), generator=g)
        m = torch.randint(1, 8, (total,), generator=g)
        target = torch.stack([tri[:, 0] * m, 2 * tri[:, 1] * m], 1) * sign          # integers, in units of 2^-20
        parts = [torch.randint(-64, 65, (total, 2), generator=g) for _ in range(n_views - 1)]
        parts.append(target - sum(parts) if parts else target)
        grads = [torch.zeros(total, grad_stride) for _ in range(n_views)]
        for vg, part in zip(grads, parts):
            vg[:, :2] = part.float() * UNIT
    for vg in grads:
        vg[:, 2:] = 1e30
    return states, grads, radii, planted


def coded(radii):
    """The radii as a gradient message carries them: fp32-coded integers (exact below 2^24)."""
    return [r.to(torch.float32) for r in radii]


def slot(grad, radii_coded):
    """One view's statistics slot as SubframeShard.put_densification_stats fills it: [N, 2] gradient rows, then N radii."""
    assert grad.shape[1] == 2
    return torch.cat([grad.reshape(-1), radii_coded])


def expected(states, grads, radii, ns, nd):
    """control_cases.batch_stats once per set -> ([new static state, new dynamic state], [visible static, visible dynamic])."""
    out, vis = [], []
    for state, row0, n in ((states[0], 0, ns), (states[1], ns, nd)):
        new, _, _, visible = C.batch_stats(state, grads, radii, row0, n, WIDTH, HEIGHT)
        out.append(new)
        vis.append(visible)
    return out, vis


def fp32_chain(states, grads, radii, ns, nd):
    """The kernel's arithmetic written with torch's fp32 CPU operations, every one rounded: the sum in view order from 0,
    the two scales, x x, y y, their sum, the root, the accumulation.  What test_stats_sets_cases_cpu.py holds against the
    restatement to show on which family torch.equal is owed."""
    out = []
    for state, row0, n in ((states[0], 0, ns), (states[1], ns, nd)):
        rows = slice(row0, row0 + n)
        gx, gy = torch.zeros(n), torch.zeros(n)
        for g in grads:
            gx = gx + g[rows, 0]
            gy = gy + g[rows, 1]
        gx, gy = gx * (WIDTH * 0.5), gy * (HEIGHT * 0.5)
        norm = torch.sqrt(gx * gx + gy * gy)
        r = torch.stack([x[rows] for x in radii]).max(dim=0).values
        vis = r > 0
        new = {k: v.clone() for k, v in state.items()}
        new["xyz_gradient_accum"][vis] = (state["xyz_gradient_accum"][:, 0] + norm)[vis][:, None]
        new["denom"][vis] += 1.0
        new["max_radii2D"][vis] = torch.maximum(state["max_radii2D"], r.float())[vis]
        out.append(new)
    return out
