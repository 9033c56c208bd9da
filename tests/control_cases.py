"""Restatements and case tables for the densification controller (mobgs_amd/helper_train.py, csrc/densify_ctl.hip), on
the CPU, sharing no code with either.  tests/test_control_cases_cpu.py ties the schedule and the bounds mask to what the
reference's own controlgaussians / removeminmax did (tests/golden/controlgaussians_trace.json) and vets the inputs of
every GPU case; tests/test_gpu_densify_control.py compares the HIP path with what is here.

batch_stats restates /root/reference/train.py:634-648 and :813-817.  Those lines sit in the middle of the 600-line
scene_reconstruction() and cannot be run on their own, so they are written out again: the gradients of the views are
added in fp32 in view order onto zeros and scaled by W * 0.5, H * 0.5 in fp32, as the reference's `+=` and `*=` do; the
norm and the accumulation follow in float64, rounded once (densify_restatement.add_densification_stats)."""
import torch

import densify_restatement as R
import test_gpu_densify_kernels as K   # _select_inputs and its PLANTED rows, THR, SIZE_THR (functions only: nothing runs)

THR, SIZE_THR = K.THR, K.SIZE_THR


# ---- statistics of a batch ----------------------------------------------------------------------------------------------
def batch_stats(state, grads, radii, row0, n, width, height):
    """state: {"xyz_gradient_accum" [n,1], "denom" [n,1], "max_radii2D" [n]}; grads / radii: per view [N_total, >= 2] fp32 and
    [N_total] int32.  -> (new state, grad_sum [n,2] fp32, radii_max [n] int32, visible [n] bool)."""
    rows = slice(row0, row0 + n)
    total = torch.zeros(n, 2, dtype=torch.float32)
    for g in grads:
        total += g[rows, :2]
    total[:, 0] *= width * 0.5
    total[:, 1] *= height * 0.5
    stacked = torch.stack([r[rows] for r in radii])
    radii_max = stacked.max(dim=0).values
    visible = (stacked > 0).any(dim=0)
    return R.add_densification_stats(state, total, visible, radii_max), total, radii_max, visible


STATS_CASES = [(n, v, s, r0) for n in (1, 255, 256, 257, 1500) for v in (1, 2, 16) for s in (2, 3) for r0 in (0, 777)]


def stats_inputs(n, n_views, grad_stride, row0, seed):
    """-> (state, steps): three steps of per-view (grads, radii) over N_total = row0 + n + 5 rows, never re-seeded.  A
    radius is positive in a view with probability 0.5 / n_views ... 0.5, so that the union is neither empty nor full."""
    g = torch.Generator().manual_seed(seed)
    total = row0 + n + 5
    state = {"xyz_gradient_accum": 1e-3 * torch.rand(n, 1, generator=g),
             "denom": torch.randint(0, 5, (n, 1), generator=g).float(),
             "max_radii2D": torch.randint(0, 30, (n,), generator=g).float()}
    steps = []
    p_seen = 1.0 - 0.5 ** (1.0 / n_views)   # a row is visible in some view with probability 1/2
    for _ in range(3):
        grads, radii = [], []
        for _ in range(n_views):
            vg = 3e-4 * torch.randn(total, grad_stride, generator=g)
            vg[torch.rand(total, generator=g) < 0.05] = 0.0
            r = torch.randint(1, 40, (total,), generator=g)
            r = torch.where(torch.rand(total, generator=g) < p_seen, r, torch.randint(-2, 1, (total,), generator=g))
            grads.append(vg)
            radii.append(r.to(torch.int32))
        steps.append((grads, radii))
    return state, steps


# ---- plan lists ---------------------------------------------------------------------------------------------------------
def _nz(mask):
    return torch.nonzero(mask).reshape(-1)


def _listed(kept, clones, parents, n_split):
    index = torch.cat([kept, -(clones + 1), *([-(parents + 1)] * n_split)]).to(torch.int32)
    counts = torch.tensor([kept.shape[0], clones.shape[0], parents.shape[0], index.shape[0]], dtype=torch.int32)
    return index, counts


def plan_pruneclone(accum, denom, scaling, thr, size_thr, n_split):
    """[rows not split | -(clone + 1) | -(split + 1), the run n_split times], each ascending -> (index int32, counts [4])."""
    clone, split = R.select(scaling, R.mean_grads(accum, denom), thr, size_thr)
    return _listed(_nz(~split), _nz(clone), _nz(split), n_split)


def keep_opacity(opacity, min_opacity):
    """!(sigmoid(opacity) < min_opacity) with the sigmoid in float64 and the threshold the fp32 number the C ABI receives."""
    t = float(torch.tensor(min_opacity, dtype=torch.float32))
    return ~(torch.sigmoid(opacity.reshape(-1).double()) < t)


def opacity_margin(opacity, min_opacity):
    """min over rows of |sigmoid(opacity) - min_opacity| / min_opacity in float64: how far the inputs stay from the decision
    (beside densify_restatement.size_margin)."""
    t = float(torch.tensor(min_opacity, dtype=torch.float32))
    s = torch.sigmoid(opacity.reshape(-1).double())
    return float(((s - t).abs() / t)[~torch.isnan(s)].min())


def bounds_mask(xyz, maxbounds, minbounds):
    """removeminmax's mask: a coordinate strictly above its upper or strictly below its lower bound (false on NaN)."""
    hi = torch.as_tensor(maxbounds, dtype=torch.float32)
    lo = torch.as_tensor(minbounds, dtype=torch.float32)
    return ((xyz > hi) | (xyz < lo)).any(dim=1)


def plan_prune(drop):
    """Rows with drop == 0, ascending -> (index, counts = [kept, 0, 0, kept])."""
    none = torch.zeros(0, dtype=torch.long)
    return _listed(_nz(~drop), none, none, 1)


PLAN_NS = [0, 1, 1023, 1024, 1025, 2049, 3001]   # (the write pass reads the block counts in one strided loop: no pieces)
PLAN_SPLITS = [1, 2, 3]
MIN_OPACITY = 0.005
MAXB, MINB = (1.5, 2.25, 3.0), (-1.25, -0.5, 0.75)


def plan_inputs(n, seed):
    """Every op's inputs at n rows: the selection inputs of the existing select test (planted rows included), opacity
    logits on both sides of logit(MIN_OPACITY) and clear of it, positions of which about a third lie outside the box
    (rows 0 .. 12: on each bound, one ulp outside each, one NaN row), a byte mask."""
    g = torch.Generator().manual_seed(seed)
    accum, denom, scaling = K._select_inputs(n, 0, g)
    logit = float(torch.log(torch.tensor(MIN_OPACITY / (1 - MIN_OPACITY), dtype=torch.float64)))
    away = 0.05 + 4.0 * torch.rand(n, generator=g)
    opacity = (logit + torch.where(torch.rand(n, generator=g) < 0.4, -away, away)).float().reshape(n, 1)
    hi, lo = torch.tensor(MAXB), torch.tensor(MINB)
    xyz = lo + (hi - lo) * (1.4 * torch.rand(n, 3, generator=g) - 0.2) if n else torch.zeros(0, 3)
    planted = [(k, bound, away_) for k in range(3) for bound, away_ in ((hi, float("inf")), (lo, float("-inf")))]
    mid = (hi + lo) / 2
    for j, (k, bound, away_) in enumerate(planted):
        for row, value in ((2 * j, bound[k]), (2 * j + 1, torch.nextafter(bound[k], torch.tensor(away_)))):
            if row < n:
                xyz[row] = mid
                xyz[row, k] = value
    if n > 12:
        xyz[12] = torch.tensor([float("nan"), float(mid[1]), float(mid[2])])
    values = torch.tensor([1, 2, 255], dtype=torch.uint8)
    mask = torch.where(torch.rand(n, generator=g) < 0.3, values[torch.randint(0, 3, (n,), generator=g)],
                       torch.zeros(n, dtype=torch.uint8))
    return dict(accum=accum, denom=denom, scaling=scaling, opacity=opacity, xyz=xyz.float().contiguous(), mask=mask)


def plan_expected(op, inp, n_split):
    if op == "PRUNECLONE":
        return plan_pruneclone(inp["accum"], inp["denom"], inp["scaling"], THR, SIZE_THR, n_split)
    if op == "PRUNE_OPACITY":
        return plan_prune(~keep_opacity(inp["opacity"], MIN_OPACITY))
    if op == "PRUNE_BOUNDS":
        return plan_prune(bounds_mask(inp["xyz"], MAXB, MINB))
    return plan_prune(inp["mask"] != 0)


PLAN_OPS = ["PRUNECLONE", "PRUNE_OPACITY", "PRUNE_BOUNDS", "PRUNE_MASK"]


# ---- the schedule -------------------------------------------------------------------------------------------------------
def schedule(options, last, is_dynamic, extent, opacity=None):
    """helper_train.py:222-258 restated -> {"calls", "flags", "final_flag"} in the layout of the trace fixture (the
    reference's method names: densify_pruneclone(grad_thres, opthr, extent, size_threshold, splitN=2), prune_points(mask),
    reset_opacity()).  opacity: what get_opacity returns, for the prune mask."""
    o = options
    calls, flags, flag = [], [], 0
    for it in range(1, last + 1):
        mine = []
        if it < o["densify_until_iter"]:
            if it > o["densify_from_iter"] and it % o["densification_interval"] == 0:
                if flag < o["desicnt"]:
                    size_threshold = 20 if it > o["opacity_reset_interval"] else None
                    thr = o["densify_grad_threshold"] * 0.5 if is_dynamic else o["densify_grad_threshold"]
                    mine.append(("densify_pruneclone", [thr, o["opthr"], extent, size_threshold], {"splitN": 2}))
                    flag += 0 if is_dynamic else 1
                else:
                    mask = [] if opacity is None else [bool(v) for v in (torch.tensor(opacity) < o["opthr"]).tolist()]
                    mine.append(("prune_points", [mask], {}))
            if it % 3000 == 0:
                mine.append(("reset_opacity", [], {}))
        calls += [{"iteration": it, "name": nm, "args": a, "kwargs": kw} for nm, a, kw in mine]
        if mine:
            flags.append([it, flag])
    return {"calls": calls, "flags": flags, "final_flag": flag}


class Recorder:
    """Stand-in for a TrainableGaussians under mobgs_amd.helper_train.controlgaussians: records the planned methods under
    the names of the reference's calls, in the layout reduced() gives the fixture's calls (pruneclone_planned takes neither
    min_opacity nor the size threshold, both of which the reference's densify_pruneclone ignores)."""

    def __init__(self, opacity):
        self.calls, self.iteration = [], 0
        self.opacity = torch.tensor(opacity)

    def _add(self, name, args, kwargs):
        self.calls.append({"iteration": self.iteration, "name": name, "args": args, "kwargs": kwargs})

    def pruneclone_planned(self, max_grad, extent, splitN=2, samples=None):
        assert samples is None
        self._add("densify_pruneclone", [float(max_grad), float(extent)], {"splitN": splitN})

    def prune_opacity_below(self, min_opacity):
        self._add("prune_points", [[bool(v) for v in (self.opacity < min_opacity).tolist()]], {})

    def reset_opacity(self):
        self._add("reset_opacity", [], {})


def reduced(calls):
    """The fixture's calls without the two arguments of densify_pruneclone that nothing reads (min_opacity, size_threshold)."""
    return [dict(c, args=[c["args"][0], c["args"][2]]) if c["name"] == "densify_pruneclone" else c for c in calls]


# ---- the controller on a table --------------------------------------------------------------------------------------------
def apply_call(state, call, extent, percent_dense, opthr, samples=None, layout=None):
    """One call of the schedule on a restated table (densify_restatement): the prune mask is taken from the table's own
    opacities, the threshold and the extent from the call."""
    if call["name"] == "densify_pruneclone":
        return R.densify_pruneclone(state, call["args"][0], extent, call["kwargs"]["splitN"], samples,
                                    percent_dense=percent_dense, layout=layout)
    if call["name"] == "prune_points":
        return R.prune_points(state, ~keep_opacity(state["opacity"], opthr))
    assert call["name"] == "reset_opacity", call
    return R.reset_opacity(state)
