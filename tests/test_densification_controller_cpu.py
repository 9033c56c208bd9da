"""mobgs_amd.helper_train.DensificationController on the CPU, over restated tables (tests/densify_restatement.py) and
against the restated schedule (tests/control_cases.schedule): a scripted range of iterations that crosses
densify_from_iter, desicnt and iteration 3000.  The controller's log, flags and tables equal what the restated calls give,
and a controller rebuilt from state_dict() continues identically."""
import copy
import types

import torch

import control_cases as C
import densify_restatement as R
from mobgs_amd.helper_train import DensificationController, scheduled_operations

OPTIONS = dict(densify_until_iter=3400, densify_from_iter=400, densification_interval=500, opacity_reset_interval=3000,
               desicnt=2, opthr=0.3, densify_grad_threshold=2.0e-4, percent_dense=0.01)
EXTENT = 5.0
LAST = 3600
NAMES = {"densify_pruneclone": "pruneclone", "prune_points": "prune_opacity", "reset_opacity": "reset_opacity"}


def _table(n, seed):
    g = torch.Generator().manual_seed(seed)
    size = OPTIONS["percent_dense"] * EXTENT
    top = torch.log(torch.tensor(size)) + torch.where(torch.rand(n, generator=g) < 0.4, 0.3, -0.3) * (1 + torch.rand(n, generator=g))
    scaling = top[:, None] - 2.0 * torch.rand(n, 3, generator=g)
    scaling[torch.arange(n), torch.randint(0, 3, (n,), generator=g)] = top
    z = lambda *s: torch.zeros(n, *s)  # noqa: E731
    return {"xyz": torch.randn(n, 3, generator=g), "scaling": scaling, "rotation": torch.randn(n, 4, generator=g),
            "opacity": torch.randn(n, 1, generator=g), "opacity.exp_avg": torch.rand(n, 1, generator=g),
            "opacity.exp_avg_sq": torch.rand(n, 1, generator=g), "xyz_gradient_accum": z(1), "denom": z(1),
            "max_radii2D": z(), "_deformation_accum": z(3)}


def _feed(state, g):
    """Statistics before a scheduled iteration: a quarter of the rows hot, opacities moved and clear of the prune decision."""
    n = state["xyz"].shape[0]
    out = dict(state)
    out["denom"] = torch.randint(0, 4, (n, 1), generator=g).float()
    out["xyz_gradient_accum"] = torch.where(torch.rand(n, 1, generator=g) < 0.25, 2.0, 0.25) * 2.0e-4 * out["denom"]
    op = state["opacity"] + torch.randn(n, 1, generator=g)     # (as training moves them: every prune finds rows)
    op[(torch.sigmoid(op.double()) - OPTIONS["opthr"]).abs() <= 1e-3 * OPTIONS["opthr"]] += 0.01
    out["opacity"] = op
    return out


def _samples(state, thr, g):
    _, split = R.select(state["scaling"], R.mean_grads(state["xyz_gradient_accum"], state["denom"]), thr,
                        OPTIONS["percent_dense"] * EXTENT)
    parents = torch.nonzero(split).reshape(-1).repeat(2)
    return torch.randn(parents.shape[0], 3, generator=g) * torch.exp(state["scaling"][parents])


class RestatedSet:
    """What controlgaussians calls on a set, on a restated table."""

    def __init__(self, state, seed):
        self.state, self.g = state, torch.Generator().manual_seed(seed)

    @property
    def get_xyz(self):
        return self.state["xyz"]

    @property
    def _xyz(self):
        return self.state["xyz"]

    def pruneclone_planned(self, max_grad, extent, splitN=2, samples=None):
        assert samples is None and splitN == 2 and extent == EXTENT
        self.state = R.densify_pruneclone(self.state, max_grad, extent, 2, _samples(self.state, max_grad, self.g),
                                          percent_dense=OPTIONS["percent_dense"])

    def prune_opacity_below(self, min_opacity):
        self.state = R.prune_points(self.state, ~C.keep_opacity(self.state["opacity"], min_opacity))

    def reset_opacity(self):
        self.state = R.reset_opacity(self.state)


def _expected(is_dynamic, table, seed, feed_seed):
    """The restated schedule applied call by call -> (log records without the set name, flag per iteration, table)."""
    want = C.schedule(OPTIONS, LAST, is_dynamic, EXTENT)
    g, fg = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(feed_seed)
    flags_after, log, flag = dict(map(tuple, want["flags"])), [], 0
    by_it = {}
    for c in want["calls"]:
        by_it.setdefault(c["iteration"], []).append(c)
    for it in sorted(by_it):
        table = _feed(table, fg)
        for c in by_it[it]:
            before = table["xyz"].shape[0]
            samples = _samples(table, c["args"][0], g) if c["name"] == "densify_pruneclone" else None
            table = C.apply_call(table, c, EXTENT, OPTIONS["percent_dense"], OPTIONS["opthr"], samples)
            log.append([it, NAMES[c["name"]], before, table["xyz"].shape[0], flag])
        flag = flags_after[it]
    return log, want, table


def _run(ctl, stat, dyn, first, last, feeds):
    changed = []
    for it in range(first, last + 1):
        if ctl.due(it):
            dyn.state = _feed(dyn.state, feeds[0])
            stat.state = _feed(stat.state, feeds[1])
        if ctl.step(it, stat, dyn):
            changed.append(it)
    return changed


def _same(a, b):
    return set(a) == set(b) and all(a[k].shape == b[k].shape and torch.equal(a[k], b[k]) for k in a)


def test_the_controller_follows_the_restated_schedule_and_its_state_round_trips():
    opt = types.SimpleNamespace(**OPTIONS)
    stat, dyn = RestatedSet(_table(300, 1), 11), RestatedSet(_table(200, 2), 12)
    ctl = DensificationController(opt, EXTENT, stat, dyn)
    assert [float(x) for x in ctl.maxbounds_s] == [float(stat.state["xyz"][:, k].max()) for k in range(3)]
    assert [float(x) for x in ctl.minbounds_d] == [float(dyn.state["xyz"][:, k].min()) for k in range(3)]
    feeds = [torch.Generator().manual_seed(21), torch.Generator().manual_seed(22)]
    changed = _run(ctl, stat, dyn, 1, 1200, feeds)
    # a copy at iteration 1200, rebuilt from plain numbers and lists
    import json
    saved = json.loads(json.dumps(ctl.state_dict()))
    stat2, dyn2 = copy.deepcopy(stat), copy.deepcopy(dyn)
    feeds2 = copy.deepcopy(feeds)
    ctl2 = DensificationController(opt, 0.0).load_state_dict(saved)
    assert ctl2.scene.cameras_extent == EXTENT and (ctl2.flag_d, ctl2.flag_s) == (ctl.flag_d, ctl.flag_s) == (0, 2)
    assert [float(x) for x in ctl2.maxbounds_d] == [float(x) for x in ctl.maxbounds_d]
    changed += _run(ctl, stat, dyn, 1201, LAST, feeds)
    changed2 = _run(ctl2, stat2, dyn2, 1201, LAST, feeds2)

    for name, pc, is_dynamic, seed, feed_seed in (("dyn", dyn, True, 12, 21), ("stat", stat, False, 11, 22)):
        want_log, want, table = _expected(is_dynamic, _table(200, 2) if is_dynamic else _table(300, 1), seed, feed_seed)
        got = [[r[0], r[2], r[3], r[4], r[5]] for r in ctl.log if r[1] == name]
        assert got == want_log, (name, got, want_log)
        assert (ctl.flag_d if is_dynamic else ctl.flag_s) == want["final_flag"]
        assert _same(pc.state, table), name
    # the range crossed densify_from_iter, desicnt and 3000, and stopped at densify_until_iter
    ops = {(r[1], r[2]) for r in ctl.log}
    assert ops == {("dyn", "pruneclone"), ("dyn", "reset_opacity"), ("stat", "pruneclone"), ("stat", "prune_opacity"),
                   ("stat", "reset_opacity")}
    assert changed == [500, 1000, 1500, 2000, 2500, 3000] and (ctl.flag_d, ctl.flag_s) == (0, 2)
    assert [r[0] for r in ctl.log if r[2] == "reset_opacity"] == [3000, 3000]
    assert all(r[3] < r[4] for r in ctl.log if r[2] == "pruneclone") and all(r[3] > r[4] for r in ctl.log if r[2] == "prune_opacity")
    # in the reference's order: the dynamic set first
    at_500 = [r[1] for r in ctl.log if r[0] == 500]
    assert at_500 == ["dyn", "stat"]
    # the round trip continued identically
    assert ctl2.log == ctl.log and changed2 == [it for it in changed if it > 1200]
    assert _same(stat2.state, stat.state) and _same(dyn2.state, dyn.state)


def test_scheduled_operations_is_the_schedule_of_controlgaussians():
    opt = types.SimpleNamespace(**OPTIONS)
    for is_dynamic in (False, True):
        want = C.schedule(OPTIONS, LAST, is_dynamic, EXTENT)
        flag, got = 0, []
        after = dict(map(tuple, want["flags"]))
        for it in range(1, LAST + 1):
            got += [(it, op) for op in scheduled_operations(opt, it, flag)]
            flag = after.get(it, flag)
        assert got == [(c["iteration"], NAMES[c["name"]]) for c in want["calls"]]
