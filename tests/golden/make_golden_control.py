"""Generate tests/golden/controlgaussians_trace.json by running the reference's OWN helper_train.controlgaussians
(densify = 2) and helper_train.removeminmax on the CPU, through ref_harness.py (which plants an empty cv2 module, the one
import of helper_train.py that is absent here).

    python tests/golden/make_golden_control.py

The schedule: controlgaussians is called for iterations 1 .. N with a recording stand-in for `gaussians`, for the static
and the dynamic set and the option sets of OPTION_SETS (desicnt reached early, late and never; an interval that does not
divide densify_from_iter; densify_until_iter inside the range; a range that crosses 3000 and 6000).  Per run the fixture
holds the calls the stand-in received -- iteration, method name, arguments as floats (None stays null) -- and `flag` after
every iteration.  Only iterations with a call are listed; flag changes only there.

The bounds: removeminmax on a planted _xyz with rows exactly on each bound, one ulp outside each bound and one NaN row;
the fixture holds the table, the bounds and the mask the reference passed to prune_points.

Data only, no reference source."""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_harness as RH  # noqa: E402

# name -> (options, last iteration)
DEFAULTS = dict(densify_until_iter=15000, densify_from_iter=500, densification_interval=100, opacity_reset_interval=3000,
                desicnt=6, opthr=0.005, densify_grad_threshold=0.0001)
OPTION_SETS = {
    "reference defaults, desicnt reached early": (dict(DEFAULTS), 6500),
    "desicnt reached late, interval 70 does not divide 500": (dict(DEFAULTS, desicnt=40, densification_interval=70,
                                                                   densify_grad_threshold=0.0002), 6500),
    "desicnt never reached": (dict(DEFAULTS, desicnt=10 ** 6, densification_interval=250), 6500),
    "densify_until_iter inside the range": (dict(DEFAULTS, densify_until_iter=3000, desicnt=3, opthr=0.01,
                                                 opacity_reset_interval=1000), 6500),
    "desicnt 0: prunes only": (dict(DEFAULTS, desicnt=0, densify_from_iter=0, densification_interval=1500), 6500),
}
EXTENT = 4.25


class Recorder:
    """What controlgaussians may touch of a GaussianModel: every method call is recorded with its arguments."""

    def __init__(self):
        self.calls = []
        self.iteration = 0
        self.get_opacity = torch.tensor([[0.001], [0.004], [0.005], [0.006], [0.02], [0.5]])

    @staticmethod
    def _plain(v):
        if v is None or isinstance(v, (bool, int)):
            return v
        if torch.is_tensor(v):
            return [bool(x) for x in v.reshape(-1).tolist()] if v.dtype == torch.bool else v.reshape(-1).tolist()
        return float(v)

    def __getattr__(self, name):
        def method(*args, **kw):
            self.calls.append({"iteration": self.iteration, "name": name, "args": [self._plain(a) for a in args],
                               "kwargs": {k: self._plain(v) for k, v in kw.items()}})
        return method


def run_schedule(control, options, last, is_dynamic):
    opt = types.SimpleNamespace(**options)
    scene = types.SimpleNamespace(cameras_extent=EXTENT)
    rec, flag, flags = Recorder(), 0, []
    for iteration in range(1, last + 1):
        rec.iteration = iteration
        before = len(rec.calls)
        flag = control(opt, rec, 2, iteration, scene, None, None, None, flag, is_dynamic=is_dynamic)
        if len(rec.calls) != before:
            flags.append([iteration, flag])
    return {"calls": rec.calls, "flags": flags, "final_flag": flag}


def planted_xyz():
    """-> (xyz [n,3] fp32, maxbounds, minbounds): inside rows, rows exactly on each of the six bounds, rows one ulp
    outside each, one NaN row."""
    f32 = np.float32
    hi, lo = np.array([1.5, 2.25, 3.0], f32), np.array([-1.25, -0.5, 0.75], f32)
    mid = (hi + lo) / f32(2)
    rows = [mid.copy(), (mid + f32(0.1)).astype(f32)]
    for k in range(3):
        for bound, away in ((hi, f32(np.inf)), (lo, f32(-np.inf))):
            on, out = mid.copy(), mid.copy()
            on[k] = bound[k]
            out[k] = np.nextafter(bound[k], away)
            rows += [on, out]
    rows.append(np.array([np.nan, mid[1], mid[2]], f32))
    rows.append(np.array([mid[0], np.nan, np.nan], f32))
    rows.append(np.array([hi[0] + f32(5), lo[1] - f32(5), mid[2]], f32))
    return np.stack(rows).astype(f32), hi, lo


def run_bounds(ht):
    xyz, hi, lo = planted_xyz()
    seen = {}
    model = types.SimpleNamespace(_xyz=torch.from_numpy(xyz), prune_points=lambda mask: seen.update(mask=mask))
    real_empty_cache = torch.cuda.empty_cache
    torch.cuda.empty_cache = lambda: None
    try:
        ht.removeminmax(model, [torch.tensor(v) for v in hi], [torch.tensor(v) for v in lo])
    finally:
        torch.cuda.empty_cache = real_empty_cache
    nan = lambda a: [None if np.isnan(v) else float(v) for v in a]  # noqa: E731  (JSON has no NaN)
    return {"xyz": [nan(r) for r in xyz], "maxbounds": [float(v) for v in hi], "minbounds": [float(v) for v in lo],
            "mask": [bool(v) for v in seen["mask"].tolist()]}


def main():
    ht = RH.ref_import("helper_train")
    real_empty_cache = torch.cuda.empty_cache
    torch.cuda.empty_cache = lambda: None
    try:
        runs = []
        for name, (options, last) in OPTION_SETS.items():
            for is_dynamic in (False, True):
                runs.append({"name": name, "options": options, "last_iteration": last, "is_dynamic": is_dynamic,
                             "extent": EXTENT, **run_schedule(ht.controlgaussians, options, last, is_dynamic)})
    finally:
        torch.cuda.empty_cache = real_empty_cache
    out = {"opacity": Recorder().get_opacity.reshape(-1).tolist(), "runs": runs, "bounds": run_bounds(ht)}
    path = os.path.join(HERE, "controlgaussians_trace.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(path, os.path.getsize(path), "bytes;", sum(len(r["calls"]) for r in runs), "calls")


if __name__ == "__main__":
    main()
