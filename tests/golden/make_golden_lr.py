"""Generate tests/golden/lr_schedule.npz: the rates of the reference's OWN get_expon_lr_func (utils/general_utils.py),
imported in place, at a handful of iterations.

    MOBGS_REFERENCE=/path/to/the/reference python tests/golden/make_golden_lr.py

Settings: the xyz, grid and deformation schedules as scene/gaussian_model.py:646-661 builds them from the
OptimizationParams defaults (arguments/__init__.py:120-130; arguments/stereo/default.py overrides none of these) with
spatial_lr_scale = 5, one schedule with a delay (lr_delay_steps = 100, lr_delay_mult = 0.01) and one with both rates zero.
Data only, no reference source: per setting the five arguments and the float64 rates at ITERATIONS.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ITERATIONS = [-1, 0, 1, 2, 99, 100, 101, 4999, 9999, 10000, 10001, 30000]
SCALE = 5.0
# name -> (lr_init, lr_final, lr_delay_steps, lr_delay_mult, max_steps)
SETTINGS = {
    "xyz": (0.00016 * SCALE, 0.0000016 * SCALE, 0, 1.0, 20000),
    "grid": (0.0016 * SCALE, 0.00016 * SCALE, 0, 1.0, 20000),
    "deformation": (0.00016 * SCALE, 0.000016 * SCALE, 0, 1.0, 20000),
    "delayed": (0.00016, 0.0000016, 100, 0.01, 20000),
    "both_zero": (0.0, 0.0, 0, 1.0, 20000),
}


def reference_helper():
    root = os.environ.get("MOBGS_REFERENCE", "/root/reference")
    spec = importlib.util.spec_from_file_location("ref_general_utils", os.path.join(root, "utils", "general_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.get_expon_lr_func


def main():
    make = reference_helper()
    out = {"iterations": np.asarray(ITERATIONS, dtype=np.int64), "names": np.asarray(list(SETTINGS))}
    for name, (a, b, steps, mult, max_steps) in SETTINGS.items():
        fn = make(lr_init=a, lr_final=b, lr_delay_steps=steps, lr_delay_mult=mult, max_steps=max_steps)
        out[name + ".args"] = np.asarray([a, b, steps, mult, max_steps], dtype=np.float64)
        out[name + ".rates"] = np.asarray([float(fn(it)) for it in ITERATIONS], dtype=np.float64)
    path = os.path.join(HERE, "lr_schedule.npz")
    np.savez(path, **out)
    print(path, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    sys.exit(main())
