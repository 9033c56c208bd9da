"""Generate tests/golden/gridreg.npz by RUNNING THE REFERENCE'S OWN compute_plane_smoothness and compute_plane_tv
(scene/regulation.py) and GaussianModel._plane_regulation / _time_regulation / _l1_regulation / compute_regulation
(scene/gaussian_model.py:1373-1415) on the CPU, in the container that holds the reference.

    python tests/golden/make_golden_gridreg.py

The model methods are called on a stub object that carries `_deformation.deformation_net.grid.grids`; nothing of the
reference is copied, packages it imports and this container lacks are stubbed (ref_harness).  The inputs: one 6-plane
level of C = 4 (spatial planes 5 x 6, time planes h = 3; time planes hold exact ones mixed with values on both sides of
1) and one 3-plane level, which must contribute 0.  The fixture holds data only: the planes, the reference's fp32 values
and autograd gradients, the float64 restatement's (tests/gridreg_restatement.py), and per value `gap_*`, the distance
between the two -- the reference's own fp32 summation error, of which the tests allow 3 x: relative for a
value, relative to the gradient's largest magnitude for a gradient.  The three weights are the reference's stereo
configuration's (arguments/stereo/default.py)."""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import gridreg_restatement as GR  # noqa: E402
import ref_harness as RH  # noqa: E402
from helpers import save_npz  # noqa: E402

C, SPATIAL_HW, TIME_HW = 4, (5, 6), (3, 6)
WEIGHTS = dict(time_smoothness_weight=0.001, l1_time_planes_weight=0.0001, plane_tv_weight=0.0002)


def make_planes():
    g = torch.Generator().manual_seed(20261)
    level = []
    for i in range(6):
        if i in GR.SPATIAL:
            level.append(torch.rand(1, C, *SPATIAL_HW, generator=g) * 0.4 + 0.1)
        else:
            p = torch.ones(1, C, *TIME_HW)
            off = (torch.rand(p.shape, generator=g) - 0.5) * 0.2
            keep = torch.rand(p.shape, generator=g) < 0.4          # exact ones stay: the kink of |1 - t|
            level.append(torch.where(keep, p, p + off))
    small = [torch.rand(1, C, *SPATIAL_HW, generator=g) for _ in range(3)]
    return [level, small]


def rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(b), 1e-300) if a != b else 0.0


def main():
    try:
        import matplotlib.pyplot  # noqa: F401  (imported by scene/regulation.py, used by none of these functions)
    except ImportError:
        sys.modules["matplotlib"] = types.ModuleType("matplotlib")
        sys.modules["matplotlib.pyplot"] = sys.modules["matplotlib"].pyplot = types.ModuleType("matplotlib.pyplot")
    for name in ("helper_model",):
        sys.modules.setdefault(name, types.ModuleType(name))
    if not hasattr(sys.modules["helper_model"], "getcolormodel"):
        sys.modules["helper_model"].getcolormodel = None
    REG = RH.ref_import("scene.regulation")
    GM = RH.ref_import("scene.gaussian_model").GaussianModel

    class Stub:
        _plane_regulation = GM._plane_regulation
        _time_regulation = GM._time_regulation
        _l1_regulation = GM._l1_regulation
        compute_regulation = GM.compute_regulation

    grids = make_planes()
    arrays = {"weights": np.array([WEIGHTS["plane_tv_weight"], WEIGHTS["time_smoothness_weight"],
                                   WEIGHTS["l1_time_planes_weight"]], dtype=np.float64)}
    for li, level in enumerate(grids):
        for pi, p in enumerate(level):
            arrays[f"plane_{li}_{pi}"] = p.numpy()

    # the two plane functions on every plane of the 6-plane level
    for pi, p in enumerate(grids[0]):
        for name, fn, val64, grad64 in (("smooth", REG.compute_plane_smoothness, GR.smoothness, GR.smoothness_grad),
                                        ("tv", REG.compute_plane_tv, GR.tv, GR.tv_grad)):
            t = p.clone().requires_grad_(True)
            v = fn(t)
            v.backward()
            g64 = grad64(p.numpy())[0]
            arrays[f"{name}_{pi}"] = v.detach().numpy()
            arrays[f"{name}_{pi}_f64"] = np.float64(val64(p.numpy()))
            arrays[f"gap_{name}_{pi}"] = np.float64(rel(v, val64(p.numpy())))
            arrays[f"g_{name}_{pi}"] = t.grad.numpy()
            arrays[f"g_{name}_{pi}_f64"] = g64
            arrays[f"gap_g_{name}_{pi}"] = np.float64(np.abs(t.grad.numpy() - g64).max() / np.abs(g64).max())

    # the model's methods on the stub
    def model():
        leaves = [[p.clone().requires_grad_(True) for p in level] for level in grids]
        s = Stub()
        s._deformation = types.SimpleNamespace(deformation_net=types.SimpleNamespace(grid=types.SimpleNamespace(grids=leaves)))
        return s, leaves

    f64 = dict(zip(("plane", "time", "l1"), GR.terms([[p.numpy() for p in level] for level in grids])))
    ones = {"plane": (1.0, 0.0, 0.0), "time": (0.0, 1.0, 0.0), "l1": (0.0, 0.0, 1.0)}
    w = arrays["weights"]
    for name, call, scales in (("plane", lambda s: s._plane_regulation(), ones["plane"]),
                               ("time", lambda s: s._time_regulation(), ones["time"]),
                               ("l1", lambda s: s._l1_regulation(), ones["l1"]),
                               ("total", lambda s: s.compute_regulation(**WEIGHTS), tuple(w))):
        s, leaves = model()
        v = call(s)
        v.backward()
        v64 = f64[name] if name != "total" else w[0] * f64["plane"] + w[1] * f64["time"] + w[2] * f64["l1"]
        arrays[f"reg_{name}"] = v.detach().numpy()
        arrays[f"reg_{name}_f64"] = np.float64(v64)
        arrays[f"gap_reg_{name}"] = np.float64(rel(v, v64))
        g64 = GR.regulation_grads([[p.numpy() for p in level] for level in grids], scales)
        for li, level in enumerate(leaves):
            for pi, leaf in enumerate(level):
                got = leaf.grad
                if li == 1:
                    assert got is None, "the 3-plane level must contribute nothing"
                    continue
                want = g64[li][pi][0]
                if got is None:                                     # a plane the term does not touch
                    assert not np.any(want), (name, pi)
                    got = torch.zeros_like(leaf)
                arrays[f"g_reg_{name}_{pi}"] = got.numpy()
                arrays[f"g_reg_{name}_{pi}_f64"] = want
                top = np.abs(want).max()
                arrays[f"gap_g_reg_{name}_{pi}"] = np.float64(np.abs(got.numpy() - want).max() / top if top > 0 else 0.0)
    assert all(np.all(np.isfinite(a)) for a in arrays.values())
    save_npz(os.path.join(HERE, "gridreg.npz"), arrays)
    for k in sorted(arrays):
        if k.startswith("gap_"):
            print(f"{k:24s} {float(arrays[k]):.3e}")


if __name__ == "__main__":
    main()
