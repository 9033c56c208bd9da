"""Pin the flow colour wheel: run the real `flow_vis` package (pip install flow_vis) on seeded flows and store what it
returns as tests/golden/flowvis_external/flow_to_color.npz.

    python scripts/dump_flowvis_vectors.py

mobgs_amd.flow_vis, csrc/report.hip and tests/report_restatement.py restate the package from memory (README, "The flow
colour wheel is UNPINNED").  With this file present, tests/test_report_cpu.py::test_flowvis_vectors compares the wheel, the
numpy path (byte for byte) and the restatement (under the one-level rule) with the package's own output; until then that
test skips.  Stored: the wheel, and per case "<name>_flow" (float32 [H,W,2]), "<name>_color" (uint8 [H,W,3]) and, where
used, "<name>_clip".  Needs numpy and flow_vis only; well under 100 kB.
"""
import os

import numpy as np


def main():
    import flow_vis
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "flowvis_external")
    os.makedirs(out, exist_ok=True)
    arrays = {"colorwheel": np.asarray(flow_vis.make_colorwheel(), dtype=np.float64)}
    g = np.random.RandomState(2024)
    cases = {"noise": (g.normal(0.0, 2.0, (48, 80, 2)).astype(np.float32), None),
             "small": (g.normal(0.0, 1e-3, (13, 17, 2)).astype(np.float32), None),
             "clipped": (g.normal(1.0, 2.0, (24, 40, 2)).astype(np.float32), 1.5),
             "zero": (np.zeros((4, 6, 2), np.float32), None)}
    ring = np.linspace(0.0, 2.0 * np.pi, 720, endpoint=False)
    cases["ring"] = (np.stack([np.cos(ring), np.sin(ring)], -1).astype(np.float32)[None] *
                     np.linspace(0.1, 3.0, 8, dtype=np.float32)[:, None, None], None)
    right = np.zeros((2, 9, 2), np.float32)
    right[0, :, 0] = np.linspace(0.5, 4.0, 9)        # v = +0, u > 0: the wrap
    right[1, :, 0] = np.linspace(0.5, 4.0, 9)
    right[1, :, 1] = -0.0                            # ... and its other side
    cases["wrap"] = (right, None)
    for name, (flow, clip) in cases.items():
        arrays[name + "_flow"] = flow
        arrays[name + "_color"] = np.asarray(flow_vis.flow_to_color(flow, clip_flow=clip, convert_to_bgr=False))
        if clip is not None:
            arrays[name + "_clip"] = np.float64(clip)
    path = os.path.join(out, "flow_to_color.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB), flow_vis {getattr(flow_vis, '__version__', '?')}")


if __name__ == "__main__":
    main()
