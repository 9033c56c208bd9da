#!/usr/bin/env python
"""Close the open pin of tOF: record what OpenCV gives on a few seeded 8-bit frame pairs, in
tests/golden/tof_external/farneback.npz.

OpenCV is not installed where this project is built and tested, so csrc/tof.hip is checked against a restatement of
calcOpticalFlowFarneback written from memory (tests/tof_restatement.py; README, "The Farneback restatement is UNPINNED").
On any machine that has cv2:

    python scripts/dump_tof_vectors.py

    farneback.npz   version; rgb [n,3,H,W] uint8 and grey [n,H,W] uint8 = cv2.cvtColor(., COLOR_RGB2GRAY) (the 14- or 15-bit
                    grey coefficients); prev, next [m,h,w] uint8 grey pairs and flow [m,h,w,2] float32 =
                    cv2.calcOpticalFlowFarneback(prev, next, None, 0.5, 3, 15, 3, 5, 1.2, 0), the reference's call
                    (metrics.py:15), at 75x50 (one level), 136x72 (two) and 262x259 (four, odd level sizes)

The suite picks the file up: tests/test_tof_cpu.py::test_opencv_vectors holds the float64 restatement to it; without the
file that test is skipped and the pin stays open.  The file is a few hundred KiB."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import tof_restatement as TR  # noqa: E402


def main():
    import cv2
    out_dir = os.path.join(ROOT, "tests", "golden", "tof_external")
    os.makedirs(out_dir, exist_ok=True)
    rgb = TR.to_uint8(TR.moving_frames(2, 64, 96, seed=9))
    rng = np.random.default_rng(0)
    rgb[1] = rng.integers(0, 256, size=rgb[1].shape, dtype=np.uint8)         # every rounding case of the fixed point
    grey = np.stack([cv2.cvtColor(np.ascontiguousarray(f.transpose(1, 2, 0)), cv2.COLOR_RGB2GRAY) for f in rgb])
    groups = {}
    for H, W in ((50, 75), (72, 136), (259, 262)):
        g = TR.grey(TR.moving_frames(3, H, W, seed=H)).astype(np.uint8)
        pairs = [(g[0], g[1]), (g[1], g[2])]
        tex = TR.texture(H, W, 3).astype(np.uint8), TR.texture(H, W, 3, shift=(1.5, -0.75)).astype(np.uint8)
        pairs.append(tex)
        groups[f"{W}x{H}"] = (np.stack([p for p, _ in pairs]), np.stack([n for _, n in pairs]),
                              np.stack([cv2.calcOpticalFlowFarneback(p, n, None, 0.5, 3, 15, 3, 5, 1.2, 0) for p, n in pairs]))
    # the test reads one size per file key triple; the largest size goes under the plain names
    prev, nxt, flow = groups["262x259"]
    extra = {f"{k}_{name}": v for k, trip in groups.items() if k != "262x259" for name, v in zip(("prev", "next", "flow"), trip)}
    np.savez_compressed(os.path.join(out_dir, "farneback.npz"), version=np.array(cv2.__version__), rgb=rgb, grey=grey,
                        prev=prev, next=nxt, flow=flow, **extra)
    print("cv2", cv2.__version__, {k: v[2].shape for k, v in groups.items()})


if __name__ == "__main__":
    main()
