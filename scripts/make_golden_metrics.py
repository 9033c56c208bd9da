"""Writes tests/golden/metrics.npz from tests/metrics_restatement.py: for every case of its CASES the float64 and the fp32
values of the seven metrics of every image, and a checksum probe of the seeded inputs (no images are stored).

    python scripts/make_golden_metrics.py

    names   [n_cases]       case names (H x W - B - mask stratum or extra)
    first   [n_cases + 1]   rows of case i are first[i] .. first[i + 1] (one row per image)
    f64     [rows, 7]       metrics_restatement.METRICS in float64 (NaN: an arm the size does not allow)
    f32     [rows, 7]       the same statements in fp32
    probe   [n_cases, 4]    metrics_restatement.probe of the case's inputs
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import metrics_restatement as MR  # noqa: E402


def main():
    f64, f32, probes, first = [], [], [], [0]
    for i in range(len(MR.CASES)):
        c = MR.make_case(i)
        f64.append(MR.evaluate(c, np.float64))
        f32.append(MR.evaluate(c, np.float32))
        assert f64[-1].dtype == np.float64 and f32[-1].dtype == np.float32
        probes.append(MR.probe(c))
        first.append(first[-1] + f64[-1].shape[0])
    out = os.path.join(ROOT, "tests", "golden", "metrics.npz")
    np.savez_compressed(out, names=np.array([MR.case_name(i) for i in range(len(MR.CASES))]), first=np.array(first),
                        f64=np.concatenate(f64), f32=np.concatenate(f32), probe=np.stack(probes))
    fx = dict(np.load(out))
    print(out, os.path.getsize(out), "bytes;", len(MR.CASES), "cases,", first[-1], "rows")
    for k, v in MR.reference_gaps(fx).items():
        print(f"  largest fp32 distance from float64, {k}: {v:.2e}")


if __name__ == "__main__":
    main()
