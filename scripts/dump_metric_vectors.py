#!/usr/bin/env python
"""Close the open pin of the evaluation metrics: record what scikit-image and the reference's jax code give on the seeded
cases of tests/metrics_restatement.py, in tests/golden/metrics_external/*.npz.

Neither package is installed where this project is built and tested, so mobgs_amd.metrics is checked against a
restatement (numpy + scipy) only, and one reading of scikit-image's source is UNPINNED: that structural_similarity called
without a data_range on float images, as /root/reference/metrics.py:124 calls it, uses R = 2 on the versions that still
accept multichannel=True (<= 0.18).  On any machine that has them:

    pip install "scikit-image<=0.18.3"                 # and, for the dycheck numbers, jax
    python scripts/dump_metric_vectors.py [--reference DIR_OF_THE_REFERENCE_CHECKOUT]

    skimage.npz   case [n], probe [n,4], version, psnr_default [n], ssim_default [n] (both as metrics.py:123-124 calls them),
                  ssim_r1 [n], ssim_r2 [n] (data_range given)
    dycheck.npz   case [n], probe [n,4], psnr [n], ssim [n]   (compute_psnr / compute_ssim of DIR/dycheck_metrics.py, which
                  this script imports and does not copy; written only with --reference)

The suite picks the files up: tests/test_metrics_cpu.py holds the float64 restatement to them, tests/test_gpu_metrics.py
the HIP path; without the files those tests are skipped and the pin stays open.  No images are stored: a case is its seed."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import metrics_restatement as MR  # noqa: E402


def hwc(c, k=0):
    pred, gt = MR.prepare(c["pred"], c["gt"], c["clamp"], c["quantize"])
    mask = None if c["mask"] is None else c["mask"][k][..., None]
    return pred[k].transpose(1, 2, 0), gt[k].transpose(1, 2, 0), mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="a checkout of the reference (for dycheck_metrics.py)")
    a = ap.parse_args()
    out_dir = os.path.join(ROOT, "tests", "golden", "metrics_external")
    os.makedirs(out_dir, exist_ok=True)
    single = [i for i, (H, W, B, what) in enumerate(MR.CASES) if B == 1]

    import skimage
    from skimage.metrics import peak_signal_noise_ratio, structural_similarity
    rows = {k: [] for k in ("case", "probe", "psnr_default", "ssim_default", "ssim_r1", "ssim_r2")}
    for i in (i for i in single if MR.CASES[i][3] in ("absent",) + MR.EXTRAS):
        c = MR.make_case(i)
        pred, gt, _ = hwc(c)
        rows["case"].append(i)
        rows["probe"].append(MR.probe(c))
        rows["psnr_default"].append(peak_signal_noise_ratio(gt, pred))
        rows["ssim_default"].append(structural_similarity(gt, pred, multichannel=True))     # metrics.py:124, verbatim
        rows["ssim_r1"].append(structural_similarity(gt, pred, multichannel=True, data_range=1.0))
        rows["ssim_r2"].append(structural_similarity(gt, pred, multichannel=True, data_range=2.0))
    np.savez_compressed(os.path.join(out_dir, "skimage.npz"), version=np.array(skimage.__version__),
                        **{k: np.array(v) for k, v in rows.items()})
    print("skimage", skimage.__version__, len(rows["case"]), "cases")

    if a.reference:
        sys.path.insert(0, a.reference)
        import dycheck_metrics as D
        rows = {k: [] for k in ("case", "probe", "psnr", "ssim")}
        for i in (i for i in single if min(MR.CASES[i][:2]) >= 11):
            c = MR.make_case(i)
            pred, gt, mask = hwc(c)
            rows["case"].append(i)
            rows["probe"].append(MR.probe(c))
            rows["psnr"].append(float(D.compute_psnr(pred, gt, mask)))
            rows["ssim"].append(float(D.compute_ssim(pred, gt, mask, max_val=c["data_range"])))
        np.savez_compressed(os.path.join(out_dir, "dycheck.npz"), **{k: np.array(v) for k, v in rows.items()})
        print("dycheck", len(rows["case"]), "cases")


if __name__ == "__main__":
    main()
