#!/usr/bin/env python
"""Record what the reference's own LPIPS model returns, on a machine that has torchvision, its pretrained AlexNet file and
a checkout of the reference (none of which the build container has):

    python scripts/dump_lpips_vectors.py --reference <checkout> [--cases 0 3 8] [--out tests/golden/lpips_external]

For the cases of tests/lpips_restatement.py (make_case: seeded, nothing stored but a checksum probe) it calls
models.PerceptualLoss(model='net-lin', net='alex', use_gpu=False, version=0.1).forward(gt, pred) exactly as
metrics.py:127-131 does (im2tensor: 2 x - 1) and writes perceptual_loss.npz: case [n], probe [n,4], first [n+1], lpips [rows]
and trunk_checksum (the float64 sum of features.0.weight of the trunk the model loaded).  With that file present,
tests/test_lpips_cpu.py::test_external_vectors checks the restatement against it when MOBGS_ALEXNET_TRUNK names the same trunk
file (README, "UNPINNED").  Runs on the CPU; needs no HIP device."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference (the directory that holds models/)")
    ap.add_argument("--cases", type=int, nargs="*", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lpips_external"))
    a = ap.parse_args()
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import lpips_restatement as LR
    sys.path.insert(0, os.path.abspath(a.reference))
    import models                                                    # the reference's package
    model = models.PerceptualLoss(model="net-lin", net="alex", use_gpu=False, version=0.1)
    net = model.model.net
    net = getattr(net, "module", net)
    trunk_checksum = float(net.net.slice1[0].weight.detach().double().sum())
    cases = list(range(len(LR.CASES))) if a.cases is None else a.cases
    values, first, probes = [], [0], []
    with torch.no_grad():
        for i in cases:
            c = LR.make_case(i)
            gt, pred = LR.prepare(c["gt"], c["pred"], c["clamp"], c["quantize"])
            v = model.forward(2 * gt - 1, 2 * pred - 1).reshape(-1).double().numpy()
            values.append(v)
            first.append(first[-1] + v.shape[0])
            probes.append(LR.probe(c))
            print(LR.case_name(i), v.tolist())
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "perceptual_loss.npz")
    np.savez_compressed(path, case=np.array(cases), probe=np.stack(probes), first=np.array(first),
                        lpips=np.concatenate(values), trunk_checksum=np.array(trunk_checksum))
    print("wrote", path)


if __name__ == "__main__":
    main()
