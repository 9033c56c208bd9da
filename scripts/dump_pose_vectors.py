#!/usr/bin/env python
"""Close the open pin of the test-time pose refinement: record what pytorch3d itself gives for the two functions that
/root/reference/eval.py:17 imports from it, in tests/golden/pose_external/pytorch3d.npz.

pytorch3d is not installed where this project is built and tested, so mobgs_amd.tto restates quaternion_to_matrix and
matrix_to_quaternion from memory of that package -- real part first, quaternion_to_matrix does NOT normalise (two_s =
2 / (q . q)) -- and that reading is UNPINNED.  On any machine that has the package:

    python scripts/dump_pose_vectors.py

    pytorch3d.npz   q [n,4] float64 (seeded; unit, scaled and negative-real quaternions), version,
                    quaternion_to_matrix [n,3,3], matrix_to_quaternion [n,4] (of those matrices)

The suite picks the file up: tests/test_tto_cpu.py::test_restatement_against_pytorch3d_vectors holds
mobgs_amd.tto.quaternion_to_matrix to the matrices and matrix_to_quaternion to the quaternions up to their sign; without
the file that test is skipped and the pin stays open."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def quaternions():
    g = torch.Generator().manual_seed(2024)
    q = torch.randn(64, 4, generator=g, dtype=torch.float64)
    q = q / q.norm(dim=-1, keepdim=True)
    scale = torch.tensor([1.0, 1.0, 1e-3, 0.5, 2.0, -1.0, 1.0, 3.0], dtype=torch.float64).repeat(8)
    q = q * scale[:, None]
    q[0] = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64)
    for axis in range(3):                      # 180 degrees about each axis
        q[1 + axis] = 0.0
        q[1 + axis, 1 + axis] = 1.0
    return q


def main():
    import pytorch3d
    from pytorch3d.transforms import matrix_to_quaternion, quaternion_to_matrix
    q = quaternions()
    R = quaternion_to_matrix(q)
    back = matrix_to_quaternion(R)
    out_dir = os.path.join(ROOT, "tests", "golden", "pose_external")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "pytorch3d.npz")
    np.savez(path, q=q.numpy(), version=np.array(pytorch3d.__version__), quaternion_to_matrix=R.numpy(),
             matrix_to_quaternion=back.numpy())
    print(f"wrote {path} (pytorch3d {pytorch3d.__version__}, {q.shape[0]} quaternions)")


if __name__ == "__main__":
    main()
