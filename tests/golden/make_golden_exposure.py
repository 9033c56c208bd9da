"""Generate tests/golden/exposure.npz by RUNNING THE REFERENCE'S OWN gaussian_renderer.get_flow_static on CPU, in the
container that holds the reference.

    python tests/golden/make_golden_exposure.py

The scene is the one make_golden.py builds for its get_flow_static fixture (900 static + 500 dynamic splats, 80 x 48,
seed 3).  Two calls through ref_harness, both splatted through the view's own camera as train.py:479-480 does: the
camera flow between a previous and a next pose, and the latent flow between the first and the last pose of a shorter
path inside the exposure.  The fixture holds data only: the scene's inputs, the five poses, the two rendered flow maps,
what the statements of train.py:482-491 (tests/exposure_restatement.py reference_chain: torch.norm, torch.quantile,
the mask, torch.median) give on them in fp32, the same estimate in float64, and `ref_gap`, the distance between the two:
the reference's own noise floor, of which the GPU tests allow 3 x."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402
import ref_harness as RH  # noqa: E402
import exposure_restatement as ER  # noqa: E402

from mobgs_amd.camera import PinholeCamera  # noqa: E402
from mobgs_amd.synth import SynthCamera  # noqa: E402

NS, ND, W, H, SEED, Q = 900, 500, 80, 48, 3, 0.01
STEP = torch.tensor([0.02, 0.01, -0.01])      # the pose change of make_golden.gen_get_flow
# translations added to the view's pose: previous / next view, first / last latent camera
OFFSETS = {"bwd": -1.0, "fwd": 1.0, "start": -0.3, "end": 0.3}


def main():
    gr = RH.ref_import("gaussian_renderer")
    scam = SynthCamera().scaled(W, H)
    w2c = MG.small_w2c()
    stat, dyn = MG.scene_params(NS, ND, scam, SEED)
    spc, dpc = MG.ref_models(stat, dyn, SEED)
    bg = torch.zeros(9)

    def camera(pose):
        return PinholeCamera(W, H, scam.K, pose, time=scam.time, max_time=scam.max_time)

    poses = {}
    for name, f in OFFSETS.items():
        poses[name] = w2c.clone()
        poses[name][:3, 3] += f * STEP
    view = camera(w2c)
    with RH.CudaToCpu(), torch.no_grad():
        _, cam_flow = gr.get_flow_static(camera(poses["bwd"]), camera(poses["fwd"]), view, spc, dpc, None, bg)
        _, latent_flow = gr.get_flow_static(camera(poses["start"]), camera(poses["end"]), view, spc, dpc, None, bg)
        ref32 = ER.reference_chain(cam_flow, latent_flow, Q)
        ref32_edge = ER.reference_chain(cam_flow, latent_flow, Q, edge=True)
    f64 = ER.estimate(cam_flow, latent_flow, Q, 1.0, torch.float64)
    f32 = ER.estimate(cam_flow, latent_flow, Q, 1.0, torch.float32)
    assert f64["updated"] == 1 and cam_flow.dtype == torch.float32
    arrays = MG.inputs_dict(stat, dyn, view, w2c, spc, dpc, bg)
    arrays.update({"in_w2c_" + k: MG.np_(v) for k, v in poses.items()})
    arrays.update({"q": np.array([Q]), "out_cam_flow": MG.np_(cam_flow), "out_latent_flow": MG.np_(latent_flow),
                   "ref_value": MG.np_(ref32).reshape(1), "ref_value_edge": MG.np_(ref32_edge).reshape(1),
                   "f64_value": MG.np_(f64["value"]).reshape(1), "f64_threshold": MG.np_(f64["threshold"]).reshape(1),
                   "f64_n_valid": np.array([f64["n_valid"]]),
                   "restated_value": MG.np_(f32["value"]).reshape(1), "restated_n_valid": np.array([f32["n_valid"]]),
                   "ref_gap": np.array([abs(float(ref32) - float(f64["value"]))])})
    print(f"reference fp32 {float(ref32):.9g}  restated fp32 {float(f32['value']):.9g}  float64 {float(f64['value']):.12g}  "
          f"ref_gap {float(arrays['ref_gap'][0]):.3e}  n_valid {f32['n_valid']} / {H * W}")
    MG.save("exposure", **arrays)


if __name__ == "__main__":
    main()
