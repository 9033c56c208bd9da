"""The projection kernels by themselves (csrc/project.hip: project_fwd_kernel, project_bwd_kernel with cotangents of its own,
camera_sum_kernel, viewmat_reduce_kernel) against oracle.gsplat_torch.fully_fused_projection in float64, row by row.

Cases, references and comparators are tests/splat_cases.py (tests/test_splat_cases_cpu.py shows from the oracle alone that
each case reaches its edge): wave and workgroup tails, rows beyond the frustum limits in x, in y and in both, rows across the
near plane, one cotangent at a time (NULL pointers in the kernel), three cameras over shared geometry (accumulate launches)
and over per-camera geometry (one launch + camera_sum_kernel, through rendering._ProjectAndBin), radius_clip / far_plane
culls, nothing visible at all, and 258 partial rows of the pose gradient.  The float64 oracle keeps every row away from the
kinks, so fp32 and float64 take the same branch everywhere: radii are compared exactly, culled rows are exactly zero in
every output and gradient, and everything else is compared in full, no flip allowance:
  * per tensor, `close_to_f64`: max |got - ref64| <= k max |ref32 - ref64| + 2^-23 max |ref64|;
  * per row within each stratum (ordinary / clamped in x / in y / in both), `rows_close_to_f64`: with
    e_i = |got_i - ref64_i|_inf / (|ref64_i|_inf + 1e-3 median row norm), max_i e_i and median_i e_i are each at most k x
    the same statistic of the fp32 oracle;
  * the pose gradient per tensor, its fourth row exactly zero.
k = 3 (three times the fp32 reference's own gap, a rule that needs no run of the code under test).

Worst k needed on an MI355X per family (docs/MEASUREMENT_LOG.md, "Per-splat kernels against float64"):

    family                               worst k needed (case, tensor / stratum)                   k
    outputs, per tensor                  0.95  (many_rows, means2d)                                 3
    outputs, per row                     1.96  (n65, conics / ordinary, 11 rows)                    3
    gradients, per tensor                1.49  (n257, v_scales)                                     3
    gradients, per row, >= 32 rows       1.54  (many_rows, v_scales / ordinary, 10665 rows)         3
    gradients, per row, < 32 rows        4.47  (n65, v_scales / ordinary, 11 rows)                  8
    pose gradient                        1.02  (clip, v_viewmats)                                   3
"""
import pytest
import torch

import splat_cases as S

pytestmark = pytest.mark.gpu

K = {"outputs": 3, "rows": 3, "pose": 3}
K_SMALL = {"outputs": None, "rows": 8}  # per-row gradients in strata of fewer than splat_cases.SMALL rows


def _run(case, dev):
    """The case through the default host path -> (radii, means2d, depths, conics), the four leaves (gradients set)."""
    from mobgs_amd import rendering
    means, quats, scales, V = (t.to(dev).requires_grad_(True) for t in (case.means, case.quats, case.scales, case.viewmats))
    Ks = case.Ks.to(dev)
    if case.own:  # per-camera geometry exists on the binning node only (rendering._project_and_bin)
        tl = rendering.TileLists()
        outs = rendering._ProjectAndBin.apply(means, quats, scales, V, Ks, case.opacities.to(dev), tl, case.W, case.H, S.EPS2D,
                                              case.near_plane, case.far_plane, case.radius_clip, False)[:4]
    else:
        outs = rendering.fully_fused_projection(means, None, quats, scales, V, Ks, case.W, case.H, eps2d=S.EPS2D,
                                                near_plane=case.near_plane, far_plane=case.far_plane,
                                                radius_clip=case.radius_clip)[:4]
    pairs = [(o, c.to(dev)) for o, c in zip(outs[1:], case.cots) if c is not None]
    torch.autograd.backward([o for o, _ in pairs], [c for _, c in pairs])
    torch.cuda.synchronize()
    if case.own:
        tl.resolve()
    return outs, (means, quats, scales, V)


@pytest.mark.parametrize("name", S.PROJ_CASES)
def test_projection_matches_float64(hip_device, name):
    case = S.proj_case(name)
    ref64, ref32 = S.proj_reference(name)
    (radii, means2d, depths, conics), (means, quats, scales, V) = _run(case, hip_device)
    tag = f"projection {name}"
    assert radii.dtype == torch.int32 and torch.equal(radii.cpu(), ref64["radii"])
    got = {"means2d": means2d, "depths": depths, "conics": conics, "v_means": means.grad, "v_quats": quats.grad,
           "v_scales": scales.grad, "v_viewmats": V.grad}
    code = S.proj_strata(case)
    for key in S.PROJ_OUTPUTS + S.PROJ_GRADS:
        assert got[key] is not None, key
        family = "outputs" if key in S.PROJ_OUTPUTS else "rows"
        S.close_to_f64(got[key], ref64[key], ref32[key], K[family], f"{tag} [{family}] {key}")
        S.rows_close_to_f64(got[key], ref64[key], ref32[key], S.proj_row_strata(case, key), S.COLS[key], K[family],
                            f"{tag} [{family}] {key}", K_SMALL[family])
        # culled rows: exactly zero (per camera, or in every camera for a gradient that sums over them)
        per_camera = key in S.PROJ_OUTPUTS or (case.own and key in ("v_means", "v_quats"))
        culled = (code if per_camera else S.union_strata(code)).reshape(-1) < 0
        assert not got[key].detach().cpu().reshape(-1, S.COLS[key])[culled].any(), f"{tag} {key}: culled rows not zero"
    S.close_to_f64(got["v_viewmats"], ref64["v_viewmats"], ref32["v_viewmats"], K["pose"], f"{tag} [pose] v_viewmats")
    assert not got["v_viewmats"][:, 3].any()
    if name == "all_culled":
        assert not any(t.any() for t in got.values()) and not radii.any()
