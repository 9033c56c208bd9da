"""Float64 restatement, in plain torch, of what GaussianModel.onedown_control_pts computes (scene/gaussian_model.py:
274-371 with utils/graphics_utils.py:24-31, :142-155), used as the yardstick of tests/golden/prune.npz and of the GPU
tests.  The reference's own function cannot run in float64 (it mixes .float() into a scatter), and its fp32
torch.linalg.lstsq is the thing whose noise the fixture measures.

It follows the reference's formulation, not the product's: the full [12, 11] system per row with its dummy equations,
solved by a batched float64 least squares -- so that agreement with mobgs_amd.scene_init (one pseudo-inverse per count)
checks that shortcut too.  One deliberate difference, the same as in the product: rows whose count is
already 4 are not candidates; they keep their points and report error 0.
"""
import torch

from oracle.render_torch import hermite

CONTROL_NUM = 12


def design_rows(times: torch.Tensor, n_new: torch.Tensor) -> torch.Tensor:
    """float64 [B, T, 11]: row t of batch b = the weights with which the first n_new[b] of 11 control points give the
    Hermite spline at times[b, t] (index clamping and one-sided end derivatives as in interpolate_cubic_hermite)."""
    B, T = times.shape
    n = n_new.reshape(B, 1).to(torch.int64)
    ts = times.double() * (n - 1)
    zero = torch.zeros_like(n)
    i = torch.minimum(torch.maximum(torch.floor(ts).long(), zero), n - 2)
    il, ir, irr = torch.maximum(i - 1, zero), torch.minimum(i + 1, n - 1), torch.minimum(i + 2, n - 1)
    u = ts - i
    h00, h10 = (1 + 2 * u) * (1 - u) ** 2, u * (1 - u) ** 2
    h01, h11 = u ** 2 * (3 - 2 * u), u ** 2 * (u - 1)
    first, last = il == i, irr == ir
    nil = torch.zeros_like(u)
    w0 = torch.where(first, nil, -h10 / 2)
    w1 = h00 + torch.where(first, -h10, nil) + torch.where(last, -h11, -h11 / 2)
    w2 = h01 + torch.where(first, h10, h10 / 2) + torch.where(last, h11, nil)
    w3 = torch.where(last, nil, h11 / 2)
    A = torch.zeros(B, T, CONTROL_NUM - 1, dtype=torch.float64)
    for idx, w in ((il, w0), (i, w1), (ir, w2), (irr, w3)):
        A.scatter_add_(2, idx[..., None], w[..., None])
    return A


def one_down_f64(control_xyz: torch.Tensor, control_num: torch.Tensor):
    """-> (new_control float64 [N,11,3], new_num int64 [N]).  Rows with count >= 5: the least-squares solution of the
    reference's system (equations k < n: the new spline at the old knot time k / (n - 1) equals old point k; equations
    k >= n: new point k - 1 equals 0).  Rows with count 4: their own points, zeros from slot 4 on, count 4."""
    c = control_xyz.double()
    N = c.shape[0]
    n = control_num.reshape(N).to(torch.int64)
    cand = n > 4
    m = torch.where(cand, n - 1, n)
    k = torch.arange(CONTROL_NUM, dtype=torch.float64)[None, :].expand(N, -1)
    A = design_rows(k / (n[:, None] - 1).double(), m)                       # [N, 12, 11]
    real = (torch.arange(CONTROL_NUM)[None, :] < n[:, None])                # equation k is a real one
    dummy = torch.zeros(CONTROL_NUM, CONTROL_NUM - 1, dtype=torch.float64)
    dummy[torch.arange(1, CONTROL_NUM), torch.arange(CONTROL_NUM - 1)] = 1.0
    lhs = torch.where(real[..., None], A, dummy[None])
    rhs = torch.where(real[..., None], c, torch.zeros_like(c))
    sol = torch.linalg.lstsq(lhs, rhs).solution                             # [N, 11, 3]
    keep = torch.where(real[:, :CONTROL_NUM - 1, None], c[:, :CONTROL_NUM - 1], torch.zeros_like(sol))
    return torch.where(cand[:, None, None], sol, keep), m


def prune_error_f64(control_xyz, control_num, new_control, new_num, w2c, times, focal, cx, cy):
    """float64 [N]: mean over the interior views of the pixel distance between the old and the new trajectory.
    w2c [V,4,4] world-to-camera (column vectors), K = [focal, 0, cx; 0, focal, cy; 0, 0, 1], both divides with the
    reference's + 1e-7.  Rows with count 4 report 0."""
    c = control_xyz.double()
    N = c.shape[0]
    n = control_num.reshape(N, 1).to(torch.int64)
    m = new_num.reshape(N, 1).to(torch.int64)
    full = torch.cat([new_control.double(), c[:, CONTROL_NUM - 1:]], 1)
    w2c = w2c.double()

    def pixels(p, M):
        h = torch.cat([p, torch.ones(N, 1, dtype=torch.float64)], 1) @ M.T
        cam = h[:, :3] / (h[:, 3:] + 0.0000001)
        d = cam[:, 2] + 0.0000001
        return torch.stack([(focal * cam[:, 0] + cx * cam[:, 2]) / d, (focal * cam[:, 1] + cy * cam[:, 2]) / d], 1)

    total = torch.zeros(N, dtype=torch.float64)
    V = w2c.shape[0]
    for v in range(1, V - 1):
        t = times[v].double()
        a = pixels(hermite(c, t, n) * 1e-2, w2c[v])
        b = pixels(hermite(full, t, m) * 1e-2, w2c[v])
        total += (a - b).norm(dim=1)
    err = total / (V - 2)
    return torch.where(n.reshape(N) > 4, err, torch.zeros_like(err))


def committed(control_xyz, control_num, new_control, new_num, prune):
    """The state after the commit: rows in `prune` [N] bool get slots 0..10 and the count of the fit, slot 11 stays."""
    c, n = control_xyz.clone(), control_num.clone().reshape(-1)
    c[prune, :CONTROL_NUM - 1] = new_control.to(c.dtype)[prune]
    n[prune] = new_num.reshape(-1)[prune]
    return c, n.reshape(control_num.shape)
