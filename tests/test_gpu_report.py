"""The report kernels on the MI355X (csrc/report.hip through mobgs_amd.scene_utils and mobgs_amd.flow_vis): statistics
bit-equal to torch, every panel kind against the float64 restatement under the one-level rule of tests/report_cases.py
(whose bound comes from an error analysis of the fp32 statements, never from a run), the sheets of a synthetic scene
against the same panels composed with torch ops, graph capture, the reference's own sheets, the files."""
import types

import numpy as np
import pytest
import torch

import report_cases as RC
import report_restatement as R
from helpers import load, same_bits

pytestmark = pytest.mark.gpu

CASES = RC.compose_cases()
POISON = 0xA5


def dev_panels(panels, dev):
    return [tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) if isinstance(x, np.ndarray) else x for x in p)
            for p in panels]


def compose(panels, H, W, dev, cam=None, **kw):
    from mobgs_amd.scene_utils import compose_sheet
    return compose_sheet(dev_panels(panels, dev), H, W, camera=cam, **kw)


# ---- mobgs_report_stats -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", RC.STAT_SIZES)
def test_stats_are_bit_equal_to_torch(hip_device, H, W):
    from mobgs_amd.scene_utils import report_stats
    g = torch.Generator().manual_seed(100 * H + W)
    depth = 4.0 * torch.rand(1, H, W, generator=g)
    signed = torch.randn(3, H, W, generator=g)
    a, b = torch.rand(3, H, W, generator=g), torch.rand(3, H, W, generator=g)
    flow = 3.0 * torch.randn(H, W, 2, generator=g)
    last = torch.rand(H * W, generator=g)
    last[0], last[-1] = -2.25, 7.5                     # the maximum is the last element, the minimum the first (1 x 1: 7.5)
    first = -last
    got = report_stats([("MINMAX", depth.to(hip_device)), ("MINMAX", signed.to(hip_device)),
                        ("SQERR", a.to(hip_device), b.to(hip_device)), ("FLOW_RAD", flow.to(hip_device)),
                        ("FLOW_RAD", flow.to(hip_device), 1.5), ("MINMAX", last.to(hip_device)),
                        ("MINMAX", first.to(hip_device))]).cpu()
    clipped = flow.clamp(0.0, 1.5)
    exprs = [depth, signed, (a - b) ** 2, torch.sqrt(flow[..., 0] * flow[..., 0] + flow[..., 1] * flow[..., 1]),
             torch.sqrt(clipped[..., 0] * clipped[..., 0] + clipped[..., 1] * clipped[..., 1]), last, first]
    assert got.shape == (len(exprs), 2) and got.dtype == torch.float32
    for k, e in enumerate(exprs):
        assert same_bits(got[k, 0], torch.amin(e)) and same_bits(got[k, 1], torch.amax(e)), (k, got[k], e.min(), e.max())
    assert float(got[5, 1]) == 7.5 and float(got[6, 0]) == -7.5 and float(got[5, 0]) == (-2.25 if H * W > 1 else 7.5)


# ---- mobgs_report_compose, per panel kind -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_compose_against_the_restatement(hip_device, case):
    name, H, W, panels = case
    L, b = RC.expected(panels, H, W)
    want = np.floor(L)
    assert not (want.reshape(H, -1) == POISON).all(1).any()          # no row whose correct bytes are all the poison value
    out = torch.full((H, len(panels) * W, 3), POISON, dtype=torch.uint8, device=hip_device)
    got = compose(panels, H, W, hip_device, RC.camera(H, W), out=out)
    assert got is out and got.dtype == torch.uint8
    RC.check_bytes(got.cpu().numpy(), L, b, name)
    # the same panels one below the other: every panel a contiguous image
    stacked = compose(panels, H, W, hip_device, RC.camera(H, W), vertical=True)
    assert stacked.shape == (len(panels), H, W, 3)
    assert torch.equal(torch.cat(list(stacked), dim=1), got)


@pytest.mark.parametrize("use_center", (True, False))
def test_normals_of_a_constant_depth(hip_device, use_center):
    """Points at one depth lie on the plane z = const: the normal is (0, 0, -1) at every pixel -- also in the last row, the
    last column and the corner, whose differences are the replicated ones -- whatever the skew and the pixel offset.
    (dv x du with du along +x and dv along +y points towards the camera.)  The bytes: (127, 127, 0)."""
    for H, W in ((2, 2), (5, 7), (48, 80)):
        cam = RC.camera(H, W, use_center)
        assert cam[3] != 0
        got = compose([("NORMALS_FD", np.full((1, H, W), 2.5, np.float32))], H, W, hip_device, cam).cpu().numpy()
        assert (got.reshape(-1, 3) == np.array([127, 127, 0])).all(), (H, W, np.unique(got.reshape(-1, 3), axis=0))
    # and a tilted depth: the border pixels repeat their inner neighbour's differences, so they follow the rule too
    H, W = 6, 9
    cam = RC.camera(H, W, use_center)
    p = RC.source("NORMALS_FD", H, W, 77)
    got = compose([p], H, W, hip_device, cam).cpu().numpy()
    L, b = R.level(R.normals_fd(p[1], cam)), RC.band("NORMALS_FD", p[1], None, cam)
    RC.check_bytes(got, L, b, f"normals, use_center={use_center}")
    with pytest.raises(ValueError):
        compose([("NORMALS_FD", np.ones((1, 1, 5), np.float32))], 1, 5, hip_device, RC.camera(1, 5))


def test_flow_special_cases(hip_device):
    from mobgs_amd import flow_vis
    H, W = 5, 7
    zero = flow_vis.flow_to_color(torch.zeros(H, W, 2, device=hip_device))
    assert zero.dtype == torch.uint8 and zero.shape == (H, W, 3) and zero.device.type == "cuda" and int(zero.min()) == 255
    # v = +0, u > 0: a = -1 exactly, wheel entry 0 = red, scaled by the radius rule
    flow = np.zeros((H, W, 2), np.float32)
    flow[..., 0] = np.linspace(0.5, 4.0, H * W, dtype=np.float32).reshape(H, W)
    got = flow_vis.flow_to_color(torch.from_numpy(flow).to(hip_device)).cpu().numpy()
    L, b = R.level(R.flow(flow)), RC.band("FLOW", flow)
    RC.check_bytes(got, L, b, "v = +0, u > 0")
    assert (got[..., 0] == 255).all() and (got[..., 1] == got[..., 2]).all() and got[-1, -1, 1] == 0
    # ... and v = -0 is the other side of the wrap: entry 54
    flow[..., 1] = -0.0
    got = flow_vis.flow_to_color(torch.from_numpy(flow).to(hip_device)).cpu().numpy()
    RC.check_bytes(got, R.level(R.flow(flow)), RC.band("FLOW", flow), "v = -0, u > 0")
    assert (got[..., 2] >= got[..., 1]).all() and (got[..., 2] > got[..., 1]).any()
    # clip_flow, and the channel order
    p = RC.source("FLOW", 13, 17, 5)[1]
    t = torch.from_numpy(p).to(hip_device)
    got = flow_vis.flow_to_color(t, clip_flow=1.5)
    RC.check_bytes(got.cpu().numpy(), R.level(R.flow(p, 1.5)), RC.band("FLOW", p, clip=1.5), "clip_flow")
    assert torch.equal(flow_vis.flow_to_color(t, clip_flow=1.5, convert_to_bgr=True), got.flip(-1))


def test_every_flow_of_a_batch_takes_its_own_rad_max(hip_device):
    H, W = 13, 17
    flows = [RC.source("FLOW", H, W, 900 + k)[1] * np.float32(0.25 * (k + 1)) for k in range(9)]
    got = compose([("FLOW", f) for f in flows], H, W, hip_device, vertical=True).cpu().numpy()
    assert got.shape == (9, H, W, 3)
    for k, f in enumerate(flows):
        RC.check_bytes(got[k], R.level(R.flow(f)), RC.band("FLOW", f), f"flow {k} of 9")
    alone = compose([("FLOW", flows[3])], H, W, hip_device).cpu().numpy()
    assert np.array_equal(alone, got[3])


def test_degenerate_statistics(hip_device):
    H, W = 5, 7
    z = np.zeros((1, H, W), np.float32)
    img = RC.source("RGB", H, W, 1)[1]
    got = compose([("GREY_DIV_MAX", z), ("ERROR", img, img.copy())], H, W, hip_device).cpu().numpy()
    assert got.shape == (H, 2 * W, 3) and not got.any()       # max = 0 -> 0 (no 0 / 0); equal images -> the 1e-8 arm -> 0


# ---- report_sheets on the synthetic scene -----------------------------------------------------------------------------
def torch_panel(kind, a, b=None, cam=None):
    """The reference's statements for one panel as torch float32 ops on the device -> float [H,W,3] before the
    conversion."""
    if kind == "RGB":
        return a.permute(1, 2, 0)
    if kind == "GREY":
        return a.reshape(1, *a.shape[-2:]).permute(1, 2, 0).repeat(1, 1, 3)
    if kind == "GREY_DIV_MAX":
        g = a.reshape(1, *a.shape[-2:]).permute(1, 2, 0)
        return (g / g.max()).repeat(1, 1, 3)
    if kind == "ERROR":
        e = (a.permute(1, 2, 0) - b.permute(1, 2, 0)) ** 2
        return (e - e.min()) / torch.clamp(e.max() - e.min(), min=1e-8)
    if kind == "SIGNED3":
        return ((a + 1) / 2).permute(1, 2, 0)
    if kind == "NORMALS_FD":
        focal, cx, cy, skew, offset = cam
        z = a.reshape(1, *a.shape[-2:]) + 1e-6
        H, W = z.shape[-2:]
        py, px = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=a.device) + offset,
                                torch.arange(W, dtype=torch.float32, device=a.device) + offset, indexing="ij")
        y = (py - cy) / focal
        x = (px - cx - y * skew) / focal
        coords = (torch.stack([x, y, torch.ones_like(x)], -1)[None] * z[..., None]).permute(0, 3, 1, 2)
        du = coords[..., :, 1:] - coords[..., :, :-1]
        du = torch.cat([du, du[..., :, -1:]], dim=-1)
        dv = coords[..., 1:, :] - coords[..., :-1, :]
        dv = torch.cat([dv, dv[..., -1:, :]], dim=-2)
        n = torch.stack([dv[:, 1] * du[:, 2] - du[:, 1] * dv[:, 2], dv[:, 2] * du[:, 0] - du[:, 2] * dv[:, 0],
                         dv[:, 0] * du[:, 1] - du[:, 0] * dv[:, 1]], dim=-3)
        return ((torch.nn.functional.normalize(n, dim=-3)[0] + 1) / 2).permute(1, 2, 0)
    raise ValueError(kind)


def torch_bytes(x):
    return (torch.clamp(x, 0, 1) * 255).to(torch.uint8)


def check_sheet(got, panels, cam, what):
    """got: uint8 device sheet; panels: device tensors.  Both the kernel's bytes and the torch composition's obey the rule
    around the restatement, and outside the bands they are equal."""
    host = [tuple(x.detach().cpu().numpy() if torch.is_tensor(x) else x for x in p) for p in panels]
    L = R.level(R.sheet(host, cam))
    b = np.concatenate([RC.band(p[0], p[1], p[2] if len(p) > 2 else None, cam) for p in host], axis=1)
    ref = torch.cat([torch_bytes(torch_panel(p[0], p[1], p[2] if len(p) > 2 else None, cam)) for p in panels], dim=1)
    assert got.shape == ref.shape and got.dtype == torch.uint8
    RC.check_bytes(got.cpu().numpy(), L, b, what)
    RC.check_bytes(ref.cpu().numpy(), L, b, what + " (torch ops)")
    free = torch.from_numpy(~RC.in_band(L, b)).to(got.device)
    assert torch.equal(got[free], ref[free]), what


class Scene:
    W, H = 80, 48

    def __init__(self, dev):
        from mobgs_amd.blce import blceKernel
        from mobgs_amd.camera import PinholeCamera
        from mobgs_amd.gaussian_model import GaussianParams
        from mobgs_amd.helper_model import Sandwich
        from mobgs_amd.synth import SynthCamera, dynamic_extras, gaussian_cloud
        W, H = self.W, self.H
        scam = SynthCamera().scaled(W, H)
        torch.manual_seed(0)
        dec = Sandwich(9, 3).to(dev)
        sp, dp = gaussian_cloud(900, scam, 0), gaussian_cloud(500, scam, 1)
        self.stat = GaussianParams(sp, None, dec, dev, requires_grad=False)
        self.dyn = GaussianParams(dp, dynamic_extras(dp["xyz"], 0), dec, dev, requires_grad=False)
        self.bg = torch.zeros(9, device=dev)
        g = torch.Generator().manual_seed(5)
        self.views = []
        for i in range(2):
            w2c = torch.eye(4)
            w2c[:3, 3] = torch.tensor([0.04 * i, -0.02 * i, 0.03 * i])
            c = PinholeCamera(W, H, scam.K, w2c, time=(5.0 + 6 * i) / 23.0, max_time=23, device=dev)
            c.uid, c.image_name = i, f"view{i}"
            c.original_image = c.image = torch.rand(3, H, W, generator=g).to(dev)
            n = torch.randn(3, H, W, generator=g)
            c.normal = (n / n.norm(dim=0, keepdim=True)).to(dev)
            c.depth = (1.0 + 3.0 * torch.rand(1, H, W, generator=g)).to(dev)
            c.mask = (torch.rand(1, H, W, generator=g) > 0.5).float().to(dev)
            c.metadata = types.SimpleNamespace(focal_length=float(scam.K[0, 0]), principal_point_x=float(scam.K[0, 2]),
                                               principal_point_y=float(scam.K[1, 2]), skew=0.0625, use_center=True)
            self.views.append(c)
        torch.manual_seed(1)
        self.blce = blceKernel(num_views=2, num_warp=9, iteration=1).to(dev)
        self.calls = []

    def render(self, *a, **k):
        from mobgs_amd.gaussian_renderer import render
        out = render(*a, **k)
        self.calls.append((k, out))
        return out


@pytest.fixture(scope="module")
def scene(hip_device):
    return Scene(hip_device)


@pytest.mark.parametrize("case", ("test", "train", "train_blur"))
def test_report_sheets_on_the_synthetic_scene(scene, case):
    from mobgs_amd.scene_utils import camera_intrinsics, report_sheets
    v, H, W = scene.views[0], Scene.H, Scene.W
    scene.calls.clear()
    sheets = report_sheets(v, scene.views[1], v, scene.stat, scene.dyn, scene.render, None, scene.bg, stage="fine",
                           cam_type="dycheck", is_train=case != "test", blcekernel=scene.blce if case == "train_blur" else None)
    pkg = scene.calls[0][1]
    r = {k: pkg[k] for k in ("render", "d_render", "s_render", "d_alpha", "depth")}
    r.update(gt=v.original_image, gt_normal=v.normal, gt_depth=v.depth)
    n_image, n_decomp = {"test": (6, 2), "train": (5, 4), "train_blur": (4, 4)}[case]
    assert sheets.image.shape == (H, n_image * W, 3) and sheets.decomp.shape == (H, n_decomp * W, 3)
    assert sheets.image.dtype == sheets.decomp.dtype == torch.uint8 and sheets.image.is_cuda
    if case == "train_blur":
        assert len(scene.calls) == 10                         # the view's render and one per latent camera; no coarse render
        latents = [c[1] for c in scene.calls[1:]]
        for k, (kw, _) in enumerate(scene.calls[1:]):
            assert kw["get_flow"] and kw["get_static"] and kw["get_dynamic"] and kw["stage"] == "fine"
            assert kw["delta_exposure"].numel() == 1
        ten = torch.mean(torch.stack([p["render"] for p in latents] + [pkg["render"]]), dim=0)
        assert same_bits(sheets.blurry, ten)
        r["blurry"] = sheets.blurry
        assert sheets.flows.shape == sheets.latents.shape == (9, H, W, 3) and sheets.flows.dtype == torch.uint8
        for k, p in enumerate(latents):
            check_sheet(sheets.latents[k], [("RGB", p["render"])], None, f"latent {k}")
            flow = p["ori_flow"].squeeze(0).cpu().numpy()
            RC.check_bytes(sheets.flows[k].cpu().numpy(), R.level(R.flow(flow)), RC.band("FLOW", flow), f"flow {k}")
    else:
        assert len(scene.calls) == 1 and sheets.flows is None and sheets.latents is None and sheets.blurry is None
    cam = camera_intrinsics(v.metadata)
    check_sheet(sheets.image, R.image_panels(case, r), None, f"{case} image")
    check_sheet(sheets.decomp, R.decomp_panels(case, r), cam, f"{case} decomp")


def test_two_launches_in_one_graph(hip_device):
    """Statistics and composition captured on one stream, replayed twice: the eager bytes, both times."""
    from mobgs_amd.scene_utils import compose_sheet
    H, W = 13, 17
    kinds = ("GREY_DIV_MAX", "ERROR", "FLOW", "NORMALS_FD", "RGB")
    panels = dev_panels([RC.source(k, H, W, 40 + i) for i, k in enumerate(kinds)], hip_device)
    cam = RC.camera(H, W)
    eager = compose_sheet(panels, H, W, camera=cam).clone()
    out = torch.zeros_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        compose_sheet(panels, H, W, camera=cam, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        compose_sheet(panels, H, W, camera=cam, out=out)
    for _ in range(2):
        out.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


# ---- the reference's own sheets ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ("test", "train", "train_blur"))
def test_fixture_of_the_references_sheets(hip_device, case):
    """tests/golden/report_sheets.npz: from the reference's own render outputs the kernels give the reference's own bytes,
    up to the one-level rule (both sides are fp32 evaluations of the same statements)."""
    fx = load("report_sheets")
    cam = tuple(float(c) for c in fx["cam"])
    H, W = fx["gt"].shape[-2:]
    r = {k: fx[f"{case}_{k}"] for k in ("render", "d_render", "s_render", "d_alpha", "depth")}
    r.update(gt=fx["gt"], gt_normal=fx["gt_normal"], gt_depth=fx["gt_depth"])
    if case == "train_blur":
        r["blurry"] = fx[f"{case}_blurry"]
    todo = [("image", R.image_panels(case, r)), ("decomp", R.decomp_panels(case, r))]
    if case == "train_blur":
        todo += [(f"latent_img_{k}", [("RGB", fx[f"{case}_latent_{k}"])]) for k in range(9)]
    for name, panels in todo:
        got = compose(panels, H, W, hip_device, cam).cpu().numpy()
        L = R.level(R.sheet(panels, cam))
        b = np.concatenate([RC.band(p[0], p[1], p[2] if len(p) > 2 else None, cam) for p in panels], axis=1)
        ref = fx[f"{case}_{name}"]
        RC.check_bytes(got, L, b, f"{case} {name}")
        free = ~RC.in_band(L, b)
        assert np.array_equal(got[free], ref[free]), f"{case} {name}: differs from the reference's bytes outside the bands"
    if case == "train_blur":                 # UNPINNED: these came out of the restatement, not out of flow_vis
        from mobgs_amd import flow_vis
        for k in (0, 4, 8):
            flow = fx[f"{case}_flow_{k}"]
            got = flow_vis.flow_to_color(torch.from_numpy(flow).to(hip_device)).cpu().numpy()
            RC.check_bytes(got, R.level(R.flow(flow)), RC.band("FLOW", flow), f"flow {k}")


# ---- files ------------------------------------------------------------------------------------------------------------
def test_render_training_image_writes_the_references_files(scene, tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image

    from mobgs_amd.scene_utils import render_training_image
    H, W = Scene.H, Scene.W
    model = types.SimpleNamespace(model_path=str(tmp_path))
    for is_train, blce, sub, n_image, n_decomp in ((False, None, "val", 6, 2), (True, scene.blce, "train", 4, 4)):
        written = render_training_image(model, scene.stat, scene.dyn, scene.views, scene.render, None, scene.bg, "fine", 300,
                                        75.0, "dycheck", is_train=is_train, blcekernel=blce)
        folder = tmp_path / "fine_render" / sub / "images"
        assert written == [str(folder / f"view{i}.jpg") for i in range(2)]
        assert (tmp_path / "fine_render" / "pointclouds").is_dir()
        expected = {f"view{i}{s}.jpg": n for i in range(2) for s, n in (("", n_image), ("_decomp", n_decomp))}
        if blce is not None:
            expected.update({f"view{i}_{kind}_{k:02d}.jpg": 1 for i in range(2) for kind in ("flow", "latent")
                             for k in range(9)})
        assert sorted(p.name for p in folder.iterdir()) == sorted(expected)
        for name, n in expected.items():
            with Image.open(folder / name) as im:
                assert im.size == (n * W, H) and im.mode == "RGB", name
    with pytest.raises(NotImplementedError):
        render_training_image(model, scene.stat, scene.dyn, scene.views, scene.render, None, scene.bg, "warm", 0, 0.0,
                              "dycheck")
