"""The Farneback kernels on the MI355X (csrc/tof.hip through the C ABI of include/mobgs_hip.h K25 and mobgs_amd.metrics) on
the cases of tests/tof_cases.py: every stage at the level shapes and contents where tiles, windows and border bands meet,
element by element against float64 under bounds that come from the arithmetic (k <= 3 of C[stage] 2^-23 T_i, per stratum,
no pixel excused; tests/test_tof_cases_cpu.py measures C on the fp32 twin of the restatement), the facts that need no
tolerance bit for bit, the whole flow and tOF at shapes and seeds whose sample positions stay clear of the in-bounds test's
jump, and the score at the block counts the workload has (two and three partial sums per thread of the finishing kernel).
tests/test_gpu_tof.py keeps the relative-to-maximum checks this one is read beside; its end-to-end tolerance is imported."""
import ctypes

import numpy as np
import pytest
import torch

import tof_cases as TC
import tof_restatement as TR
from helpers import same_bits
from test_gpu_tof import allowed, call, level_record, rel_err

pytestmark = pytest.mark.gpu

NAN = float("nan")
SCORE_SIZES = {"752x752": (752, 752, 265, 2), "1352x1014": (1014, 1352, 636, 3)}     # H, W, blocks, partial sums per thread
SCORE_THREADS, SCORE_PER_BLOCK = 256, 2048


@pytest.fixture(scope="module")
def lib():
    from mobgs_amd import _lib
    return _lib.load(build_if_missing=False)


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def update(lib, device, R, flow, sh, sw, want_used=True):
    """mobgs_tof_update_matrices on R [2,5,h,w] (one pair) -> (M [1,5,h,w], the flow it used [1,h,w,2] or None)."""
    h, w = R.shape[-2:]
    M = torch.full((1, 5, h, w), NAN, device=device)
    used = torch.full((1, h, w, 2), NAN, device=device) if want_used else None
    call(lib, "mobgs_tof_update_matrices", 1, h, w, R, flow, sh, sw, used, M)
    return M, used


@pytest.mark.parametrize("kind", TC.CONTENTS)
@pytest.mark.parametrize("shape", TC.SHAPES)
def test_stage_kernels(shape, kind, lib, hip_device):
    c = TC.stage_case(shape, kind)
    h, w = c.h, c.w
    if c.image:
        H, W = c.image
        grey = dev(c.stage["pyramid"].inp, hip_device)
        out = torch.full((2, h, w), NAN, device=hip_device)
        rec = level_record(c.level)
        call(lib, "mobgs_tof_pyramid_level", 2, H, W, grey, ctypes.cast(ctypes.pointer(rec), ctypes.c_void_p), out)
        TC.compare(c, "pyramid", out.cpu().numpy(), "kernel")
        # the finest level (sigma 0) equals float64 exactly: every intermediate is a multiple of 1/16 below 256
        finest = TR.levels(H, W)[-1]
        full = torch.full((2, H, W), NAN, device=hip_device)
        rec = level_record(finest)
        call(lib, "mobgs_tof_pyramid_level", 2, H, W, grey, ctypes.cast(ctypes.pointer(rec), ctypes.c_void_p), full)
        assert np.array_equal(full.cpu().numpy().astype(np.float64), np.stack([TR.pyramid_level(g, finest) for g in c.grey]))
    # polynomial expansion
    R_out = torch.full((2, 5, h, w), NAN, device=hip_device)
    call(lib, "mobgs_tof_polyexp", 2, h, w, dev(c.stage["polyexp"].inp, hip_device), R_out)
    TC.compare(c, "polyexp", R_out.cpu().numpy(), "kernel")
    # update matrices of a flow of the level's own size: it is used as given, and no pixel is excused
    R32, flow32 = c.stage["update"].inp
    R, flow = dev(R32, hip_device), dev(flow32, hip_device)
    M, used = update(lib, hip_device, R, flow, h, w)
    assert same_bits(used, flow)
    TC.compare(c, "update", M.cpu().numpy(), "kernel", T=c.stage["update"].T_exact)     # (no position rounding granted)
    # ... and of the coarser level's flow: the upsampled flow, then the matrices of exactly that flow
    coarse = c.stage["upsample"].inp
    M_up, used = update(lib, hip_device, R, dev(coarse, hip_device), coarse.shape[1], coarse.shape[2])
    TC.compare(c, "upsample", used.cpu().numpy(), "kernel")
    again, _ = update(lib, hip_device, R, used, h, w, want_used=False)
    assert same_bits(M_up, again)
    used32, R64 = used.cpu().numpy()[0], R32.astype(np.float64)
    TC.compare(c, "update", M_up.cpu().numpy(), "kernel (upsampled flow)",
               ref=TR.update_matrices(R64[0], R64[1], used32)[None], T=TR.update_terms(R64[0], R64[1], used32, position=False)[None])
    # box mean and solve, plain and fused with the next update
    M32, _ = c.stage["solve"].inp
    M_in = dev(M32, hip_device)
    solved = torch.full((1, h, w, 2), NAN, device=hip_device)
    call(lib, "mobgs_tof_blur_solve", 1, h, w, M_in, solved, None, None)
    TC.compare(c, "solve", solved.cpu().numpy(), "kernel")
    solved2, M_out = torch.full_like(solved, NAN), torch.full_like(M_in, NAN)
    call(lib, "mobgs_tof_blur_solve", 1, h, w, M_in, solved2, R, M_out)
    separate, _ = update(lib, hip_device, R, solved, h, w, want_used=False)
    assert same_bits(solved, solved2) and same_bits(M_out, separate)


@pytest.mark.parametrize("shape", ["48x48", "49x65"])
def test_flat_half_is_exactly_zero(shape, lib, hip_device):
    """The flat half of const_half, through the kernels' own outputs: the expansion is exactly 0 in every tile whose patch
    is flat (tests/tof_cases.exact_zero_regions: the fact holds per tile, not per window -- in a tile whose patch reaches
    the textured half the flat pixels carry coefficients of up to 1.4e-6 (docs/MEASUREMENT_LOG.md), which the comparator
    of test_stage_kernels bounds), and from those coefficients the update matrices and the flow are exactly 0 too."""
    c = TC.stage_case(shape, "const_half")
    h, w = c.h, c.w
    flow_in = TR.smooth_flow(h, w, seed=3, amplitude=0.5)[None]          # at most 1 px: the taps reach two columns
    regions = TC.exact_zero_regions(c, flow_in[0])
    assert all(m.any() for m in regions.values()) and 0.5 < np.abs(flow_in).max() <= 1.0
    R = torch.full((2, 5, h, w), NAN, device=hip_device)
    call(lib, "mobgs_tof_polyexp", 2, h, w, dev(c.stage["polyexp"].inp, hip_device), R)
    got = R.cpu().numpy()
    window = TC.case_strata(c, "polyexp")["const"] & ~regions["polyexp"]
    print(f"[tof] flat half {shape}: largest coefficient where the window is flat but the tile's patch is not: "
          f"{np.abs(got[..., window]).max() if window.any() else 0.0:.2e} ({int(window.sum())} px)")
    assert np.all(got[..., regions["polyexp"]] == 0) and np.abs(got).max() > 1e-2
    M, _ = update(lib, hip_device, R, dev(flow_in, hip_device), h, w)
    assert np.all(M.cpu().numpy()[..., regions["update"]] == 0)
    flow, M2 = torch.full((1, h, w, 2), NAN, device=hip_device), torch.full_like(M, NAN)
    call(lib, "mobgs_tof_blur_solve", 1, h, w, M, flow, R, M2)
    got = flow.cpu().numpy()
    assert np.isfinite(got).all() and np.all(TC.planes(got)[..., regions["solve"]] == 0) and np.abs(got).max() > 1e-2
    print(f"[tof] flat half {shape}: exact zeros over {int(regions['polyexp'].sum())} / {int(regions['update'].sum())} / "
          f"{int(regions['solve'].sum())} px of the expansion / matrices / flow")


@pytest.mark.parametrize("name", list(TC.END_TO_END))
def test_flow_and_tof_end_to_end(name, lib, hip_device):
    """Whole flows at seeds whose float64 trace keeps every sample position clear of the in-bounds test's jump
    (tests/test_tof_cases_cpu.py::test_kink_margins), under the tolerance of tests/test_gpu_tof.py."""
    from mobgs_amd.metrics import TofTarget, farneback_flow, grey_frames, temporal_of
    rgb, grey = TC.frames(name)
    want, _ = TC.flow_trace(name)
    g = dev(grey.astype(np.float32), hip_device)
    flow = farneback_flow(g)
    err = rel_err(flow.cpu().numpy(), want)
    print(f"[tof] flow {name} end to end: largest flow {np.abs(want).max():.3f} px, relative error {err:.2e} "
          f"(allowed {allowed('flow'):.2e})")
    assert np.abs(want).max() > 1.0 and err <= allowed("flow")
    assert same_bits(flow, farneback_flow(g))
    frames = dev(rgb, hip_device)
    assert np.array_equal(grey_frames(frames).cpu().numpy().astype(np.float64), grey)
    # tOF against the same flows reversed in sign: every flow that is compared is one of the vetted trace
    got = temporal_of(frames, TofTarget(-flow))
    want_tof = np.array([TR.score(-f, f) for f in want])
    e = float(np.abs(got.cpu().numpy() - want_tof).max() / np.abs(want_tof).max())
    print(f"[tof] tOF {name}: {got.tolist()}, float64 {want_tof.tolist()}, relative error {e:.2e} "
          f"(allowed {allowed('tof'):.2e})")
    assert want_tof.min() > 0.1 and e <= allowed("tof")


@pytest.mark.parametrize("size", list(SCORE_SIZES))
def test_score_at_real_block_counts(size, lib, hip_device):
    """tof_score_finish_kernel gives each of its 256 threads ceil(blocks / 256) partial sums: 2 at 752x752 (thread 132 holds
    a single one, the threads after it none), 3 at 1352x1014 (thread 212 starts at r0 = blocks).  Plain and with a mask
    that is zero over the whole first block and the crop's last row."""
    from mobgs_amd.metrics import flow_distance
    H, W, blocks, per = SCORE_SIZES[size]
    cy, cx, ch, cw = TR.crop_window(H, W)
    assert -(-ch * cw // SCORE_PER_BLOCK) == blocks and -(-blocks // SCORE_THREADS) == per
    assert int(lib.mobgs_tof_score_scratch_doubles(1, H, W)) == 2 * blocks
    assert (blocks % per == 1) if per == 2 else ((SCORE_THREADS - 1) * per > blocks and blocks % per == 0)
    rng = np.random.default_rng(H)
    fa = (rng.normal(size=(1, H, W, 2)) * 3.0).astype(np.float32)
    fb = (fa + rng.normal(size=fa.shape) * 0.3).astype(np.float32)
    mask = rng.uniform(0.0, 1.0, size=(1, H, W)).astype(np.float32)
    window = mask[0, cy:cy + ch, cx:cx + cw].copy()
    window.reshape(-1)[:SCORE_PER_BLOCK] = 0.0                        # the whole first workgroup: its sums are exactly 0
    window[ch - 1] = 0.0
    mask[0, cy:cy + ch, cx:cx + cw] = window
    a, b, m = (dev(t, hip_device) for t in (fa, fb, mask))
    bound = 8 * 2.0 ** -53 * np.sqrt(blocks)
    for what, mk, mt in (("no mask", None, None), ("mask", mask[0], m)):
        got = flow_distance(a, b, mt)
        want = TR.score(fa[0], fb[0], mk)
        err = abs(float(got[0]) - want) / abs(want)
        print(f"[tof] score {size} ({blocks} blocks, {per} per thread) {what}: {float(got[0])!r}, float64 {want!r}, relative "
              f"error {err:.2e} (allowed {bound:.2e})")
        assert got.dtype == torch.float64 and got.shape == (1,) and err <= bound
        assert same_bits(got, flow_distance(a, b, mt))
    assert torch.equal(flow_distance(a, a), torch.zeros(1, dtype=torch.float64, device=hip_device))
    assert torch.equal(flow_distance(a, a, m), torch.zeros(1, dtype=torch.float64, device=hip_device))
