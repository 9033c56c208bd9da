"""CPU checks around tOF (include/mobgs_hip.h K25, mobgs_amd.metrics.temporal_of).  None of them rests on anyone's memory
of OpenCV: the grey arithmetic against numpy, crop_8x8 against the reference's statements, the pyramid's sizes written out,
the polynomial expansion on an exact quadratic, identical frames, and an analytically translated texture, which fixes the
axis order, the sign and the solve of tests/tof_restatement.py.  The host entry points of the built library are called
through ctypes; nothing here launches a kernel."""
import ctypes
import os

import numpy as np
import pytest

import tof_restatement as TR
from helpers import GOLDEN

# (H, W) -> [(width, height)] coarsest first, and the taps of the scales 1/8, 1/4, 1/2, 1
LEVEL_SIZES = {
    (50, 75): [(75, 50)],
    (72, 136): [(68, 36), (136, 72)],
    (259, 262): [(33, 32), (66, 65), (131, 130), (262, 259)],
    (288, 512): [(64, 36), (128, 72), (256, 144), (512, 288)],
    (1014, 1352): [(169, 127), (338, 254), (676, 507), (1352, 1014)],
}
TAPS = [19, 9, 3, 3]
SIGMAS = [3.5, 1.5, 0.5, 0.0]
# docs/MEASUREMENT_LOG.md, "The Farneback restatement on a translated texture": the largest |median flow - shift| the float64
# restatement shows over the two shifts and both channels at 262x259 is 6.3e-3 px; three times that is allowed
SHIFT_OBSERVED = 6.3e-3


def test_grey_round_trip_table():
    """All 256 values of k -> trunc(fl32(fl32(k / 255) * 255)) against numpy, formed as metrics.py:100, :109-110 form it."""
    k = np.arange(256)
    direct = ((np.float32(k.astype(np.uint8)) / 255) * 255.0)
    assert direct.dtype == np.float32
    want = direct.astype(np.uint8)
    got = TR.round_trip_table()
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    changed = k[want != k]
    print(f"[tof] 8-bit values the fp32 round trip changes: {changed.tolist()}")
    assert np.all((want == k) | (want == k - 1))
    # the quantisation of a prediction lands on the same fp32 values k / 255
    q = TR.quantize8((k + 0.5) / 255.0)
    assert np.array_equal(q, np.float32(k) / np.float32(255)) and np.array_equal(TR.to_uint8(q), want)


def test_rgb_to_grey_fixed_point():
    rgb = np.zeros((4, 3, 1, 1), np.uint8)
    rgb[0, :, 0, 0] = (255, 255, 255)
    rgb[1, :, 0, 0] = (255, 0, 0)
    rgb[2, :, 0, 0] = (0, 255, 0)
    rgb[3, :, 0, 0] = (0, 0, 255)
    assert TR.rgb_to_grey(rgb).reshape(-1).tolist() == [255, 76, 150, 29]
    assert 4899 + 9617 + 1868 == 1 << 14


def reference_crop(ori_h, ori_w):
    """metrics.py:32-47, its statements."""
    h = (ori_h // 32) * 32
    w = (ori_w // 32) * 32
    while (h > ori_h - 16):
        h = h - 32
    while (w > ori_w - 16):
        w = w - 32
    y = (ori_h - h) // 2
    x = (ori_w - w) // 2
    return y, x, h, w


def test_crop_8x8_sizes_48_to_1400():
    from mobgs_amd import metrics as M
    yxhw = (ctypes.c_int32 * 4)()
    from mobgs_amd import _lib
    lib = _lib.load()
    for n in range(48, 1401):
        other = 48 + (n * 7) % 1353
        want = reference_crop(n, other)
        assert TR.crop_window(n, other) == want
        assert lib.mobgs_tof_crop(n, other, ctypes.cast(yxhw, ctypes.c_void_p)) == 0 and tuple(yxhw) == want, (n, other)
        assert want[2] >= 32 and want[3] >= 32 and want[0] >= 8 and want[1] >= 8
    assert M.crop_window(1014, 1352) == (11, 20, 992, 1312)
    img = np.arange(50 * 75 * 2).reshape(50, 75, 2)
    win, y, x = M.crop_8x8(img)
    assert (y, x) == (9, 21) and win.shape == (32, 32, 2) and np.array_equal(win, TR.crop_8x8(img))
    assert lib.mobgs_tof_crop(47, 100, ctypes.cast(yxhw, ctypes.c_void_p)) != 0
    with pytest.raises(ValueError, match="crop_8x8"):
        M.crop_8x8(np.zeros((47, 100)))


def test_levels_through_the_library():
    from mobgs_amd import _lib
    lib = _lib.load()
    out = (_lib.MobgsTofLevel * 4)()
    for (H, W), sizes in LEVEL_SIZES.items():
        n = lib.mobgs_tof_levels(H, W, ctypes.cast(out, ctypes.c_void_p))
        assert n == len(sizes), (H, W)
        got = [(out[i].width, out[i].height) for i in range(n)]
        assert got == sizes, (H, W)
        assert [out[i].taps for i in range(n)] == TAPS[4 - n:] and [out[i].sigma for i in range(n)] == SIGMAS[4 - n:]
        assert [(w, h, t, s) for w, h, t, s in TR.levels(H, W)] == [(w, h, t, s) for (w, h), t, s in
                                                                   zip(sizes, TAPS[4 - n:], SIGMAS[4 - n:])]
    assert lib.mobgs_tof_levels(47, 512, ctypes.cast(out, ctypes.c_void_p)) == 0
    assert lib.mobgs_tof_levels(288, 512, None) == 0


def test_size_queries_and_refusals_without_a_device():
    from mobgs_amd import _lib
    lib = _lib.load()
    assert lib.mobgs_tof_scratch_bytes(1, 288, 512) == 0 and lib.mobgs_tof_scratch_bytes(3, 47, 512) == 0
    assert lib.mobgs_tof_scratch_bytes(3, 288, 1 << 15) == 0 and lib.mobgs_tof_score_scratch_doubles(0, 288, 512) == 0
    H, W, F = 288, 512, 24
    plane = H * W
    want = 4 * plane * (F + 5 * F + 2 * 5 * (F - 1)) + 2 * 8 * (F - 1) * 256 * 144
    got = lib.mobgs_tof_scratch_bytes(F, H, W)
    assert want <= got <= want + 6 * 256 and got % 256 == 0
    assert lib.mobgs_tof_score_scratch_doubles(23, H, W) == 23 * 2 * -(-(256 * 480) // 2048)
    # every refusal comes before any launch: none of these touches a device
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 2)
    level = _lib.MobgsTofLevel(256, 144, 3, 0.5)
    lp = ctypes.cast(ctypes.pointer(level), ctypes.c_void_p)
    refused = [
        lib.mobgs_tof_flow(1, H, W, p, p, p, None), lib.mobgs_tof_flow(3, 40, W, p, p, p, None),
        lib.mobgs_tof_flow(3, H, W, None, p, p, None), lib.mobgs_tof_flow(3, H, W, p, None, p, None),
        lib.mobgs_tof_flow(3, H, W, p, p, odd, None), lib.mobgs_tof_grey(2, H, W, None, 0, p, None),
        lib.mobgs_tof_grey(2, H, W, p, 4, p, None), lib.mobgs_tof_grey(0, H, W, p, 0, p, None),
        lib.mobgs_tof_pyramid_level(2, H, W, p, None, p, None), lib.mobgs_tof_pyramid_level(2, H, W, odd, lp, p, None),
        lib.mobgs_tof_polyexp(2, 1, 64, p, p, None), lib.mobgs_tof_polyexp(2, 64, 64, p, None, None),
        lib.mobgs_tof_update_matrices(1, 36, 64, None, None, 0, 0, None, p, None),
        lib.mobgs_tof_update_matrices(1, 36, 64, p, p, 72, 128, None, p, None),
        lib.mobgs_tof_blur_solve(1, 36, 64, p, p, None, p, None), lib.mobgs_tof_blur_solve(1, 36, 64, None, p, None, None, None),
        lib.mobgs_tof_score(1, H, W, p, None, None, p, p, None), lib.mobgs_tof_score(1, 40, W, p, p, None, p, p, None),
        lib.mobgs_tof_score(1, H, W, p, p, None, ctypes.c_void_p(p.value + 4), p, None),
    ]
    assert all(rc == _lib._DEFINES["MOBGS_E_INVALID"] for rc in refused), refused
    for bad in ((256, 144, 4, 0.5), (256, 144, 21, 0.5), (256, 144, 5, 0.0), (1024, 144, 3, 0.5), (256, 144, 3, -1.0)):
        level = _lib.MobgsTofLevel(*bad)
        lp = ctypes.cast(ctypes.pointer(level), ctypes.c_void_p)
        assert lib.mobgs_tof_pyramid_level(2, H, W, p, lp, p, None) == _lib._DEFINES["MOBGS_E_INVALID"], bad
    assert b"mobgs_tof_pyramid_level" in lib.mobgs_last_error()


def test_polynomial_expansion_of_an_exact_quadratic():
    h, w = 37, 45
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    for c in ((3.0, 0.5, -0.25, 0.01, -0.02, 0.015), (100.0, -2.0, 1.0, 0.0, 0.03, -0.01), (7.0, 0.0, 0.0, 0.0, 0.0, 0.0)):
        img = c[0] + c[1] * xs + c[2] * ys + c[3] * xs * xs + c[4] * ys * ys + c[5] * xs * ys
        want = np.stack([c[1] + 2 * c[3] * xs + c[5] * ys, c[2] + 2 * c[4] * ys + c[5] * xs, np.full_like(xs, c[3]),
                         np.full_like(xs, c[4]), np.full_like(xs, c[5])])
        got = TR.poly_exp(img)
        err = np.abs(got - want)[:, 5:-5, 5:-5].max()
        print(f"[tof] polynomial expansion of an exact quadratic {c}: largest error {err:.2e} (allowed 1e-9)")
        assert got.shape == (5, h, w) and err <= 1e-9


def test_stage_pieces_of_the_restatement():
    # the resize is the identity at equal sizes and exact on a linear ramp away from the clamped ends
    a = np.random.default_rng(0).normal(size=(9, 11))
    assert np.array_equal(TR.resize_bilinear(a, 9, 11), a)
    ramp = np.arange(20.0)[None, :].repeat(4, 0)
    up = TR.resize_bilinear(ramp, 4, 40)
    assert np.allclose(up[0, 1:-1], (np.arange(40)[1:-1] + 0.5) / 2 - 0.5, atol=1e-12) and up[0, 0] == 0 and up[0, -1] == 19
    # reflect-101 and replicate borders
    assert TR.correlate_axis(np.array([[1.0, 2.0, 4.0]]), np.array([1.0, 0.0, 0.0]), 1, "reflect").tolist() == [[2.0, 1.0, 2.0]]
    assert TR.correlate_axis(np.array([[1.0, 2.0, 4.0]]), np.array([1.0, 0.0, 0.0]), 1, "edge").tolist() == [[1.0, 1.0, 2.0]]
    for taps, sigma in zip(TAPS, SIGMAS):
        g = TR.gaussian_taps(taps, sigma)
        assert len(g) == taps and abs(g.sum() - 1) < 1e-15 and np.array_equal(g, g[::-1])
    # the border factor: the product of the four sides
    s = TR.border_factor(12, 30)
    assert s[6, 15] == 1 and s[0, 15] == 0.14 and s[6, 2] == 0.4472 and abs(s[0, 29] - 0.14 * 0.14) < 1e-18
    assert abs(TR.border_factor(8, 30)[3, 15] - 0.4472 * 0.4472) < 1e-18      # both sides of a narrow image
    # a flow that leaves the image takes the out-of-bounds arm: no sample of R1 enters
    rng = np.random.default_rng(1)
    R0, R1 = rng.normal(size=(5, 12, 14)), rng.normal(size=(5, 12, 14))
    out = np.full((12, 14, 2), 40.0)
    assert np.array_equal(TR.update_matrices(R0, R1, out), TR.update_matrices(R0, 7 * R1, out))
    assert TR.near_bounds_test(np.zeros((12, 14, 2))).sum() == 2 * 12 + 2 * 14 - 4


def test_identical_frames():
    """With equal frames and a zero flow every in-bounds pixel has b = (R0 - S) / 2 = 0 exactly, so its h is 0 and the flow
    stays exactly 0 -- wherever no window reaches the last row or column, whose pixels take the OUT-of-bounds arm
    (floor(x + 0) = w - 1 is not < w - 1) and so carry b = R0 / 2.  Three rounds of a 15x15 window reach 21 pixels; a finer
    level inherits the coarser one's.  Hence: exactly 0 outside that margin on a one-level image, a flat image exactly
    flat, and tOF exactly 0 for equal sequences at all four levels."""
    a = TR.texture(50, 75, 5)
    assert len(TR.levels(50, 75)) == 1
    flow = TR.farneback(a, a)
    assert np.all(flow[:50 - 22, :75 - 22] == 0.0)
    assert np.abs(flow).max() > 1e-3                                # (the margin is NOT zero: that is the algorithm)
    b, c = TR.texture(259, 262, 7), TR.texture(259, 262, 7, shift=(2.0, 1.0))
    assert len(TR.levels(259, 262)) == 4 and TR.get_tOF(b, c, b, c) == 0.0
    moved = TR.farneback(b, c)
    assert TR.score(moved, moved, mask=(np.arange(259 * 262).reshape(259, 262) % 3 == 0)) == 0.0
    assert TR.score(moved, np.zeros_like(moved)) > 0.5


@pytest.mark.parametrize("shift", [(1.5, -0.75), (6.0, 3.0)])
def test_translated_texture(shift):
    """A band-limited texture (12 sinusoids, periods 8 to 64 px, 8-bit) and the same texture evaluated at (x - sx, y - sy):
    the median flow over the cropped interior is the shift, channel 0 = x = columns, prev to next.  If this fails the
    restatement is wrong, and no kernel may be fitted to it."""
    H, W = 259, 262
    prev, nxt = TR.texture(H, W, 3), TR.texture(H, W, 3, shift=shift)
    assert prev.min() >= 0 and prev.max() <= 255 and np.array_equal(prev, np.rint(prev)) and prev.std() > 20
    flow = TR.crop_8x8(TR.farneback(prev, nxt))
    med = np.median(flow.reshape(-1, 2), 0)
    err = np.abs(med - np.array(shift))
    print(f"[tof] shift {shift}: median flow {med.tolist()}, error {err.tolist()} px (allowed {3 * SHIFT_OBSERVED:.2e})")
    assert err.max() <= 3 * SHIFT_OBSERVED


def test_update_test_flows_stay_under_the_cap():
    """The flows the GPU test of the update matrices uses: about 10 % of the samples out of bounds, and at most 1 % of the
    pixels within 1e-3 px of the in-bounds test's jump (those may be left out of the comparison there)."""
    for h, w in ((50, 75), (72, 136), (259, 262)):
        flows = TR.update_test_flows(h, w)
        share = np.mean([TR.out_of_bounds_share(f) for f in flows])
        near = np.mean([TR.near_bounds_test(f).mean() for f in flows])
        print(f"[tof] update test flows {w}x{h}: {share:.1%} out of bounds, {near:.3%} within 1e-3 px of the jump")
        assert 0.05 <= share <= 0.2 and near <= 0.01


def test_score_follows_the_reference_statements():
    rng = np.random.default_rng(2)
    fa, fb = rng.normal(size=(72, 136, 2)).astype(np.float32), rng.normal(size=(72, 136, 2)).astype(np.float32)
    mask = (rng.uniform(size=(72, 136, 1)) < 0.4).astype(np.float64)
    y, x, h, w = reference_crop(72, 136)
    diff = np.absolute(fa.astype(np.float64) - fb.astype(np.float64))[y:y + h, x:x + w]
    norm = np.sqrt(np.sum(diff * diff, axis=-1))
    m = mask.squeeze()[y:y + h, x:x + w]
    assert abs(TR.score(fa, fb) - norm.mean()) <= 1e-14
    assert abs(TR.score(fa, fb, mask.squeeze()) - (norm * m).sum() / m.sum()) <= 1e-14


def test_opencv_vectors():
    """Present only after scripts/dump_tof_vectors.py ran where OpenCV is installed; skipped otherwise (README, "UNPINNED")."""
    path = os.path.join(GOLDEN, "tof_external", "farneback.npz")
    if not os.path.exists(path):
        pytest.skip("no tests/golden/tof_external/farneback.npz (scripts/dump_tof_vectors.py): UNPINNED")
    ex = dict(np.load(path))
    assert np.array_equal(TR.rgb_to_grey(ex["rgb"]), ex["grey"])
    for pre in (k[:-4] for k in ex if k.endswith("prev")):               # "" (262x259), "75x50_", "136x72_"
        for i in range(len(ex[pre + "prev"])):
            got = TR.farneback(ex[pre + "prev"][i].astype(np.float64), ex[pre + "next"][i].astype(np.float64))
            want = ex[pre + "flow"][i].astype(np.float64)
            # OpenCV works in fp32: 1e-3 of the largest flow covers its rounding through four levels; a wrong border
            # mode, table entry or level count shows as 1e-1 and more
            assert np.abs(got - want).max() <= 1e-3 * max(1.0, np.abs(want).max()), (pre, i)
