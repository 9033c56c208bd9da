"""tests/deform_cases.py checked from the oracle alone (no GPU): every case keeps its near-kink filter under the 5 % cap,
reaches the edge it is named after, and the comparator at its widest (k = 8) notices one missing row and one missing
64-row tile in the weight and plane gradients."""
import pytest
import torch

import deform_cases as C


@pytest.mark.parametrize("name", C.HEX_CASES)
def test_hexplane_case_filter_and_size(name):
    case = C.hex_case(name)
    print(f"HexPlane {name}: N {case.N}, dropped {case.dropped:.2%} of the candidates")
    assert case.dropped <= C.MAX_DROP
    assert case.pts.shape == (case.N, 3) and case.times.shape == (case.N, 1) and case.cot.shape == (case.N, 96)
    assert [tuple(p.shape) for p in case.planes] == C.plane_shapes(case.base)
    assert all(p.is_contiguous(memory_format=torch.channels_last) for p in case.planes)
    if name != "border":
        assert not C.hex_near_kink(case.pts, case.times, case.aabb, case.base).any()


@pytest.mark.parametrize("name", C.MLP_CASES)
def test_mlp_case_filter_and_size(name):
    case = C.mlp_case(name)
    print(f"MLP {name}: N {case.N}, dropped {case.dropped:.2%} of the candidates")
    assert case.dropped <= C.MAX_DROP
    assert case.feat.shape == (case.N, 96) and [c.shape[0] for c in case.cots] == [case.N] * 3
    assert not C.mlp_near_kink(case.feat, case.W)[0].any()


def test_sizes_cover_the_tile_and_block_edges():
    assert C.HEX_SIZES == (0, 1, 2, 3, 31, 33, 511, 512, 513, 1025)
    assert C.MLP_SIZES == (0, 1, 63, 64, 65, 127, 128)
    q = C.normalised(*(getattr(C.hex_case("n1025"), k) for k in ("pts", "times", "aabb")))
    outside = float((q[:, :3].abs() > 1).any(dim=1).double().mean())
    print(f"n1025: {outside:.1%} of the points outside the box")
    assert 0.02 <= outside <= 0.10
    assert float(q[:, 3].abs().max()) > 1.0  # some times beyond the time planes


def test_border_rows_are_exact_and_reach_every_border():
    case = C.hex_case("border")
    q = C.normalised(case.pts, case.times, case.aabb)
    assert torch.equal(q * 16, (q * 16).round())  # at most 4 fractional bits
    a = case.aabb
    q32 = torch.cat([(case.pts - a[0]) * (2.0 / (a[1] - a[0])) - 1.0, case.times], dim=1)  # the kernels' fp32 statements
    assert torch.equal(q32.double(), q)
    for axis in range(4):
        for m in (C.MULTIRES if axis < 3 else (1,)):
            r = case.base[axis] * m
            assert torch.equal(C.grid_coordinate(q32[:, axis], r).double(), C.grid_coordinate(q[:, axis], r))
    v = q[:, :3]
    for axis in range(3):
        for s in (-1.0, 1.0):
            assert (v[:, axis] == s).any() and (s * v[:, axis] > 1).any()  # on the face, outside on that side
    on = (v.abs() == 1).sum(dim=1)
    assert (on == 3).sum() == 8 and (on == 2).any() and (on == 1).any()  # corners, edges, faces
    assert set(case.times.reshape(-1).tolist()) == {-1.0, 1.0, 1.5, -1.5, 0.0, 0.25}
    # what the GPU test then demands bit for bit: no gradient through a clipped axis or a time on / beyond the border
    ref64, _ = C.hex_reference("border")
    assert torch.equal(ref64["v_pts"] == 0, v.abs() >= 1)
    assert torch.equal(ref64["v_times"] == 0, q[:, 3:].abs() >= 1)


def test_pileup_runs_exceed_one_slice_and_span_two_workgroups():
    case = C.hex_case("pileup")
    cells = C.hex_cells(case)
    for p in range(18):
        run = int(torch.bincount(cells[:, p]).max())
        assert run > 64, (p, run)
        assert run == case.N == 600  # one cell per plane: 10 slices of 64 entries
        assert cells[0, p] == cells[512, p]  # the rows of both 512-point workgroups meet in it
    assert C.hot_cells(case.base) <= C.HOT_MAX
    assert float(case.times.min()) == float(case.times.max())


def test_hot_table_edges():
    assert C.hot_cells(C.hex_case("hot_full").base) == 73 * 336 <= C.HOT_MAX
    assert C.hot_cells(C.hex_case("cold").base) == 74 * 336 > C.HOT_MAX
    ref = C.hex_case("cold_ref")
    assert C.hot_cells(ref.base) == 33600 > C.HOT_MAX and ref.N == 1025
    assert float(ref.times.min()) == float(ref.times.max())
    for name in ("n513", "border"):
        assert C.hot_cells(C.hex_case(name).base) <= C.HOT_MAX


def test_clamp_case_clamps():
    case = C.mlp_case("clamp")
    assert case.N == 130 and case.W["scl_b2"].tolist() == [6.0, -6.0, 0.0]
    out = case.ds.abs() > C.LOG100
    share = float(out.any(dim=1).double().mean())
    print(f"clamp: {share:.1%} of the rows clamp a channel; per channel {out.double().mean(dim=0).tolist()}")
    assert share >= 0.9
    assert (~out).any(dim=1).all()  # every row keeps a channel strictly inside
    assert not out[:, 2].any() and (case.ds[:, 0] > 0).all() and (case.ds[:, 1] < 0).all()
    # channels that clamp in every row get no cotangent at all: their weight gradients are exactly 0 in the reference
    ref64, _ = C.mlp_reference("clamp")
    for ch in range(3):
        if out[:, ch].all():
            assert not ref64["scl_w2"][ch].any() and ref64["scl_b2"][ch] == 0
    assert ref64["scl_w2"][2].any()
    assert torch.equal(ref64["g_scales"], case.cots[1].double())
    for name in C.MLP_CASES:  # everywhere else the clamp is idle
        if name != "clamp":
            assert not (C.mlp_case(name).ds.abs() > C.LOG100).any()


def test_parked_case_walks_second_tiles_and_ends_on_one_row():
    n = C.mlp_case("parked").N
    assert -(-n // 64) > 256 and n % 64 == 1


def _rejected(got, ref64, ref32, what):
    try:
        C.close_to_f64(got, ref64, ref32, 8, what)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("missing", ["last row", "rows 64..127"])
def test_comparator_notices_missing_rows(missing):
    """A result that lacks one row, or one 64-row tile, is outside the bound at the widest k the GPU tests may use."""
    for kind, name, evaluate, reference, tensors in (
            ("MLP", "n128", C.mlp_eval, C.mlp_reference, C.W_KEYS),
            ("HexPlane", "n513", C.hex_eval, C.hex_reference, [f"plane{i}" for i in range(18)])):
        case = (C.mlp_case if kind == "MLP" else C.hex_case)(name)
        rows = torch.arange(case.N)
        keep = rows[:-1] if missing == "last row" else rows[(rows < 64) | (rows >= 128)]
        ref64, ref32 = reference(name)
        short = evaluate(case, torch.float64, keep)
        for t in tensors:
            assert _rejected(short[t], ref64[t], ref32[t], f"{kind} {name} {t} without {missing}"), (kind, t)
            C.close_to_f64(ref32[t], ref64[t], ref32[t], 1, f"{kind} {name} {t} fp32 reference")  # and accepts the honest one
