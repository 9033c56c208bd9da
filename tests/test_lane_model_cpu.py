"""The yardstick of tests/test_gpu_lane_primitives.py, checked without a GPU: the CPU model of wave_shared.h and
reduce_shared.h gives exact totals and the documented placement on the counting and placement vectors, its order-sensitive
inputs do separate the documented order from the left-to-right sum and from the other pairing tree, the comparison the
GPU test asserts with reports each planted defect, and mobgs_lane_probe refuses bad arguments before any launch."""
import ctypes

import numpy as np
import pytest

import lane_model as M

F32, F64, I32 = np.float32, np.float64, np.int32


def _exact(vectors, span):
    """The totals of each `span` consecutive lanes, in float64 (exact for the counting vectors), repeated to every lane."""
    t = vectors.astype(np.float64).reshape(len(vectors), -1, span).sum(-1, keepdims=True)
    return np.broadcast_to(t, t.shape[:2] + (span,)).reshape(vectors.shape)


@pytest.mark.parametrize("fn,dtype,span", [(M.wave_sum, F32, 64), (M.wave_sum, F64, 64), (M.wave_sum, I32, 64),
                                           (M.row_allreduce, F32, 16), (M.half_wave_sum, F32, 32),
                                           (M.wave_allreduce, F32, 64)], ids=lambda p: getattr(p, "__name__", str(p)))
def test_counting_vectors_give_the_exact_total_in_every_lane(fn, dtype, span):
    v = M.counting(dtype)
    out = fn(v)
    assert out.dtype == v.dtype and np.array_equal(out.astype(np.float64), _exact(v, span))


def test_min_max_of_the_counting_vectors_and_the_specials():
    for dtype in (F32, I32):
        v = M.counting(dtype)
        assert np.array_equal(M.wave_min(v), np.broadcast_to(v.min(-1, keepdims=True), v.shape))
        assert np.array_equal(M.wave_max(v), np.broadcast_to(v.max(-1, keepdims=True), v.shape))
    s = M.specials(I32)
    assert M.wave_min(s)[0, 0] == -2**31 and M.wave_max(s)[0, 0] == 2**31 - 1 and M.wave_max(s)[2, 0] == -2**31
    s = M.specials(F32)
    lo, hi = M.wave_min(s)[:, 0], M.wave_max(s)[:, 0]
    assert np.signbit(lo[1]) and not np.signbit(hi[1]) and np.signbit(lo[2]) and not np.signbit(hi[2])   # -0 < +0
    assert np.signbit(hi[0]) and hi[3] == np.inf and lo[4] == -np.inf
    assert lo[6] == -20.0 and hi[6] == 43.0                      # a NaN loses against a number (fminf / fmaxf)
    assert np.isnan(M.wave_sum(s)[5]).all() and np.isnan(M.wave_sum(s)[6]).all()
    assert M.wave_sum(s)[7, 0] == np.finfo(F32).smallest_subnormal * 2080 and np.signbit(M.wave_sum(s)[0]).all()


def test_dpp_lane_maps_and_single_steps():
    for ctrl, src in M.DPP_SRC.items():
        assert sorted(src) == list(range(64)) and np.array_equal(src >> 4, M.LANES >> 4), hex(ctrl)   # a permutation of each row
    assert np.array_equal(M.dpp_mov(M.dpp_mov(M.LANES, 0x141), 0x1B), M.LANES ^ 4)                # isect.hip's lane ^ 4
    assert np.array_equal(M.DPP_SRC[0x128], M.LANES ^ 8) and M.DPP_SRC[0x124][0] == 12 and M.DPP_SRC[0x124][21] == 17
    lanes = M.LANES.astype(F32)
    assert np.array_equal(M.dpp_add_xor4(lanes), lanes + (M.LANES ^ 4))
    minus = np.full(64, -0.0, F32)
    assert not np.signbit(M.dpp_add_xor4(minus)).any()          # v + (up + dn) = -0 + (-0 + +0) = +0, as written
    assert np.signbit(M.dpp_add(minus, 0xB1)).all()


@pytest.mark.parametrize("nvp", M.NVPS)
def test_component_placement(nvp):
    """Register k of every lane of row r holds the total of component (r >> 1) NVP/2 + (r & 1) NVP/4 + k."""
    x = M.placement(nvp)
    y = M.wave_reduce_components(x.transpose(0, 2, 1)).transpose(0, 2, 1)          # (G, 64, nvp / 4)
    assert y.shape == (len(x), 64, nvp // 4)
    weights = x[:4, :, 0].astype(np.float64).sum(1)             # the sum of the lanes' powers of two: 240, 240, 240, 96
    assert weights.tolist() == [240.0, 240.0, 240.0, 96.0] and weights.max() * nvp < 2**24
    for lane in range(64):
        r = lane >> 4
        for k in range(nvp // 4):
            c = M.component_of(nvp, r, k)
            assert c == (lane >> 5) * (nvp // 2) + ((lane >> 4) & 1) * (nvp // 4) + k      # the store's `base + k`
            assert (y[:4, lane, k] == weights * (c + 1)).all() and (y[4:, lane, k] == c + 1).all(), (lane, k)
    if nvp == 8:   # raster.hip: "row r: components 16 + (r >> 1) * 4 + (r & 1) * 2 + {0, 1}"
        assert all(16 + M.component_of(8, r, k) == 16 + (r >> 1) * 4 + (r & 1) * 2 + k for r in range(4) for k in (0, 1))


def test_pair_placement_and_fence():
    x = M.placement(2)
    y = M.wave_reduce_pair(x[:, :, 0], x[:, :, 1])
    weights = np.array([240.0, 240.0, 240.0, 96.0])[:, None]
    assert (y[:4, :32] == weights).all() and (y[:4, 32:] == 2 * weights).all() and (y[4:, :32] == 1.0).all() and (y[4:, 32:] == 2.0).all()
    f = M.wave_fence(M.LANES.astype(np.uint32))
    assert np.array_equal(f[:, 0], 63 - M.LANES) and np.array_equal(f[:, 1], 63 - ((M.LANES - 17) & 63))


def test_block_and_row_sums_on_counting_vectors():
    v = M.counting(F64, M.BLOCK)
    assert np.array_equal(M.block_sum(v), v.sum(-1)) and np.array_equal(M.block_sum4(v.astype(F32)), v.sum(-1))
    # lane 0 of the __shfl_down chain ends with the butterfly's tree
    w = M.order_table("wave_sum_f64")
    assert np.array_equal(M.bits_of(M.shfl_down_lane0(w)), M.bits_of(M.wave_sum(w)[:, 0]))
    rows = np.arange(M.ROW_COUNTS[-1], dtype=F64)
    for n in M.ROW_COUNTS:
        for stride in M.STRIDES:
            p = M.strided(rows, n, stride)
            assert M.rows_sum(p, n, stride) == n * (n - 1) / 2 == M.wave_rows_sum(p, n, stride), (n, stride)
            assert stride == 1 or n == 0 or np.isnan(M.rows_sum(p, n, 1)) or n == 1     # a wrong stride meets the NaNs
    runs = M.run_sums(rows, 515, 1, M.BLOCK)                     # ceil(515 / 256) = 3 rows per thread: 171 full runs, one of 2
    assert runs[0] == 3 and runs[171] == 513 + 514 and (runs[172:] == 0).all()


ORDERS = {   # primitive -> (its model on (N, width) vectors, width of one sum, the other tree)
    "wave_sum_f32": (lambda v: M.wave_sum(v)[:, 0], 64, lambda v: M.tree_sum(v, M.ROW_FIRST_BITS)),
    "wave_sum_f64": (lambda v: M.wave_sum(v)[:, 0], 64, lambda v: M.tree_sum(v, M.ROW_FIRST_BITS)),
    "row_allreduce": (lambda v: M.row_allreduce(np.tile(v, 4))[:, 0], 16, lambda v: M.tree_sum(v, (3, 2, 1, 0))),
    "half_wave_sum": (lambda v: M.half_wave_sum(np.tile(v, 2))[:, 0], 32, lambda v: M.tree_sum(v, (4, 3, 2, 1, 0))),
    "wave_allreduce": (lambda v: M.wave_allreduce(v)[:, 0], 64, lambda v: M.tree_sum(v, M.BUTTERFLY_BITS)),
    "wave_reduce_pair": (lambda v: M.wave_reduce_pair(v, v)[:, 0], 64, lambda v: M.tree_sum(v, M.BUTTERFLY_BITS)),
    "block_sum": (M.block_sum, 256, lambda v: M.waves_in_order(v, M.ROW_FIRST_BITS)),
    "block_sum4": (M.block_sum4, 256, lambda v: M.waves_in_order(v, M.ROW_FIRST_BITS)),
    "rows_sum": (lambda p: M.rows_sum(p, 515, 1), 515,
                 lambda p: M.waves_in_order(M.run_sums(p, 515, 1, M.BLOCK), M.ROW_FIRST_BITS)),
    "wave_rows_sum": (lambda p: M.wave_rows_sum(p, 515, 1), 515,
                      lambda p: M.tree_sum(M.run_sums(p, 515, 1, M.WAVE), M.ROW_FIRST_BITS)),
}
for _nvp in M.NVPS:
    ORDERS[f"wave_reduce_components_{_nvp}"] = (lambda v: M.wave_allreduce(v)[:, 0], 64,
                                                lambda v: M.tree_sum(v, M.BUTTERFLY_BITS))


@pytest.mark.parametrize("name", sorted(ORDERS))
def test_order_sensitive_inputs_separate_the_orders(name):
    """Every vector: the modelled result differs in bits from the left-to-right sum and from the other tree (row-first
    for the butterflies, descending bits for the DPP reductions).  Nothing is skipped: the table redraws."""
    model, width, other = ORDERS[name]
    table = M.order_table(name)
    if table.ndim == 3:                         # (G, 64, KI): every component of every vector is one sum
        table = table.transpose(0, 2, 1)
    v = table.reshape(-1, width)                # rows, halves and components as sums of their own
    assert len(v) >= M.N_ORDER
    want = M.bits_of(model(v))
    assert (want != M.bits_of(M.left_to_right(v))).all() and (want != M.bits_of(other(v))).all()
    assert np.log2(np.abs(v).max() / np.abs(v).min()) > 28 and ((v < 0).any(-1) & (v > 0).any(-1)).all()


def test_every_case_agrees_with_the_separate_models():
    """The tables handed to the GPU test: shapes, and the component / pair cases against wave_allreduce on one register."""
    ops = [c.op for c in M.all_cases()]
    assert len(set(ops)) == 35 and len(M.rows_cases()) == 2 * len(M.ROW_COUNTS) * len(M.STRIDES)
    for c in M.all_cases():
        assert c.expected.shape == (c.G, c.T, c.KO) and c.T in (64, 256) and not M.mismatches(c.expected, c.expected)
        if c.op.startswith("MOBGS_LANE_REDUCE_COMPONENTS"):
            nvp = c.inputs.shape[2]
            for lane in (0, 17, 38, 63):
                for k in range(nvp // 4):
                    total = M.wave_allreduce(c.inputs[:, :, M.component_of(nvp, lane >> 4, k)])[:, 0]
                    assert np.array_equal(M.bits_of(total), M.bits_of(c.expected[:, lane, k]))
        if c.span:
            assert not M.not_uniform(c.expected, c.span), c


def _case(op):
    return next(c for c in M.all_cases() if c.op == op)


def test_planted_defects_are_reported():
    """What the GPU test compares with must see each of these in at least one vector of the table."""
    # lane 37 dropped, lane 36 counted twice
    for op, fn in (("MOBGS_LANE_WAVE_SUM_F32", M.wave_sum), ("MOBGS_LANE_WAVE_ALLREDUCE", M.wave_allreduce),
                   ("MOBGS_LANE_ROW_ALLREDUCE", M.row_allreduce), ("MOBGS_LANE_WAVE_MAX_I32", M.wave_max)):
        c = _case(op)
        x = c.inputs[:, :, 0].copy()
        x[:, 37] = x[:, 36]
        assert M.mismatches(fn(x)[:, :, None], c.expected), op
    c = _case("MOBGS_LANE_BLOCK_SUM")
    x = c.inputs.copy()
    x[:, 37] = x[:, 36]
    bad = np.broadcast_to(np.stack([M.block_sum(x[:, :, 0]), M.block_sum(x[:, :, 1])], -1)[:, None], c.expected.shape)
    assert M.mismatches(bad.copy(), c.expected, c.threads)
    # row_half_mirror replaced by an identity
    identity = dict(M.DPP_SRC)
    identity[0x141] = M.LANES
    c = _case("MOBGS_LANE_ROW_ALLREDUCE")
    assert M.mismatches(M.row_allreduce(c.inputs[:, :, 0], identity)[:, :, None], c.expected)
    c = _case("MOBGS_LANE_DPP_MOV_HALF_MIRROR")
    assert M.mismatches(M.dpp_mov(c.inputs[:, :, 0], 0x141, identity)[:, :, None], c.expected)
    # the two halves of wave_reduce_pair exchanged
    c = _case("MOBGS_LANE_REDUCE_PAIR")
    assert M.mismatches(c.expected[:, M.LANES ^ 32], c.expected)
    # the rows of wave_reduce_components exchanged (the total in the wrong row)
    c = _case("MOBGS_LANE_REDUCE_COMPONENTS_8")
    assert M.mismatches(c.expected[:, M.LANES ^ 16], c.expected)
    # a run length of floor(n / BLOCK) instead of ceil
    found = 0
    for c in M.rows_cases():
        if c.op == "MOBGS_LANE_ROWS_SUM":
            bad = np.broadcast_to(M.rows_sum(c.inputs, c.n, c.stride, ceil=False)[:, None, :], c.expected.shape).copy()
            found += bool(M.mismatches(bad, c.expected, c.threads))
    assert found >= 10      # every count that is no multiple of BLOCK (0 excepted), at both strides
    # a wrong stride
    c = next(c for c in M.rows_cases() if c.op == "MOBGS_LANE_WAVE_ROWS_SUM" and c.n == 65 and c.stride == 2)
    bad = np.broadcast_to(M.wave_rows_sum(c.inputs[:, 0], c.n, 1)[:, None, None], c.expected.shape).copy()
    assert M.mismatches(bad, c.expected)
    # one lane's result differing in the last bit; a NaN where a number belongs; a thread outside the contract is not read
    for c in (_case("MOBGS_LANE_WAVE_SUM_F64"), _case("MOBGS_LANE_HALF_WAVE_SUM"), _case("MOBGS_LANE_BLOCK_SUM4")):
        bad = c.expected.copy()
        M.bits_of(bad)[-12, 41, 0] ^= 1
        assert M.mismatches(bad, c.expected) == [(c.G - 12, 41, 0)] and M.not_uniform(bad, c.span)
        bad = c.expected.copy()
        bad[0, 3, 0] = np.nan
        assert M.mismatches(bad, c.expected) == [(0, 3, 0)]
    c = _case("MOBGS_LANE_BLOCK_SUM")
    bad = c.expected.copy()
    bad[:, 1:] = 0.0
    assert not M.mismatches(bad, c.expected, c.threads) and M.mismatches(bad, c.expected)


def test_lane_probe_refuses_bad_arguments_before_any_launch():
    """MOBGS_E_INVALID under the entry point's own name, with no device: an unknown op, NULL pointers, n_groups < 1, n < 0,
    stride < 1, misaligned pointers."""
    from mobgs_amd import _lib
    h = _lib.load()
    D = _lib._DEFINES
    assert D["MOBGS_LANE_OPS"] == 35 and sorted(v for k, v in D.items() if k.startswith("MOBGS_LANE_") and k != "MOBGS_LANE_OPS") \
        == list(range(35))
    assert {c.op for c in M.all_cases()} == {k for k in D if k.startswith("MOBGS_LANE_") and k != "MOBGS_LANE_OPS"}
    buf = ctypes.create_string_buffer(64)
    base = (ctypes.addressof(buf) + 15) & ~15
    good, none = ctypes.c_void_p(base), ctypes.c_void_p(None)
    f32, f64 = D["MOBGS_LANE_WAVE_SUM_F32"], D["MOBGS_LANE_ROWS_SUM"]
    for args in ((-1, 1, 0, 1, good, good), (D["MOBGS_LANE_OPS"], 1, 0, 1, good, good), (f32, 1, 0, 1, none, good),
                 (f32, 1, 0, 1, good, none), (f32, 0, 0, 1, good, good), (f32, -3, 0, 1, good, good),
                 (f32, 1, -1, 1, good, good), (f32, 1, 0, 0, good, good), (f64, 1, 4, -2, good, good),
                 (f32, 1, 0, 1, ctypes.c_void_p(base + 2), good), (f32, 1, 0, 1, good, ctypes.c_void_p(base + 1)),
                 (f64, 1, 4, 1, ctypes.c_void_p(base + 4), good), (f64, 1, 4, 1, good, ctypes.c_void_p(base + 4)),
                 (f64, 4096, 2**30, 2, good, good)):
        h.mobgs_raster_bwd_reduce(0, 5, 3, 0, *[none] * 12)     # leaves another entry point's message behind
        assert h.mobgs_lane_probe(*args, none) == D["MOBGS_E_INVALID"] == -1, args
        assert b"mobgs_lane_probe" in h.mobgs_last_error(), (args, h.mobgs_last_error())
