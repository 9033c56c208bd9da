"""GPU probes of the cross-lane primitives (csrc/wave_shared.h) and the fixed-order sums (csrc/reduce_shared.h): every
function and instantiation the kernel files use, one mobgs_lane_probe launch over the whole input table of the case,
compared BIT FOR BIT with the CPU model of the headers' comments and statements (tests/lane_model.py; the model itself is
checked in tests/test_lane_model_cpu.py).  Nothing here has a tolerance: NaN results are compared as NaN-ness, everything
else as bits.

Each case asserts: out equals the model in every thread the contract specifies; where the header promises "the same bits in
each" lane, all lanes of the wave (row, half) hold one pattern; the documented register and row of each component; each of two
block sums in a row returns its own total; the same launch again, and the same data at base pointers moved by 8 bytes, give
the same bits; and, the output lying in memory pre-filled with 0xFF bytes, nothing outside the documented extent is touched
and nothing inside it is left unwritten."""
import ctypes

import numpy as np
import pytest
import torch

import lane_model as M

pytestmark = pytest.mark.gpu

GUARD = 512     # bytes of 0xFF on either side of the output


def probe(case, device, shift=0):
    """One launch; in and out `shift` bytes past a 256-byte boundary.  Returns out as (G, T, KO)."""
    from mobgs_amd import _lib
    h = _lib.load()
    raw = np.ascontiguousarray(case.raw_inputs).tobytes()
    src = torch.zeros(len(raw) + 64, dtype=torch.uint8, device=device)
    if raw:
        src[shift:shift + len(raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
    size = case.expected.nbytes
    buf = torch.full((GUARD + size + GUARD,), 0xFF, dtype=torch.uint8, device=device)
    assert src.data_ptr() % 256 == 0 and buf.data_ptr() % 256 == 0
    lo = GUARD // 2 + shift
    rc = h.mobgs_lane_probe(_lib._DEFINES[case.op], case.G, case.n, case.stride, ctypes.c_void_p(src.data_ptr() + shift),
                            ctypes.c_void_p(buf.data_ptr() + lo), _lib.stream())
    _lib.check(rc, "mobgs_lane_probe")
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:lo] == 0xFF).all() and (host[lo + size:] == 0xFF).all(), "written outside the documented extent"
    out = host[lo:lo + size].copy().view(case.dtype).reshape(case.expected.shape)
    ones = np.iinfo(M.bits_of(out).dtype).max
    assert (M.bits_of(case.expected) != ones).all() and (M.bits_of(out) != ones).all(), "an element was left unwritten"
    return out


@pytest.mark.parametrize("case", M.all_cases(), ids=repr)
def test_primitive_matches_the_model_bit_for_bit(hip_device, case):
    out = probe(case, hip_device)
    bad = M.mismatches(out, case.expected, case.threads)
    assert not bad, (case, len(bad), [(ix, out[ix], case.expected[ix]) for ix in bad[:6]])
    if case.span:
        assert not M.not_uniform(out, case.span), (case, M.not_uniform(out, case.span)[:6])
    if case.op.startswith("MOBGS_LANE_REDUCE_COMPONENTS"):
        # placement, from the header's formula alone: the placement vectors' totals are weight (component + 1), exact
        nvp = case.inputs.shape[2]
        placed = len(M.placement(nvp))
        weights = case.inputs[:placed, :, 0].astype(np.float64).sum(1)
        for lane in range(M.WAVE):
            r = lane >> 4
            for k in range(nvp // 4):
                component = (r >> 1) * (nvp // 2) + (r & 1) * (nvp // 4) + k
                if nvp == 8:    # raster.hip's comment at its wave_reduce_components<8> call, as the same formula
                    assert 16 + component == 16 + (r >> 1) * 4 + (r & 1) * 2 + k
                assert np.array_equal(out[:placed, lane, k], weights * (component + 1)), (case, lane, k)
    if case.op == "MOBGS_LANE_REDUCE_PAIR":
        placed = len(M.placement(2))
        weights = case.inputs[:placed, :, 0].astype(np.float64).sum(1)[:, None]
        assert np.array_equal(out[:placed, :32, 0], np.broadcast_to(weights, (placed, 32)))          # e0 in lanes 0-31
        assert np.array_equal(out[:placed, 32:, 0], np.broadcast_to(2 * weights, (placed, 32)))      # e1 in lanes 32-63
    if case.KO == 2 and case.T == M.BLOCK:
        # two block sums in a row on one LDS array: each call's own total (the tables pair different totals)
        first, second = M.bits_of(case.expected[:, 0, 0]), M.bits_of(case.expected[:, 0, 1])
        assert (first != second).any() or (case.op == "MOBGS_LANE_ROWS_SUM" and case.n == 0)
        assert np.array_equal(M.bits_of(out[:, 0, 0]), first) or np.isnan(case.expected[:, 0, 0]).any()
        assert np.array_equal(M.bits_of(out[:, 0, 1]), second) or np.isnan(case.expected[:, 0, 1]).any()
    again = probe(case, hip_device)
    assert np.array_equal(M.bits_of(again), M.bits_of(out)), (case, "the same launch again")
    moved = probe(case, hip_device, shift=8)
    assert np.array_equal(M.bits_of(moved), M.bits_of(out)), (case, "base pointers moved by 8 bytes")
