"""CPU checks of the binning launchers' host side (csrc/isect_launch.h, isect.hip, pipeline.hip) against what the library
answered before its guards, its scratch layout and its argument lists were made one of each (tests/golden/
isect_host.npz, make_golden_isect_host.py): the buffer sizes a caller allocates from, and return code + message of every
argument set an entry point refuses before its first HIP call.  Nothing here launches: no GPU needed."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

from helpers import load  # noqa: E402
import make_golden_isect_host as G  # noqa: E402


def test_buffer_sizes_match_the_recording():
    from mobgs_amd import _lib
    fx = load("isect_host")
    assert fx["n_gauss"].tolist() == G.N_GAUSS and fx["n_tiles"].tolist() == G.N_TILES
    assert fx["capacity"].tolist() == G.CAPACITY and fx["seg_stride"].tolist() == G.SEG_STRIDE
    assert fx["scratch_bytes"].size == 10 * 13 * 12 and fx["seg_keys_len"].size == 13 * 7
    got = G.sizes(_lib.load())
    for key in ("keep_scan_len", "tile_order_len", "seg_keys_len", "max_seg_stride"):
        assert np.array_equal(got[key], fx[key]), (key, got[key].tolist(), fx[key].tolist())
    bad = np.argwhere(got["scratch_bytes"] != fx["scratch_bytes"])
    assert len(bad) == 0, [(G.N_GAUSS[i], G.N_TILES[j], G.CAPACITY[k], int(got["scratch_bytes"][i, j, k]),
                            int(fx["scratch_bytes"][i, j, k])) for i, j, k in bad[:8]]


def test_refusals_match_the_recording():
    """Same return code and same message, word for word, for each recorded case; the one accepted call (no listed
    intersections: nothing to emit) returns MOBGS_OK."""
    from mobgs_amd import _lib
    fx = load("isect_host")
    got = G.refusals(_lib.load())
    assert fx["refusal_names"].tolist() == got["refusal_names"].tolist() and len(fx["refusal_names"]) == 18
    assert int((fx["refusal_codes"] == -1).sum()) == 17 and int((fx["refusal_codes"] == 0).sum()) == 1
    for name, rc, msg, rc_ref, msg_ref in zip(got["refusal_names"], got["refusal_codes"], got["refusal_messages"],
                                              fx["refusal_codes"], fx["refusal_messages"]):
        assert int(rc) == int(rc_ref) and str(msg) == str(msg_ref), (str(name), int(rc), str(msg), int(rc_ref), str(msg_ref))
