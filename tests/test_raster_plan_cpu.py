"""CPU checks of the compositors' host side (csrc/raster_launch.h): the decision table mobgs_raster_path() reports --
the record the launchers themselves choose their kernels from -- against the table recorded before the two were made
one (tests/golden/raster_path.npz, make_golden_raster_path.py), the channel table against rendering._SUPPORTED, and
the refusal of a channel count the slot reduction has no kernel for.  Nothing here launches: no GPU needed."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

from helpers import load  # noqa: E402
import make_golden_raster_path as G  # noqa: E402


def test_decision_table_matches_the_recording():
    from mobgs_amd import _lib
    fx = load("raster_path")
    tunings = G.tuning_rows()
    assert fx["channels"].tolist() == G.CHANNELS == list(range(29))
    assert fx["class_filter"].tolist() == G.CLASS_FILTER and fx["n_tiles"].tolist() == G.N_TILES
    assert np.array_equal(fx["tunings"], tunings) and len(tunings) == 1 + 3 * 5 * 3 * 3
    assert fx["bits"].size == 31552
    got = G.query(_lib.load(), tunings)
    bad = np.argwhere(got != fx["bits"])
    assert len(bad) == 0, [(int(fx["channels"][i]), int(fx["class_filter"][j]), int(fx["n_tiles"][k]), tunings[m].tolist(),
                            int(got[i, j, k, m]), int(fx["bits"][i, j, k, m])) for i, j, k, m in bad[:8]]


def test_channel_table_is_the_one_the_host_wrapper_pads_to():
    from mobgs_amd import _lib, rendering
    h = _lib.load()
    for d in range(33):
        assert h.mobgs_raster_channels_supported(d) == (d in rendering._SUPPORTED), d


def test_slot_reduction_refuses_more_than_26_channels():
    """27 total channels = records of 36 floats, which no slot_reduce kernel sums: MOBGS_E_UNSUPPORTED, before any launch
    (the pointers are NULL)."""
    from mobgs_amd import _lib
    h = _lib.load()
    none = ctypes.c_void_p(None)
    for channels, has_extra in ((27, 0), (26, 1)):
        rc = h.mobgs_raster_bwd_reduce(1, 5, channels, has_extra, none, none, none, none, none, none, none, none, none, none,
                                       none, none)
        assert rc == -3 and b"mobgs_raster_bwd_reduce" in h.mobgs_last_error(), (rc, h.mobgs_last_error())
