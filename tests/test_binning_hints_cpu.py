"""CPU replay of the binning stage's host-side hint policy (mobgs_amd/rendering.py: arena capacities, list-length hint,
sticky key-segment stride, StaticCapacity) against the recording made before the five per-workload tables became one
record (tests/golden/binning_hints.npz, make_golden_binning_hints.py): what every binning call of every scripted
sequence is handed, what resolve() answers, the counters and the workload's state afterwards -- value for value.
Nothing here launches: the fast-path module, the landing rows and the synchronous rebuild are stand-ins."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

from helpers import load  # noqa: E402
import make_golden_binning_hints as G  # noqa: E402


@pytest.fixture(scope="module")
def replay():
    return G.record()


def test_the_recording_covers_every_sequence():
    fx = load("binning_hints")
    assert fx["columns"].tolist() == list(G.COLUMNS)
    names = sorted(k for k in fx if k != "columns")
    assert names == sorted([s + t for s in "abcdefhijk" for t in ("", "_final")]
                           + [g + t for g in ("g15", "g20") for t in ("", "_checks", "_final")])
    assert [len(fx[s]) for s in "abcdefhijk"] == [4, 24, 6, 3, 6, 12, 5, 7, 5, 5]
    a = fx["a"]   # the trace of the issue this recording was made for: (cap_box, cap_listed, len_hint, seg_stride), rebuilt
    assert a[:, :4].tolist() == [[17024, 8512, 0, 0], [51024, 25512, 700, 912], [51024, 25512, 665, 912],
                                 [52274, 26137, 1200, 1968]]
    assert a[:, 5].tolist() == [1, 0, 1, 0] and fx["a_final"].tolist() == [[52274, 26137, 1140, 20000, 5000, 1968]]
    assert fx["g15"][5, :4].tolist() == [31024, 8524, 1710, 0] and fx["g15_checks"][:, 0].tolist() == [1, 1, 0]
    assert fx["g15_checks"][2, 4:6].tolist() == [90000, 7000]


def test_replay_matches_the_recording(replay):
    fx = load("binning_hints")
    assert sorted(replay) == sorted(fx)
    for name in sorted(fx):
        if name == "columns":
            continue
        got, want = replay[name], fx[name]
        assert got.shape == want.shape, (name, got.shape, want.shape)
        bad = np.argwhere(got != want)
        cols = G.COLUMNS if got.shape[1] == len(G.COLUMNS) else (("check",) if name.endswith("_checks") else ()) + G.STATE
        assert len(bad) == 0, [(name, int(i), cols[j], int(got[i, j]), int(want[i, j])) for i, j in bad[:8]]


def test_replay_leaves_the_module_as_it_found_it(replay):
    import mobgs_amd.rendering as R
    from mobgs_amd import _fast
    assert R._stats_slots is None or not isinstance(R._stats_slots, G._Rows)
    assert _fast.get.__module__ == "mobgs_amd._fast" and R.stream_int.__module__ == "mobgs_amd._lib"
    assert R.build_tile_lists.__module__ == "mobgs_amd.rendering" and R.SPECULATIVE_BINNING is True
