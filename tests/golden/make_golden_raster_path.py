"""Generate tests/golden/raster_path.npz: what mobgs_raster_path() of the library built from the CURRENT tree answers
over the whole decision table -- which backward kernel, which forward kernel and which heavy-tile threshold a
compositing pass takes per channel count, pass kind, grid size and MobgsTuning.

    python tests/golden/make_golden_raster_path.py

The query launches nothing, so this runs without a GPU.  It was run once, on the commit BEFORE the launchers were made
to read their kernel choice from the same record the query packs (csrc/raster_launch.h raster_plan): the fixture pins
the table that hand-kept pair of copies produced, and tests/test_raster_plan_cpu.py holds every later library to it.
Re-running it on a later commit records that commit's table -- only do so when a selection is changed on purpose.

The fixture holds data only: the axes (total channels 0..28, class_filter 0 / 1, four grid sizes around the small-grid
threshold of 1024 tiles, and the tunings: row 0 = a NULL pointer, then every combination of heavy_tile_len x bwd_mfma x
bwd_block_walk x block_walk with all other fields -1) and the returned bit field per combination.
"""
from __future__ import annotations

import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from helpers import save_npz  # noqa: E402

CHANNELS = list(range(29))
CLASS_FILTER = [0, 1]
N_TILES = [1, 1024, 1025, 100000]
TUNING_FIELDS = ("heavy_tile_len", "bwd_mfma", "bwd_block_walk", "block_walk")
TUNING_VALUES = ([-1, 0, 64], [-1, 0, 1, 2, 3], [-1, 0, 1], [-1, 0, 1])


def tuning_rows() -> np.ndarray:
    """[1 + 135, 5] int32: column 0 = 1 for the NULL tuning (row 0; its other columns are unused), then TUNING_FIELDS."""
    rows = [(1, -1, -1, -1, -1)] + [(0, *v) for v in itertools.product(*TUNING_VALUES)]
    return np.array(rows, dtype=np.int32)


def query(lib, tunings: np.ndarray) -> np.ndarray:
    """mobgs_raster_path over CHANNELS x CLASS_FILTER x N_TILES x tunings -> int32 [29, 2, 4, len(tunings)]."""
    from mobgs_amd import _lib
    every = {name: -1 for name, _ in _lib.MobgsTuning._fields_}
    refs = []
    for row in tunings:
        t = None if row[0] else _lib.MobgsTuning(**{**every, **dict(zip(TUNING_FIELDS, map(int, row[1:])))})
        refs.append(t)
    out = np.empty((len(CHANNELS), len(CLASS_FILTER), len(N_TILES), len(tunings)), dtype=np.int32)
    for i, d in enumerate(CHANNELS):
        for j, cf in enumerate(CLASS_FILTER):
            for k, nt in enumerate(N_TILES):
                for m, t in enumerate(refs):
                    out[i, j, k, m] = lib.mobgs_raster_path(d, cf, nt, t.ref() if t is not None else None)
    return out


def main():
    from mobgs_amd import _lib
    lib = _lib.load()
    tunings = tuning_rows()
    bits = query(lib, tunings)
    assert bits.size == 31552
    out = {"channels": np.array(CHANNELS, dtype=np.int32), "class_filter": np.array(CLASS_FILTER, dtype=np.int32),
           "n_tiles": np.array(N_TILES, dtype=np.int32), "tunings": tunings, "bits": bits}
    path = os.path.join(HERE, "raster_path.npz")
    files = save_npz(path, out)
    size = sum(os.path.getsize(f) for f in files)
    assert len(files) == 1
    print(f"wrote {files[0]}  ({size / 1024:.1f} KiB, {bits.size} entries, {len(np.unique(bits))} distinct values, "
          f"library {lib.mobgs_version().decode()})")
    for name, mask, shift in (("backward kernel", 3, 0), ("block-walk forward", 1, 2), ("heavy tiles", 1, 3)):
        vals, counts = np.unique((bits >> shift) & mask, return_counts=True)
        print(f"  {name}: " + ", ".join(f"{int(v)} x {int(c)}" for v, c in zip(vals, counts)))


if __name__ == "__main__":
    main()
