"""Generate tests/golden/isect_host.npz: what the host side of the binning entry points (csrc/isect.hip,
csrc/pipeline.hip) of the library built from the CURRENT tree answers without a device --

  sizes     mobgs_isect_scratch_bytes, mobgs_keep_scan_len, mobgs_tile_order_len, mobgs_fused_seg_keys_len and
            mobgs_fused_max_seg_stride over a grid of (n_gauss, n_tiles, capacity, seg_stride);
  refusals  return code and the first words of mobgs_last_error() for the argument sets every binning entry point
            refuses BEFORE its first HIP call (so nothing here launches, copies or clears anything).

    python tests/golden/make_golden_isect_host.py

It was run once, on the commit BEFORE the binning launchers were given one geometry record, one scratch layout and
argument bundles (csrc/isect_launch.h): the fixture pins what the hand-kept copies of the guards and of the layout
answered, and tests/test_isect_host_cpu.py holds every later library to it.  Re-running it on a later commit records
that commit's answers -- only do so when one is changed on purpose.

The pointers handed over are small made-up addresses with the alignment a case needs; no refused call reads them.
"""
from __future__ import annotations

import ctypes
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from helpers import save_npz  # noqa: E402

# 0 and 1; either side of 2048 (scan / keep_scan chunk), 8192 (LDS-ranked binning) and 1024 (SCHED_SMALL_GRID); the
# benchmark's default scene (300 k splats, 1352 x 1014 = 85 x 64 tiles, arena 16 n + 1024) and its small scene
# (9 k splats, 320 x 240 = 20 x 15 tiles)
N_GAUSS = [0, 1, 2047, 2048, 2049, 8191, 8192, 8193, 9000, 300_000]
N_TILES = [0, 1, 300, 1023, 1024, 1025, 2047, 2048, 2049, 5440, 8191, 8192, 8193]
CAPACITY = [0, 1, 2047, 2048, 2049, 4096, 8191, 8192, 8193, 145_024, 1_000_000, 4_801_024]  # multiples of 2048 and not
SEG_STRIDE = [0, 1, 511, 512, 2047, 2048, 2049]

MSG_WORDS = 160  # bytes of mobgs_last_error() kept per refusal


def sizes(lib) -> dict:
    scratch = np.array([[[lib.mobgs_isect_scratch_bytes(n, t, c) for c in CAPACITY] for t in N_TILES] for n in N_GAUSS],
                       dtype=np.int64)
    return {"n_gauss": np.array(N_GAUSS, dtype=np.int64), "n_tiles": np.array(N_TILES, dtype=np.int64),
            "capacity": np.array(CAPACITY, dtype=np.int64), "seg_stride": np.array(SEG_STRIDE, dtype=np.int64),
            "scratch_bytes": scratch,
            "keep_scan_len": np.array([lib.mobgs_keep_scan_len(c) for c in CAPACITY], dtype=np.int64),
            "tile_order_len": np.array([lib.mobgs_tile_order_len(t) for t in N_TILES], dtype=np.int64),
            "seg_keys_len": np.array([[lib.mobgs_fused_seg_keys_len(t, s) for s in SEG_STRIDE] for t in N_TILES],
                                     dtype=np.int64),
            "max_seg_stride": np.array([lib.mobgs_fused_max_seg_stride()], dtype=np.int64)}


def _ptrs():
    """Made-up, never dereferenced addresses: distinct, 256-byte aligned."""
    return (ctypes.c_void_p(a) for a in itertools.count(0x10000, 0x100))


def _project_and_bin_args(p, *, C=1, N=100, opacities=True, capacity_box=4 * 100 + 2, scratch=0x4000,
                          capacity_listed=1000):
    """The 30 leading arguments mobgs_project_and_bin_speculative and _fused share (C .. flatten_ids)."""
    nx = lambda: next(p)  # noqa: E731
    return [C, N, nx(), nx(), nx(), nx(), nx(), nx() if opacities else None, 0, 64, 48, 0.3, 0.01, 1e10, 0.0, 1,
            nx(), nx(), nx(), nx(), nx(), nx(), nx(), nx(), nx(), capacity_box, nx(), ctypes.c_void_p(scratch),
            capacity_listed, nx()]


def refusal_cases(lib) -> list:
    """[(name, callable -> return code)]: every case is refused (or, for n_isects = 0, answered) before the first HIP call
    of its entry point -- confirmed by reading the code path of the commit this was recorded on."""
    from mobgs_amd import _lib
    p = _ptrs()
    nx = lambda: next(p)  # noqa: E731
    none = None

    def offsets(C=1, N=100, capacity=1000, scratch=0x4000):
        # C, N, tile_w, tile_h, width, height, cull, capacity | tiles_per_gauss, means2d, radii, conics, opacities |
        # opac_per_camera | cum_tiles, keep_scan, tile_offsets, tile_order | capacity_listed | stats, scratch | tuning, stream
        return lib.mobgs_isect_offsets(C, N, 4, 3, 64, 48, 1, capacity, nx(), nx(), nx(), nx(), nx(), 0, nx(), nx(), nx(),
                                       nx(), 0, nx(), ctypes.c_void_p(scratch), none, none)

    def emit(n_isects):
        return lib.mobgs_isect_emit_sort(1, 100, 4, 3, 1000, n_isects, 10, nx(), nx(), nx(), ctypes.c_void_p(0x4000), nx(),
                                         nx(), nx(), none)

    def emit_spec(stats_dev=True, capacity_listed=1000):
        return lib.mobgs_isect_emit_sort_speculative(1, 100, 4, 3, 1000, capacity_listed, 10, nx(), nx(), nx(),
                                                     nx() if stats_dev else none, ctypes.c_void_p(0x4000), nx(), nx(),
                                                     nx(), none)

    def speculative(stats_host=True, pack_colors=True, pack_records=False):
        # ... sort_keys, isect_ids, hint, stats_host_pinned, stats_seq, pack_colors, colors_per_camera, pack_channels,
        # pack_records, tuning, stream
        return lib.mobgs_project_and_bin_speculative(*_project_and_bin_args(p), nx(), nx(), 0, nx() if stats_host else none,
                                                     0, nx() if pack_colors else none, 0, 3,
                                                     nx() if pack_records else none, none, none)

    def fused(seg_stride=256, seg_keys=True, **kw):
        # ... seg_keys, seg_stride, enum_order, isect_ids, hint, stats_host_pinned, stats_seq, pack_colors,
        # colors_per_camera, pack_channels, pack_records, tuning, stream
        return lib.mobgs_project_and_bin_fused(*_project_and_bin_args(p, **kw), nx() if seg_keys else none, seg_stride,
                                               none, nx(), 100, nx(), 0, none, 0, 3, none, none, none)

    def prep(ns=60, nd=40, with_prep=True, means=True):
        pin = _lib.MobgsPrepInputs(ns, nd, *[next(p) for _ in range(16)])
        ref = ctypes.cast(ctypes.pointer(pin), ctypes.c_void_p) if with_prep else none
        # prep, means, quats, scales, viewmats, Ks, opacities, width .. cull, radii .. stats_dev, capacity_box, keep_scan,
        # scratch, capacity_listed, flatten_ids, seg_keys, seg_stride, enum_order, isect_ids, hint, stats_host_pinned,
        # stats_seq, pack_records, tuning, stream
        return lib.mobgs_prep_project_and_bin_fused(ref, nx() if means else none, nx(), nx(), nx(), nx(), nx(), 64, 48, 0.3,
                                                    0.01, 1e10, 0.0, 1, nx(), nx(), nx(), nx(), nx(), nx(), nx(), nx(),
                                                    nx(), 4 * 100 + 2, nx(), ctypes.c_void_p(0x4000), 1000, nx(), nx(),
                                                    256, none, nx(), 100, nx(), 0, nx(), none, none)

    return [
        ("isect_offsets C=0", lambda: offsets(C=0)),
        ("isect_offsets capacity=0", lambda: offsets(capacity=0)),
        ("isect_offsets scratch 4-byte aligned", lambda: offsets(scratch=0x4004)),
        ("isect_emit_sort n_isects<0", lambda: emit(-1)),
        ("isect_emit_sort n_isects=0", lambda: emit(0)),
        ("isect_emit_sort_speculative no stats_dev", lambda: emit_spec(stats_dev=False)),
        ("isect_emit_sort_speculative capacity_listed=0", lambda: emit_spec(capacity_listed=0)),
        ("project_and_bin_speculative no stats_host_pinned", lambda: speculative(stats_host=False)),
        ("project_and_bin_speculative pack_records without pack_colors",
         lambda: speculative(pack_colors=False, pack_records=True)),
        ("project_and_bin_fused seg_stride=0", lambda: fused(seg_stride=0)),
        ("project_and_bin_fused no seg_keys", lambda: fused(seg_keys=False)),
        ("project_and_bin_fused capacity_box=4CN+1", lambda: fused(capacity_box=4 * 100 + 1)),
        ("project_and_bin_fused scratch 64-byte aligned", lambda: fused(scratch=0x4040)),
        ("project_and_bin_fused no opacities", lambda: fused(opacities=False)),
        ("prep_project_and_bin_fused NULL prep", lambda: prep(with_prep=False)),
        ("prep_project_and_bin_fused NULL means", lambda: prep(means=False)),
        ("prep_project_and_bin_fused Ns+Nd=0", lambda: prep(ns=0, nd=0)),
        ("prep_project_and_bin_fused Ns<0", lambda: prep(ns=-1)),
    ]


def refusals(lib) -> dict:
    """-> names, return codes and, for the refused ones, the first MSG_WORDS bytes of the message ("" for an accepted
    call: it leaves the last message alone)."""
    names, codes, msgs = [], [], []
    for name, call in refusal_cases(lib):
        rc = int(call())
        names.append(name)
        codes.append(rc)
        msgs.append(lib.mobgs_last_error()[:MSG_WORDS].decode() if rc != 0 else "")
    return {"refusal_names": np.array(names), "refusal_codes": np.array(codes, dtype=np.int32),
            "refusal_messages": np.array(msgs)}


def main():
    from mobgs_amd import _lib
    lib = _lib.load()
    out = {**sizes(lib), **refusals(lib)}
    path = os.path.join(HERE, "isect_host.npz")
    files = save_npz(path, out)
    assert len(files) == 1
    print(f"wrote {files[0]}  ({os.path.getsize(files[0]) / 1024:.1f} KiB, library {lib.mobgs_version().decode()})")
    for n, c, m in zip(out["refusal_names"], out["refusal_codes"], out["refusal_messages"]):
        print(f"  {int(c):3d}  {n}: {m}")


if __name__ == "__main__":
    main()
