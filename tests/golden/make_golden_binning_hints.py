"""Generate tests/golden/binning_hints.npz: the host-side hint policy of the binning stage (mobgs_amd/rendering.py) --
which arena capacities, list-length hint and key-segment stride every binning call is handed, what resolve() answers
and what the per-workload state holds afterwards -- over scripted frame sequences, without a device.

    python tests/golden/make_golden_binning_hints.py

It was run once, on the commit BEFORE the five per-workload tables of rendering.py (_capacity, _cap_listed, _len_hint,
_last_counts, _seg_sticky) became one record per workload and the speculative arms of _ProjectAndBin.forward one body:
the fixture pins what that commit's policy did, and tests/test_binning_hints_cpu.py replays record() against every later
tree, value for value.  Re-running it on a later commit records that commit's policy -- only do so when a rule is
changed on purpose.  (_values() / _forget() read either layout, the five tables or the records, so that the same
generator runs on both sides of that change.)

The policy runs through the real SharedProjection(...) and tl.resolve() with four stand-ins: _fast.get() returns a
module whose project_and_bin_speculative logs what it was handed and returns CPU tensors of the right shapes;
rendering.stream_int returns 0; rendering._stats_slots hands out plain numpy rows (page-locking needs a device);
rendering.build_tile_lists returns a TileLists carrying the scripted counts.  The "device" is the script writing
row[:3] = counts, row[3] = seq before resolve().  Two more sequences (j, k) drive the real build_tile_lists and the
synchronous arm of the binning node against a stand-in library that answers the scripted counts.
"""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

# one row per binning call
COLUMNS = ("cap_box", "cap_listed", "len_hint", "seg_stride", "order_kept",        # what the call was handed
           "rebuilt", "n_box", "n_isects", "max_tile_len",                          # resolve() and the counts it left
           "tl_rebuilds", "list_rebuilds", "seg_overflows", "fused_calls",         # counters (since the sequence began)
           "capacity", "listed", "longest", "last_box", "last_listed", "stride")   # the workload's state afterwards
STATE = COLUMNS[-6:]


def _forget(R):
    if hasattr(R, "forget_hints"):
        R.forget_hints()
    else:
        for table in (R._capacity, R._cap_listed, R._len_hint, R._last_counts, R._seg_sticky):
            table.clear()


def _values(R, key):
    """-> the six numbers of STATE for one workload key."""
    if hasattr(R, "hint_record"):
        rec = R.hint_record(key)
        return [rec.cap_box, rec.cap_listed, rec.longest, *rec.last_counts, rec.seg_stride]
    return [R._capacity.get(key, 0), R._cap_listed.get(key, 0), R._len_hint.get(key, 0), *R._last_counts.get(key, (0, 0)),
            R._seg_sticky.get(key, 0)]


class _Rows:
    """rendering._stats_slots without page-locked memory."""

    def __init__(self):
        self.seq = 0

    def take(self):
        return np.zeros(4, dtype=np.int64), None, 0, None

    def next_seq(self):
        self.seq += 1
        return self.seq

    def give(self, i):
        pass


class _FastPath:
    """_fast.get(): logs what the speculative call is handed, returns empty CPU outputs and rc = 0."""

    def __init__(self, log):
        self.log = log

    def project_and_bin_speculative(self, means, quats, scales, viewmats, Ks, opac, width, height, eps2d, near, far, clip,
                                    cull, want_ids, sched, pack, cap_box, cap_listed, len_hint, row_addr, seq, tuning,
                                    stream, seg_stride, order, prep):
        self.log.append((cap_box, cap_listed, len_hint, seg_stride, int(order is not None)))
        C, N = viewmats.shape[0], means.shape[-2]
        i32 = dict(dtype=torch.int32)
        outs = [torch.zeros(C, N, **i32), torch.zeros(C, N, 2), torch.zeros(C, N), torch.zeros(C, N, 3),
                torch.zeros(C, N, **i32), torch.zeros(C * N + 1, **i32), torch.zeros(8, **i32), torch.zeros(8, **i32),
                torch.zeros(cap_listed, **i32)]
        return 0, outs, None, None, None


class _Library:
    """_lib_() for the sequences that run the synchronous entry points: the two calls that would launch answer the
    scripted counts instead (and log the capacities and the hint they were handed); the size functions are the real
    library's."""

    def __init__(self, real, log):
        self.real, self.log, self.counts = real, log, (0, 0, 0)

    def __getattr__(self, name):
        return getattr(self.real, name)

    @staticmethod
    def _hint(tuning_ref):
        from mobgs_amd._lib import MobgsTuning
        return int(ctypes.cast(tuning_ref, ctypes.POINTER(MobgsTuning)).contents.longest_list_hint)

    def mobgs_isect_offsets(self, *a):
        self.log.append((a[7], 0, self._hint(a[21]), 0, 0))
        a[19][:] = torch.tensor(self.counts, dtype=torch.int64)
        return 0

    def mobgs_isect_emit_sort(self, *a):
        return 0

    def mobgs_project_and_bin(self, *a):
        self.log.append((a[25], a[28], self._hint(a[33]), 0, 0))
        a[32][0], a[32][1], a[32][2] = self.counts
        return -4 if (self.counts[0] > a[25] or self.counts[1] > a[28]) else 0


class Harness:
    def __init__(self):
        import mobgs_amd.rendering as R
        from mobgs_amd import _fast
        self.R, self._fast = R, _fast
        self.log = []
        self.scripted = (0, 0, 0)
        self.saved = {n: getattr(R, n) for n in ("stream_int", "stream", "ptr", "_lib_", "_stats_slots", "build_tile_lists",
                                                 "FUSED_LISTS", "FUSED_ARENA_BYTES", "SPECULATIVE_BINNING")}
        self.saved_get = _fast.get
        self.counters0 = (R.list_rebuilds[0], R.seg_overflows[0], R.fused_calls[0])
        fast = _FastPath(self.log)
        _fast.get = lambda: fast
        R.stream_int = lambda: 0
        R._stats_slots = _Rows()
        R.build_tile_lists = self._built
        self.keys = []
        self._inputs = {}
        _forget(R)

    def close(self):
        for n, v in self.saved.items():
            setattr(self.R, n, v)
        self._fast.get = self.saved_get
        self.R.list_rebuilds[0], self.R.seg_overflows[0], self.R.fused_calls[0] = self.counters0
        _forget(self.R)

    def begin(self):
        """A new sequence: no hints, counters at zero, every switch at its default."""
        R = self.R
        _forget(R)
        R.list_rebuilds[0] = R.seg_overflows[0] = R.fused_calls[0] = 0
        for n in ("FUSED_LISTS", "FUSED_ARENA_BYTES", "SPECULATIVE_BINNING", "ptr", "stream", "_lib_"):
            setattr(R, n, self.saved[n])
        R.build_tile_lists = self._built
        self.keys = []

    def _built(self, *args, **kw):
        tl = self.R.TileLists()
        tl.cum_tiles = tl.keep_scan = tl.tile_offsets = tl.tile_order = tl.tiles_per_gauss = None
        n_box, n_isects, max_len = self.scripted
        tl._set_counts(n_box, n_isects, max_len, torch.zeros(n_isects, dtype=torch.int32), None)
        return tl

    def inputs(self, N, C):
        if (N, C) not in self._inputs:
            g = torch.Generator().manual_seed(N)
            self._inputs[N, C] = (torch.rand(N, 3, generator=g), torch.rand(N, 4, generator=g), torch.rand(N, 3, generator=g),
                                  torch.rand(N, generator=g), torch.eye(4)[None].repeat(C, 1, 1),
                                  torch.eye(3)[None].repeat(C, 1, 1))
        return self._inputs[N, C]

    def key(self, N, W, H, C):
        k = self.R._workload_key(torch.device("cpu"), C, N, W, H)
        if k not in self.keys:
            self.keys.append(k)
        return k

    def _row(self, call, rebuilt, tl, key):
        R = self.R
        return [*call, rebuilt, tl._n_box, tl._n_isects, tl._max_tile_len, tl.rebuilds, R.list_rebuilds[0], R.seg_overflows[0],
                R.fused_calls[0], *_values(R, key)]

    def frame(self, counts, N=1000, W=64, H=48, C=1, order=None, token=None, static=None):
        """One SharedProjection + resolve() whose device reports `counts`; under `static` (a StaticCapacity that has been
        entered) nothing is resolved: the counts land in the context's row.  -> the call's row of COLUMNS."""
        R = self.R
        self.scripted = counts
        if token is not None:
            with R.hint_scope(token):
                return self.frame(counts, N, W, H, C, order, None, static)
        key = self.key(N, W, H, C)
        n_calls = len(self.log)
        sp = R.SharedProjection(*self.inputs(N, C), W, H, order=order)
        assert len(self.log) == n_calls + 1
        tl = sp.tl
        if static is not None:
            assert not tl.pending
            static.rows[-1][0][:3] = counts
            return self._row(self.log[-1], -1, tl, key)
        pending = tl._pending
        pending.row[:3] = counts
        pending.row[3] = pending.seq
        rebuilt = int(tl.resolve())
        return self._row(self.log[-1], rebuilt, tl, key)

    def static(self, margin, max_calls=8):
        """StaticCapacity(margin) around a plain int64 pool (its __init__ page-locks one)."""
        sc = self.R.StaticCapacity.__new__(self.R.StaticCapacity)
        sc.margin, sc.rows, sc._prev = float(margin), [], None
        sc.pool = torch.zeros(max_calls, 4, dtype=torch.int64)
        sc.pool_np = sc.pool.numpy()
        return sc

    def final(self):
        return [_values(self.R, k) for k in self.keys]

    def synchronous(self):
        """From here to the next begin(): the synchronous entry points run for real against _Library."""
        R = self.R
        lib = _Library(self.saved["_lib_"](), self.log)
        R._lib_ = lambda: lib
        R.ptr = lambda t: t
        R.stream = lambda: None
        R.build_tile_lists = self.saved["build_tile_lists"]
        return lib


def record() -> dict:
    """Every sequence -> {name: int64 [calls, len(COLUMNS)], name + "_final": [keys, 6], ...}."""
    h = Harness()
    out = {"columns": np.array(COLUMNS)}
    i64 = lambda rows: np.array(rows, dtype=np.int64)  # noqa: E731
    try:
        R = h.R
        # a. first frame overflows the guess, a steady frame, a segment overflow, a shrunken frame
        h.begin()
        out["a"] = i64([h.frame(c) for c in ((40000, 9000, 700), (41000, 9100, 650), (41000, 9100, 1200), (20000, 5000, 300))])
        out["a_final"] = i64(h.final())
        # b. growth past the sticky stride (25 % headroom), then shrinkage below half of it (memory given back)
        h.begin()
        out["b"] = i64([h.frame(c) for c in [(40000, 9000, 700), (40000, 9000, 800), (40000, 9000, 800), (40000, 9000, 1000)]
                        + [(40000, 9000, 100)] * 20])
        out["b_final"] = i64(h.final())
        # c. a stride beyond the one-launch sort, an arena beyond FUSED_ARENA_BYTES (12 tiles x 8 copies x 912 x 8 bytes =
        # 700 416), and an arena that admits the needed stride (1040) but not the 25 % headroom (1312)
        h.begin()
        rows = [h.frame(c) for c in ((40000, 9000, 3000), (40000, 9000, 3000))]
        h.begin()
        rows.append(h.frame((40000, 9000, 700)))
        R.FUSED_ARENA_BYTES = 500_000
        rows.append(h.frame((40000, 9000, 700)))
        R.FUSED_ARENA_BYTES = h.saved["FUSED_ARENA_BYTES"]
        rows.append(h.frame((40000, 9000, 800)))
        R.FUSED_ARENA_BYTES = 900_000
        rows.append(h.frame((40000, 9000, 800)))
        out["c"] = i64(rows)
        out["c_final"] = i64(h.final())
        # d. single-pass lists switched off
        h.begin()
        R.FUSED_LISTS = False
        out["d"] = i64([h.frame(c) for c in ((40000, 9000, 700), (40000, 9000, 700), (40000, 9000, 1500))])
        out["d_final"] = i64(h.final())
        # e. enumeration orders: on the first frame (two-pass: dropped), of the right form (kept), of the wrong length, of
        # the wrong dtype
        h.begin()
        good = torch.arange(1000, dtype=torch.int32)
        out["e"] = i64([h.frame((40000, 9000, 700), order=good), h.frame((40000, 9000, 700), order=good),
                        h.frame((40000, 9000, 700), order=good[:999]), h.frame((40000, 9000, 700), order=good.to(torch.int64)),
                        h.frame((40000, 9000, 700), order=R.COHERENT), h.frame((40000, 9000, 700))])
        out["e_final"] = i64(h.final())
        # f. two scenes and two image sizes interleaved
        h.begin()
        rows = []
        for rep in range(3):
            rows.append(h.frame((40000 + rep, 9000, 700 - 10 * rep), token=1))
            rows.append(h.frame((30000 + rep, 8000, 400 + 10 * rep), token=2))
            rows.append(h.frame((60000 + rep, 20000, 900), token=1, W=128, H=96))
            rows.append(h.frame((10000 + rep, 3000, 200), token=2, W=128, H=96, C=2))
        out["f"] = i64(rows)
        out["f_final"] = i64(h.final())
        # g. StaticCapacity, entered before and after a resolved frame, check() true and false
        for margin in (1.5, 2.0):
            h.begin()
            rows, checks = [], []
            sc = h.static(margin)
            with sc:   # no frame resolved yet: the default capacities
                rows.append(h.frame((12000, 4000, 300), static=sc))
            checks.append([int(sc.check()), *_values(R, h.keys[0])])
            for c in ((40000, 9000, 700), (41000, 9100, 650), (41000, 9100, 1200), (20000, 5000, 300)):
                rows.append(h.frame(c))
            sc = h.static(margin)
            with sc:
                rows.append(h.frame((21000, 5100, 310), static=sc))
                rows.append(h.frame((22000, 5200, 1500), static=sc))
            checks.append([int(sc.check()), *_values(R, h.keys[0])])
            sc = h.static(margin)
            with sc:
                rows.append(h.frame((30000, 7000, 500), static=sc))
                rows.append(h.frame((90000, 7000, 500), static=sc))
            checks.append([int(sc.check()), *_values(R, h.keys[0])])
            rows.append(h.frame((20000, 5000, 300)))   # ... and the frame after the context
            name = "g%d" % int(margin * 10)
            out[name], out[name + "_checks"], out[name + "_final"] = i64(rows), i64(checks), i64(h.final())
        # h. splat counts in one 1/8-octave bucket (1000, 1020) and in the next (1030)
        h.begin()
        out["h"] = i64([h.frame((40000, 9000, 700), N=1000), h.frame((40000, 9000, 700), N=1020),
                        h.frame((40000, 9000, 700), N=1030), h.frame((41000, 9000, 600), N=1000),
                        h.frame((41000, 9000, 600), N=1030)])
        out["h_final"] = i64(h.final())
        # i. the 5 % decay under a falling longest list
        h.begin()
        out["i"] = i64([h.frame((40000, 9000, m)) for m in (1000, 990, 900, 700, 500, 300, 100)])
        out["i_final"] = i64(h.final())
        # j. the real build_tile_lists (grow-and-redo on the box arena; the hint overwritten, not decayed), then what the
        # next speculative call makes of it
        h.begin()
        lib = h.synchronous()
        x = h.inputs(1000, 1)
        key = h.key(1000, 64, 48, 1)
        rows = []
        for counts in ((40000, 9000, 700), (20000, 5000, 300), (41000, 9100, 650)):
            lib.counts = counts
            n_calls = len(h.log)
            tl = R.build_tile_lists(torch.zeros(1, 1000, 2), torch.zeros(1, 1000, dtype=torch.int32), torch.zeros(1, 1000),
                                    torch.zeros(1, 1000, 3), x[3], torch.zeros(1, 1000, dtype=torch.int32), 64, 48)
            for call in h.log[n_calls:]:
                rows.append(h._row(call, 0, tl, key))
        R.build_tile_lists = h._built
        rows.append(h.frame((41000, 9100, 650)))
        out["j"] = i64(rows)
        out["j_final"] = i64(h.final())
        # k. the synchronous arm of the binning node (SPECULATIVE_BINNING off): grow-and-redo on MOBGS_E_CAPACITY
        h.begin()
        lib = h.synchronous()
        R.SPECULATIVE_BINNING = False
        key = h.key(1000, 64, 48, 1)
        rows = []
        for counts in ((40000, 9000, 700), (20000, 5000, 300), (20000, 30000, 300)):
            lib.counts = counts
            n_calls = len(h.log)
            sp = R.SharedProjection(*x, 64, 48)
            assert not sp.tl.pending
            for call in h.log[n_calls:]:
                rows.append(h._row(call, 0, sp.tl, key))
        out["k"] = i64(rows)
        out["k_final"] = i64(h.final())
    finally:
        h.close()
    return out


def main():
    from helpers import save_npz
    out = record()
    path = os.path.join(HERE, "binning_hints.npz")
    files = save_npz(path, out)
    assert len(files) == 1
    print(f"wrote {files[0]}  ({os.path.getsize(files[0]) / 1024:.1f} KiB)")
    for name in sorted(k for k in out if k != "columns"):
        print(name)
        for row in out[name]:
            print("   ", row.tolist())


if __name__ == "__main__":
    main()
