"""The tile-list kernels (mobgs_amd/csrc/isect.hip) on constructed lists: every sort arm, every radix edge, stale
speculative hints, the scan / pass-A seams and the fused single-pass path, against the numpy restatement of upstream
binning (tests/isect_cases.py; tests/test_isect_cases_cpu.py proves that each case reaches its edge).  Integers only:
every comparison is exact, and guard words around every output buffer catch writes outside it."""
import numpy as np
import pytest
import torch

import isect_cases as IC
from helpers import check_tile_order

pytestmark = pytest.mark.gpu

NAMES = IC.case_names()


def _check(out, ref, what, lists=True):
    I_box, I_listed, longest = ref["stats"]
    assert out["guards_ok"], f"{what}: guard words overwritten around {out['broken_guards']}"
    assert out["stats"] == ref["stats"], what
    assert np.array_equal(out["cum_tiles"], ref["cum_tiles"]), what
    assert np.array_equal(out["slots"], ref["slots"]), what
    if lists:
        assert np.array_equal(out["tile_offsets"], ref["tile_offsets"]), what
        assert np.array_equal(out["flatten_ids"][:I_listed], ref["flatten_ids"]), what
        assert np.array_equal(out["isect_ids"][:I_listed], ref["isect_ids"]), what
        check_tile_order(out["tile_order"], ref["nt"], out["tile_offsets"])


# ---- two-pass, synchronous ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_two_pass_lists_equal_the_reference(hip_device, name):
    ref = IC.ref_of(name)
    _check(IC.run_two_pass(IC.cases()[name], ref, hip_device), ref, name)


def test_two_pass_culled_lists_equal_the_reference(hip_device):
    ref = IC.ref_of("cull", 1)
    assert 0 < ref["stats"][1] < ref["stats"][0]
    _check(IC.run_two_pass(IC.cases()["cull"], ref, hip_device, cull=1), ref, "cull = 1")


@pytest.mark.parametrize("delta", (0, 1, -1))
@pytest.mark.parametrize("name", ("ibox2047", "ibox2048", "ibox2049", "ibox4096", "ibox6144", "cull"))
def test_arena_capacity_at_the_box_count(hip_device, name, delta):
    """capacity = I_box, I_box + 1 and I_box - 1.  The last reports the true I_box, numbers the slots of the
    intersections it holds (0 .. capacity) and writes nothing past the arena; the caller calls again."""
    cull = 1 if name == "cull" else 0
    cap = IC.ref_of(name, cull)["stats"][0] + delta
    ref = IC.reference(IC.cases()[name], cull, capacity=cap)
    out = IC.run_two_pass(IC.cases()[name], ref, hip_device, cull=cull, capacity=cap)
    if delta >= 0:
        _check(out, ref, f"{name} capacity {cap}")
    else:
        assert out["guards_ok"], out["broken_guards"]
        assert out["stats"][0] == ref["stats"][0] == cap + 1
        assert np.array_equal(out["cum_tiles"], ref["cum_tiles"])
        assert len(out["slots"]) == cap + 1 and np.array_equal(out["slots"], ref["slots"])


# ---- stale speculative hints ----------------------------------------------------------------------------------------
_SYNC = {}


def _sync_result(name, dev):
    if name not in _SYNC:
        _SYNC[name] = IC.run_two_pass(IC.cases()[name], IC.ref_of(name), dev)
    return _SYNC[name]


@pytest.mark.parametrize("hint", IC.HINTS)
@pytest.mark.parametrize("truth", IC.HINT_TRUTHS)
def test_a_stale_hint_changes_no_entry(hip_device, truth, hint):
    """max_tile_len_hint only selects the sort build: whatever last frame's longest list was, this frame's lists equal
    the synchronous call's entry for entry (and the reference)."""
    name = f"pile{truth}_g1"
    ref = IC.ref_of(name)
    out = IC.run_two_pass(IC.cases()[name], ref, hip_device, hint=hint)
    _check(out, ref, f"hint {hint}, longest {truth}")
    sync = _sync_result(name, hip_device)
    for k in ("cum_tiles", "tile_offsets", "flatten_ids", "isect_ids", "slots"):
        assert np.array_equal(out[k], sync[k]), k
    assert out["stats"] == sync["stats"]


@pytest.mark.parametrize("hint", (0, 40000))
def test_a_stale_hint_on_mixed_lists(hip_device, hint):
    ref = IC.ref_of("mixed")
    _check(IC.run_two_pass(IC.cases()["mixed"], ref, hip_device, hint=hint), ref, f"mixed, hint {hint}")


def test_listed_arena_too_small_hands_out_empty_lists(hip_device):
    ref = IC.ref_of("mixed")
    out = IC.run_two_pass(IC.cases()["mixed"], ref, hip_device, hint=16385, capacity_listed=ref["stats"][1] - 1)
    assert out["guards_ok"], out["broken_guards"]
    assert out["stats"] == ref["stats"]
    assert not out["tile_offsets"].any()
    poison = np.frombuffer(bytes([0x6B] * 4), np.int32)[0]
    assert (out["flatten_ids"] == poison).all()   # nothing was emitted


# ---- fused single-pass path -----------------------------------------------------------------------------------------
def _fused(s, dev, cull, hint, stride, reverse, monkeypatch):
    """SharedProjection on a fused pile with a dictated hint and key-segment stride.  -> (tl, took_fused, case dict of the
    call's own projection outputs, enumeration order the lists ended up with)."""
    import mobgs_amd.rendering as R
    n, W, H = s["means"].shape[0], s["W"], s["H"]
    tiles = (W // 16) * (H // 16)

    def forced(self, len_hint, C, N, nt, cap_box):
        self.seg_stride = stride
        return stride
    monkeypatch.setattr(R._Hints, "stride", forced)
    monkeypatch.setattr(R, "FUSED_LISTS", True)
    t = {k: torch.from_numpy(v).to(dev) for k, v in s.items() if isinstance(v, np.ndarray)}
    key = R._workload_key(dev, 1, n, W, H)
    R._hints.pop(key, None)
    rec = R.hint_record(key)
    rec.longest, rec.cap_box, rec.cap_listed = hint, tiles * n + 4096, tiles * n + 4096
    order = torch.arange(n - 1, -1, -1, dtype=torch.int32, device=dev) if reverse else None
    old = R.get_tile_culling()
    R.set_tile_culling(bool(cull))
    try:
        before = R.fused_calls[0]
        sp = R.SharedProjection(t["means"], t["quats"], t["scales"], t["opacities"], t["viewmats"], t["Ks"], W, H,
                                want_isect_ids=True, order=order)
        took = R.fused_calls[0] > before
        tl = sp.tl
        tl.resolve()
    finally:
        R.set_tile_culling(old)
        R._hints.pop(key, None)
    case = dict(means2d=sp.means2d.detach().cpu().numpy(), radii=sp.radii.cpu().numpy(),
                depths=sp.depths.detach().cpu().numpy(), conics=sp.conics.detach().cpu().numpy(),
                opacities=s["opacities"], W=W, H=H, C=1)
    used = None if tl.order is None else tl.order.cpu().numpy()
    return tl, took, case, used


def _check_fused(tl, case, used_order, cull, n, runs, what):
    ref = IC.reference(case, cull, order=used_order)
    # the edge, from the call's own projection outputs: every list has exactly n entries, the runs are as built
    assert ref["stats"] == (n * ref["nt"], n * ref["nt"], n), what
    assert (ref["lens"] == n).all(), what
    assert IC.runs_of(ref["isect_ids"][:n]) == sorted(runs), what
    if cull:
        assert (ref["sigma"] <= 0.5 * ref["tau"]).all(), what
    assert (tl.n_box, tl.n_isects, tl.max_tile_len) == ref["stats"], what
    assert np.array_equal(tl.cum_tiles.cpu().numpy(), ref["cum_tiles"]), what
    assert np.array_equal(tl.tile_offsets.cpu().numpy(), ref["tile_offsets"]), what
    assert np.array_equal(tl.flatten_ids.cpu().numpy(), ref["flatten_ids"]), what
    assert np.array_equal(tl.isect_ids.cpu().numpy(), ref["isect_ids"]), what
    assert np.array_equal(IC.slots_from_keep_scan(tl.keep_scan.cpu().numpy(), tl.n_box), ref["slots"]), what
    check_tile_order(tl.tile_order.cpu().numpy(), ref["nt"], tl.tile_offsets.cpu().numpy())


@pytest.mark.parametrize("cull", (0, 1))
@pytest.mark.parametrize("grid", IC.FUSED_GRIDS)
@pytest.mark.parametrize("n", IC.FUSED_N)
def test_fused_piles_equal_the_reference(hip_device, monkeypatch, n, grid, cull):
    """seg_stride = the longest list (no overflow, lists exact) and one below it (every list handed out empty, one
    two-pass rebuild, lists exact), each in splat order and in a reversed enumeration order."""
    runs = [(0, 2), (n - 48, 48)]
    s = IC.fused_pile(n, grid, runs)
    for reverse in (False, True):
        tl, took, case, used = _fused(s, hip_device, cull, n, n, reverse, monkeypatch)
        assert took and tl.rebuilds == 0, (reverse, "stride = longest")
        assert (used is not None) == reverse
        _check_fused(tl, case, used, cull, n, runs, f"n {n} grid {grid} cull {cull} reverse {reverse}, stride = longest")
        tl, took, case, used = _fused(s, hip_device, cull, n - 1, n - 1, reverse, monkeypatch)
        assert took and tl.rebuilds == 1, (reverse, "stride = longest - 1")
        _check_fused(tl, case, used, cull, n, runs, f"n {n} grid {grid} cull {cull} reverse {reverse}, stride = longest - 1")


@pytest.mark.parametrize("hint", (1, 513, 1025))
@pytest.mark.parametrize("n", (512, 513, 1024, 1025))
def test_fused_lists_under_each_sort_build(hip_device, monkeypatch, n, hint):
    """Lists of 512 / 513 and 1024 / 1025 entries under the 8-, 16- and 32-keys-per-lane builds of the segment sort
    (the hint picks the build; a list beyond 64 x epl entries takes the workgroup's LDS network)."""
    runs = [(5, 47)]
    s = IC.fused_pile(n, 4, runs)
    tl, took, case, used = _fused(s, hip_device, 1, hint, IC.SHORT_SORT_LDS_KEYS, False, monkeypatch)
    assert took and tl.rebuilds == 0
    _check_fused(tl, case, used, 1, n, runs, f"n {n} hint {hint}")


def test_fused_2049_overflows_and_rebuilds(hip_device, monkeypatch):
    import mobgs_amd.rendering as R
    runs = [(1000, 49)]
    s = IC.fused_pile(2049, 4, runs)
    over = R.seg_overflows[0]
    tl, took, case, used = _fused(s, hip_device, 1, 2048, IC.SHORT_SORT_LDS_KEYS, True, monkeypatch)
    assert took and tl.rebuilds == 1 and R.seg_overflows[0] == over + 1
    _check_fused(tl, case, used, 1, 2049, runs, "n 2049")


# ---- run to run -----------------------------------------------------------------------------------------------------
def _schedule(order):
    """What a schedule fixes from run to run: WHICH tiles are heavy and which light (the position of a tile among the
    tiles of its length class is the order of an atomic, and isect.hip says so)."""
    ids = np.asarray(order)
    ids = ids[ids >= 0]
    heavy = (ids & (1 << 30)) != 0
    return np.sort(ids[heavy]), np.sort(ids[~heavy])


def test_two_runs_agree_bit_for_bit(hip_device, monkeypatch):
    """The mixed case twice through the synchronous and the speculative two-pass calls, a pile twice through the fused
    path: every list output bit for bit, the slot numbering (the words of keep_scan the header defines) and the
    schedule's heavy and light sets.
    Not compared word for word, on purpose: tile_order -- a tile's position among the tiles of its length class is what
    `atomicAdd(&hist[bucket(length_of(i))], 1)` returns in tile_scan_kernel / tile_finish_kernel (mobgs_amd/csrc/isect.hip,
    the loop under "heavy = every tile in a length class above class B"), and the comment there promises a deterministic
    heavy SET only -- and the words of keep_scan past position I_box, which no call writes."""
    case, ref = IC.cases()["mixed"], IC.ref_of("mixed")
    for kw in (dict(), dict(hint=2049)):
        a, b = (IC.run_two_pass(case, ref, hip_device, **kw) for _ in range(2))
        for k in ("cum_tiles", "tile_offsets", "flatten_ids", "isect_ids", "slots"):
            assert np.array_equal(a[k], b[k]), (kw, k)
        assert a["stats"] == b["stats"]
        for x, y in zip(_schedule(a["tile_order"]), _schedule(b["tile_order"])):
            assert np.array_equal(x, y), kw
    s = IC.fused_pile(1025, 6, [(3, 48)])
    runs = []
    for _ in range(2):
        tl, took, _, _ = _fused(s, hip_device, 1, 1025, 1025, False, monkeypatch)
        assert took and tl.rebuilds == 0
        runs.append([t.cpu().numpy().copy() for t in (tl.cum_tiles, tl.tile_offsets, tl.flatten_ids, tl.isect_ids)]
                    + [IC.slots_from_keep_scan(tl.keep_scan.cpu().numpy(), tl.n_box)]
                    + list(_schedule(tl.tile_order.cpu().numpy())))
    for x, y in zip(*runs):
        assert np.array_equal(x, y)
