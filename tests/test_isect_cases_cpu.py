"""The constructed tile-list cases (tests/isect_cases.py) prove themselves without a GPU: the numpy restatement equals
the C oracle, and every case reaches the edge it names -- asserted from the reference alone."""
import numpy as np
import pytest

import isect_cases as IC

NAMES = IC.case_names()


def test_thresholds_the_cases_aim_at():
    """Restated once here: the values pinned by the static_asserts on sort_plan / short_sort_epl in
    mobgs_amd/csrc/isect_launch.h (512, 1024, 2048, 12288, 16384) and the constants RADIX_MAX_RUN (48) and OWNER_LDS
    (4096) of isect.hip.  A retuned header means new cases."""
    assert IC.THRESHOLDS == dict(EPL8_MAX=512, EPL16_MAX=1024, SHORT_SORT_LDS_KEYS=2048, HUGE_FROM=12288,
                                 LONG_SORT_LDS_KEYS=16384, RADIX_MAX_RUN=48, OWNER_LDS=4096)
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mobgs_amd", "csrc")
    head = open(os.path.join(root, "isect_launch.h")).read()
    body = open(os.path.join(root, "isect.hip")).read()
    for text, pat, want in ((head, r"SHORT_SORT_LDS_KEYS = (\d+)", 2048), (head, r"LONG_SORT_LDS_KEYS = (\d+)", 16384),
                            (head, r"DENSE_MAX_TILES = (\d+)", 8192), (head, r"TC_COPIES = (\d+)", 8),
                            (body, r"RADIX_MAX_RUN = (\d+)", 48), (body, r"OWNER_LDS = (\d+)", 4096),
                            (body, r"RADIX_CAP = (\d+)", 16384)):
        assert int(re.search(pat, text).group(1)) == want, pat
    for frag in ("sort_plan(512, 1, 1).epl == 8 && sort_plan(513, 1, 1).epl == 16",
                 "sort_plan(1024, 1, 1).epl == 16 && sort_plan(1025, 1, 1).epl == 32",
                 "!sort_plan(12288, 12, 8).huge && sort_plan(12289, 12, 8).huge"):
        assert frag in head, frag
    # every arm switch and the first merge-pass steps have a pile on both sides
    for edge in (64, 512, 1024, 2048, 12288, 16384, 32768):
        assert edge in IC.PILE_N and edge + 1 in IC.PILE_N, edge
    assert 65537 in IC.PILE_N   # beyond 16384 << 2


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_the_c_oracle(name):
    from oracle import gsplat_cpu
    case, ref = IC.cases()[name], IC.ref_of(name)
    tpg, ids, flat, offs = gsplat_cpu.isect(case["means2d"], case["radii"], case["depths"], case["W"], case["H"])
    assert np.array_equal(tpg.reshape(-1), ref["tiles_per_gauss"])
    assert np.array_equal(ids, ref["isect_ids"])
    assert np.array_equal(flat, ref["flatten_ids"])
    assert np.array_equal(offs.reshape(-1), ref["tile_offsets"][:-1])
    assert ref["stats"][0] == ref["stats"][1] == len(flat) == int(ref["tile_offsets"][-1])
    assert np.array_equal(ref["slots"], np.arange(ref["stats"][0] + 1))


@pytest.mark.parametrize("name", NAMES)
def test_rects_sit_a_quarter_tile_from_a_rounding_seam(name):
    case = IC.cases()[name]
    m = case["means2d"].reshape(-1, 2).astype(np.float64)
    r = case["radii"].reshape(-1).astype(np.float64)
    vis = r > 0
    for v in ((m[vis, 0] - r[vis]) / 16, (m[vis, 0] + r[vis]) / 16, (m[vis, 1] - r[vis]) / 16, (m[vis, 1] + r[vis]) / 16):
        assert (np.abs(v - np.round(v)) >= 0.25).all()


def _tile_lists(ref):
    off = ref["tile_offsets"]
    return [ref["isect_ids"][off[t]:off[t + 1]] for t in range(ref["nt"])]


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_edge(name):
    case, ref = IC.cases()[name], IC.ref_of(name)
    e = case["edge"]
    I_box, I_listed, longest = ref["stats"]
    if "longest" in e:
        assert longest == e["longest"]
    if "lists" in e:   # piles: EVERY list has exactly that length
        assert ref["nt"] == e["lists"] and (ref["lens"] == e["longest"]).all()
    if "lens" in e:
        assert ref["lens"].tolist() == e["lens"]
    lists = _tile_lists(ref)
    if "runs" in e:   # exactly these runs of equal depth bits, at these positions of the sorted list; inside: by flat id
        assert IC.runs_of(lists[0]) == sorted(e["runs"])
        for p, length in e["runs"]:
            ids = ref["flatten_ids"][p:p + length]
            assert (np.diff(ids) > 0).all()
        lens = [length for _, length in e["runs"]]
        assert max(lens) <= IC.RADIX_MAX_RUN or 49 in lens
        if "desc_chunks" in e:
            # The run reaches the sort with FALLING ids, whatever the atomics do: a member's four intersections lie in ONE
            # bin_kernel chunk, the chunk ranks through counter copy chunk & 7, and a tile's segment is laid out copy by
            # copy (tile_scan_kernel: tile_base[c * nt + i] = at; at += cnt[c]) -- so a member of a lower copy precedes a
            # member of a higher copy in the sort's input.  Asserted: lower copy <=> higher id, for every pair of members
            # in different copies, and more than one copy.  The list takes radix_sort_long (2048 < n <= 16384).
            (p, length), = e["runs"]
            ids = ref["flatten_ids"][p:p + length].astype(np.int64)
            cum = ref["cum_tiles"].astype(np.int64)
            first, last = cum[ids] >> 11, (cum[ids] + ref["tiles_per_gauss"][ids] - 1) >> 11
            assert (first == last).all()
            assert sorted(set(first.tolist()), reverse=True) == list(e["desc_chunks"])
            copy = first & 7
            assert len(set(copy.tolist())) == len(e["desc_chunks"]) >= 2
            a, b = np.meshgrid(np.arange(length), np.arange(length), indexing="ij")
            differ = copy[a] != copy[b]
            assert ((copy[a] < copy[b]) == (ids[a] > ids[b]))[differ].all()
            assert IC.SHORT_SORT_LDS_KEYS < longest <= IC.LONG_SORT_LDS_KEYS and ref["nt"] == 4
            assert length in (48, 49)
    elif "pattern" in e:
        bits = case["depths"].reshape(-1).view(np.uint32)
        varying = [b for b in range(4) if len(np.unique((bits >> (8 * b)) & 255)) > 1]
        assert varying == dict(byte0=[0], byte3=[3], bytes12=[1, 2], bytes0123=[0, 1, 2, 3], equal=[])[e["pattern"]]
        runs = [length for _, length in IC.runs_of(lists[0])]
        if e["pattern"] == "equal":
            assert runs == [3000]
        else:
            assert max(runs, default=0) <= 24   # below RADIX_MAX_RUN: the radix fix-up, not the fallback
    elif name.startswith("pile") or name == "mixed":
        assert all(IC.runs_of(l) == [] for l in lists)
    if name.endswith("_sorted"):
        assert (np.diff(case["depths"].reshape(-1).view(np.uint32).astype(np.int64)) > 0).all()
    if name.endswith("_reversed"):
        assert (np.diff(case["depths"].reshape(-1).view(np.uint32).astype(np.int64)) < 0).all()
    if "ibox" in e:
        assert I_box == e["ibox"]
        if name.startswith("ibox"):
            assert I_box % 2048 == {2047: 2047, 2048: 0, 2049: 1, 4096: 0, 6144: 0}[I_box]
    if "span" in e:
        assert IC.chunk_owner_span(ref, 0) == e["span"] and I_box > 2048
        assert (e["span"] <= IC.OWNER_LDS) == (e["span"] in (4095, 4096))
        radii = case["radii"].reshape(-1)
        assert (radii[-e["trailing"]:] == 0).all() and radii[-e["trailing"] - 1] > 0   # trailing invisible splats
    if "scan_chunks" in e:
        n = case["radii"].size
        assert -(-n // IC.KEEP_CHUNK) == e["scan_chunks"] > IC.SCAN_LOOKBACK
        assert int((case["radii"] > 0).sum()) == 300 and case["radii"].reshape(-1)[-1] == 0
    if "wide" in e:
        assert ref["tiles_per_gauss"][e["wide_id"]] == e["wide"] > IC.KEEP_CHUNK
        start = int(ref["cum_tiles"][e["wide_id"]])
        inside = [c for c in range(1, I_box // 2048 + 1) if start < c * 2048 < start + e["wide"]]
        assert len(inside) >= (1 if e["wide"] == 3072 else 16)   # chunk starts inside the one splat
        assert e["wide"] == 3072 or ref["nt"] > IC.DENSE_MAX_TILES
    if "widths" in e:
        x0, _, x1, _ = IC.tile_rects(case["means2d"].reshape(-1, 2), case["radii"].reshape(-1), ref["tile_w"], ref["tile_h"])
        assert (x1 - x0).tolist() == e["widths"]
    if "counts" in e:
        N = case["radii"].shape[1]
        cam = ref["owner"] // N
        assert np.bincount(cam, minlength=3).tolist() == list(e["counts"])
        assert ref["nt"] <= IC.DENSE_MAX_TILES
        assert sorted(np.flatnonzero(ref["lens"]).tolist()) == [1, 16 + 6, 32 + 11]   # a pile per camera, different tiles
        if "boundary_inside_cam" in e:
            b = e["boundary"]
            assert b % 2048 == 0 and cam[b - 1] == cam[b] == e["boundary_inside_cam"]
            assert cam[b - 2048] == cam[b - 1]   # ... and that chunk lies in one camera
        if "straddle" in e:
            c = e["chunk"]
            assert cam[c * 2048] == e["straddle"][0] and e["straddle"][1] in cam[c * 2048:(c + 1) * 2048]


def test_culling_case_has_a_factor_two_margin_everywhere():
    """For every (splat, tile) pair of the culling case the float64 minimum of sigma over the tile's pixel-centre
    rectangle is at most HALF of ln(255 op) (kept) or at least TWICE it, plus 0.1 (dropped: the kernel's threshold is
    1.02 ln(255 op) + 0.05, so for op = 1/255, ln = 0, "twice" alone would say nothing) -- or the opacity test / the
    degenerate conic decides.  The kept set is therefore known exactly."""
    case, ref = IC.cases()["cull"], IC.ref_of("cull", 1)
    sigma, tau, deg, keep = ref["sigma"], ref["tau"], ref["degenerate"], ref["keep"]
    listed = np.isfinite(tau)
    by_sigma = listed & ~deg
    assert (sigma[by_sigma & keep] <= 0.5 * tau[by_sigma & keep]).all()
    assert (sigma[by_sigma & ~keep] >= 2.0 * tau[by_sigma & ~keep] + 0.1).all()
    assert keep[listed & deg].all() and not keep[~listed].any()
    kinds = case["edge"]["kinds"][ref["owner"]]
    per_kind = {k: int(keep[kinds == k].sum()) / max(1, int((np.diff(ref["owner"][kinds == k], prepend=-1) != 0).sum()))
                for k in range(9)}
    assert per_kind == {0: 9, 1: 1, 2: 0, 3: 0, 4: 0, 5: 1, 6: 1, 7: 9, 8: 9}
    assert np.isnan(case["opacities"]).any() and (case["opacities"] == IC.OP_EXACT).any()
    assert 0 < IC.OP_BELOW < IC.OP_EXACT
    # kept and dropped inside chunk 0 and on both sides of position 2048; chunk 2 keeps nothing; the lists end mixed
    assert keep[:2048].any() and (~keep[:2048]).any() and keep[2048:2200].any() and (~keep[2048:2200]).any()
    c = case["edge"]["empty_chunk"]
    assert not keep[c * 2048:(c + 1) * 2048].any() and len(keep) > (c + 1) * 2048
    assert keep[(c + 1) * 2048:].any()
    assert 0 < ref["stats"][1] < ref["stats"][0]
    assert ref["slots"][-1] == ref["stats"][1] and len(ref["slots"]) == ref["stats"][0] + 1


def test_capacity_truncation_is_restated():
    """capacity = I_box - 1: the true I_box is reported, the flags stop at the arena."""
    ref = IC.reference(IC.cases()["ibox2048"], capacity=2047)
    assert ref["stats"][0] == 2048 and len(ref["slots"]) == 2048 and ref["stats"][1] == 2047


def test_hint_matrix_truths_are_pile_cases():
    for n in IC.HINT_TRUTHS:
        assert IC.ref_of(f"pile{n}_g1")["stats"] == (n, n, n)
    assert IC.HINTS == (0, 512, 513, 1025, 2049, 12289, 40000)


@pytest.mark.parametrize("grid", IC.FUSED_GRIDS)
def test_fused_piles_fill_the_counter_copies_they_name(grid):
    """Every splat of a fused pile covers every tile, so the intersections are enumerated splat-major and chunk c holds
    those of splats c * 2048 / tiles ...: one chunk (one counter copy) on the 1-tile image, all 8 copies on the 6x6 image
    at every N, and on the 4x4 image from N = 1023 on."""
    tiles = grid * grid
    for n in IC.FUSED_N:
        chunks = -(-n * tiles // IC.KEEP_CHUNK)
        if grid == 1:
            assert chunks == 1
        elif grid == 6:
            assert chunks >= IC.TC_COPIES
        else:
            assert (chunks >= IC.TC_COPIES) == (n >= 1023)
        s = IC.fused_pile(n, grid, runs=[(0, 2), (n - 48, 48)])
        z = np.sort(s["means"][:, 2].view(np.uint32))
        assert IC.runs_of(z) == [(0, 2), (n - 48, 48)] and (s["means"][:, 2] >= 1).all() and (s["means"][:, 2] < 2).all()
