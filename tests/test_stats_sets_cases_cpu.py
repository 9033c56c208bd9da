"""Vets tests/stats_sets_cases.py, the inputs and expectations of tests/test_gpu_densify_stats_sets.py, on the CPU: the
restatement of mobgs_densify_stats_sets is control_cases.batch_stats once per set; the fp32-coded radii of a gradient
message give the same arrays as the int32 ones; on the `exact` family a chain of rounded fp32 operations IS the float64
restatement (so the GPU test owes torch.equal there), on the `random` family it is within the existing test's rtol; and
the case list holds what the GPU test needs."""
import pytest
import torch

import control_cases as C
import stats_sets_cases as S


def test_the_case_list_covers_block_edges_the_seam_and_both_encodings():
    assert set(S.SETS_ROWS) == {(257, 255), (0, 300), (300, 0), (1, 1), (1025, 63)}
    assert set(S.VIEWS) == {1, 2, 16} and set(S.STRIDES) == {2, 3}   # 16 = MOBGS_STATS_MAX_VIEWS
    assert len(S.CASES) == len(S.SETS_ROWS) * 3 * 2 * 2 and {c[4] for c in S.CASES} == {"INT32", "FP32"}
    assert any(ns % 256 and nd for ns, nd in S.SETS_ROWS)            # a workgroup that holds rows of both sets
    assert any((ns + nd) % 256 == 0 for ns, nd in S.SETS_ROWS)       # a full last workgroup
    assert any(ns == 0 for ns, _ in S.SETS_ROWS) and any(nd == 0 for _, nd in S.SETS_ROWS)


@pytest.mark.parametrize("ns,nd", S.SETS_ROWS)
@pytest.mark.parametrize("n_views", S.VIEWS)
def test_planted_rows_and_radii_values(ns, nd, n_views):
    _, grads, radii, planted = S.inputs(ns, nd, n_views, 3, "exact", 1)
    stacked = torch.stack(radii)
    assert stacked.shape == (n_views, ns + nd + S.PAD) and all(g.shape == (ns + nd + S.PAD, 3) for g in grads)
    for row in planted.get(0, []):      # visible only in the last view, at the largest radius
        assert int(stacked[-1, row]) == S.BIG and bool((stacked[:-1, row] <= 0).all())
    for row in planted.get(1, []):      # visible in none
        assert bool((stacked[:, row] <= 0).all())
    for row in planted.get(2, []):
        assert int(stacked[0, row]) == 1 and bool((stacked[1:, row] == 0).all())
    assert planted.get(0) and planted.get(1), "every case has a last-view-only row and an invisible row"
    values = set(stacked.reshape(-1).tolist())
    assert {0, S.BIG} <= values and (ns + nd < 3 or 1 in values)
    assert int(stacked.abs().max()) < 2 ** 24
    assert all(bool((g[:, 2:] == 1e30).all()) for g in grads)


@pytest.mark.parametrize("family", ["exact", "random"])
@pytest.mark.parametrize("ns,nd", S.SETS_ROWS)
@pytest.mark.parametrize("n_views", S.VIEWS)
def test_coded_radii_give_the_arrays_of_the_int32_ones(ns, nd, n_views, family):
    states, grads, radii, _ = S.inputs(ns, nd, n_views, 2, family, 7 + n_views)
    fp = S.coded(radii)
    assert all(f.dtype == torch.float32 and torch.equal(f.to(torch.int32), r) for f, r in zip(fp, radii))   # exact both ways
    want, vis = S.expected(states, grads, radii, ns, nd)
    got, vis_fp = S.expected(states, grads, fp, ns, nd)
    for a, b, va, vb in zip(want, got, vis, vis_fp):
        assert torch.equal(va, vb)
        assert set(a) == set(b) and all(a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]) for k in a)
    # the slot of a message is the gradient rows followed by the coded radii
    n = ns + nd + S.PAD
    s = S.slot(grads[0], fp[0])
    assert s.shape == (3 * n,) and torch.equal(s[:2 * n].view(n, 2), grads[0]) and torch.equal(s[2 * n:], fp[0])


@pytest.mark.parametrize("ns,nd", S.SETS_ROWS)
@pytest.mark.parametrize("n_views", S.VIEWS)
@pytest.mark.parametrize("stride", S.STRIDES)
def test_on_the_exact_family_rounded_fp32_operations_are_the_restatement(ns, nd, n_views, stride):
    states, grads, radii, _ = S.inputs(ns, nd, n_views, stride, "exact", 100 * n_views + stride)
    want, vis = S.expected(states, grads, radii, ns, nd)
    chain = S.fp32_chain(states, grads, radii, ns, nd)
    for a, b in zip(want, chain):
        assert all(torch.equal(a[k], b[k]) for k in a)
    # ... and the order of the views does not matter there, nor does float64: every partial sum is an integer x 2^-20
    total = sum(g[:, :2].double() for g in grads)
    assert torch.equal(total.float().double(), total)
    scaled = total[:ns + nd] * torch.tensor([S.WIDTH * 0.5, S.HEIGHT * 0.5], dtype=torch.float64)
    root = torch.sqrt((scaled ** 2).sum(1))
    assert torch.equal(root * root, (scaled ** 2).sum(1)) and torch.equal(root.float().double(), root)
    # something happens: visible rows exist, invisible rows exist, and the accumulators move
    seen = torch.cat(vis)
    assert bool(seen.any()) and bool((~seen).any())
    moved = torch.cat([w["xyz_gradient_accum"] != s["xyz_gradient_accum"] for w, s in zip(want, states)])
    assert ns + nd < 200 or int(moved.sum()) > (ns + nd) // 4


@pytest.mark.parametrize("ns,nd", [(257, 255), (1025, 63)])
@pytest.mark.parametrize("n_views", [2, 16])
def test_on_the_random_family_the_chain_stays_within_the_existing_bound(ns, nd, n_views):
    states, grads, radii, _ = S.inputs(ns, nd, n_views, 2, "random", 5)
    want, _ = S.expected(states, grads, radii, ns, nd)
    chain = S.fp32_chain(states, grads, radii, ns, nd)
    differs = False
    for a, b in zip(want, chain):
        assert torch.equal(a["denom"], b["denom"]) and torch.equal(a["max_radii2D"], b["max_radii2D"])
        assert torch.allclose(a["xyz_gradient_accum"], b["xyz_gradient_accum"], rtol=3e-7, atol=0)
        differs = differs or not torch.equal(a["xyz_gradient_accum"], b["xyz_gradient_accum"])
    assert differs, "the random family is there because its roundings show"
