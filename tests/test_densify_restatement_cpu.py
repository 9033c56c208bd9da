"""tests/densify_restatement.py against the states the reference's GaussianModel recorded (tests/golden/densify.npz,
make_golden.py:gen_densify): the same sequence and the same criteria as tests/test_gpu_densify_parity.py holds the HIP
path to, so that the GPU tests which compare kernels with the restatement compare them with something the reference
has vouched for."""
import torch

import densify_restatement as R
from helpers import load

AUX = ["xyz_gradient_accum", "denom", "max_radii2D", "_deformation_table", "_deformation_accum"]


def _table(fx, tag):
    return {k[len(tag) + 1:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(tag + ".")}


def _check(state, fx, tag, loose=()):
    names = [k[len(tag) + 1:] for k in fx if k.startswith(tag + ".")]
    assert set(AUX) <= set(names) and "xyz.exp_avg_sq" in names   # (every recorded array is compared, none skipped)
    assert set(names) <= set(state), sorted(set(names) - set(state))
    for name in names:
        ref, got = torch.from_numpy(fx[f"{tag}.{name}"]), state[name]
        assert got.shape == ref.shape and got.dtype == ref.dtype, (tag, name, got.shape, ref.shape, got.dtype)
        if name in loose:
            assert torch.allclose(got, ref, rtol=2e-6, atol=2e-6), (tag, name, float((got - ref).abs().max()))
        elif name == "xyz_gradient_accum":
            assert torch.allclose(got, ref, rtol=3e-7, atol=0), (tag, name)
        else:
            assert torch.equal(got, ref), (tag, name)


def _stats(state, fx):
    for it in range(2):
        state = R.add_densification_stats(state, torch.from_numpy(fx[f"stats{it}.viewspace_grad"]),
                                          torch.from_numpy(fx[f"stats{it}.visible"]),
                                          radii=torch.from_numpy(fx[f"stats{it}.radii"]))
    return state


def test_restatement_replays_the_recorded_sequence():
    fx = load("densify")
    T = lambda k: torch.from_numpy(fx[k])  # noqa: E731
    thr, extent = float(fx["max_grad"]), float(fx["extent"])
    st = _stats(_table(fx, "s0"), fx)
    _check(st, fx, "s1")
    st["xyz_gradient_accum"] = T("s1.xyz_gradient_accum").clone()   # (later stages bit for bit, as the GPU test does)
    st = R.densify_and_clone(st, T("grads"), thr, extent)
    _check(st, fx, "s2")
    lay = {}
    st = R.densify_and_splitv2(st, T("grads"), thr, extent, 2, T("split.samples"), layout=lay)
    assert lay["children"] == T("split.samples").shape[0] > 0 and lay["clones"] == 0
    _check(st, fx, "s3", loose=("xyz", "scaling"))
    st["xyz"], st["scaling"] = T("s3.xyz").clone(), T("s3.scaling").clone()
    st = R.prune_points(st, T("prune.mask"))
    _check(st, fx, "s4")
    st = R.reset_opacity(st)
    _check(st, fx, "s5", loose=("opacity",))


def test_restatement_fused_pruneclone_reaches_the_recorded_split_state():
    fx = load("densify")
    lay = {}
    st = R.densify_pruneclone(_table(fx, "s1"), float(fx["max_grad"]), float(fx["extent"]), 2,
                              torch.from_numpy(fx["split.samples"]), layout=lay)
    assert lay["clones"] > 0 and lay["children"] == fx["split.samples"].shape[0]
    assert lay["kept"] + lay["clones"] + lay["children"] == fx["s3.xyz"].shape[0]
    _check(st, fx, "s3", loose=("xyz", "scaling"))


def test_restatement_leaves_its_input_alone_and_new_rows_start_from_zero():
    fx = load("densify")
    s1 = _table(fx, "s1")
    before = {k: v.clone() for k, v in s1.items()}
    lay = {}
    st = R.densify_pruneclone(s1, float(fx["max_grad"]), float(fx["extent"]), 3,
                              torch.from_numpy(fx["split.samples"]).repeat(2, 1)[:3 * fx["split.samples"].shape[0] // 2],
                              layout=lay)
    assert all(torch.equal(s1[k], before[k]) for k in before)
    new = slice(lay["kept"], None)
    for k, v in st.items():
        if k.endswith(".exp_avg") or k.endswith(".exp_avg_sq"):
            assert not v[new].any() and v[:lay["kept"]].any(), k
        if k in R.STATS:
            assert not v.any(), k
    assert lay["children"] == 3 * (lay["children"] // 3) and lay["parents"].shape[0] == lay["children"]


def test_split_allowance_is_three_times_the_measured_fp32_gap():
    """The bound of the GPU split tests: torch's fp32 evaluation of the split formulas against the float64 one, on the
    very inputs of tests/test_gpu_densify_kernels.py (observed 2.73e-7 of |xyz| + |sample|_1 and 1.16e-7 of
    1 + |scaling|)."""
    gx, gs = R.split_fp32_gap()
    print(f"fp32 vs float64 split children: xyz {gx:.3e}, scaling {gs:.3e}")
    for got, noted, allowed in zip((gx, gs), R.SPLIT_OBSERVED, R.SPLIT_ALLOWED):
        # (another host's vectorised exp / log may differ in the last bit: the noted figure within a factor of 1.5)
        assert noted / 1.5 <= got <= 1.5 * noted and allowed == 3 * noted


def test_selection_edges_decide_as_documented():
    """0 / 0 counts as 0, x / 0 as +-inf, g == thr is hot and one ulp below is not; a clone goes by |g|, a split by the
    signed g (the rows tests/test_gpu_densify_kernels.py plants)."""
    thr = torch.tensor(2.0e-4, dtype=torch.float32)
    below = torch.nextafter(thr, torch.tensor(0.0))
    accum = torch.tensor([0.0, 3e-4, -3e-4, thr, below, -thr, -below, -1e-3, 2 * thr])
    denom = torch.tensor([0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 2.0])
    g = R.mean_grads(accum, denom)
    small = torch.full((9, 3), -6.0)
    clone, split = R.select(small, g, 2.0e-4, 0.04)
    assert clone.tolist() == [False, True, True, True, False, True, False, True, True] and not bool(split.any())
    clone, split = R.select(small + 6.0, g, 2.0e-4, 0.04)
    assert split.tolist() == [False, True, False, True, False, False, False, False, True] and not bool(clone.any())
    clone, split = R.select(small + 6.0, g[:3], 2.0e-4, 0.04)     # rows past the gradients count as 0
    assert split.tolist() == [False, True, False] + [False] * 6
