"""The regularisation terms without a GPU: the fixture (tests/golden/regterms.npz, make_golden_regterms.py) replayed
through the restatement -- fp32 bit for bit against the reference's recorded values and gradients, float64 against the
recorded truth --, the C ABI's size query and refusals, and the public names with their refusal of host tensors."""
import ctypes

import numpy as np
import pytest
import torch

import regterms_restatement as RR
from helpers import load, same_bits

GRADS = ("g_depth", "g_alpha", "g_entropy", "g_sparsity")


@pytest.fixture(scope="module")
def fx():
    return load("regterms")


LOG_FREE = ("depth_loss", "sparsity", "g_depth", "g_sparsity")     # +, -, *, /, abs, sign: the same bits on every CPU


def same_log_as_the_generator(fx):
    """torch.log on the CPU goes through a vector math library that is chosen by the processor it runs on, and two of
    them differ in the last bit for a few per cent of the arguments.  The fixture records what the generating machine
    gave for the 3922 arguments of case 1: where this machine gives the same, it evaluates the reference's statements
    as the generator did."""
    c, _ = RR.fixture_case(fx, 1)
    return same_bits(torch.log(c["alpha"].reshape(-1) + RR.EPS), fx["log_probe"])


@pytest.mark.parametrize("i", range(len(RR.CASES)))
def test_fp32_restatement_reproduces_the_reference(fx, i):
    """Bit for bit.  On a processor whose logarithm rounds differently from the generator's (see above) that cannot
    hold for the values that pass through a logarithm; those are then held to the rounding chain of an fp32 result,
    8 x 2^-24 (relative; of the largest magnitude for a map; in dB for the PSNR), and the others still to the bit."""
    c, want = RR.fixture_case(fx, i)
    B, H, W = RR.CASES[i]
    assert tuple(fx["shapes"][i]) == (B, H, W) and c["alpha"].shape == (B, 1, H, W) and c["image"].shape == (B, 3, H, W)
    got = RR.block(c["depth"], c["gt_depth"], c["alpha"], c["image"], c["gt_image"], torch.float32)
    got.update({k: v for k, v in RR.alone(c["alpha"], torch.float32).items() if k.startswith("g_")})
    same_log = same_log_as_the_generator(fx)
    for k in RR.SCALARS + ("psnr",) + GRADS:
        assert got[k].dtype == torch.float32
        ref = torch.from_numpy(want["ref_" + k])
        mine = got[k].reshape(ref.shape)
        if same_log or k in LOG_FREE:
            assert same_bits(mine, ref), k
        elif k == "psnr":
            assert RR.db_gap(mine, ref) <= RR.FLOOR_DB, k
        else:
            assert RR.map_gap(mine, ref) <= RR.FLOOR, k
    alone = RR.alone(c["alpha"], torch.float32)
    assert torch.equal(alone["entropy"], got["entropy"]) and torch.equal(alone["sparsity"], got["sparsity"])


@pytest.mark.parametrize("i", range(len(RR.CASES)))
def test_float64_restatement_matches_the_fixture(fx, i):
    c, want = RR.fixture_case(fx, i)
    got = RR.block(c["depth"], c["gt_depth"], c["alpha"], c["image"], c["gt_image"], torch.float64)
    got.update({k: v for k, v in RR.alone(c["alpha"], torch.float64).items() if k.startswith("g_")})
    for k in RR.SCALARS + ("psnr",) + GRADS:
        assert got[k].dtype == torch.float64 and want["f64_" + k].dtype == np.float64
        assert np.array_equal(got[k].numpy().reshape(want["f64_" + k].shape), want["f64_" + k]), k
    # the recorded gaps are the distances between the two recorded results
    for k in RR.SCALARS:
        assert want["ref_gap_" + k][0] == RR.rel_gap(want["ref_" + k][0], want["f64_" + k][0])
    for k in GRADS:
        assert want["ref_gap_" + k][0] == RR.map_gap(want["ref_" + k], want["f64_" + k])
    assert want["ref_gap_psnr"][0] == RR.db_gap(want["ref_psnr"], want["f64_psnr"])


def test_fixture_holds_the_edge_values(fx):
    eps32 = np.float32(1e-6)
    for i, (B, H, W) in enumerate(RR.CASES):
        c, want = RR.fixture_case(fx, i)
        a = c["alpha"].numpy()
        assert (a[:, :, ::3, :] == 0).all() and (a == 1).any() and (a == np.float32(1) + np.float32(2.0 ** -23)).sum() == 1
        assert (a == np.float32(1e-30)).sum() == 1 and ((a > 0) & (a < eps32)).sum() >= 2
        d = (c["depth"] - c["gt_depth"]).numpy()
        assert (d == 0).any() and (d > 0).any() and (d < 0).any()
        g = want["ref_g_depth"]
        assert set(np.unique(np.abs(g)).tolist()) == {0.0, float(np.float32(0.2) / np.float32(B * H * W))}
        assert ((g == 0) == (d == 0)).all()
    assert (3 * 37 * 53) % 4 != 0           # the second image of case 1 does not start on a 16-byte boundary
    assert np.isnan(fx["nan_ref_entropy"][0]) and fx["nan_in_alpha"].tolist().count(1.5) == 1
    assert np.isnan(fx["nan_ref_g_entropy"]).tolist() == [False, True, False, False]


def test_tolerance_rule():
    assert RR.FLOOR == 8 * 2.0 ** -24 and RR.allowed(0.0) == RR.FLOOR and RR.allowed(1e-6) == 3e-6
    assert RR.allowed(1e-7) == RR.FLOOR and RR.allowed(0.0, RR.FLOOR_DB) == 10 / np.log(10) * 8 * 2.0 ** -24


def test_abi_entries_blocks_and_refusals():
    from mobgs_amd import _lib, build
    assert "regterms.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["regterms.hip"]
    h = _lib.load()
    assert _lib.ABI_VERSION >= 14 and h.mobgs_abi_version() == _lib.ABI_VERSION
    for name in ("mobgs_reg_terms_blocks", "mobgs_reg_terms_fwd", "mobgs_reg_terms_bwd"):
        assert name in _lib._SIGS and hasattr(h, name)
    # the size query: a host computation, monotone, capped, 0 for a size outside the range
    ns = [1, 2, 15, 1023, 1024, 1025, 1961, 15360, 512 * 288 * 2, 1352 * 1014 * 2, 1 << 22, 1 << 31, 1 << 40]
    nb = [h.mobgs_reg_terms_blocks(n) for n in ns]
    assert nb[0] == 1 and all(b >= a for a, b in zip(nb, nb[1:])) and nb[-1] == nb[-2] == nb[-3] <= 2048
    assert nb[ns.index(1024)] == 1 and nb[ns.index(1025)] == 2
    assert [h.mobgs_reg_terms_blocks(n) for n in (0, -1, (1 << 40) + 1)] == [0, 0, 0]
    none = ctypes.c_void_p(None)
    buf = (ctypes.c_double * 64)()                     # host memory: every call below is refused before any launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 2)
    both = 3

    def fwd(n_d=8, depth=p, gt=p, n_a=8, alpha=p, terms=both, B=0, H=0, W=0, image=none, gt_image=none, partial=p,
            out=p):
        return h.mobgs_reg_terms_fwd(n_d, depth, gt, n_a, alpha, terms, 0.2, 1e-7, 1e-7, B, H, W, image, gt_image,
                                     partial, out, none)

    def bwd(n_d=8, depth=p, gt=p, n_a=8, alpha=p, terms=both, v_loss=p, v_depth=p, v_alpha=p):
        return h.mobgs_reg_terms_bwd(n_d, depth, gt, n_a, alpha, terms, 0.2, 1e-7, 1e-7, v_loss, v_depth, v_alpha, none)

    refused = [
        (fwd, dict(n_d=0)), (fwd, dict(n_d=-4)), (fwd, dict(n_a=0)), (fwd, dict(n_a=(1 << 40) + 1)),
        (fwd, dict(gt=none)), (fwd, dict(depth=none)), (fwd, dict(depth=none, gt=none, n_d=5)),
        (fwd, dict(alpha=none, n_a=0)), (fwd, dict(terms=0)), (fwd, dict(terms=4)),
        (fwd, dict(depth=none, gt=none, n_d=0, alpha=none, n_a=0, terms=0)),
        (fwd, dict(image=p, gt_image=p)), (fwd, dict(image=p, gt_image=p, B=2, H=0, W=5)),
        (fwd, dict(image=p, gt_image=p, B=65, H=2, W=2)), (fwd, dict(image=p, B=1, H=2, W=2)), (fwd, dict(B=2, H=4, W=4)),
        (fwd, dict(partial=none)), (fwd, dict(out=none)), (fwd, dict(depth=odd)), (fwd, dict(alpha=odd)),
        (fwd, dict(partial=ctypes.c_void_p(p.value + 4))),
        (bwd, dict(n_d=0)), (bwd, dict(n_a=-1)), (bwd, dict(gt=none)), (bwd, dict(terms=8)), (bwd, dict(v_loss=none)),
        (bwd, dict(v_depth=none, v_alpha=none)), (bwd, dict(depth=none, gt=none, n_d=0)),
        (bwd, dict(alpha=none, n_a=0, terms=0)), (bwd, dict(v_alpha=odd)),
    ]
    for fn, kw in refused:
        assert fn(**kw) == -1, (fn.__name__, kw)
        assert ("mobgs_reg_terms_" + fn.__name__ + ":").encode() in h.mobgs_last_error(), (fn.__name__, kw)


def test_public_names_and_refusal_of_host_tensors():
    from mobgs_amd.loss_utils import entropy_loss, regularisation_terms, sparsity_loss
    a = torch.rand(2, 1, 4, 5)
    for fn in (entropy_loss, sparsity_loss):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(a)
        with pytest.raises(ValueError, match="non-empty"):
            fn(a[:0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        regularisation_terms(a, a.clone(), a.clone())
    assert regularisation_terms.__kwdefaults__ == {"depth_weight": 0.2, "entropy_weight": 1e-7, "sparsity_weight": 1e-7,
                                                   "image": None, "gt_image": None}
