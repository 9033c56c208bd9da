"""The cross-lane primitives live in mobgs_amd/csrc/wave_shared.h and nowhere else: read as text, the kernel files hold no
second copy of the wave fence, of an xor butterfly or of a DPP / permlane-swap reduction.  Kernels that promise each other
bit-identical results keep that promise by calling one definition; a private copy "kept in sync by a comment" is the
thing this file is here to refuse."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mobgs_amd", "csrc")
HEADER = "wave_shared.h"

BUILTINS = ("__builtin_amdgcn_wave_barrier", "__builtin_amdgcn_update_dpp", "__builtin_amdgcn_permlane16_swap",
            "__builtin_amdgcn_permlane32_swap")

# file -> ({builtin: occurrences}, reason).  Two entries, and not to be extended: a new cross-lane step goes into the header.
ALLOWED = {
    "isect.hip": ({"__builtin_amdgcn_permlane16_swap": 1, "__builtin_amdgcn_permlane32_swap": 1},
                  "lane_xor32, the partner fetch of the in-register bitonic network: it SELECTS one of the two swap results "
                  "by the lane's own bit instead of adding them; its DPP moves are the header's dpp_mov"),
    "raster_bwd_mfma.hip": ({"__builtin_amdgcn_permlane16_swap": 1, "__builtin_amdgcn_permlane32_swap": 1},
                            "the block combine of the MFMA accumulators: the order of its two swaps and adds is part of "
                            "that kernel's fixed summation order"),
}

OLD_NAMES = ("l_fence", "fl_wave_fence", "wave_lds_order", "dec_wave_fence", "l_eval", "LEval", "l_dpp_add", "l_wave_reduce",
             "l_wave_allreduce", "wave_sum_f", "wave_max_i", "allow_lds", "allow_dynamic_lds")

SHARED = ("wave_lds_fence", "wave_sum", "wave_min", "wave_max", "dpp_add", "dpp_mov", "row_allreduce", "wave_allreduce",
          "half_wave_sum", "wave_reduce_components", "wave_reduce_pair")

# for (int X = 32 | MOBGS_WAVE / 2; ...) ... __shfl_xor(.., X, 64 | MOBGS_WAVE) within the next few lines
LOOP_HEAD = re.compile(r"for\s*\(\s*int\s+(\w+)\s*=\s*(?:32|MOBGS_WAVE\s*/\s*2)\s*;")


def _sources():
    out = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h", ".cpp")):
            with open(os.path.join(CSRC, name)) as f:
                out[name] = f.read()
    assert HEADER in out and len(out) > 30
    return out


def _butterflies(text):
    found = []
    for m in LOOP_HEAD.finditer(text):
        window = text[m.end():m.end() + 400]
        if re.search(r"__shfl_xor\s*\([^;]*?,\s*%s\s*,\s*(?:64|MOBGS_WAVE)\s*\)" % re.escape(m.group(1)), window):
            found.append(text.count("\n", 0, m.start()) + 1)
    return found


def _defines(text, name):
    return len(re.findall(r"^(?:__host__ |__device__ |inline |static |__forceinline__ )+[\w:<>]+\s+%s\s*\(" % name, text,
                          re.MULTILINE))


def test_the_pattern_finds_a_butterfly():
    """The search itself: it sees the header's loop and the spellings a hand-written copy takes, and leaves the shorter
    row-local and one-step shuffles alone."""
    assert len(_butterflies(_sources()[HEADER])) == 1
    assert _butterflies("#pragma unroll\n    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);\n") == [2]
    assert _butterflies("for (int s = 32; s >= 1; s >>= 1) v = fminf(v, __shfl_xor(v, s, 64));") == [1]
    assert _butterflies("for (int off = MOBGS_WAVE / 2; off > 0; off >>= 1) {\n    lo = fminf(lo, __shfl_xor(lo, off, "
                        "MOBGS_WAVE));\n}") == [1]
    assert _butterflies("for (int off = 8; off > 0; off >>= 1) top = max(top, __shfl_xor(top, off, 64));") == []
    assert _butterflies("gb0 += __shfl_xor(gb0, 32, 64);") == []


def test_cross_lane_builtins_only_in_the_header():
    assert len(ALLOWED) <= 2 and all(reason for _, reason in ALLOWED.values())
    src = _sources()
    for b in BUILTINS:
        assert b in src[HEADER], b
    for name, text in src.items():
        if name == HEADER:
            continue
        allowed = ALLOWED.get(name, ({}, ""))[0]
        for b in BUILTINS:
            assert text.count(b) == allowed.get(b, 0), (name, b, text.count(b))


def test_no_butterfly_outside_the_header():
    for name, text in _sources().items():
        if name != HEADER:
            assert _butterflies(text) == [], (name, _butterflies(text))
            assert "#define MOBGS_WAVE_FOLD" not in text, name


def test_one_definition_of_each_primitive_and_no_old_name():
    src = _sources()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', src[HEADER]) == ["common.h"]
    for name in SHARED:
        assert _defines(src[HEADER], name) == 1, name
        for other, text in src.items():
            if other != HEADER:
                assert _defines(text, name) == 0, (other, name)
    for other, text in src.items():
        for old in OLD_NAMES:
            assert not re.search(r"\b%s\b" % old, text), (other, old)
    # the layered pass evaluates a (pixel, splat) pair with raster_shared.h's sequence, not a copy of it
    layers = src["raster_layers.hip"]
    assert "eval_splat(" in layers and not re.search(r"\bL_(ALPHA_MIN|ALPHA_MAX|T_STOP)\b", layers)
