"""CPU checks of the drop-in boundary: the C-ABI library loads here (no GPU), exports every symbol that
include/mobgs_hip.h declares, and the host-side wrappers refuse what they do not implement / CPU tensors."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mobgs_hip.h")


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mobgs_[a-z0-9_]+)\s*\(", text)))


def test_library_builds_loads_and_exports_every_declared_symbol():
    from mobgs_amd import _lib, build
    path = build.build_extension()
    assert os.path.exists(path)
    lib = ctypes.CDLL(str(path))
    syms = declared_symbols()
    assert len(syms) >= 18
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, f"declared in the header but not exported: {missing}"
    h = _lib.load()
    assert h.mobgs_version().decode().startswith("mobgs_hip")
    assert h.mobgs_record_stride(10) == 16 and h.mobgs_record_stride(1) == 8 and h.mobgs_record_stride(2) == 8
    assert h.mobgs_raster_channels_supported(10) == 1 and h.mobgs_raster_channels_supported(7) == 0
    # the bound names are exactly the declared ones
    assert sorted(_lib._SIGS) == syms


def test_size_queries_need_no_gpu():
    from mobgs_amd import _lib
    h = _lib.load()
    assert h.mobgs_project_bwd_scratch_floats(1, 300000) == ((300000 + 255) // 256) * 16
    assert h.mobgs_isect_scratch_bytes(300000, 5440, 1 << 22) > 4 * (5440 + 3 * (1 << 22))  # counters + 3 ints per slot
    assert h.mobgs_decoder_bwd_blocks(1352 * 1014) >= 256


def test_bad_arguments_are_refused_before_any_launch():
    """Error behaviour of the C ABI: a bad argument returns MOBGS_E_INVALID with a message, without touching a device
    (so this runs here).  mobgs_raster_bwd_reduce needs the packed records since the gradient slots carry raw sums."""
    from mobgs_amd import _lib
    h = _lib.load()
    none = ctypes.c_void_p(None)
    rc = h.mobgs_raster_bwd_reduce(1, 5, 3, 0, none, none, none, none, none, none, none, none, none, none, none, none)
    assert rc == -1 and b"mobgs_raster_bwd_reduce" in h.mobgs_last_error()
    rc = h.mobgs_raster_bwd_reduce(0, 5, 3, 0, none, none, none, none, none, none, none, none, none, none, none, none)
    assert rc == -1
    with pytest.raises(RuntimeError, match="mobgs_raster_bwd_reduce"):
        _lib.check(rc, "mobgs_raster_bwd_reduce")


def test_prep_records_are_refused_before_any_launch():
    """mobgs_prep_fwd / mobgs_prep_bwd take their inputs and gradient buffers as host records: a NULL record, K = 0 and a
    negative Ns return MOBGS_E_INVALID under their own name, without touching a device."""
    from mobgs_amd import _lib
    h = _lib.load()
    none = ctypes.c_void_p(None)
    grads = ctypes.byref(_lib.MobgsLeafGrads())

    def fwd(K, rec):
        return h.mobgs_prep_fwd(K, rec, 0, none, none, none, none, none, none)

    def bwd(K, rec, g=grads):
        return h.mobgs_prep_bwd(K, rec, none, none, none, none, none, none, none, g, 0, 0, none)

    ok = ctypes.byref(_lib.MobgsPrepInputs(Ns=3, Nd=2))
    negative = ctypes.byref(_lib.MobgsPrepInputs(Ns=-1, Nd=2))
    for call, name in ((fwd, b"mobgs_prep_fwd"), (bwd, b"mobgs_prep_bwd")):
        for args in ((1, none), (0, ok), (1, negative)):
            h.mobgs_raster_bwd_reduce(0, 5, 3, 0, *[none] * 12)  # leaves another entry point's message behind
            assert call(*args) == _lib._DEFINES["MOBGS_E_INVALID"] == -1, (name, args)
            assert name in h.mobgs_last_error(), (name, args, h.mobgs_last_error())
    assert bwd(1, ok, none) == -1 and b"mobgs_prep_bwd" in h.mobgs_last_error()
    assert fwd(65536, ok) == -1 and b"mobgs_prep_fwd" in h.mobgs_last_error()
    empty = ctypes.byref(_lib.MobgsPrepInputs())  # Ns + Nd = 0: nothing to do, no launch
    assert fwd(1, empty) == 0 and bwd(1, empty) == 0


def test_signatures_are_read_from_the_header():
    """A handful of signatures spelled out by hand pin the header parser of mobgs_amd/_lib.py."""
    from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_void_p as P
    from mobgs_amd import _lib
    S = _lib._SIGS
    assert S["mobgs_version"] == (c_char_p, [])
    assert S["mobgs_last_error"] == (c_char_p, [])
    assert S["mobgs_fused_max_seg_stride"] == (c_int, [])
    assert S["mobgs_isect_scratch_bytes"] == (c_size_t, [c_int, c_int, c_int])
    assert S["mobgs_exposure_scratch_bytes"] == (c_size_t, [c_int64])
    assert S["mobgs_adam_step"] == (c_int, [c_int, P, c_double, c_double, c_double, P])
    assert S["mobgs_cotangent_probe"] == (c_int, [c_int, P, P, P, P])  # const float* const*, const size_t*, int32_t*
    assert S["mobgs_isect_emit_sort"] == (c_int, [c_int] * 5 + [c_int64, c_int64] + [P] * 8)
    assert S["mobgs_knn3_mean_dist2"] == (c_int, [c_int, P, P, P, c_size_t, P])
    assert S["mobgs_normals_fwd"] == (c_int, [c_int, c_int] + [c_float] * 6 + [P, P, P])
    assert S["mobgs_prep_fwd"] == (c_int, [c_int, P, c_int, P, P, P, P, P, P])
    assert S["mobgs_prep_bwd"] == (c_int, [c_int, P] + [P] * 7 + [P, c_int, c_int, P])
    assert S["mobgs_project_bwd"] == (c_int, [c_int, c_int, c_int] + [P] * 5 + [c_int, c_int, c_float] + [P] * 11)
    assert _lib.ABI_VERSION == _lib._DEFINES["MOBGS_ABI_VERSION"]
    from mobgs_amd import loss_utils
    assert (loss_utils.REG_ENTROPY, loss_utils.REG_SPARSITY) == (1, 2)
    h = _lib.load()
    for name, (restype, argtypes) in S.items():
        assert getattr(h, name).restype is restype and list(getattr(h, name).argtypes) == argtypes, name


def test_header_parser_fails_loudly():
    """What the parser cannot type raises with the offending text; nothing is skipped."""
    from mobgs_amd import _lib
    good = "#define MOBGS_X (-3)\ntypedef struct A { int32_t n; const float *a, *b; } A;\nint mobgs_f(int n, const A* a);\n"
    defines, structs, sigs = _lib._parse_header(good)
    assert defines == {"MOBGS_X": -3} and [n for n, _ in structs["A"]] == ["n", "a", "b"]
    assert sigs == {"mobgs_f": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p])}
    for bad, what in (("int mobgs_f(int n, unsigned flags);", "unsigned"),          # a scalar type it does not know
                      ("int mobgs_f(int n, long long count);", "long long count"),
                      ("MobgsThing mobgs_f(int n);", "MobgsThing"),                  # a return type it does not know
                      ("int mobgs_f(int n, void (*callback)(int));", "callback"),   # a function pointer
                      ("int mobgs_f(int n) int mobgs_g(int n);", "mobgs_g"),        # two declarations before one `;`
                      ("static const int k = 3;", "static const int k"),            # not a function of the library
                      ("typedef struct A { uint8_t flag; } A;", "uint8_t"),         # a struct field of unknown type
                      ("typedef struct A { float v[3]; } A;", "v[3]"),
                      ("#define MOBGS_SCALE 1.5f", "MOBGS_SCALE")):                 # a constant that is no integer
        with pytest.raises(ValueError, match=re.escape(what)):
            _lib._parse_header(good + bad)
    text = open(HEADER).read()
    with pytest.raises(ValueError, match="MobgsTuning"):   # a header field without a default in _lib.py
        _lib._tuning_defaults(_lib._parse_header(text.replace("int32_t cover_slots;", "int32_t cover_slots, new_knob;"))[1])


def test_struct_layouts_match_a_c_compile_of_the_header(tmp_path):
    """ctypes.sizeof and every field offset of the structs Python fills equal what the host C compiler reports."""
    from mobgs_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no host C compiler")
    structs = {"MobgsTuning": _lib.MobgsTuning, "MobgsPrepInputs": _lib.MobgsPrepInputs,
               "MobgsLeafGrads": _lib.MobgsLeafGrads}
    lines = []
    for name, cls in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "mobgs_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    reported = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                            text=True).stdout.splitlines())
    expected = {}
    for name, cls in structs.items():
        expected[name] = str(ctypes.sizeof(cls))
        expected.update({f"{name}.{f}": str(getattr(cls, f).offset) for f, _ in cls._fields_})
    assert reported == expected
    assert len(_lib.MobgsPrepInputs._fields_) == 18 and len(_lib.MobgsLeafGrads._fields_) == 13


def test_abi_version_is_checked():
    """The bindings refuse a library whose mobgs_abi_version() differs from the header they were written against
    (a signature changed mid-list without any version signal)."""
    from mobgs_amd import _lib
    h = _lib.load()
    text = open(HEADER).read()
    assert h.mobgs_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define MOBGS_ABI_VERSION (\d+)", text).group(1))


def test_no_cpu_fallback():
    from mobgs_amd.rendering import fully_fused_projection, rasterization
    n = 8
    a = dict(means=torch.rand(n, 3), quats=torch.rand(n, 4), scales=torch.rand(n, 3), opacities=torch.rand(n),
             colors=torch.rand(n, 3), viewmats=torch.eye(4)[None], Ks=torch.eye(3)[None], width=32, height=32)
    with pytest.raises(RuntimeError, match="HIP device"):
        rasterization(packed=False, **a)
    with pytest.raises(RuntimeError, match="HIP device"):
        fully_fused_projection(a["means"], None, a["quats"], a["scales"], a["viewmats"], a["Ks"], 32, 32)


def test_unsupported_gsplat_options_raise():
    from mobgs_amd.rendering import _pad_channels, fully_fused_projection, rasterization
    n = 4
    a = dict(means=torch.rand(n, 3), quats=torch.rand(n, 4), scales=torch.rand(n, 3), opacities=torch.rand(n),
             colors=torch.rand(n, 3), viewmats=torch.eye(4)[None], Ks=torch.eye(3)[None], width=32, height=32)
    for kw in (dict(packed=True), dict(packed=False, sh_degree=3), dict(packed=False, absgrad=True),
               dict(packed=False, rasterize_mode="antialiased"), dict(packed=False, camera_model="fisheye"),
               dict(packed=False, tile_size=8), dict(packed=False, sparse_grad=True),
               dict(packed=False, distributed=True)):
        with pytest.raises(NotImplementedError):
            rasterization(**a, **kw)
    with pytest.raises(ValueError):
        rasterization(packed=False, render_mode="XYZ", **a)
    with pytest.raises(NotImplementedError):
        fully_fused_projection(a["means"], torch.rand(n, 3, 3), None, None, a["viewmats"], a["Ks"], 32, 32)
    assert [_pad_channels(d) for d in (1, 2, 3, 4, 5, 9, 10, 11, 13, 17, 26)] == [1, 2, 3, 4, 9, 9, 10, 12, 16, 26, 26]
    with pytest.raises(NotImplementedError):
        _pad_channels(27)


def test_render_cluster_argument_raises_like_the_reference():
    from mobgs_amd.gaussian_renderer import render
    with pytest.raises(NameError):
        render(None, None, None, None, None, cluster=1)


def test_host_fast_path_builds_loads_and_binds():
    """csrc/fastpath.cpp (the autograd-node bodies in C++) compiles against the installed libtorch with g++, loads,
    and binds every C-ABI entry point it calls from the ctypes handle."""
    from mobgs_amd import _fast
    _fast.reset(True)
    try:
        m = _fast.get()
        assert m is not None, _fast.load_error
        for name in ("prep_fwd", "prep_bwd", "raster_fwd", "raster_bwd", "raster_bwd_reduce", "decoder_fwd",
                     "decoder_bwd", "project_bwd"):
            assert callable(getattr(m, name))
        # the names it binds come from the extension's own list, and each is an entry point of the header
        syms = m.symbols()
        assert len(syms) >= 20 and len(set(syms)) == len(syms) and set(syms) <= set(declared_symbols())
        assert {"mobgs_abi_version", "mobgs_prep_fwd", "mobgs_prep_bwd", "mobgs_project_bwd"} <= set(syms)
        assert not hasattr(_fast, "_SYMBOLS")
    finally:
        _fast.reset(None)
