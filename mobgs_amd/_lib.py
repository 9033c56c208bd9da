"""ctypes binding of libmobgs_hip.so (the C ABI declared in include/mobgs_hip.h).

The product path has NO CPU fallback: if the library cannot be loaded, or a tensor is not on a HIP device,
the call raises.  PyTorch is used only for device memory and the current stream.
"""
from __future__ import annotations

import ctypes
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p
from pathlib import Path
from typing import Optional

import torch

from .build import LIB_PATH, build_extension, is_stale

_lib: Optional[ctypes.CDLL] = None
# always the repository's own header, also when MOBGS_LIB names a foreign build of the library: load() compares
# mobgs_abi_version() with the header's MOBGS_ABI_VERSION and refuses a mismatch
HEADER = Path(__file__).resolve().parent.parent / "include" / "mobgs_hip.h"
_SCALARS = {"int": c_int, "int32_t": c_int32, "int64_t": c_int64, "size_t": c_size_t, "float": c_float,
            "double": c_double}
_RETURNS = {"const char*": c_char_p, **_SCALARS}


def _scalar(type_text: str, where: str):
    if type_text not in _SCALARS:
        raise ValueError(f"mobgs_hip.h: unknown scalar type {type_text!r} in {where!r}")
    return _SCALARS[type_text]


def _parse_header(text: str):
    """include/mobgs_hip.h -> (defines {name: int}, structs {name: [(field, ctype)]}, sigs {name: (restype, [argtypes])}).

    The bindings have no table of their own: every signature, struct layout and constant is read from the header, so a
    changed declaration cannot be driven with shifted arguments.  Conventions of the header this relies on:
      - one declaration per `;`, every function named mobgs_* and returning int, size_t or const char*;
      - no function-pointer parameters and no macros in parameter lists (parameters are split at commas);
      - a declarator containing `*` is a pointer (c_void_p: device and host pointers travel as integers), anything else
        a scalar whose type must be in _SCALARS; `(void)` is an empty list;
      - structs are `typedef struct Name { ... } Name;` with plain fields, several declarators per type allowed
        (`const float *a, *b;`), no bit-fields, arrays or nested structs;
      - every `#define` with a value is an integer constant (optionally parenthesised);
      - enums are `typedef enum Name { A = 0, B = 1 } Name;` with every value written out: the enumerators join the
        defines, and a function takes the value as a plain `int`.
    Anything else raises with the offending text; nothing is skipped."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    defines = {}
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M):  # (not the include guard)
        if not re.fullmatch(r"\(?-?\d+\)?", m[2]):
            raise ValueError(f"mobgs_hip.h: #define {m[1]} {m[2]!r} is not an integer constant")
        defines[m[1]] = int(m[2].strip("()"))
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)                   # preprocessor lines
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)    # the linkage block's braces
    structs = {}

    def take_struct(m):
        if m[1] != m[3]:
            raise ValueError(f"mobgs_hip.h: struct {m[1]} is typedef'd as {m[3]}")
        fields = []
        for decl in filter(None, (d.strip() for d in m[2].split(";"))):
            d = re.fullmatch(r"(?:const\s+)?(\w+)\b\s*(.*)", decl, flags=re.S)
            names = [re.fullmatch(r"(\*?)\s*(\w+)", n.strip()) for n in d[2].split(",")] if d else [None]
            if not all(names):
                raise ValueError(f"mobgs_hip.h: cannot read the field declaration {decl!r} of struct {m[1]}")
            fields += [(n[2], c_void_p if n[1] else _scalar(d[1], decl)) for n in names]
        structs[m[1]] = fields
        return " "

    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", take_struct, text, flags=re.S)

    def take_enum(m):
        if m[1] != m[3]:
            raise ValueError(f"mobgs_hip.h: enum {m[1]} is typedef'd as {m[3]}")
        for item in filter(None, (e.strip() for e in m[2].split(","))):
            e = re.fullmatch(r"(\w+)\s*=\s*(-?\d+)", item)   # every enumerator carries its value
            if not e:
                raise ValueError(f"mobgs_hip.h: cannot read the enumerator {item!r} of enum {m[1]}")
            defines[e[1]] = int(e[2])
        return " "

    text = re.sub(r"typedef\s+enum\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", take_enum, text, flags=re.S)
    sigs = {}
    for decl in filter(None, (" ".join(d.split()) for d in text.split(";"))):
        m = re.fullmatch(r"(.*?)\s*\b(mobgs_\w+) ?\((.*)\)", decl)
        if not m or m[1].replace(" *", "*") not in _RETURNS:
            raise ValueError(f"mobgs_hip.h: cannot read the declaration {decl!r}")
        argtypes = []
        for param in ([] if m[3].strip() in ("", "void") else m[3].split(",")):
            if "(" in param or ")" in param:
                raise ValueError(f"mobgs_hip.h: cannot read the parameter {param.strip()!r} of {m[2]}")
            if "*" in param:
                argtypes.append(c_void_p)
            else:
                words = [w for w in param.split() if w != "const"]
                if len(words) != 2:
                    raise ValueError(f"mobgs_hip.h: cannot read the parameter {param.strip()!r} of {m[2]}")
                argtypes.append(_scalar(words[0], decl))
        sigs[m[2]] = (_RETURNS[m[1].replace(" *", "*")], argtypes)
    return defines, structs, sigs


_DEFINES, _STRUCTS, _SIGS = _parse_header(HEADER.read_text())
ABI_VERSION = _DEFINES["MOBGS_ABI_VERSION"]


def _tuning_defaults(structs) -> list:
    """MobgsTuning's defaults (-1 = library default; see the header's comment on each field), in the header's field
    order.  A field of the header without a default here raises."""
    defaults = dict(heavy_tile_len=-1, longest_list_hint=-1, quadrant_culling=-1, block_walk=-1, bwd_block_walk=-1,
                    geometry_per_camera=0, bwd_mfma=-1, gate_zero_cotangent=0, coherent_order=0, static_rows=0,
                    cover_slots=0)
    names = [n for n, _ in structs["MobgsTuning"]]
    if set(names) != set(defaults):
        raise ValueError(f"mobgs_hip.h: MobgsTuning's fields {names} and the defaults in mobgs_amd/_lib.py "
                         f"{list(defaults)} differ: every field needs a default")
    return [(n, defaults[n]) for n in names]


_TUNING_DEFAULTS = _tuning_defaults(_STRUCTS)


class MobgsTuning(ctypes.Structure):
    """include/mobgs_hip.h MobgsTuning: per-call policy (-1 = library default).  The library keeps no state; a
    caller-side instance (mobgs_amd.rendering.tuning) is passed by pointer with every call that consults it."""
    _fields_ = _STRUCTS["MobgsTuning"]

    def __init__(self, *args, **fields):
        super().__init__(*args, **{**dict(_TUNING_DEFAULTS[len(args):]), **fields})

    def copy(self, **overrides):
        """A per-call copy with some fields replaced."""
        t = MobgsTuning(*[getattr(self, n) for n, _ in self._fields_])
        for k, v in overrides.items():
            setattr(t, k, v)
        return t

    def ref(self):
        return ctypes.cast(ctypes.pointer(self), c_void_p)

    def address(self) -> int:
        return ctypes.addressof(self)


class MobgsPrepInputs(ctypes.Structure):
    """include/mobgs_hip.h MobgsPrepInputs: the raw parameters of the two sets (device pointers)."""
    _fields_ = _STRUCTS["MobgsPrepInputs"]


class MobgsLeafGrads(ctypes.Structure):
    """include/mobgs_hip.h MobgsLeafGrads: the 13 leaf-gradient buffers (device pointers, ops._LEAF_NAMES order)."""
    _fields_ = _STRUCTS["MobgsLeafGrads"]


class MobgsLpipsWeights(ctypes.Structure):
    """include/mobgs_hip.h MobgsLpipsWeights: packed convolution weights, biases and head weights of the five layers
    (device pointers)."""
    _fields_ = _STRUCTS["MobgsLpipsWeights"]


class MobgsLpipsBwdWeights(ctypes.Structure):
    """include/mobgs_hip.h MobgsLpipsBwdWeights: the weights of layers 2 .. 5 packed for the backward-data pass (device
    pointers)."""
    _fields_ = _STRUCTS["MobgsLpipsBwdWeights"]


class MobgsTofLevel(ctypes.Structure):
    """include/mobgs_hip.h MobgsTofLevel: one scale of the Farneback pyramid (width, height, taps, sigma)."""
    _fields_ = _STRUCTS["MobgsTofLevel"]


class MobgsReportStat(ctypes.Structure):
    """include/mobgs_hip.h MobgsReportStat: one map of mobgs_report_stats (kind, element count, device pointers, clip)."""
    _fields_ = _STRUCTS["MobgsReportStat"]


class MobgsReportPanel(ctypes.Structure):
    """include/mobgs_hip.h MobgsReportPanel: one panel of a report sheet (kind, statistics slot, device pointers, clip)."""
    _fields_ = _STRUCTS["MobgsReportPanel"]


class MobgsGridPlane(ctypes.Structure):
    """include/mobgs_hip.h MobgsGridPlane: one plane of a grid-regulariser call (device pointers, sizes, element strides,
    term kind, output slot, reciprocal counts)."""
    _fields_ = _STRUCTS["MobgsGridPlane"]


def _bind(lib, name, restype, argtypes):
    fn = getattr(lib, name)
    fn.restype = restype
    fn.argtypes = argtypes


def load(build_if_missing: bool = True) -> ctypes.CDLL:
    """Load (building first if the .so is missing or older than its sources and hipcc is available)."""
    global _lib
    if _lib is not None:
        return _lib
    if build_if_missing and is_stale():
        try:
            build_extension()
        except Exception as exc:  # noqa: BLE001
            if not LIB_PATH.exists():
                raise RuntimeError(
                    f"libmobgs_hip.so is missing and could not be built ({exc}); the mobgs_amd product path "
                    "has no CPU fallback") from exc
    if not LIB_PATH.exists():
        raise RuntimeError(f"{LIB_PATH} not found; run `python -m mobgs_amd.build`")
    lib = ctypes.CDLL(str(LIB_PATH))
    # include/mobgs_hip.h MOBGS_ABI_VERSION these bindings were read from: a stale or foreign build of the
    # library (MOBGS_LIB) with other signatures / scratch formats must not be driven with shifted arguments
    got = lib.mobgs_abi_version() if hasattr(lib, "mobgs_abi_version") else 0
    if got != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH}: mobgs_abi_version() = {got}, these bindings need {ABI_VERSION} "
                           "(rebuild with `python -m mobgs_amd.build`)")
    for name, (restype, argtypes) in _SIGS.items():
        _bind(lib, name, restype, argtypes)
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().mobgs_last_error().decode()
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


NO_CPU_PATH = "tensors must live on a HIP device (device='cuda'); there is no CPU path"


def device_tensor(what: str, name: str, t) -> torch.Tensor:
    """t, if it is a tensor on a HIP device: TypeError for anything but a tensor, RuntimeError for a host tensor."""
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: {name} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{what}: {NO_CPU_PATH}")
    return t


def ptr(t: Optional[torch.Tensor]):
    """Device pointer of a contiguous HIP tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"mobgs_amd: {NO_CPU_PATH}")
    if not t.is_contiguous():
        raise RuntimeError("mobgs_amd: internal error, non-contiguous tensor passed to the C ABI")
    return c_void_p(t.data_ptr())


class DerivedCache:
    """One-entry memo for a small tensor derived from other tensors (a padded background row, packed camera
    parameters ...): rebuilt unless the SAME tensor objects, unmodified since (Tensor._version), are passed again.
    The sources are kept alive by the entry, so a recycled address can never alias them.  Sources that require grad
    are never cached (the derived tensor must stay in their autograd graph)."""

    def __init__(self):
        self.srcs, self.versions, self.value = (), (), None

    def get(self, srcs, build):
        if any(t.requires_grad for t in srcs):
            return build()
        if len(srcs) == len(self.srcs) and all(a is b for a, b in zip(srcs, self.srcs)) and \
                all(t._version == v for t, v in zip(srcs, self.versions)):
            return self.value
        value = build()
        self.srcs, self.versions, self.value = tuple(srcs), tuple(t._version for t in srcs), value
        return value


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def stream():
    """The current HIP stream of the current device as a void*.  (torch.cuda.current_stream() builds a Stream object
    through several Python layers, ~7 us a call -- 17 calls per render step made it 0.1 ms of a host-bound step.)"""
    return c_void_p(stream_int())


def stream_int() -> int:
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def f32c(t: torch.Tensor) -> torch.Tensor:
    """float32 + contiguous (no copy when already so)."""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def attr_c(t: torch.Tensor, half: bool) -> torch.Tensor:
    """A per-splat attribute array in the storage type the kernel was chosen for: contiguous, and float16 when
    `half` (no copy when it already is -- the fp16-storage path never widens in HBM), float32 otherwise."""
    want = torch.float16 if half else torch.float32
    if t.dtype != want:
        global attr_conversions
        attr_conversions += 1
        t = t.to(want)
    return t.contiguous()


attr_conversions = 0  # dtype conversions of attribute arrays on the way into a kernel (tests assert none happen)
