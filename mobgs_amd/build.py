"""Build libmobgs_hip.so (gfx950) in-tree with hipcc.

hipcc cross-compiles without a GPU, so this runs in the CPU-only build container; the resulting .so is
git-ignored but travels to the GPU box with the repo snapshot.
"""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

CSRC = Path(__file__).resolve().parent / "csrc"
# MOBGS_LIB: load another build of the same library instead (A/B timing of kernel variants on one GPU box)
LIB_PATH = Path(os.environ["MOBGS_LIB"]).resolve() if os.environ.get("MOBGS_LIB") else CSRC / "libmobgs_hip.so"
SOURCES = ["project.hip", "isect.hip", "raster.hip", "raster_bwd_mfma.hip", "raster_layers.hip", "pipeline.hip", "prep.hip", "decoder.hip", "deform.hip", "deform_bwd.hip", "hexplane_bwd.hip", "blce.hip", "loss.hip", "flowloss.hip", "densify.hip", "adam_dev.hip", "normals.hip", "knn.hip", "control_prune.hip", "scene_seed.hip", "exposure.hip", "regterms.hip", "metrics.hip", "pose.hip", "lpips.hip", "tof.hip", "report.hip", "gridreg.hip", "snapshot.hip", "lane_probe.hip", "densify_ctl.hip"]
ARCH = "gfx950"
# host fast path (csrc/fastpath.cpp): a plain C++ torch extension, no device code, no link against libmobgs_hip.so
FAST_SRC = CSRC / "fastpath.cpp"
FAST_PATH = CSRC.parent / "_mobgs_fast.so"
# Per-file extra flags.  -fno-slp-vectorize: the SLP vectoriser pairs independent fp32 FMAs into v_pk_fma_f32,
# which on gfx950 issues at half rate (no gain) and needs v_mov shuffles to build the 64-bit operand pairs:
# +6% renders/s on the compositing kernels without it (measured).
NOSLP_FILES = os.environ.get("MOBGS_NOSLP_FILES", "raster.hip,raster_bwd_mfma.hip,raster_layers.hip").split(",")
EXTRA_FLAGS = {f: ["-fno-slp-vectorize"] for f in NOSLP_FILES if f}
# project.hip: no implicit FMA contraction.  radii (= ceil(3 sqrt(lambda_max))), tile rectangles and the cull tests
# are integer / boolean functions of float expressions; with the compiler free to fuse a * b + c differently from the
# written order, one splat in ~8000 of an extreme scene (near-plane, 6x scales) landed on the other side of an integer
# boundary than the oracles, which evaluate the expressions as written (scripts/soak_parity.py).  The kernels are
# HBM-bound: no measurable cost.
EXTRA_FLAGS.setdefault("project.hip", [])
EXTRA_FLAGS["project.hip"] = EXTRA_FLAGS["project.hip"] + ["-ffp-contract=off"]
# knn.hip: no FMA contraction either.  The 3-NN result must not depend on the row order or on which boxes were pruned:
# every squared distance is the one expression (dx dx + dy dy) + dz dz, symmetric in its two points, and the box bound
# is the same expression on the gaps to the box, so that fp32 monotonicity makes the pruning exact (csrc/knn.hip).
EXTRA_FLAGS["knn.hip"] = EXTRA_FLAGS.get("knn.hip", []) + ["-ffp-contract=off"]
# scene_seed.hip: the same for the nearest-track search: (dx dx + dy dy) compares bit-equal with torch's
# square().sum(-1).argmin(-1), so ties between tracks resolve to the same (lowest) index (csrc/scene_seed.hip).
EXTRA_FLAGS["scene_seed.hip"] = EXTRA_FLAGS.get("scene_seed.hip", []) + ["-ffp-contract=off"]
# exposure.hip: the same for the flow magnitudes sqrt(x x + y y) and the quantile's interpolation a + w (b - a): evaluated
# as written they are bit-equal with torch on the CPU, and the selected order statistics are exact (csrc/exposure.hip).
EXTRA_FLAGS["exposure.hip"] = EXTRA_FLAGS.get("exposure.hip", []) + ["-ffp-contract=off"]
# regterms.hip: the same for the loss terms a log(a + eps) + (1 - a) log(1 - a + eps), w_e E + w_s S and the depth
# gradient (g w_d) / n: each operation is rounded as the reference's torch statements round it (csrc/regterms.hip).
EXTRA_FLAGS["regterms.hip"] = EXTRA_FLAGS.get("regterms.hip", []) + ["-ffp-contract=off"]
# metrics.hip: the same for the SSIM maps: with equal (or flat) images the numerator and the denominator of a map value are
# then the same operations on the same values, and the map is exactly 1 (csrc/metrics.hip).
EXTRA_FLAGS["metrics.hip"] = EXTRA_FLAGS.get("metrics.hip", []) + ["-ffp-contract=off"]
# pose.hip: the same for the pose head and the -PSNR loss: the head inside the fused step kernel gives the bits of the
# stand-alone head kernels, and a squared difference is the fp32 value the reference forms (csrc/pose.hip).
EXTRA_FLAGS["pose.hip"] = EXTRA_FLAGS.get("pose.hip", []) + ["-ffp-contract=off"]
# tof.hip: the same for the Farneback kernels: the update matrices inside the fused blur-and-solve kernel give the bits of
# the stand-alone update kernel, and with equal frames and a zero flow the sampled coefficients cancel exactly (csrc/tof.hip).
EXTRA_FLAGS["tof.hip"] = EXTRA_FLAGS.get("tof.hip", []) + ["-ffp-contract=off"]
# report.hip: the same for the report sheets: a panel's byte is floor(255 x) of the reference's numpy float32 statements, one
# rounding per written operation, so it can differ from the float64 restatement only where 255 x is within a few ulp of an
# integer, and the flow radius sqrt(u u + v v) is bit-equal with torch's (csrc/report.hip).  HBM-bound: no measurable cost.
EXTRA_FLAGS["report.hip"] = EXTRA_FLAGS.get("report.hip", []) + ["-ffp-contract=off"]
# gridreg.hip: the same for the grid regularisers: a second difference is (t[k+2] - t[k+1]) - (t[k+1] - t[k]) with each of
# the three subtractions rounded to fp32, as the reference's slice statements round them (csrc/gridreg.hip).  Memory-bound kernels: no cost.
EXTRA_FLAGS["gridreg.hip"] = EXTRA_FLAGS.get("gridreg.hip", []) + ["-ffp-contract=off"]
# densify_ctl.hip: the same for the batch statistics: the gradient of a row is ((0 + g_0) + g_1 + ...) s with every addition
# and the scaling rounded to fp32 in view order, as the reference's `+=` over the views and `*= W * 0.5` round them, so
# grad_sum is bit-equal with torch and the norm starts from the same two numbers (csrc/densify_ctl.hip).  HBM-bound: no cost.
EXTRA_FLAGS["densify_ctl.hip"] = EXTRA_FLAGS.get("densify_ctl.hip", []) + ["-ffp-contract=off"]
# normals.hip: the same for the back-projected differences d_r z_r - d_l z_l: fused into fma(d_r, z_r, -(d_l z_l)) the
# difference of two equal products is one product's rounding error, not 0, and the normals of a flat patch or of a depth
# hole get components of 1e-8 where the reference's are exactly 0 (tests/test_gpu_loss_kernels.py).  15 us kernels.
EXTRA_FLAGS["normals.hip"] = EXTRA_FLAGS.get("normals.hip", []) + ["-ffp-contract=off"]
# raster.hip: top-down pre-RA machine scheduling.  The compositing loops are long straight-line blocks bound by VALU
# issue; of ten scheduler settings swept in round 4 (scripts/ab/build_variant_raster.sh + kernel_ab2.sh, three A/B
# repetitions on one box) this is the only one outside the noise: raster_bwd<10> 512 -> 506 us, raster_fwd_blocks<10>
# 219 -> 213.5 us, <12> forward -2 %, <16> backward -1 % (raster_fwd<16> +4 %).  Same instructions in another order:
# results are bit-identical.
EXTRA_FLAGS["raster.hip"] = EXTRA_FLAGS.get("raster.hip", []) + ["-mllvm", "-misched-prera-direction=topdown"]
for _f in ("raster.hip", "raster_bwd_mfma.hip", "raster_layers.hip"):  # experiment hook: extra flags for the compositing kernels
    EXTRA_FLAGS.setdefault(_f, [])
    EXTRA_FLAGS[_f] = EXTRA_FLAGS[_f] + os.environ.get("MOBGS_RASTER_EXTRA_FLAGS", "").split()


class _BuildLock:
    """One builder at a time per output file (several ranks of one node start together and all find the same stale
    .so): an exclusive flock on <target>.lock; the artefact itself is written to a temporary name and moved into place
    with os.replace, so a concurrent loader sees the old file or the new one, never a half-written one."""

    def __init__(self, target: Path):
        self.path = str(target) + ".lock"
        self.fd = None

    def __enter__(self):
        import fcntl
        self.fd = os.open(self.path, os.O_CREAT | os.O_RDWR, 0o644)
        fcntl.flock(self.fd, fcntl.LOCK_EX)
        return self

    def __exit__(self, *exc):
        import fcntl
        fcntl.flock(self.fd, fcntl.LOCK_UN)
        os.close(self.fd)
        return False


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: cannot build libmobgs_hip.so")


def sources() -> list[Path]:
    return [CSRC / s for s in SOURCES if (CSRC / s).exists()]


def headers() -> list[Path]:
    """What every translation unit may include: all of csrc/*.h and the public header."""
    return sorted(CSRC.glob("*.h")) + [CSRC.parent.parent / "include" / "mobgs_hip.h"]


def is_stale() -> bool:
    if os.environ.get("MOBGS_LIB"):
        return False
    if not LIB_PATH.exists():
        return True
    t = LIB_PATH.stat().st_mtime
    return any(d.exists() and d.stat().st_mtime > t for d in sources() + headers())


def build_extension(force: bool = False, verbose: bool = False) -> Path:
    if not force and not is_stale():
        return LIB_PATH
    with _BuildLock(LIB_PATH):
        if not force and not is_stale():  # another process built it while this one waited for the lock
            return LIB_PATH
        return _build_extension_locked(force, verbose)


def _build_extension_locked(force: bool, verbose: bool) -> Path:
    objs = []
    hipcc = _hipcc()
    flags = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value"]
    procs = []
    newest_header = max(h.stat().st_mtime for h in headers())
    for src in sources():
        obj = src.with_suffix(".o")
        objs.append(obj)
        if not force and obj.exists() and obj.stat().st_mtime > max(src.stat().st_mtime, newest_header):
            continue
        cmd = [hipcc, *flags, *EXTRA_FLAGS.get(src.name, []), "-c", str(src), "-o", str(obj)]
        if verbose:
            print(" ".join(cmd))
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{out}")
        if verbose and out.strip():
            print(out)
    tmp = LIB_PATH.with_name(LIB_PATH.name + f".tmp{os.getpid()}")
    cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", *map(str, objs), "-o", str(tmp)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stdout}")
    os.replace(tmp, LIB_PATH)
    return LIB_PATH


def fastpath_is_stale() -> bool:
    if not FAST_PATH.exists():
        return True
    t = FAST_PATH.stat().st_mtime
    deps = [FAST_SRC, CSRC.parent.parent / "include" / "mobgs_hip.h"]
    return any(d.exists() and d.stat().st_mtime > t for d in deps)


def build_fastpath(force: bool = False, verbose: bool = False) -> Path:
    """g++ -shared against the installed libtorch (~30 s).  Needs no GPU and no hipcc."""
    if not force and not fastpath_is_stale():
        return FAST_PATH
    with _BuildLock(FAST_PATH):
        if not force and not fastpath_is_stale():
            return FAST_PATH
        return _build_fastpath_locked(verbose)


def _build_fastpath_locked(verbose: bool) -> Path:
    import sysconfig

    import torch
    import torch.utils.cpp_extension as ce
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    if not cxx:
        raise RuntimeError("no C++ compiler found: cannot build the host fast path")
    libdir = os.path.join(os.path.dirname(torch.__file__), "lib")
    tmp = FAST_PATH.with_name(FAST_PATH.name + f".tmp{os.getpid()}")
    cmd = [cxx, "-O2", "-std=c++17", "-shared", "-fPIC", str(FAST_SRC), "-o", str(tmp),
           "-DTORCH_EXTENSION_NAME=_mobgs_fast", f"-D_GLIBCXX_USE_CXX11_ABI={int(torch._C._GLIBCXX_USE_CXX11_ABI)}",
           "-I" + sysconfig.get_paths()["include"], *["-I" + i for i in ce.include_paths()],
           "-L" + libdir, "-ltorch", "-ltorch_cpu", "-lc10", "-ltorch_python", "-Wl,-rpath," + libdir,
           "-Wno-unused-function"]
    if verbose:
        print(" ".join(cmd))
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"host fast path: compile failed:\n{r.stdout[-4000:]}")
    os.replace(tmp, FAST_PATH)
    return FAST_PATH


if __name__ == "__main__":
    print(build_extension(force="--force" in os.sys.argv, verbose=True))
