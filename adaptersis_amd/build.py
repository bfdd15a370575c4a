"""Build libasis_hip.so (gfx950) in-tree with hipcc.

    python -m adaptersis_amd.build [--force] [--verbose]

hipcc cross-compiles without a GPU.  Objects go to ``adaptersis_amd/csrc/build/`` and the
shared library to ``adaptersis_amd/lib/libasis_hip.so`` (git-ignored, but it travels to the GPU
box with the gpurun snapshot).  Only sources newer than their object are recompiled.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "build")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libasis_hip.so")
ARCH = "gfx950"
FLAGS = ["-O3", "-fPIC", "-std=c++17", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-function",
         "-Wno-unused-variable", "-Wno-unused-but-set-variable"]


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (ROCm toolchain required to build adaptersis_amd)")


# Libraries beside libasis_hip.so: file name -> its sources.  The training step loads libasis_hip.so alone, whose source list and
# link line do not change when an optional op arrives; such an op lives in a library of its own, loaded on first use
# (adaptersis_amd/_lib_distill.py, _lib_consist.py, _lib_mix.py, _lib_semi.py), linked against libasis_hip.so for the error plumbing
# (asis_set_error_ / asis_last_error).  The first two are instantiations of one kernel, csrc/soft_target.h, which neither exports;
# the third holds the batch-mixing kernels and that kernel's instantiation over a mixed batch; the fourth is the fused loss of
# loss.hip (csrc/seg_loss_body.h) instantiated with an ignore label; the fifth (_lib_strong.py) holds the strong student view (colour
# jitter, greyscale, blur) that follows the augmentation; the sixth (_lib_adapt.py) is that kernel again with a threshold per
# class, with the statistics of the teacher's maps and the update of the thresholds from them.
SIDE_LIBS = {"libasis_distill.so": ("distill.hip",), "libasis_consist.so": ("consist.hip",), "libasis_mix.so": ("mix.hip",),
             "libasis_semi.so": ("semi.hip",), "libasis_strong.so": ("strongaug.hip",), "libasis_adapt.so": ("adapt.hip",)}


def sources():
    side = {f for fs in SIDE_LIBS.values() for f in fs}
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip") and f not in side)


def _deps_mtime() -> float:
    """the newest header: every .h of csrc/ and every file of include/ (a change of one recompiles every source)"""
    inc = os.path.join(os.path.dirname(HERE), "include")
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [os.path.join(inc, f) for f in os.listdir(inc)]
    return max(os.path.getmtime(h) for h in hdrs)


# per-file additions to FLAGS
# attention.hip: beside MFMAs a packed f32 op costs several single ones (MI355X_MICROARCH.md): keep the softmax arithmetic of the
# folded kernel unpacked
# adapt.hip: the registers and scratch of its kernels are on record; --verbose prints the remarks
FILE_FLAGS = {"attention.hip": ("-fno-slp-vectorize",), "attn_bwd_pipe.hip": ("-fno-slp-vectorize",),
              "adapt.hip": ("-Rpass-analysis=kernel-resource-usage",)}


def _compile(src: str, verbose: bool) -> str:
    obj = os.path.join(OBJ, os.path.basename(src)[:-4] + ".o")
    cmd = [_hipcc(), *FLAGS, *FILE_FLAGS.get(os.path.basename(src), ()), "-c", src, "-o", obj]
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stdout}\n{r.stderr}")
    if verbose and r.stderr.strip():
        print(r.stderr)
    return obj


def build_library(force: bool = False, verbose: bool = False) -> str:
    """Idempotent and safe to call from several ranks at once: an exclusive file lock serialises the builders (the first
    one compiles, the others find everything up to date)."""
    import fcntl
    os.makedirs(OBJ, exist_ok=True)
    os.makedirs(LIBDIR, exist_ok=True)
    with open(os.path.join(OBJ, ".lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        try:
            return _build_locked(force, verbose)
        finally:
            fcntl.flock(lk, fcntl.LOCK_UN)


def _stale(out: str, than: float, force: bool = False) -> bool:
    """`out` has to be made again: forced, missing, or older than the time `than`"""
    return force or not os.path.exists(out) or os.path.getmtime(out) < than


def _make(out: str, srcs, dep_t: float, force: bool, verbose: bool, link_args=(), after: float = 0.0) -> None:
    """Compile the sources whose object is stale and link `out` from all the objects, if one was compiled or `out` is older
    than an object or than the time `after`."""
    objs = [os.path.join(OBJ, os.path.basename(s)[:-4] + ".o") for s in srcs]
    todo = [s for s, o in zip(srcs, objs) if _stale(o, max(os.path.getmtime(s), dep_t), force)]
    if todo:
        workers = min(len(todo), max(1, (os.cpu_count() or 4) // 2))
        with cf.ThreadPoolExecutor(workers) as ex:
            list(ex.map(lambda s: _compile(s, verbose), todo))
    if todo or _stale(out, max([after] + [os.path.getmtime(o) for o in objs])):
        cmd = [_hipcc(), "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", out, *objs, *link_args]
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link of {out} failed:\n{r.stdout}\n{r.stderr}")


def _build_locked(force: bool, verbose: bool) -> str:
    dep_t = _deps_mtime()
    _make(LIB, sources(), dep_t, force, verbose)
    for name, files in SIDE_LIBS.items():  # relinked when libasis_hip.so is newer
        _make(os.path.join(LIBDIR, name), [os.path.join(CSRC, f) for f in files], dep_t, force, verbose,
              (f"-L{LIBDIR}", "-l:libasis_hip.so", "-Wl,-rpath,$ORIGIN"), os.path.getmtime(LIB))
    return LIB


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--verbose", action="store_true")
    a = ap.parse_args()
    print(build_library(a.force, a.verbose))


if __name__ == "__main__":
    sys.exit(main())
