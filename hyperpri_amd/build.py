"""Build the HIP extension in-tree: hyperpri_amd/lib/libhyperpri_hip.so and libhyperpri_hip_f16.so (gfx950 only).

hipcc cross-compiles without a GPU, so this runs in the build container; the .so travels to the
GPU box with the repo snapshot (it is git-ignored, not gpurun-ignored).
"""
from __future__ import annotations

import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
# The product is TWO libraries built from the same sources: libhyperpri_hip.so (16-bit type of the plane paths = bf16: precision modes
# fp32 / bf16 / bf16x3 / bf16x6) and libhyperpri_hip_f16.so (-DHPRI_H16_F16: IEEE half, precision mode "f16"; csrc/common.h).
LIB = os.path.join(LIBDIR, "libhyperpri_hip.so")
LIB_F16 = os.path.join(LIBDIR, "libhyperpri_hip_f16.so")
SOURCES = ["api.cpp", "conv_fwd.hip", "conv_bf16v3.hip", "gemm_bf16v3.hip", "gemm_f32v2.hip", "wgrad_bf16v3.hip", "conv_wino.hip", "conv_wino4.hip", "conv_wgrad.hip", "conv_wgrad_bf16v2.hip", "pack.hip", "bn.hip", "elementwise.hip", "step.hip", "ingest.hip", "conv_ingest.hip", "cache.hip", "cache_warp.hip", "cache_deform.hip", "segmap.hip", "multiclass.hip", "segloss.hip", "tta.hip", "components.hip", "distance.hip", "spectral.hip", "skeleton.hip", "detect.hip", "cluster.hip", "mixture.hip", "sort.hip", "unmix.hip", "guided.hip", "ridge.hip", "crf.hip", "crf_grad.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function"]


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _stamp(flags=None) -> str:
    h = hashlib.sha256()
    for f in sorted(os.listdir(CSRC)):
        if not os.path.isfile(os.path.join(CSRC, f)):
            continue
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    h.update(" ".join(FLAGS if flags is None else flags).encode())
    return h.hexdigest()


def build(force: bool = False, verbose: bool = True) -> str:
    """Build both product libraries; returns the path of libhyperpri_hip.so."""
    _build_one(LIB, FLAGS, ".o", force, verbose)
    _build_one(LIB_F16, FLAGS + ["-DHPRI_H16_F16"], "_f16.o", force, verbose)
    return LIB


def _build_one(lib: str, flags, osuffix: str, force: bool, verbose: bool) -> str:
    os.makedirs(LIBDIR, exist_ok=True)
    stamp_file = lib + ".stamp"
    stamp = _stamp(flags)
    if not force and os.path.exists(lib) and os.path.exists(stamp_file) and open(stamp_file).read() == stamp:
        return lib
    hipcc = _hipcc()
    objs = []
    procs = []
    for s in SOURCES:
        o = os.path.join(LIBDIR, s.rsplit(".", 1)[0] + osuffix)
        objs.append(o)
        cmd = [hipcc, *flags, "-x", "hip", "-c", os.path.join(CSRC, s), "-o", o, "-I", CSRC]
        procs.append((s, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for s, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed on {s}:\n{out}")
        if verbose and out.strip():
            print(out)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, *objs]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("link failed:\n" + r.stdout)
    with open(stamp_file, "w") as f:
        f.write(stamp)
    if verbose:
        print("built", lib)
    return lib


if __name__ == "__main__":
    build(force="--force" in sys.argv)
