"""Builds the product library ``libmcrt.so`` (HIP kernels for gfx950 + C-ABI host code) in-tree.

    python -m minecraftskin_raytracer_amd.build [--force] [--verbose]

hipcc cross-compiles for gfx950 without a GPU.  Flags that matter for parity:
``-ffp-contract=off`` (no fused multiply-add except the explicit fma() calls of mcrt_detmath.h) and
hipcc's default correctly-rounded fp32 divide/sqrt.  No fast-math.

``SOURCES`` is the one list of the library's sources: the variant builds of ``tools/`` call ``build(out=..., extra_flags=...)``.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
OUT = os.path.join(PKG, "libmcrt.so")
SOURCES = ["render_kernels.hip", "pass_kernels.hip", "util_kernels.hip", "render_plan.cpp", "api.cpp", "render_enqueue.cpp", "device_stores.cpp", "probes.cpp",
           "flatten.cpp", "scene_builder.cpp", "png_writer.cpp"]
HEADERS = ["flat_scene.h", "flatten.h", "host_internal.h", "kernel_common.h", "kernels.h", "launch_shapes.h", "rt_core.h"]
ARCH = "gfx950"
JOBS = 8  # compiles at a time (the three kernel files take nearly all of the time)


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or add /opt/rocm/bin to PATH)")


def _stale(out: str) -> bool:
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS]
    deps += [os.path.join(ROOT, "include", f) for f in ("mcrt.h", "mcrt_detmath.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False, out: str | None = None, extra_flags=()) -> str:
    """Builds the library at ``out`` (default: in the package); ``extra_flags`` go to every compile (the variants' -D / -I)."""
    out = out or OUT
    if not force and not _stale(out):
        return out
    hipcc = _hipcc()
    flags = [
        f"--offload-arch={ARCH}",
        "-O3",
        "-std=c++17",
        "-ffp-contract=off",
        "-fPIC",
        "-Wall",
        "-Wno-unused-function",
        f"-I{os.path.join(ROOT, 'include')}",
        f"-I{CSRC}",
    ]
    if verbose:
        flags += ["-Rpass-analysis=kernel-resource-usage"]
    flags += os.environ.get("MCRT_EXTRA_FLAGS", "").split()
    flags += list(extra_flags)

    def run(cmd):
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)

    # every source is a code object of its own: compiled a few at a time into a scratch directory, then linked
    with tempfile.TemporaryDirectory(prefix="mcrt_build_") as tmp:
        objs = [os.path.join(tmp, s + ".o") for s in SOURCES]
        with ThreadPoolExecutor(max_workers=1 if verbose else JOBS) as pool:  # (verbose: a kernel's remarks stay together)
            list(pool.map(lambda so: run([hipcc, *flags, "-c", os.path.join(CSRC, so[0]), "-o", so[1]]), zip(SOURCES, objs)))
        run([hipcc, f"--offload-arch={ARCH}", "-fPIC", "-shared", *objs, "-o", out, "-lpthread"])
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="--verbose" in sys.argv))
