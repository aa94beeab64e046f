"""In-tree build of the native libraries (no cmake; hipcc cross-compiles gfx950 without a GPU).

  lib/librtmi.so     HIP kernels + the C ABI of include/rtmi.h       (hipcc --offload-arch=gfx950)
  lib/librt_host.so  C++ host mirror + its C bindings, links librtmi (g++)

Flags that matter for parity: -ffp-contract=off on both (no implicit FMA), no fast-math
(IEEE division/sqrt are correctly rounded by default under hipcc).
"""
import glob
import os
import shutil
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
LIB_DIR = os.environ.get("RTMI_LIB_DIR") or os.path.join(_PKG, "lib")
INCLUDE = os.path.join(_ROOT, "include")

# The translation units of librtmi.so, compiled side by side, and whether each takes the iterative-maxocc scheduler
# (build_rtmi): the headline kernels and the host side of the C ABI up to the whole-image modes (rtmi_device), the lean
# instantiations (rtmi_lean), the one-tree instantiation of the headline kernel (rtmi_onetree), the two alternative kernels
# kept for the parity tests (rtmi_alt), then one unit per render mode, named after its header in include/, and the
# kernel-less host unit of the multi-device handle (rtmi_multi), the path probe over its scripted word source
# (rtmi_probe_path), the scene updates: a kernel-less host unit and the unit of its two kernels (rtmi_update,
# rtmi_update_dev), the kernel-less host unit of the batch modes (rtmi_batch), and the lights
# that follow an update: again a kernel-less host unit and the unit of its kernel (rtmi_relight, rtmi_relight_dev; §44).
_RTMI_UNITS = (("rtmi_device.hip", True), ("rtmi_lean.hip", False), ("rtmi_onetree.hip", True), ("rtmi_alt.hip", True), ("rtmi_f64.hip", False),
               ("rtmi_adaptive.hip", True), ("rtmi_features.hip", True), ("rtmi_denoise.hip", False), ("rtmi_nee.hip", True),
               ("rtmi_env.hip", True), ("rtmi_adaptive_nee.hip", True), ("rtmi_roulette.hip", True),
               ("rtmi_light_coop.hip", True), ("rtmi_roulette_coop.hip", True), ("rtmi_session.hip", False),
               ("rtmi_query.hip", True), ("rtmi_radiance.hip", True), ("rtmi_light_tree.hip", True),
               ("rtmi_gather.hip", True), ("rtmi_temporal.hip", False), ("rtmi_frame.hip", False),
               ("rtmi_tonemap.hip", False), ("rtmi_upscale.hip", False), ("rtmi_sparse.hip", True),
               ("rtmi_pixelwise.hip", True), ("rtmi_window.hip", True), ("rtmi_batch_coop.hip", True),
               ("rtmi_multi.hip", False), ("rtmi_probe_path.hip", False), ("rtmi_update.hip", False),
               ("rtmi_update_dev.hip", False), ("rtmi_batch.hip", False), ("rtmi_relight.hip", False),
               ("rtmi_relight_dev.hip", False))
_PUBLIC_HEADERS = sorted(glob.glob(os.path.join(INCLUDE, "*.h")))
RTMI_SRC = [os.path.join(_PKG, "csrc", name) for name, _ in _RTMI_UNITS]
HOST_SRC = [os.path.join(_PKG, "host", "rt_host.cpp"), os.path.join(_PKG, "host", "rt_host_c.cpp")]
RTMI_DEPS = RTMI_SRC + sorted(glob.glob(os.path.join(_PKG, "csrc", "*.hpp"))) + sorted(
    glob.glob(os.path.join(_PKG, "csrc", "*.inc"))) + _PUBLIC_HEADERS
HOST_DEPS = HOST_SRC + [os.path.join(_PKG, "host", "rt_host.hpp")] + _PUBLIC_HEADERS

LIBRTMI = os.path.join(LIB_DIR, "librtmi.so")
LIBHOST = os.path.join(LIB_DIR, "librt_host.so")
REFTESTS = os.path.join(LIB_DIR, "rt_reference_tests")  # C++ counterpart of the reference's #[test] drivers
REFTESTS_SRC = os.path.join(_PKG, "host", "reference_scenes.cpp")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def source_hash(extra=None, default_sched=None):
    """sha256 (16 hex digits) of everything that decides the device code: csrc/*, include/*.h and the compile flags.
    Compiled into librtmi.so (rtmi_build_hash()); tools/pmc_summary.py records it with the committed counter profiles and
    bench.py marks them stale when the library it runs is another build."""
    import hashlib

    h = hashlib.sha256()
    for path in sorted(RTMI_DEPS):
        h.update(os.path.basename(path).encode() + b"\0")
        h.update(open(path, "rb").read())
    extra = os.environ.get("RTMI_EXTRA_CFLAGS", "") if extra is None else extra
    default_sched = bool(os.environ.get("RTMI_DEFAULT_SCHED")) if default_sched is None else default_sched
    h.update(("|".join(_COMMON_FLAGS) + "|" + extra + "|" + str(default_sched)).encode())
    return h.hexdigest()[:16]


_COMMON_FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC", "-std=c++17"]


def _hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def unit_command(maxocc, build_hash, include=INCLUDE, verbose=False):
    """The hipcc command line of one translation unit of librtmi.so, up to its own arguments (-c / -S, source, output).
    `maxocc`: the unit's entry in _RTMI_UNITS.  build_rtmi and tools/device_asm.py both compile with it."""
    # -fno-slp-vectorize: ROCm 7.2's SLP vectoriser packs the scalar F3 arithmetic into v_pk_mul/add_f32 and gets the
    # operand selection wrong in at least one place (hit point/normal of a sphere under Rotate about Z: every
    # pixel differed from the oracle, found by tests/test_random_scenes.py; fine with the function out of line,
    # fine without SLP).  The scalar code is also 2-3 % faster on this VALU-bound path.
    # -amdgpu-sched-strategy=iterative-maxocc: the machine scheduler that first gets the register pressure under the
    # occupancy target and then schedules for latency.  Same instructions (8.75 k static in the headline kernel either
    # way), a better order: final_scene +2.4 %, random_spheres +1.7 % against the default strategy; max-ilp -1.2 %,
    # max-memory-clause -1.4 %, iterative-ilp +0.6 %, iterative-minreg -6 % (profiles/r03_experiments/sched_strategy_ab.log).
    # RTMI_EXTRA_CFLAGS: experiment switches (-DRTMI_...) for A/B builds into another RTMI_LIB_DIR (tools/ab_build.sh)
    # The lean instantiations of the cooperative kernel (scenes without BVH items) lose 2 % under that strategy: they are a
    # translation unit of their own (csrc/rtmi_lean.hip) with the default one.
    extra = os.environ.get("RTMI_EXTRA_CFLAGS", "").split()
    sched = [] if os.environ.get("RTMI_DEFAULT_SCHED") else ["-mllvm", "-amdgpu-sched-strategy=iterative-maxocc"]
    analysis = ["-Rpass-analysis=kernel-resource-usage"] if verbose else []
    return [_hipcc()] + analysis + _COMMON_FLAGS + ["-I" + include, '-DRTMI_BUILD_HASH="%s"' % build_hash] + (
        sched if maxocc else []) + extra


def build_rtmi(force=False, verbose=False):
    if not force and not _stale(LIBRTMI, RTMI_DEPS):
        return LIBRTMI
    os.makedirs(LIB_DIR, exist_ok=True)
    build_hash = source_hash()
    objs, procs = [], []
    for src, (_, maxocc) in zip(RTMI_SRC, _RTMI_UNITS):
        obj = os.path.join(LIB_DIR, os.path.basename(src)[:-4] + ".o")
        procs.append((src, subprocess.Popen(unit_command(maxocc, build_hash, verbose=verbose) + ["-c", src, "-o", obj])))
        objs.append(obj)
    failed = [src for src, p in procs if p.wait() != 0]
    if failed:
        raise subprocess.CalledProcessError(1, "hipcc -c " + " ".join(failed))
    subprocess.run([_hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared", "-o", LIBRTMI] + objs, check=True)
    return LIBRTMI


def build_host(force=False):
    if not force and not _stale(LIBHOST, HOST_DEPS + [LIBRTMI]):
        return LIBHOST
    os.makedirs(LIB_DIR, exist_ok=True)
    cmd = ["g++", "-O2", "-march=x86-64-v3", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-Wall",
           "-I" + INCLUDE, "-o", LIBHOST] + HOST_SRC + [
               "-L" + LIB_DIR, "-lrtmi", "-Wl,-rpath,$ORIGIN"]
    subprocess.run(cmd, check=True)
    return LIBHOST


def build_reference_tests(force=False):
    if not force and not _stale(REFTESTS, [REFTESTS_SRC, LIBHOST, os.path.join(_PKG, "host", "rt_host.hpp")]):
        return REFTESTS
    cmd = ["g++", "-O2", "-march=x86-64-v3", "-ffp-contract=off", "-std=c++17", "-Wall", "-I" + INCLUDE,
           "-I" + os.path.join(_PKG, "host"), "-o", REFTESTS, REFTESTS_SRC, "-L" + LIB_DIR, "-lrt_host", "-lrtmi",
           "-Wl,-rpath,$ORIGIN"]
    subprocess.run(cmd, check=True)
    return REFTESTS


def build_all(force=False, verbose=False):
    build_rtmi(force, verbose)
    build_host(force)
    build_reference_tests(force)
    return LIBRTMI, LIBHOST


if __name__ == "__main__":
    import sys

    build_all(force="--force" in sys.argv, verbose="-v" in sys.argv)
    print(LIBRTMI)
    print(LIBHOST)
