#!/usr/bin/env python3
"""Device assembly of every translation unit of librtmi.so, for comparing two trees:

    python tools/device_asm.py <tree root> <output directory> [unit.hip ...]

Each unit of build._RTMI_UNITS is compiled with build_rtmi's command line (the per-unit scheduler choice,
RTMI_EXTRA_CFLAGS and RTMI_DEFAULT_SCHED included) plus --cuda-device-only -S, a fixed RTMI_BUILD_HASH and a fixed -cuid (the
compilation-unit id names a symbol and is otherwise a hash of the paths), from <tree root> as the working directory with
relative paths, into <output directory>/<unit>.s.  The flags are those of the tree this tool
is in; the sources are those of <tree root> (a `git worktree` of another commit, say).  A refactor that leaves the device
code alone leaves `diff -r` of the two output directories empty.  Needs no GPU.
"""
import os
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from raytracing_rust_amd import build  # noqa: E402


def main(root, out, only):
    out = os.path.abspath(out)
    os.makedirs(out, exist_ok=True)
    procs = []
    for name, maxocc in build._RTMI_UNITS:
        if only and name not in only:
            continue
        cmd = build.unit_command(maxocc, "0" * 16, include="include") + [
            "--cuda-device-only", "-S", "-cuid=" + name[:-4], os.path.join("raytracing_rust_amd", "csrc", name), "-o",
            os.path.join(out, name[:-4] + ".s")]
        procs.append((name, subprocess.Popen(cmd, cwd=root)))
    failed = [name for name, p in procs if p.wait() != 0]
    if failed:
        sys.exit("hipcc failed: " + " ".join(failed))


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2], sys.argv[3:])
