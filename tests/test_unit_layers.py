"""The division of librtmi.so into translation units, read from the sources: the build list names every
unit, and a host unit launches nothing itself."""
import glob
import os

from raytracing_rust_amd import build

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "raytracing_rust_amd", "csrc")
HOST_UNITS = ("rtmi_batch.hip", "rtmi_multi.hip", "rtmi_update.hip")


def test_build_list_names_every_unit():
    on_disk = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hip")))
    assert on_disk == sorted(name for name, _ in build._RTMI_UNITS)


def test_host_units_launch_nothing():
    for name in HOST_UNITS:
        src = open(os.path.join(CSRC, name)).read()
        for word in ("__global__", "hipLaunchKernelGGL", "<<<"):
            assert word not in src, (name, word)
