"""The ray queries' public interface (include/rtmi_query.h), without a GPU.

* the header compiles as C99 and its three records have the sizes and offsets the kernels read them with;
* librtmi.so and librt_host.so export the four entries, abi.py and sys.rs declare them;
* the Rust structs list the fields of the ctypes structures, in order and size;
* every bad argument that is refused before a device is touched gives its code and names the entry."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from raytracing_rust_amd import abi, primary_rays
from raytracing_rust_amd.host import HIT_DTYPE, RAY_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtmi_query.h")
SYS = open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()
ENTRIES = ["rtmi_occluded", "rtmi_occluded_device", "rtmi_trace", "rtmi_trace_device"]


def test_header_is_c99_with_the_documented_layout(tmp_path):
    checks = {"rtmi_ray": (32, {"o": 0, "t_min": 12, "d": 16, "t_max": 28}),
              "rtmi_hit": (48, {"t": 0, "u": 4, "v": 8, "p": 12, "n": 24, "item": 36, "prim": 40, "material": 44}),
              "rtmi_query_params": (24, {"n": 0, "flags": 4, "seed": 8, "first_ray": 16})}
    lines = ['#include <stddef.h>', '#include "rtmi_query.h"']
    for name, (size, offs) in checks.items():
        lines.append("typedef char size_%s[sizeof(%s) == %d ? 1 : -1];" % (name, name, size))
        for f, o in offs.items():
            lines.append("typedef char off_%s_%s[offsetof(%s, %s) == %d ? 1 : -1];" % (name, f, name, f, o))
    lines.append("int main(void) { (void)&rtmi_trace; (void)&rtmi_occluded; (void)&rtmi_trace_device; "
                 "(void)&rtmi_occluded_device; return 0; }")
    src = tmp_path / "c99.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-c", "-o", str(tmp_path / "c99.o")], check=True)


def test_ctypes_and_numpy_records_match_the_header():
    for cty, size, offs in ((abi.Ray, 32, {"o": 0, "t_min": 12, "d": 16, "t_max": 28}),
                            (abi.Hit, 48, {"t": 0, "u": 4, "v": 8, "p": 12, "n": 24, "item": 36, "prim": 40, "material": 44}),
                            (abi.QueryParams, 24, {"n": 0, "flags": 4, "seed": 8, "first_ray": 16})):
        assert C.sizeof(cty) == size
        assert {n: getattr(cty, n).offset for n, _ in cty._fields_} == offs
    for dt, cty in ((RAY_DTYPE, abi.Ray), (HIT_DTYPE, abi.Hit)):
        assert dt.itemsize == C.sizeof(cty)
        assert {n: dt.fields[n][1] for n in dt.names} == {n: getattr(cty, n).offset for n, _ in cty._fields_}


def test_exports_and_declarations_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rtmi_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(abi.RTMI_QUERY_SYMBOLS) == sorted(ENTRIES + ["rtmi_scene_attach_flips"])
    lib = abi.load_rtmi()
    for n in declared:
        assert hasattr(lib, n), n
        assert re.search(r"pub fn %s\(" % n, SYS), n
    others = (set(abi.RTMI_SYMBOLS) | set(abi.RTMI_F64_SYMBOLS) | set(abi.RTMI_ADAPTIVE_SYMBOLS) | set(abi.RTMI_FEATURES_SYMBOLS) |
              set(abi.RTMI_DENOISE_SYMBOLS) | set(abi.RTMI_NEE_SYMBOLS) | set(abi.RTMI_ENV_SYMBOLS) |
              set(abi.RTMI_ADAPTIVE_NEE_SYMBOLS) | set(abi.RTMI_ROULETTE_SYMBOLS) | set(abi.SESSION_SYMBOLS))
    assert not set(declared) & others
    host = abi.load_host()
    for n in ("rth_trace", "rth_occluded", "rth_trace_device", "rth_occluded_device"):
        assert hasattr(host, n), n


def test_rust_structs_match_ctypes():
    scalar = {"i32": 4, "u32": 4, "f32": 4, "u64": 8, "f64": 8, "u8": 1}
    for rname, cty in {"RtmiRay": abi.Ray, "RtmiHit": abi.Hit, "RtmiQueryParams": abi.QueryParams}.items():
        body = re.search(r"pub struct %s \{(.*?)\n\}" % rname, SYS, re.S).group(1)
        rf = []
        for fname, ty in re.findall(r"pub (\w+): ([^,\n]+),", body):
            m = re.match(r"\[(\w+); (\d+)\]", ty.strip())
            rf.append((fname, scalar[m.group(1)] * int(m.group(2)) if m else scalar[ty.strip()]))
        assert rf == [(n, C.sizeof(t)) for n, t in cty._fields_], rname


def _call(entry, n=4, flags=0, scene=None, params=True, rays=True, out=True):
    lib = abi.load_rtmi()
    p = abi.QueryParams(n, flags, 7, 0)
    r = np.zeros(max(n, 1), RAY_DTYPE)
    r["d"][:, 2] = 1.0
    r["t_max"] = np.inf
    o = np.zeros(max(n, 1), HIT_DTYPE)
    args = [scene, C.byref(p) if params else None, r.ctypes.data if rays else None, None, o.ctypes.data if out else None, None]
    rc = getattr(lib, entry)(*args)
    return rc, (lib.rtmi_last_error() or b"").decode()


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_before_any_device_work(entry):
    rc, msg = _call(entry)
    assert rc == 1 and msg.startswith(entry + ":") and "scene" in msg, msg  # every value valid: the NULL scene is refused
    rc, msg = _call(entry, params=False)
    assert rc == 1 and msg.startswith(entry + ":") and "params" in msg, msg
    rc, msg = _call(entry, n=0)
    assert rc == 1 and "scene" in msg, msg  # an empty batch still needs a handle
    for flag in (abi.RTMI_FLAG_SYNC, abi.RTMI_FLAG_PATH_SIG, abi.RTMI_FLAG_SKY, abi.RTMI_FLAG_REF_TREE, 1 << 11, 1 << 20):
        rc, msg = _call(entry, flags=flag | abi.RTMI_FLAG_FAST_CULL)
        assert rc == 2 and msg.startswith(entry + ":") and "flags" in msg, (flag, msg)
    rc, msg = _call(entry, flags=abi.RTMI_FLAG_FAST_CULL)
    assert rc == 1 and "scene" in msg, msg  # the accepted flag reaches the scene check


def test_attach_flips_refuses_a_null_scene():
    lib = abi.load_rtmi()
    gaps = (C.c_uint32 * 2)(0, 1)
    assert lib.rtmi_scene_attach_flips(None, gaps, 1, gaps, 1) == 1
    assert (lib.rtmi_last_error() or b"").decode().startswith("rtmi_scene_attach_flips: scene")


def test_lowering_records_where_the_flips_sit(tmp_path):
    """the flip table of the C++ lowering, through a driver against rt_host.hpp: parities equal the description's flags and
    the places are the wrappers' (no GPU: nothing is uploaded)"""
    from raytracing_rust_amd import build

    src = tmp_path / "gaps.cpp"
    src.write_text(r'''
#include <cstdio>
#include "rt_host.hpp"
using namespace rt;
int main() {
    auto tex = std::make_shared<SolidTexture>(0.5, 0.5, 0.5);
    auto lam = std::make_shared<Lambertian>(tex);
    auto rect = [&] { return std::make_shared<Rect>(Plane::XY, 0.0, 0.0, 1.0, 1.0, 2.0, lam); };
    auto world = std::make_shared<HittableList>();
    world->push(std::make_shared<FlipNormals>(rect()));                                                       // plain: prim bit 0
    world->push(std::make_shared<Rotate>(Axis::Z, std::make_shared<FlipNormals>(rect()), 200.0));            // item bit 1
    world->push(std::make_shared<FlipNormals>(std::make_shared<Rotate>(Axis::Z, rect(), 200.0)));            // item bit 0
    std::vector<HittablePtr> leaves = {std::make_shared<Rotate>(Axis::Z, std::make_shared<FlipNormals>(rect()), 200.0),
                                       std::make_shared<FlipNormals>(std::make_shared<Sphere>(Vec3(0, 0, 0), 1.0, lam))};
    world->push(std::make_shared<BVHNode>(leaves, 0.0, 1.0));                                                  // prim bits 1 and 0
    const LoweredScene ls = lower_scene(*world);
    for (uint32_t g : ls.prim_flip_gaps) std::printf("p%u ", g);
    for (uint32_t g : ls.item_flip_gaps) std::printf("i%u ", g);
    for (size_t i = 0; i < ls.prim_meta.size(); i++)
        if ((uint32_t)__builtin_parity(ls.prim_flip_gaps[i]) != (ls.prim_meta[i].flags & 1u)) return 1;
    for (size_t i = 0; i < ls.items.size(); i++)
        if ((uint32_t)__builtin_parity(ls.item_flip_gaps[i]) != (ls.items[i].flags & 1u)) return 2;
    return ls.prim_flip_gaps.size() == ls.prim_meta.size() && ls.item_flip_gaps.size() == ls.items.size() ? 0 : 3;
}
''')
    exe = tmp_path / "gaps"
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "raytracing_rust_amd", "host"),
                    str(src), "-o", str(exe), "-L" + build.LIB_DIR, "-lrt_host", "-lrtmi", "-Wl,-rpath," + build.LIB_DIR], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert sorted(g for g in out if g.startswith("p")) == ["p0", "p0", "p1", "p1", "p2"], out
    assert [g for g in out if g.startswith("i")] == ["i0", "i2", "i1", "i0"], out


def test_primary_rays_are_the_pixel_centres():
    c = abi.Camera()
    c.origin[:] = [1.0, 2.0, 3.0]
    c.lower_left_corner[:] = [-1.0, -0.5, -1.0]
    c.horizontal[:] = [2.0, 0.0, 0.0]
    c.vertical[:] = [0.0, 1.0, 0.0]
    o, d = primary_rays(c, 4, 2)
    assert o.shape == d.shape == (2, 4, 3) and o.dtype == d.dtype == np.float32
    assert np.array_equal(o, np.broadcast_to(np.array([1.0, 2.0, 3.0], np.float32), (2, 4, 3)))
    # row 0 is the top row: v = 0.75; column 0: u = 0.125
    assert np.array_equal(d[0, 0], np.array([-1.0 + 0.25 - 1.0, -0.5 + 0.75 - 2.0, -1.0 - 3.0], np.float32))
    assert np.array_equal(d[1, 3], np.array([-1.0 + 1.75 - 1.0, -0.5 + 0.25 - 2.0, -1.0 - 3.0], np.float32))
