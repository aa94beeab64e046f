"""The light tree's public interface (include/rtmi_light_tree.h), without a GPU.

* the header compiles as C99 and its two structs have the documented sizes, in the header, in ctypes and in sys.rs;
* librtmi.so and librt_host.so export the entries, abi.py and sys.rs declare them, and no other symbol list names them;
* bad arguments are refused before a device is touched;
* RTMI_FLAG_LIGHT_TREE is a flag of rtmi_render_nee alone: there it reaches the scene check, beside RTMI_FLAG_LIGHT_COOP it
  is RTMI_ERR_UNSUPPORTED, and every other lighting entry answers it as an unknown flag."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import light_tree_scenes as lts
from raytracing_rust_amd import abi, default_params
from raytracing_rust_amd.host import LIGHT_NODE_DTYPE, LIGHT_PATH_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtmi_light_tree.h")
SYS = open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()
ENTRIES = ["rtmi_light_tree_from_desc", "rtmi_light_tree_pick", "rtmi_light_tree_pmf", "rtmi_probe_light_tree",
           "rtmi_scene_attach_light_tree"]
FLAG = abi.RTMI_FLAG_LIGHT_TREE


def test_header_is_c99_with_the_documented_layout(tmp_path):
    lines = ['#include <stddef.h>', '#include "rtmi_light_tree.h"',
             "typedef char size_node[sizeof(rtmi_light_node) == 32 ? 1 : -1];",
             "typedef char size_path[sizeof(rtmi_light_path) == 8 ? 1 : -1];",
             "typedef char off_link[offsetof(rtmi_light_node, link) == 20 ? 1 : -1];",
             "typedef char off_depth[offsetof(rtmi_light_path, depth) == 4 ? 1 : -1];",
             "int main(void) { (void)&rtmi_light_tree_from_desc; (void)&rtmi_light_tree_pick; (void)&rtmi_light_tree_pmf;",
             "  (void)&rtmi_scene_attach_light_tree; (void)&rtmi_probe_light_tree;",
             "  return RTMI_FLAG_LIGHT_TREE == 262144u && RTMI_LIGHT_TREE_PROBE_PMF == 1 ? 0 : 1; }"]
    src = tmp_path / "c99.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-c", "-o", str(tmp_path / "c99.o")], check=True)


def test_ctypes_numpy_and_rust_match_the_header():
    assert C.sizeof(abi.LightNode) == LIGHT_NODE_DTYPE.itemsize == 32
    assert C.sizeof(abi.LightPath) == LIGHT_PATH_DTYPE.itemsize == 8
    assert FLAG == 1 << 18 and re.search(r"pub const RTMI_FLAG_LIGHT_TREE: u32 = 262144;", SYS)
    size = {"u32": 4, "f32": 4, "[f32; 3]": 12, "[u32; 2]": 8}
    for rust, ct, dt in (("RtmiLightNode", abi.LightNode, LIGHT_NODE_DTYPE), ("RtmiLightPath", abi.LightPath, LIGHT_PATH_DTYPE)):
        assert re.search(r"#\[repr\(C\)\]\n#\[derive\(Clone, Copy\)\]\npub struct %s" % rust, SYS)
        body = re.search(r"pub struct %s \{(.*?)\n\}" % rust, SYS, re.S).group(1)
        rf = [(name, size[ty.strip()]) for name, ty in re.findall(r"pub (\w+): (\[[^\]]+\]|[^,\n]+),", body)]
        assert rf == [(n, C.sizeof(t)) for n, t in ct._fields_]
        assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == [
            (n, getattr(ct, n).offset, C.sizeof(t)) for n, t in ct._fields_]


def test_exports_and_declarations_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rtmi_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(abi.RTMI_LIGHT_TREE_SYMBOLS) == ENTRIES
    lib = abi.load_rtmi()
    for n in declared:
        assert hasattr(lib, n), n
        assert re.search(r"pub fn %s\(" % n, SYS), n
    others = set()
    for name in dir(abi):
        if name.endswith("_SYMBOLS") and name != "RTMI_LIGHT_TREE_SYMBOLS":
            others |= set(getattr(abi, name))
    assert len(others) > 40 and not set(declared) & others
    host = abi.load_host()
    for n in ("rth_attach_light_tree", "rth_probe_light_tree"):
        assert hasattr(host, n), n


def _err(lib):
    return (lib.rtmi_last_error() or b"").decode()


def test_argument_errors_of_the_host_functions(host):
    lib = abi.load_rtmi()
    sc = host.lower(lts.build(host, "mixed", 16, 16)[1])
    d = sc.desc()
    nodes, paths = sc.light_tree()
    cnt = C.c_uint32(0)
    node_p, path_p = C.POINTER(abi.LightNode), C.POINTER(abi.LightPath)
    assert lib.rtmi_light_tree_from_desc(None, None, 0, C.byref(cnt), None) == 1
    assert lib.rtmi_light_tree_from_desc(C.byref(d), None, 0, None, None) == 1
    assert lib.rtmi_light_tree_from_desc(C.byref(d), None, 4, C.byref(cnt), None) == 1  # a cap without a buffer
    assert lib.rtmi_light_tree_from_desc(C.byref(d), None, 0, C.byref(cnt), None) == 0 and cnt.value == len(nodes)
    bad = abi.SceneDesc.from_buffer_copy(d)
    bad.abi_version = d.abi_version + 1
    assert lib.rtmi_light_tree_from_desc(C.byref(bad), None, 0, C.byref(cnt), None) == 1 and "abi_version" in _err(lib)
    assert lib.rtmi_scene_attach_light_tree(None, C.byref(d)) == 1
    assert lib.rtmi_probe_light_tree(None, 0, None, None, 0, None, None) == 1 and "scene" in _err(lib)

    x = np.zeros((4, 3), np.float32)
    u = np.zeros(4, np.float32)
    li = np.zeros(4, np.uint32)
    p = np.zeros(4, np.float32)
    pick, pmf = lib.rtmi_light_tree_pick, lib.rtmi_light_tree_pmf
    assert pick(nodes.ctypes.data, len(nodes), x.ctypes.data, u.ctypes.data, 4, li.ctypes.data, p.ctypes.data) == 0
    assert pick(None, len(nodes), x.ctypes.data, u.ctypes.data, 4, li.ctypes.data, p.ctypes.data) == 1
    assert pick(nodes.ctypes.data, len(nodes), None, u.ctypes.data, 4, li.ctypes.data, p.ctypes.data) == 1
    assert pick(nodes.ctypes.data, len(nodes), x.ctypes.data, None, 4, li.ctypes.data, p.ctypes.data) == 1
    assert pick(nodes.ctypes.data, 0, x.ctypes.data, u.ctypes.data, 4, li.ctypes.data, p.ctypes.data) == 1
    assert pick(nodes.ctypes.data, len(nodes) - 1, x.ctypes.data, u.ctypes.data, 4, li.ctypes.data, p.ctypes.data) == 1
    broken = nodes.copy()
    broken["link"][1] = len(nodes)  # the root's children would lie behind the array
    assert pick(broken.ctypes.data, len(nodes), x.ctypes.data, u.ctypes.data, 4, li.ctypes.data, p.ctypes.data) == 1
    assert "link" in _err(lib)
    assert pmf(nodes.ctypes.data, len(nodes), paths.ctypes.data, x.ctypes.data, li.ctypes.data, 4, p.ctypes.data) == 0
    assert pmf(nodes.ctypes.data, len(nodes), None, x.ctypes.data, li.ctypes.data, 4, p.ctypes.data) == 1
    assert pmf(nodes.ctypes.data, len(nodes), paths.ctypes.data, x.ctypes.data, li.ctypes.data, 4, None) == 1
    li[2] = len(paths)
    assert pmf(nodes.ctypes.data, len(nodes), paths.ctypes.data, x.ctypes.data, li.ctypes.data, 4, p.ctypes.data) == 1
    assert "outside the table" in _err(lib)
    del node_p, path_p


def _nee(flags):
    lib = abi.load_rtmi()
    p = default_params(16, 16, 2, flags=flags)
    cam = abi.Camera()
    rc = lib.rtmi_render_nee(None, C.byref(cam), C.byref(p), None, None, None, None, None)
    return rc, _err(lib)


def test_the_flag_on_render_nee():
    FC = abi.RTMI_FLAG_FAST_CULL
    for flags in (FLAG, FLAG | FC, FLAG | FC | abi.RTMI_FLAG_SYNC | abi.RTMI_FLAG_REF_TREE | abi.RTMI_FLAG_PATH_SIG):
        rc, msg = _nee(flags)
        assert rc == 1 and "scene" in msg, (flags, rc, msg)  # accepted: the call reaches the scene check
    rc, msg = _nee(FLAG | abi.RTMI_FLAG_LIGHT_COOP | FC)
    assert rc == 2 and "flags" in msg and "LIGHT_TREE" in msg, (rc, msg)
    rc, msg = _nee(FLAG | (1 << 20))
    assert rc == 2, (rc, msg)


@pytest.mark.parametrize("entry", ["rtmi_render_env", "rtmi_render_roulette", "rtmi_render_adaptive_nee", "rtmi_radiance",
                                   "rtmi_render_adaptive", "rtmi_render_features"])
def test_every_other_entry_answers_the_flag_as_unknown(entry):
    lib = abi.load_rtmi()
    FC = abi.RTMI_FLAG_FAST_CULL
    cam = abi.Camera()
    ad = abi.Adaptive(2, 2, 0.0, 0.0)

    def call(flags):
        p = default_params(16, 16, 4, flags=flags)
        if entry == "rtmi_render_env":
            o = abi.EnvRender(1, 0.5)
            return lib.rtmi_render_env(None, C.byref(cam), C.byref(p), C.byref(o), None, None, None, None, None)
        if entry == "rtmi_render_roulette":
            o = abi.Roulette(abi.RTMI_ROULETTE_NEE, 3, 0.05, 0.5)
            return lib.rtmi_render_roulette(None, C.byref(cam), C.byref(p), C.byref(o), None, None, None, None, None)
        if entry == "rtmi_render_adaptive_nee":
            return lib.rtmi_render_adaptive_nee(None, C.byref(cam), C.byref(p), C.byref(ad), None, None, None, None, None)
        if entry == "rtmi_render_adaptive":
            return lib.rtmi_render_adaptive(None, C.byref(cam), C.byref(p), C.byref(ad), None, None, None, None, None)
        if entry == "rtmi_render_features":
            return lib.rtmi_render_features(None, C.byref(cam), C.byref(p), None, None, None, None, None, None)
        rp = abi.RadianceParams(4, 2, abi.RTMI_ROULETTE_NEE, flags, 50, 0.001, 7, 0, 0, 0, 0.5)
        rays = np.zeros(4, np.dtype([("o", "<f4", (3,)), ("t_min", "<f4"), ("d", "<f4", (3,)), ("t_max", "<f4")]))
        rays["d"][:, 2] = 1.0
        rays["t_max"] = np.inf
        out = np.zeros(16, np.float32)
        return lib.rtmi_radiance(None, C.byref(rp), rays.ctypes.data, None, out.ctypes.data, None, None, None)

    assert call(FC) == 1 and "scene" in _err(lib), _err(lib)  # the control: without the bit the call reaches the scene check
    assert call(FC | FLAG) == 2, _err(lib)
