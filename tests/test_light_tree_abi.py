"""The light tree's public interface (include/rtmi_light_tree.h), without a GPU.

* the header compiles as C99 and its two structs have the documented sizes, in the header, in ctypes and in sys.rs;
* librtmi.so and librt_host.so export the entries, abi.py and sys.rs declare them, and no other symbol list names them;
* bad arguments are refused before a device is touched;
* RTMI_FLAG_LIGHT_TREE is a flag of rtmi_render_nee alone: there it reaches the scene check, beside RTMI_FLAG_LIGHT_COOP it
  is RTMI_ERR_UNSUPPORTED, and every other lighting entry answers it as an unknown flag."""
import ctypes as C

import numpy as np
import pytest

import light_tree_scenes as lts
import abi_kit as kit
from raytracing_rust_amd import abi, default_params
from raytracing_rust_amd.host import LIGHT_NODE_DTYPE, LIGHT_PATH_DTYPE

ENTRIES = ["rtmi_light_tree_from_desc", "rtmi_light_tree_pick", "rtmi_light_tree_pmf", "rtmi_probe_light_tree",
           "rtmi_scene_attach_light_tree"]
FLAG = abi.RTMI_FLAG_LIGHT_TREE


FAMILY = kit.Family("rtmi_light_tree.h", ENTRIES, {"rtmi_light_node": (abi.LightNode, "RtmiLightNode", 32, None),
                                                   "rtmi_light_path": (abi.LightPath, "RtmiLightPath", 8, None)},
                    word="light_tree", includes=["rtmi_nee.h"], host=("rth_attach_light_tree", "rth_probe_light_tree"))


def test_header_is_c99_with_the_documented_layout(tmp_path):
    FAMILY.c99(tmp_path, holds="RTMI_FLAG_LIGHT_TREE == 262144u && RTMI_LIGHT_TREE_PROBE_PMF == 1 && "
               "offsetof(rtmi_light_node, link) == 20 && offsetof(rtmi_light_path, depth) == 4")


def test_ctypes_numpy_and_rust_match_the_header():
    FAMILY.layout()
    kit.assert_plain_repr_c("RtmiLightNode", "RtmiLightPath")
    assert "RTMI_FLAG_LIGHT_TREE" in FAMILY.constants()[1] and FLAG == 1 << 18
    kit.assert_rust_const("RTMI_FLAG_LIGHT_TREE", "u32", 262144)
    for ct, dt in ((abi.LightNode, LIGHT_NODE_DTYPE), (abi.LightPath, LIGHT_PATH_DTYPE)):
        assert C.sizeof(ct) == dt.itemsize
        assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == [
            (n, getattr(ct, n).offset, C.sizeof(t)) for n, t in ct._fields_]


def test_exports_and_declarations_agree():
    FAMILY.exports()
    FAMILY.isolation()


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
