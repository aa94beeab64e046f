"""Next-event estimation's public interface (include/rtmi_nee.h), without a GPU.

* the header compiles as C99 and rtmi_light is the 48-byte record it states;
* librtmi.so and librt_host.so export the functions, abi.py and sys.rs declare them, and the NEE list is disjoint
  from the other lists;
* every bad argument, unsupported flag, tile split and missing light table is refused before any device work."""
import ctypes as C
import os

import pytest

import abi_kit as kit
from raytracing_rust_amd import abi
from raytracing_rust_amd.host import default_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


FIELDS = ["item", "prim", "kind", "material", "area", "weight", "select_p", "cdf"]
# isolated=False: "nee" names the estimator in every later lighting header, and is part of rtmi_render_adaptive_nee
FAMILY = kit.Family("rtmi_nee.h", ["rtmi_lights_from_desc", "rtmi_render_nee", "rtmi_scene_attach_lights"],
                    {"rtmi_light": (abi.Light, "RtmiLight", 48, FIELDS)}, word="nee", isolated=False,
                    host=("rth_render_nee", "rth_attach_lights"))


def test_header_is_c99(tmp_path):
    FAMILY.c99(tmp_path)


def test_light_record_layout():
    FAMILY.layout()


def test_exports_and_declarations_agree():
    FAMILY.exports()


def test_the_header_keeps_to_itself():
    FAMILY.isolation()
    FAMILY.constants()


def _call(params=None, scene=None, cam=True, params_null=False):
    lib = abi.load_rtmi()
    p = default_params(32, 24, 16) if params is None else params
    c = abi.Camera()
    rc = lib.rtmi_render_nee(scene, C.byref(c) if cam else None, None if params_null else C.byref(p), None, None, None,
                             None, None)
    return rc, (lib.rtmi_last_error() or b"").decode()


def test_null_arguments_and_bad_params_are_invalid():
    rc, msg = _call()
    assert rc == 1 and "scene" in msg, msg  # every value valid: the NULL scene is what is refused
    rc, msg = _call(cam=False)
    assert rc == 1 and "NULL" in msg, msg
    rc, msg = _call(params_null=True)
    assert rc == 1 and "NULL" in msg, msg
    for bad in (default_params(0, 24, 16), default_params(32, 0, 16), default_params(32, 24, 0)):
        rc, msg = _call(params=bad)
        assert rc == 1 and "positive" in msg, msg
    rc, msg = _call(params=default_params(32, 24, 16, tile_rank=2, tile_world=2))
    assert rc == 1 and "tile_rank" in msg, msg


@pytest.mark.parametrize("flag", [abi.RTMI_FLAG_PROFILE, abi.RTMI_FLAG_ASYNC, abi.RTMI_FLAG_BLOCK_COOP,
                                  abi.RTMI_FLAG_PROGRESSIVE, abi.RTMI_FLAG_TEST_OVERFLOW, 1 << 11, 3 << 8, 1 << 20])
def test_unsupported_flags(flag):
    rc, msg = _call(params=default_params(32, 24, 16, flags=flag | abi.RTMI_FLAG_FAST_CULL))
    assert rc == 2 and "flags" in msg, msg


def test_tile_split_is_unsupported():
    rc, msg = _call(params=default_params(32, 24, 16, tile_rank=1, tile_world=2))
    assert rc == 2 and "tile_world" in msg, msg


def test_accepted_flags_reach_the_scene_check():
    accepted = (abi.RTMI_FLAG_FAST_CULL | abi.RTMI_FLAG_SYNC | abi.RTMI_FLAG_REF_TREE | abi.RTMI_FLAG_SKY |
                abi.RTMI_FLAG_FACE_FORWARD | abi.RTMI_FLAG_UV_BOOK | abi.RTMI_FLAG_PATH_SIG)
    rc, msg = _call(params=default_params(32, 24, 16, flags=accepted))
    assert rc == 1 and "scene" in msg, msg


def test_attach_and_table_arguments():
    lib = abi.load_rtmi()
    n = C.c_uint32(7)
    assert lib.rtmi_scene_attach_lights(None, None) == 1
    assert lib.rtmi_lights_from_desc(None, None, 0, C.byref(n)) == 1
    d = abi.SceneDesc()
    assert lib.rtmi_lights_from_desc(C.byref(d), None, 0, None) == 1  # count is NULL
    assert lib.rtmi_lights_from_desc(C.byref(d), None, 0, C.byref(n)) == 1  # abi_version 0
    assert "abi_version" in lib.rtmi_last_error().decode()
    d.abi_version = abi.RTMI_ABI_VERSION
    assert lib.rtmi_lights_from_desc(C.byref(d), None, 4, C.byref(n)) == 1  # cap without a buffer
    assert lib.rtmi_lights_from_desc(C.byref(d), None, 0, C.byref(n)) == 0 and n.value == 0  # the empty world


def test_missing_attach_is_checked_before_device_work():
    """The refusal of a handle without a light table (RTMI_ERR_INVALID) is tested on the device
    (tests/test_gpu_nee.py); here: the check precedes the entry point's first device call."""
    src = open(os.path.join(ROOT, "raytracing_rust_amd", "csrc", "rtmi_device.hip")).read()

    def body_of(signature):
        body = src[src.index(signature):]
        return body[:body.index("\n}\n")]

    # the entry point hands over to render_fixed, which begins with begin_call; neither touches the device before that
    entry = body_of('extern "C" int rtmi_render_nee(')
    assert "hip" not in entry[:entry.index("render_fixed(")]
    fixed = body_of("static int render_fixed(")
    assert "hip" not in fixed[:fixed.index("begin_call(")]
    # begin_call makes the check (check_attached, no device call in it) before the path's first device call
    begin = body_of("int begin_call(")
    assert begin.index("check_attached(") < begin.index("hipSetDevice")
    attached = body_of("int check_attached(")
    assert "!s->has_lights" in attached and "hip" not in attached
