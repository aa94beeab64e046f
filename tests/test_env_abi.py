"""Environment lighting's public interface (include/rtmi_env.h), without a GPU.

* the header compiles as C99 -pedantic; rtmi_env_map and rtmi_env_render agree across header, ctypes and sys.rs;
* librtmi.so exports the functions the header declares, abi.py and sys.rs declare them, and the list is disjoint from the
  other lists;
* every bad argument, the SKY flag, unsupported flags, a tile split and a bad map are refused before any device work;
* read_pfm inverts pfm_bytes."""
import ctypes as C
import os

import numpy as np
import pytest

from raytracing_rust_amd import abi, pfm_bytes, read_pfm
from raytracing_rust_amd.host import default_params

import abi_kit as kit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"rtmi_env_map": (abi.EnvMap, "RtmiEnvMap", 16, ["width", "height", "rgb"]),
           "rtmi_env_render": (abi.EnvRender, "RtmiEnvRender", 8, ["nee", "env_select_p"])}
# isolated=False: every later lighting header takes rtmi_env_render or names the map, and "env" is part of other words
FAMILY = kit.Family("rtmi_env.h", ["rtmi_env_tables", "rtmi_probe_env", "rtmi_render_env", "rtmi_scene_attach_env"], STRUCTS,
                    word="env", isolated=False, host=("rth_attach_env", "rth_render_env", "rth_probe_env"))


def test_header_is_c99(tmp_path):
    FAMILY.c99(tmp_path, before=("stdio.h",))


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_layout_chain_header_ctypes_rust(name):
    FAMILY.layout(only=name)


def test_exports_and_declarations_agree():
    FAMILY.exports()


def test_the_header_keeps_to_itself():
    FAMILY.isolation()
    FAMILY.constants()


def _call(params=None, cam=True, params_null=False, opts="default"):
    lib = abi.load_rtmi()
    p = default_params(32, 24, 16) if params is None else params
    c = abi.Camera()
    o = abi.EnvRender(1, 0.5) if opts == "default" else opts
    rc = lib.rtmi_render_env(None, C.byref(c) if cam else None, None if params_null else C.byref(p),
                             C.byref(o) if o is not None else None, None, None, None, None, None)
    return rc, (lib.rtmi_last_error() or b"").decode()


def test_null_arguments_and_bad_params_are_invalid():
    rc, msg = _call()
    assert rc == 1 and "scene" in msg, msg  # every value valid: the NULL scene is what is refused
    for kw in (dict(cam=False), dict(params_null=True), dict(opts=None)):
        rc, msg = _call(**kw)
        assert rc == 1 and "NULL" in msg, (kw, msg)
    for bad in (default_params(0, 24, 16), default_params(32, 0, 16), default_params(32, 24, 0)):
        rc, msg = _call(params=bad)
        assert rc == 1 and "positive" in msg, msg
    rc, msg = _call(params=default_params(32, 24, 16, tile_rank=2, tile_world=2))
    assert rc == 1 and "tile_rank" in msg, msg


def test_sky_is_invalid():
    rc, msg = _call(params=default_params(32, 24, 16, flags=abi.RTMI_FLAG_SKY))
    assert rc == 1 and "SKY" in msg, msg
    rc, msg = _call(params=default_params(32, 24, 16, flags=abi.RTMI_FLAG_SKY | abi.RTMI_FLAG_FAST_CULL))
    assert rc == 1 and "SKY" in msg, msg


@pytest.mark.parametrize("opts,word", [(abi.EnvRender(2, 0.5), "nee"), (abi.EnvRender(1, 0.0), "env_select_p"),
                                       (abi.EnvRender(0, -0.5), "env_select_p"), (abi.EnvRender(1, 1.0000001), "env_select_p"),
                                       (abi.EnvRender(1, float("nan")), "env_select_p")])
def test_bad_options_are_invalid(opts, word):
    rc, msg = _call(opts=opts)
    assert rc == 1 and word in msg, msg


@pytest.mark.parametrize("flag", [abi.RTMI_FLAG_PROFILE, abi.RTMI_FLAG_ASYNC, abi.RTMI_FLAG_BLOCK_COOP,
                                  abi.RTMI_FLAG_PROGRESSIVE, abi.RTMI_FLAG_TEST_OVERFLOW, 1 << 11, 3 << 8, 1 << 20])
def test_unsupported_flags(flag):
    rc, msg = _call(params=default_params(32, 24, 16, flags=flag | abi.RTMI_FLAG_FAST_CULL))
    assert rc == 2 and "flags" in msg, msg


def test_tile_split_is_unsupported():
    rc, msg = _call(params=default_params(32, 24, 16, tile_rank=1, tile_world=2))
    assert rc == 2 and "tile_world" in msg, msg


def test_accepted_flags_and_options_reach_the_scene_check():
    accepted = (abi.RTMI_FLAG_FAST_CULL | abi.RTMI_FLAG_SYNC | abi.RTMI_FLAG_REF_TREE | abi.RTMI_FLAG_FACE_FORWARD |
                abi.RTMI_FLAG_UV_BOOK | abi.RTMI_FLAG_PATH_SIG)
    for o in (abi.EnvRender(0, 0.5), abi.EnvRender(1, 1.0), abi.EnvRender(1, 1e-6)):
        rc, msg = _call(params=default_params(32, 24, 16, flags=accepted), opts=o)
        assert rc == 1 and "scene" in msg, msg


def _map(w, h, data=None):
    a = np.ones((h, w, 3), np.float32) if data is None else data
    return abi.EnvMap(w, h, a.ctypes.data), a


@pytest.mark.parametrize("w,h", [(0, 4), (4, 0), (16385, 1), (1, 16385), (8192, 4097)])
def test_bad_map_sizes_are_invalid(w, h):
    lib = abi.load_rtmi()
    m = abi.EnvMap(w, h, np.ones(3, np.float32).ctypes.data)  # the size check comes before any texel is read
    assert lib.rtmi_env_tables(C.byref(m), None, None, None, None, None) == 1
    assert "width and height" in lib.rtmi_last_error().decode()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, -1e-30, -1.0])
def test_bad_texels_are_invalid(bad):
    lib = abi.load_rtmi()
    a = np.ones((3, 5, 3), np.float32)
    a[2, 4, 1] = bad
    m, _ = _map(5, 3, a)
    assert lib.rtmi_env_tables(C.byref(m), None, None, None, None, None) == 1
    assert "finite" in lib.rtmi_last_error().decode()


def test_map_and_probe_arguments():
    lib = abi.load_rtmi()
    assert lib.rtmi_env_tables(None, None, None, None, None, None) == 1
    m = abi.EnvMap(4, 2, None)
    assert lib.rtmi_env_tables(C.byref(m), None, None, None, None, None) == 1
    m, keep = _map(4, 2)
    total = C.c_double(-1.0)
    assert lib.rtmi_env_tables(C.byref(m), None, None, None, None, C.byref(total)) == 0 and total.value > 0
    assert lib.rtmi_scene_attach_env(None, C.byref(m)) == 1
    assert lib.rtmi_scene_attach_env(None, None) == 1
    buf = np.zeros(8, np.float32)
    assert lib.rtmi_probe_env(None, 0, buf.ctypes.data, buf.ctypes.data, 1) == 1
    a = np.ones((2, 2, 3), np.float32)
    a[0, 0, 0] = np.nan
    bad, _ = _map(2, 2, a)
    # a bad map is refused before the handle is touched (the handle here is not even valid)
    assert lib.rtmi_scene_attach_env(C.c_void_p(8), C.byref(bad)) == 1


def test_checks_come_before_device_work():
    """The refusals of a handle without a map or light table are tested on the device (tests/test_gpu_env.py); here: the
    checks precede the entry points' first device call."""
    src = open(os.path.join(ROOT, "raytracing_rust_amd", "csrc", "rtmi_device.hip")).read()

    def body_of(signature):
        body = src[src.index(signature):]
        return body[:body.index("\n}\n")]

    # The entry point calls the two option checks, then hands over to render_fixed, which begins with begin_call; none of
    # them touches the device before that.
    entry = body_of('extern "C" int rtmi_render_env(')
    assert entry.index("refuse_sky(") < entry.index("check_env_opts(") < entry.index("render_fixed(")
    assert "hip" not in entry[:entry.index("render_fixed(")]
    assert "RTMI_FLAG_SKY" in body_of("static int refuse_sky(") and "hip" not in body_of("static int refuse_sky(")
    assert "env_select_p" in body_of("static int check_env_opts(") and "hip" not in body_of("static int check_env_opts(")
    fixed = body_of("static int render_fixed(")
    assert "hip" not in fixed[:fixed.index("begin_call(")]
    # begin_call makes the attach checks (check_attached, no device call in it) before the path's first device call
    begin = body_of("int begin_call(")
    assert begin.index("check_attached(") < begin.index("hipSetDevice")
    attached = body_of("int check_attached(")
    for check in ("!s->has_env", "!s->has_lights"):
        assert check in attached and "hip" not in attached, check
    body = src[src.index('extern "C" int rtmi_scene_attach_env('):]
    assert body.index("rtmi_env_build_tables") < body.index("hipSetDevice")
    body = src[src.index('extern "C" int rtmi_probe_env('):]
    assert body.index("!s->has_env") < body.index("hipSetDevice")


@pytest.mark.parametrize("shape", [(1, 1, 3), (7, 5, 3), (3, 4), (64, 32, 3)])
def test_read_pfm_inverts_pfm_bytes(shape):
    a = np.random.default_rng(5).random(shape).astype(np.float32) * np.float32(1e4)
    b = read_pfm(pfm_bytes(a))
    assert b.dtype == np.float32 and b.shape == a.shape and b.tobytes() == a.tobytes()


def test_read_pfm_big_endian_and_errors():
    a = np.arange(12, dtype=np.float32).reshape(2, 2, 3)
    data = b"PF\n2 2\n1.0\n" + np.ascontiguousarray(a[::-1], dtype=">f4").tobytes()
    assert read_pfm(data).tobytes() == a.tobytes()
    for bad in (b"P6\n2 2\n-1.0\n" + bytes(48), b"PF\n2 2\n-1.0\n" + bytes(40), b"PF\n2\n"):
        with pytest.raises(ValueError):
            read_pfm(bad)
