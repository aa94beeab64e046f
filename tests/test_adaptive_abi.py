"""Adaptive sampling's public interface (include/rtmi_adaptive.h), without a GPU.

* the header compiles as C99; the layout of rtmi_adaptive holds through header -> ctypes (abi.py) -> #[repr(C)]
  (bindings/rust/src/sys.rs), with the machinery of test_abi_layout.py;
* librtmi.so exports exactly the functions the header declares, and abi.py and sys.rs declare them;
* every bad argument is refused before any device work: RTMI_ERR_INVALID for bad values and a NULL scene,
  RTMI_ERR_UNSUPPORTED for the flags and the tile split the mode does not carry."""
import ctypes as C

import pytest

from raytracing_rust_amd import abi
from raytracing_rust_amd.host import default_params

import abi_kit as kit

FIELDS = ["min_spp", "step_spp", "abs_tol", "rel_tol"]
# isolated=False: the later adaptive headers (NEE, roulette, per pixel, windowed) take rtmi_adaptive and say the word
FAMILY = kit.Family("rtmi_adaptive.h", ["rtmi_render_adaptive"], {"rtmi_adaptive": (abi.Adaptive, "RtmiAdaptive", 24, FIELDS)},
                    word="adaptive", isolated=False, host=("rth_render_adaptive",))


def test_header_is_c99(tmp_path):
    FAMILY.c99(tmp_path, body="rtmi_adaptive a = {2u, 1u, 0.0, 0.0}; (void)a;")


def test_layout_chain_header_ctypes_rust():
    FAMILY.layout()
    assert kit.compiled_layout("rtmi_adaptive.h")["rtmi_adaptive"][:2] == (24, 8)


def test_exports_and_declarations_agree():
    FAMILY.exports()


def test_the_header_keeps_to_itself():
    FAMILY.isolation()
    FAMILY.constants()


def _call(params=None, adaptive=None, scene=None, cam=True):
    lib = abi.load_rtmi()
    p = default_params(32, 24, 16) if params is None else params
    a = abi.Adaptive(4, 4, 0.0, 0.0) if adaptive is None else adaptive
    c = abi.Camera()
    rc = lib.rtmi_render_adaptive(scene, C.byref(c) if cam else None, C.byref(p), C.byref(a), None, None, None, None, None)
    return rc, (lib.rtmi_last_error() or b"").decode()


@pytest.mark.parametrize("adaptive, what", [
    (abi.Adaptive(1, 4, 0.0, 0.0), "min_spp"),
    (abi.Adaptive(0, 4, 0.0, 0.0), "min_spp"),
    (abi.Adaptive(17, 4, 0.0, 0.0), "min_spp"),
    (abi.Adaptive(4, 0, 0.0, 0.0), "step_spp"),
    (abi.Adaptive(4, 4, -1e-3, 0.0), "abs_tol"),
    (abi.Adaptive(4, 4, 0.0, -0.5), "rel_tol"),
    (abi.Adaptive(4, 4, float("nan"), 0.0), "abs_tol"),
    (abi.Adaptive(4, 4, 0.0, float("nan")), "rel_tol"),
    (abi.Adaptive(4, 4, float("inf"), 0.0), "abs_tol"),
])
def test_bad_adaptive_arguments_are_invalid_without_a_device(adaptive, what):
    rc, msg = _call(adaptive=adaptive)
    assert rc == 1 and what in msg, msg


def test_null_arguments_and_bad_params_are_invalid():
    assert _call()[0] == 1 and "scene" in _call()[1]  # every value valid: the NULL scene is what is refused
    assert _call(cam=False)[0] == 1
    lib = abi.load_rtmi()
    p = default_params(32, 24, 16)
    assert lib.rtmi_render_adaptive(None, C.byref(abi.Camera()), C.byref(p), None, None, None, None, None, None) == 1
    assert lib.rtmi_render_adaptive(None, C.byref(abi.Camera()), None, C.byref(abi.Adaptive(4, 4, 0.0, 0.0)), None, None, None, None,
                                    None) == 1
    assert _call(params=default_params(0, 24, 16))[0] == 1
    assert _call(params=default_params(32, 24, 16), adaptive=abi.Adaptive(16, 4, 0.0, 0.0))[0] == 1  # statistics only: valid values
    assert "scene" in _call(params=default_params(32, 24, 16), adaptive=abi.Adaptive(16, 4, 0.0, 0.0))[1]


@pytest.mark.parametrize("flag", [abi.RTMI_FLAG_PATH_SIG, 4, abi.RTMI_FLAG_ASYNC, 32768, abi.RTMI_FLAG_PROGRESSIVE, 8192, 1 << 11, 3 << 8])
def test_unsupported_flags(flag):
    rc, msg = _call(params=default_params(32, 24, 16, flags=flag | abi.RTMI_FLAG_FAST_CULL))
    assert rc == 2 and "flags" in msg, msg


def test_tile_split_is_unsupported():
    rc, msg = _call(params=default_params(32, 24, 16, tile_rank=1, tile_world=2))
    assert rc == 2 and "tile_world" in msg, msg


def test_accepted_flags_reach_the_scene_check():
    accepted = (abi.RTMI_FLAG_FAST_CULL | abi.RTMI_FLAG_SYNC | abi.RTMI_FLAG_REF_TREE | abi.RTMI_FLAG_SKY |
                abi.RTMI_FLAG_FACE_FORWARD | abi.RTMI_FLAG_UV_BOOK)
    rc, msg = _call(params=default_params(32, 24, 16, flags=accepted))
    assert rc == 1 and "scene" in msg, msg
