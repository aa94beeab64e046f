"""The public interface of adaptive sampling with NEE or environment lighting (include/rtmi_adaptive_nee.h), without a
GPU.

* the header compiles as C99 -pedantic;
* librtmi.so exports exactly the functions the header declares, abi.py lists them, sys.rs and the host library declare
  them, and the list is disjoint from every other list;
* every bad argument is refused before any device work: RTMI_ERR_INVALID for bad values, SKY (env form) and a NULL
  scene, RTMI_ERR_UNSUPPORTED for the flags and the tile split the modes do not carry."""
import ctypes as C

import pytest

import abi_kit as kit
from raytracing_rust_amd import abi
from raytracing_rust_amd.host import default_params

FORMS = ["nee", "env"]


# no word: the two names share theirs with rtmi_render_adaptive and rtmi_render_adaptive_roulette
FAMILY = kit.Family("rtmi_adaptive_nee.h", ["rtmi_render_adaptive_env", "rtmi_render_adaptive_nee"],
                    includes=["rtmi.h", "rtmi_adaptive.h", "rtmi_env.h"], host=("rth_render_adaptive_nee", "rth_render_adaptive_env"))


def test_header_is_c99(tmp_path):
    FAMILY.c99(tmp_path, body="rtmi_adaptive a = {2u, 1u, 0.0, 0.0}; rtmi_env_render o = {1u, 0.5f}; (void)a; (void)o;")


def test_exports_and_declarations_agree():
    FAMILY.exports()
    assert abi.RTMI_ADAPTIVE_NEE_SYMBOLS == ["rtmi_render_adaptive_env", "rtmi_render_adaptive_nee"]
    FAMILY.layout()  # the header defines no struct
    FAMILY.isolation()
    FAMILY.constants()


def _call(form, params=None, adaptive=None, opts=None, scene=None, cam=True, null_adaptive=False, null_opts=False,
          null_params=False):
    lib = abi.load_rtmi()
    p = default_params(32, 24, 16) if params is None else params
    a = abi.Adaptive(4, 4, 0.0, 0.0) if adaptive is None else adaptive
    o = abi.EnvRender(1, 0.5) if opts is None else opts
    c = abi.Camera()
    pc, ac, cc = (None if null_params else C.byref(p)), (None if null_adaptive else C.byref(a)), (C.byref(c) if cam else None)
    if form == "nee":
        rc = lib.rtmi_render_adaptive_nee(scene, cc, pc, ac, None, None, None, None, None)
    else:
        rc = lib.rtmi_render_adaptive_env(scene, cc, pc, None if null_opts else C.byref(o), ac, None, None, None, None, None)
    return rc, (lib.rtmi_last_error() or b"").decode()


@pytest.mark.parametrize("form", FORMS)
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
    (abi.Adaptive(4, 4, 0.0, float("-inf")), "rel_tol"),
])
def test_bad_adaptive_arguments_are_invalid_without_a_device(form, adaptive, what):
    rc, msg = _call(form, adaptive=adaptive)
    assert rc == 1 and what in msg, msg


@pytest.mark.parametrize("form", FORMS)
def test_null_arguments_and_bad_params_are_invalid(form):
    rc, msg = _call(form)
    assert rc == 1 and "scene" in msg, msg  # every value valid: the NULL scene is what is refused
    for kw in ({"cam": False}, {"null_adaptive": True}, {"null_params": True}):
        rc, msg = _call(form, **kw)
        assert rc == 1 and "NULL" in msg, (kw, msg)
    if form == "env":
        rc, msg = _call(form, null_opts=True)
        assert rc == 1 and "NULL" in msg, msg
    assert _call(form, params=default_params(0, 24, 16))[0] == 1
    rc, msg = _call(form, adaptive=abi.Adaptive(16, 4, 0.0, 0.0))  # statistics only: valid values
    assert rc == 1 and "scene" in msg, msg


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("flag", [abi.RTMI_FLAG_PATH_SIG, abi.RTMI_FLAG_PROFILE, abi.RTMI_FLAG_ASYNC, abi.RTMI_FLAG_BLOCK_COOP,
                                  abi.RTMI_FLAG_PROGRESSIVE, abi.RTMI_FLAG_TEST_OVERFLOW, 1 << 11, 1 << 20, 3 << 8])
def test_unsupported_flags(form, flag):
    rc, msg = _call(form, params=default_params(32, 24, 16, flags=flag | abi.RTMI_FLAG_FAST_CULL))
    assert rc == 2 and "flags" in msg, msg


@pytest.mark.parametrize("form", FORMS)
def test_tile_split_is_unsupported(form):
    rc, msg = _call(form, params=default_params(32, 24, 16, tile_rank=1, tile_world=2))
    assert rc == 2 and "tile_world" in msg, msg
    rc, msg = _call(form, params=default_params(32, 24, 16, tile_rank=0, tile_world=2))
    assert rc == 2 and "tile_world" in msg, msg


def test_env_form_refuses_sky_and_bad_options():
    rc, msg = _call("env", params=default_params(32, 24, 16, flags=abi.RTMI_FLAG_SKY))
    assert rc == 1 and "SKY" in msg, msg
    for o, what in ((abi.EnvRender(2, 0.5), "nee"), (abi.EnvRender(0xffffffff, 0.5), "nee"),
                    (abi.EnvRender(1, 0.0), "env_select_p"), (abi.EnvRender(0, -0.25), "env_select_p"),
                    (abi.EnvRender(1, 1.0000001), "env_select_p"), (abi.EnvRender(1, float("nan")), "env_select_p"),
                    (abi.EnvRender(1, float("inf")), "env_select_p")):
        rc, msg = _call("env", opts=o)
        assert rc == 1 and what in msg, (o.nee, o.env_select_p, msg)
    for o in (abi.EnvRender(0, 1.0), abi.EnvRender(1, 1e-6), abi.EnvRender(0, 0.5)):
        rc, msg = _call("env", opts=o)
        assert rc == 1 and "scene" in msg, msg


@pytest.mark.parametrize("form", FORMS)
def test_accepted_flags_reach_the_scene_check(form):
    accepted = (abi.RTMI_FLAG_FAST_CULL | abi.RTMI_FLAG_SYNC | abi.RTMI_FLAG_REF_TREE | abi.RTMI_FLAG_FACE_FORWARD |
                abi.RTMI_FLAG_UV_BOOK)
    if form == "nee":
        accepted |= abi.RTMI_FLAG_SKY
    for flags in (accepted, 0, abi.RTMI_FLAG_SYNC, abi.RTMI_FLAG_REF_TREE):
        rc, msg = _call(form, params=default_params(32, 24, 16, flags=flags))
        assert rc == 1 and "scene" in msg, (flags, msg)
