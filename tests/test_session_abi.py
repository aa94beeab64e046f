"""The public interface of render sessions (include/rtmi_session.h), without a GPU.

* the header compiles alone as C99 -pedantic and the options struct has the size of its ctypes mirror;
* librtmi.so exports exactly the functions the header declares, abi.SESSION_SYMBOLS lists them, the host library has
  the pass-throughs, and no exported name carries the family word of another header (the other *_abi tests match their
  exports by those substrings);
* nothing was added to rtmi.h;
* every bad argument is refused before any device work: RTMI_ERR_INVALID or RTMI_ERR_UNSUPPORTED with the documented
  message, a NULL scene being what a valid call is refused for."""
import ctypes as C
import os

import pytest

import abi_kit as kit
from raytracing_rust_amd import abi
from raytracing_rust_amd.host import default_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY_WORDS = ("roulette", "nee", "env", "adaptive", "denoise", "features", "f64", "light")
INVALID, UNSUPPORTED = 1, 2


# rust=False: bindings/rust/src/sys.rs declares nothing of this header yet (a gap older than the kit; adding the block is its own change)
FAMILY = kit.Family("rtmi_session.h", ["rtmi_session_create", "rtmi_session_destroy", "rtmi_session_export", "rtmi_session_image",
                                       "rtmi_session_import", "rtmi_session_merge", "rtmi_session_refine", "rtmi_session_render",
                                       "rtmi_session_spp"],
                    {"rtmi_session_opts": (abi.SessionOpts, None, 32, None)}, word="session", rust=False, includes=["rtmi.h", "rtmi_roulette.h"],
                    host=tuple("rth_session_" + n for n in ("create", "close", "render", "refine", "image", "export", "import", "merge", "spp")))


def test_header_is_c99(tmp_path):
    FAMILY.c99(tmp_path, body="rtmi_session_opts o = {RTMI_ROULETTE_ENV_NEE, 1u, 2u, 0.25f, 0.5f, 0u, 8u, 8u}; (void)o;",
               holds="sizeof(rtmi_session_opts) == 32 && RTMI_SESSION_BLOB_HEADER == 216u")


def test_options_struct_mirror():
    FAMILY.layout()
    assert sorted(FAMILY.constants()[0]) == ["RTMI_SESSION_BLOB_HEADER", "RTMI_SESSION_BLOB_IDENTITY", "RTMI_SESSION_BLOB_VERSION"]


def test_exports_and_declarations_agree():
    FAMILY.exports()
    for n in FAMILY.entries:
        assert n.startswith("rtmi_session_") and not any(w in n for w in FAMILY_WORDS), n


def test_nothing_was_added_to_rtmi_h():
    FAMILY.isolation()
    # ... and the session header defines no flag bit of its own
    assert "RTMI_FLAG_" not in kit.header_text("rtmi_session.h")


def _opts(estimator=1, rr=0, min_depth=0, q_min=0.0, env_select_p=0.5, first_sample=0, min_spp=0, step_spp=0):
    return abi.SessionOpts(estimator, rr, min_depth, q_min, env_select_p, first_sample, min_spp, step_spp)


def _create(params=None, opts=None, cam=True, null_opts=False, null_params=False, null_out=False):
    lib = abi.load_rtmi()
    p = default_params(32, 24, 1) if params is None else params
    o = _opts() if opts is None else opts
    c = abi.Camera()
    out = C.c_void_p(0)
    rc = lib.rtmi_session_create(None, C.byref(c) if cam else None, None if null_params else C.byref(p),
                                 None if null_opts else C.byref(o), None if null_out else C.byref(out))
    assert not out.value
    return rc, (lib.rtmi_last_error() or b"").decode()


def test_null_arguments_and_bad_params_are_invalid():
    rc, msg = _create()
    assert rc == INVALID and "rtmi_session_create: scene is NULL" in msg, msg  # every value valid: the NULL scene is refused
    for kw in ({"cam": False}, {"null_opts": True}, {"null_params": True}, {"null_out": True}):
        rc, msg = _create(**kw)
        assert rc == INVALID and "NULL argument" in msg, (kw, msg)
    assert _create(params=default_params(0, 24, 1))[0] == INVALID
    rc, msg = _create(params=default_params(32, 24, 0))  # ns is not read
    assert rc == INVALID and "scene is NULL" in msg, msg


@pytest.mark.parametrize("opts, what", [
    (_opts(estimator=4), "estimator"), (_opts(estimator=0xffffffff), "estimator"), (_opts(rr=2), "rr"),
    (_opts(rr=1, min_depth=0, q_min=0.25), "min_depth"), (_opts(rr=1, min_depth=2, q_min=0.0), "q_min"),
    (_opts(rr=1, min_depth=2, q_min=1.0000001), "q_min"), (_opts(rr=1, min_depth=2, q_min=float("nan")), "q_min"),
    (_opts(estimator=3, env_select_p=0.0), "env_select_p"), (_opts(estimator=3, env_select_p=float("nan")), "env_select_p"),
    (_opts(min_spp=1, step_spp=8), "min_spp"), (_opts(min_spp=0, step_spp=8), "min_spp"), (_opts(min_spp=8, step_spp=0), "step_spp"),
    (_opts(min_spp=8, step_spp=8, first_sample=7), "first_sample"), (_opts(first_sample=1 << 31), "first_sample"),
])
def test_bad_options_are_invalid_without_a_device(opts, what):
    rc, msg = _create(opts=opts)
    assert rc == INVALID and what in msg and msg.startswith("rtmi_session_create: "), msg


def test_valid_options_reach_the_scene_check():
    # the roulette fields are read with rr = 1 only, env_select_p by ENV_NEE only
    for o in (_opts(estimator=0), _opts(estimator=0, min_depth=0, q_min=-1.0), _opts(estimator=1, env_select_p=float("nan")),
              _opts(estimator=2, env_select_p=-1.0), _opts(estimator=3, env_select_p=1.0), _opts(rr=1, min_depth=2, q_min=0.25),
              _opts(rr=1, min_depth=1000, q_min=1.0), _opts(min_spp=2, step_spp=1), _opts(first_sample=7)):
        rc, msg = _create(opts=o)
        assert rc == INVALID and "scene is NULL" in msg, msg


@pytest.mark.parametrize("est", [0, 1, 2, 3])
def test_sky_is_refused_with_the_map_estimators_only(est):
    rc, msg = _create(opts=_opts(estimator=est), params=default_params(32, 24, 1, flags=abi.RTMI_FLAG_SKY))
    assert rc == INVALID and ("SKY" if est >= 2 else "scene is NULL") in msg, msg


@pytest.mark.parametrize("flag, what", [
    (abi.RTMI_FLAG_PATH_SIG, "PATH_SIG"), (abi.RTMI_FLAG_PROFILE, "flags"), (abi.RTMI_FLAG_ASYNC, "flags"),
    (abi.RTMI_FLAG_BLOCK_COOP, "flags"), (abi.RTMI_FLAG_PROGRESSIVE, "flags"), (abi.RTMI_FLAG_TEST_OVERFLOW, "flags"),
    (1 << 11, "flags"), (1 << 20, "flags"), (3 << 8, "flags")])
def test_unsupported_flags(flag, what):
    rc, msg = _create(params=default_params(32, 24, 1, flags=flag | abi.RTMI_FLAG_FAST_CULL))
    assert rc == UNSUPPORTED and what in msg, msg


def test_tile_split_is_unsupported():
    for rank in (0, 1):
        rc, msg = _create(params=default_params(32, 24, 1, tile_rank=rank, tile_world=2))
        assert rc == UNSUPPORTED and "tile_world" in msg, msg
    rc, msg = _create(opts=_opts(first_sample=1 << 26))
    assert rc == UNSUPPORTED and "2^26" in msg, msg


def test_accepted_flags_reach_the_scene_check():
    accepted = (abi.RTMI_FLAG_FAST_CULL | abi.RTMI_FLAG_SYNC | abi.RTMI_FLAG_REF_TREE | abi.RTMI_FLAG_FACE_FORWARD |
                abi.RTMI_FLAG_UV_BOOK)
    for est in (0, 1, 2, 3):
        for flags in (accepted | (abi.RTMI_FLAG_SKY if est < 2 else 0), 0, abi.RTMI_FLAG_FAST_CULL | abi.RTMI_FLAG_LIGHT_COOP,
                      abi.RTMI_FLAG_FAST_CULL | abi.RTMI_FLAG_ROULETTE_COOP):
            rc, msg = _create(opts=_opts(estimator=est), params=default_params(32, 24, 1, flags=flags))
            assert rc == INVALID and "scene is NULL" in msg, (est, flags, msg)


def test_calls_on_a_null_session_are_invalid():
    lib = abi.load_rtmi()
    st, need, lo = abi.Stats(), C.c_size_t(0), C.c_uint32(0)
    for name, rc in (("render", lib.rtmi_session_render(None, 4, C.byref(st))),
                     ("refine", lib.rtmi_session_refine(None, 0.0, 0.0, 16, C.byref(st))),
                     ("image", lib.rtmi_session_image(None, None, None, None, None, None)),
                     ("export", lib.rtmi_session_export(None, None, 0, C.byref(need))),
                     ("import", lib.rtmi_session_import(None, b"x", 1)),
                     ("merge", lib.rtmi_session_merge(None, None)),
                     ("spp", lib.rtmi_session_spp(None, C.byref(lo), None))):
        assert rc == INVALID, name
    lib.rtmi_session_destroy(None)  # a no-op


def test_entry_points_check_before_the_device():
    src = open(os.path.join(ROOT, "raytracing_rust_amd", "csrc", "rtmi_session.hip")).read()

    def body_of(signature):
        body = src[src.index(signature):]
        return body[:body.index("\n}\n")]

    create = body_of('extern "C" int rtmi_session_create(')
    assert "hip" not in create[:create.index("begin_call(")]
    for name in ("render", "refine"):
        entry = body_of('extern "C" int rtmi_session_%s(' % name)
        assert "hip" not in entry[:entry.index("session_begin(")].replace("hipcc", ""), name
    begin = body_of("static int session_begin(")
    assert begin.index("begin_call(") < begin.index("reserve_texels(")
