"""The frame pipeline's public interface (include/rtmi_frame.h), without a GPU.

* the header compiles as C99 and its two structs have the size and offsets the host reads them with, in the header, in
  ctypes and in sys.rs;
* librtmi.so exports the entries the header declares, abi.py and sys.rs declare them, the package exports Frame, and no
  other family's list holds one of them;
* the numpy restatement of the un-tiling (tests/frame_ref.py) inverts a tiling written out by hand;
* every bad argument that needs no device is refused, with its code and the entry's name, in the documented order.  create
  is called with a NULL scene, which is checked after every argument and flag, so a valid set of arguments ends at "scene
  is NULL" on every machine; render checks its handle last, so a NULL handle shows every other refusal (the refusals that
  need a live handle: tests/test_gpu_frame.py)."""
import ctypes as C

import numpy as np
import pytest

import frame_ref as ref
import temporal_ref
import abi_kit as kit
from raytracing_rust_amd import Frame, Scene, abi

ENTRIES = ["rtmi_frame_create", "rtmi_frame_destroy", "rtmi_frame_render", "rtmi_frame_render_device", "rtmi_frame_reset",
           "rtmi_probe_frame_untile"]
OPTS_OFFSETS = {"estimator": 0, "env_select_p": 4, "temporal": 8, "denoise": 40, "flags": 72, "reserved": 76}
OUT_FIELDS = ["linear", "rgb8", "noisy_linear", "noisy_stderr", "albedo", "normal", "depth", "hits", "accum_linear",
              "accum_stderr", "history", "motion"]
INVALID, UNSUPPORTED = 1, 2
# isolated=False: "frame" is an everyday word of the other headers' comments; the test below holds "rtmi_frame" out of them
FAMILY = kit.Family("rtmi_frame.h", ENTRIES, {"rtmi_frame_opts": (abi.FrameOpts, "RtmiFrameOpts", 96, OPTS_OFFSETS),
                                              "rtmi_frame_out": (abi.FrameOut, "RtmiFrameOut", 96, {f: 8 * k for k, f in enumerate(OUT_FIELDS)})},
                    word="frame", isolated=False, includes=["rtmi.h", "rtmi_denoise.h", "rtmi_roulette.h", "rtmi_temporal.h"],
                    documented=True, host=("rth_frame_create", "rth_frame_close", "rth_frame_render", "rth_frame_reset"))


# ---- layout -----------------------------------------------------------------------------------------------------------------
def test_header_is_c99_with_the_documented_layout(tmp_path):
    FAMILY.c99(tmp_path, holds="RTMI_FRAME_NO_TEMPORAL == 1u && RTMI_FRAME_NO_FILTER == 2u")


def test_ctypes_and_rust_match_the_header():
    FAMILY.layout()
    kit.assert_plain_repr_c("RtmiFrameOpts", "RtmiFrameOut")
    assert all(ty in ("*mut f32", "*mut u8", "*mut u32") for _, ty in kit.rust_fields("RtmiFrameOut"))
    kit.assert_rust_const("RTMI_FRAME_NO_TEMPORAL", "u32", 1)
    kit.assert_rust_const("RTMI_FRAME_NO_FILTER", "u32", 2)
    in_abi, in_rust = FAMILY.constants()
    assert in_abi == in_rust == ["RTMI_FRAME_NO_TEMPORAL", "RTMI_FRAME_NO_FILTER"]
    assert abi.RTMI_FRAME_NO_TEMPORAL == 1 and abi.RTMI_FRAME_NO_FILTER == 2


def test_exports_and_declarations_agree():
    FAMILY.exports()  # the seams of rtmi_frame_launch.hpp are hidden
    assert Frame.render.__doc__ and Frame.__doc__ and Scene.frame.__doc__


def test_nothing_was_added_to_the_other_headers():
    FAMILY.isolation()
    for other in ("rtmi.h", "rtmi_temporal.h", "rtmi_denoise.h", "rtmi_features.h"):
        assert "rtmi_frame" not in kit.header_text(other, comments=True), other
    assert "RTMI_FLAG_" not in kit.header_text("rtmi_frame.h")


# ---- the restatement --------------------------------------------------------------------------------------------------------
def test_the_restatement_inverts_a_tiling_written_by_hand():
    for nx, ny in ((1, 1), (1, 17), (8, 8), (9, 8), (37, 23)):
        tx, ty = ref.tiles(nx, ny)
        tex = np.zeros((ref.texel_count(nx, ny), 4), np.uint32)
        se = np.zeros((ref.texel_count(nx, ny), 3), np.float32)
        img = np.arange(nx * ny * 3, dtype=np.float32).reshape(ny, nx, 3) + 0.5
        for y in range(ny):
            for x in range(nx):
                k = ((y // 8) * tx + x // 8) * 64 + (y % 8) * 8 + x % 8
                tex[k, :3] = img[y, x].view(np.uint32)
                se[k] = -img[y, x]
        lin, e, poisoned = ref.untile(nx, ny, tex, se)
        assert lin.tobytes() == img.tobytes() and e.tobytes() == (-img).tobytes() and poisoned == 0
        assert ref.untile(nx, ny, tex)[1] is None
        pad = ref.padding_texels(nx, ny)
        assert len(pad) == tx * ty * 64 - nx * ny and not tex[pad].any()
        tex[pad, 3] = ref.POISON  # the padding is never counted
        assert ref.untile(nx, ny, tex)[2] == 0
        tex[ref.tiled_index(nx, ny)[ny - 1, nx - 1], 3] |= ref.POISON
        tex[ref.tiled_index(nx, ny)[0, 0], 3] |= ref.POISON
        assert ref.untile(nx, ny, tex)[2] == (1 if nx * ny == 1 else 2)


# ---- refusals without a device ------------------------------------------------------------------------------------------------
FC = abi.RTMI_FLAG_FAST_CULL
ACCEPTED = (abi.RTMI_FLAG_FAST_CULL, abi.RTMI_FLAG_SYNC, abi.RTMI_FLAG_REF_TREE, abi.RTMI_FLAG_SKY, abi.RTMI_FLAG_FACE_FORWARD,
            abi.RTMI_FLAG_UV_BOOK)
REFUSED = (abi.RTMI_FLAG_PATH_SIG, abi.RTMI_FLAG_PROFILE, abi.RTMI_FLAG_ASYNC, abi.RTMI_FLAG_BLOCK_COOP,
           abi.RTMI_FLAG_TEST_OVERFLOW, abi.RTMI_FLAG_PROGRESSIVE, abi.RTMI_FLAG_ROULETTE_COOP, abi.RTMI_FLAG_LIGHT_TREE,
           256, 512, 1024, 2048, 1 << 19, 1 << 31)
T_DEFAULT = dict(max_history=32, alpha_min=0.0, depth_tol=0.05, normal_min=0.9, albedo_min=1e-3, flags=0, reserved=(0, 0))
D_DEFAULT = dict(iterations=5, normal_power=128, sigma_l=4.0, sigma_z=1.0, eps_l=1e-10, eps_z=1e-3, albedo_min=1e-3, flags=0)


def _create(params=True, opts=True, out=True, nx=8, ny=8, flags=FC, tile_rank=0, tile_world=1, estimator=0, env_select_p=0.5,
            opt_flags=0, reserved=(0, 0, 0, 0, 0), temporal=None, denoise=None):
    lib = abi.load_rtmi()
    p = abi.RenderParams()
    p.nx, p.ny, p.ns, p.max_depth, p.t_min, p.flags = nx, ny, 0, 50, 0.001, flags  # ns is not read
    p.tile_rank, p.tile_world = tile_rank, tile_world
    t = dict(T_DEFAULT, **(temporal or {}))
    d = dict(D_DEFAULT, **(denoise or {}))
    o = abi.FrameOpts(estimator, env_select_p,
                      abi.TemporalParams(t["max_history"], t["alpha_min"], t["depth_tol"], t["normal_min"], t["albedo_min"],
                                         t["flags"], (C.c_uint32 * 2)(*t["reserved"])),
                      abi.DenoiseParams(d["iterations"], d["normal_power"], d["sigma_l"], d["sigma_z"], d["eps_l"], d["eps_z"],
                                        d["albedo_min"], d["flags"]),
                      opt_flags, (C.c_uint32 * 5)(*reserved))
    h = C.c_void_p(0x1234)  # a failure must clear it
    rc = lib.rtmi_frame_create(None, C.byref(p) if params else None, C.byref(o) if opts else None, C.byref(h) if out else None)
    assert rc != 0  # the scene is NULL
    if out:
        assert h.value is None
    return rc, (lib.rtmi_last_error() or b"").decode()


def _refused(code, word, **kw):
    rc, msg = _create(**kw)
    assert rc == code and msg.startswith("rtmi_frame_create: ") and word in msg, (kw, rc, msg)


def test_create_argument_refusals():
    nan, inf = float("nan"), float("inf")
    _refused(INVALID, "scene is NULL")  # every value valid: the refusals end at the scene
    for null in ("params", "opts", "out"):
        _refused(INVALID, "NULL argument", **{null: False})
    for nx, ny in ((0, 8), (8, 0), (32769, 8), (8, 32769), (2 ** 32 - 1, 1)):
        _refused(INVALID, "nx and ny", nx=nx, ny=ny)
    _refused(INVALID, "scene is NULL", nx=32768, ny=1)
    _refused(INVALID, "scene is NULL", nx=1, ny=32768)
    _refused(INVALID, "tile_rank/tile_world", tile_world=0)
    _refused(INVALID, "tile_rank/tile_world", tile_rank=2, tile_world=2)
    for e in (4, 5, 2 ** 32 - 1):
        _refused(INVALID, "estimator", estimator=e)
    for e in (0, 1, 2, 3):  # every estimator's attach checks come after the scene
        _refused(INVALID, "scene is NULL", estimator=e)
    for v in (0.0, -0.5, 1.000001, nan, inf):
        _refused(INVALID, "env_select_p", env_select_p=v)
    for v in (1e-6, 1.0):
        _refused(INVALID, "scene is NULL", env_select_p=v)
    _refused(INVALID, "RTMI_FLAG_SKY", estimator=2, flags=FC | abi.RTMI_FLAG_SKY)
    _refused(INVALID, "RTMI_FLAG_SKY", estimator=3, flags=abi.RTMI_FLAG_SKY)
    _refused(INVALID, "scene is NULL", estimator=1, flags=abi.RTMI_FLAG_SKY)
    for k in range(5):
        _refused(INVALID, "reserved", reserved=tuple(7 if j == k else 0 for j in range(5)))


def test_create_embedded_parameter_refusals():
    nan, inf = float("nan"), float("inf")
    # the ranges of rtmi_temporal.h: each end is accepted, what lies beyond is refused
    for ok in (dict(max_history=1), dict(max_history=65535), dict(alpha_min=1.0), dict(depth_tol=0.0), dict(depth_tol=3e38),
               dict(normal_min=-1.0), dict(normal_min=1.0), dict(albedo_min=1e-45), dict(flags=abi.RTMI_TEMPORAL_NO_DEMODULATE)):
        _refused(INVALID, "scene is NULL", temporal=ok)
    for field, values in (("max_history", (0, 65536, 2 ** 32 - 1)), ("alpha_min", (-1e-6, 1.000001, nan, inf)),
                          ("depth_tol", (-1e-6, nan, inf)), ("normal_min", (-1.000001, 1.000001, nan, -inf)),
                          ("albedo_min", (0.0, -1.0, nan, inf))):
        for v in values:
            _refused(INVALID, field, temporal={field: v})
    _refused(INVALID, "reserved", temporal=dict(reserved=(0, 1)))
    _refused(INVALID, "reserved", temporal=dict(reserved=(7, 0)))
    # the ranges of rtmi_denoise.h
    for ok in (dict(iterations=0), dict(iterations=10), dict(normal_power=0), dict(normal_power=1), dict(normal_power=1024),
               dict(sigma_l=0.0), dict(sigma_z=0.0), dict(eps_l=1e-45), dict(albedo_min=3e38)):
        _refused(INVALID, "scene is NULL", denoise=ok)
    for v in (11, 2 ** 32 - 1):
        _refused(INVALID, "iterations", denoise=dict(iterations=v))
    for v in (3, 96, 2048, 2 ** 31):
        _refused(INVALID, "normal_power", denoise=dict(normal_power=v))
    for field in ("sigma_l", "sigma_z"):
        for v in (-1e-6, nan, inf):
            _refused(INVALID, "sigma_l and sigma_z", denoise={field: v})
    for field in ("eps_l", "eps_z", "albedo_min"):
        for v in (0.0, -1.0, nan, inf):
            _refused(INVALID, "eps_l, eps_z and albedo_min", denoise={field: v})


def test_create_flag_refusals():
    for bit in ACCEPTED:
        _refused(INVALID, "scene is NULL", flags=bit)
    _refused(INVALID, "scene is NULL", flags=sum(ACCEPTED))
    for bit in REFUSED:
        _refused(UNSUPPORTED, "frames accept the flags", flags=FC | bit)
        _refused(UNSUPPORTED, "frames accept the flags", flags=FC | bit, estimator=1)
    # LIGHT_COOP goes to the lit render: refused with the plain estimator, whose render is cooperative by default
    _refused(UNSUPPORTED, "frames accept the flags", flags=FC | abi.RTMI_FLAG_LIGHT_COOP)
    for e in (1, 2, 3):
        _refused(INVALID, "scene is NULL", flags=FC | abi.RTMI_FLAG_LIGHT_COOP, estimator=e)
    for bit in (2, 4, 1 << 16, 1 << 31, 3):
        _refused(UNSUPPORTED, "temporal.flags", temporal=dict(flags=bit))
    for bit in (1, 2, 1 << 31):
        _refused(UNSUPPORTED, "denoise.flags", denoise=dict(flags=bit))
    for bit in (4, 8, 1 << 31, 7):
        _refused(UNSUPPORTED, "flags bit of opts", opt_flags=bit)
    for ok in (abi.RTMI_FRAME_NO_TEMPORAL, abi.RTMI_FRAME_NO_FILTER, abi.RTMI_FRAME_NO_TEMPORAL | abi.RTMI_FRAME_NO_FILTER):
        _refused(INVALID, "scene is NULL", opt_flags=ok)  # both together: the noisy image and its quantisation
    _refused(UNSUPPORTED, "tile_world must be 1", tile_world=2)
    _refused(UNSUPPORTED, "tile_world must be 1", tile_rank=1, tile_world=3)


def test_create_checks_in_the_documented_order():
    bad_t, bad_d = dict(max_history=0), dict(iterations=11)
    _refused(INVALID, "NULL argument", params=False, opts=False)
    _refused(INVALID, "nx and ny", nx=0, tile_world=0, estimator=9)
    _refused(INVALID, "tile_rank/tile_world", tile_world=0, estimator=9)
    _refused(INVALID, "estimator", estimator=9, env_select_p=2.0, temporal=bad_t)
    _refused(INVALID, "env_select_p", env_select_p=2.0, temporal=bad_t, denoise=bad_d)
    _refused(INVALID, "max_history", temporal=bad_t, denoise=bad_d, reserved=(1, 0, 0, 0, 0))
    _refused(INVALID, "iterations", denoise=bad_d, reserved=(1, 0, 0, 0, 0))
    _refused(INVALID, "reserved", reserved=(1, 0, 0, 0, 0), estimator=2, flags=abi.RTMI_FLAG_SKY)
    # every argument error before every flag
    _refused(INVALID, "RTMI_FLAG_SKY", estimator=2, flags=abi.RTMI_FLAG_SKY | abi.RTMI_FLAG_PATH_SIG)
    _refused(INVALID, "iterations", denoise=bad_d, flags=abi.RTMI_FLAG_PATH_SIG, tile_world=2)
    _refused(INVALID, "max_history", temporal=dict(max_history=0, flags=2), opt_flags=64)
    # the flags: params, temporal, denoise, opts, tile_world
    _refused(UNSUPPORTED, "frames accept the flags", flags=abi.RTMI_FLAG_PATH_SIG, temporal=dict(flags=2), tile_world=2)
    _refused(UNSUPPORTED, "temporal.flags", temporal=dict(flags=2), denoise=dict(flags=1))
    _refused(UNSUPPORTED, "denoise.flags", denoise=dict(flags=1), opt_flags=64)
    _refused(UNSUPPORTED, "flags bit of opts", opt_flags=64, tile_world=2)
    # ... and all of it before the scene
    _refused(UNSUPPORTED, "tile_world must be 1", tile_world=2)


def _render(entry="rtmi_frame_render", handle=None, cam=True, out=True, ns=4, **cam_fields):
    lib = abi.load_rtmi()
    c = temporal_ref.pinhole((278.0, 278.0, -800.0), (278.0, 278.0, 0.0))
    for k, v in cam_fields.items():
        setattr(c, k, (C.c_float * 3)(*v) if isinstance(v, tuple) else v)
    lin = np.zeros((4, 4, 3), np.float32)
    o = abi.FrameOut()
    o.linear = lin.ctypes.data
    st = abi.Stats()
    rc = getattr(lib, entry)(handle, C.byref(c) if cam else None, ns, 7, C.byref(o) if out else None, C.byref(st))
    assert not lin.any()
    return rc, (lib.rtmi_last_error() or b"").decode()


@pytest.mark.parametrize("entry", ["rtmi_frame_render", "rtmi_frame_render_device"])
def test_render_refusals_before_any_device_work(entry):
    def refused(code, word, **kw):
        rc, msg = _render(entry, **kw)
        assert rc == code and msg.startswith(entry + ": ") and word in msg, (kw, rc, msg)

    nan, inf = float("nan"), float("inf")
    refused(INVALID, "NULL handle")  # every other argument valid: the NULL handle (what destroy leaves a caller with)
    refused(INVALID, "NULL handle", ns=2)
    refused(INVALID, "NULL handle", ns=2 ** 26 - 1)
    refused(INVALID, "NULL argument", cam=False)
    refused(INVALID, "NULL argument", out=False)
    for ns in (0, 1):
        refused(INVALID, "ns must be at least 2", ns=ns)
    refused(UNSUPPORTED, "ns must be below 2^26", ns=2 ** 26)
    refused(INVALID, "singular", horizontal=(0.0, 2.0, 0.0), vertical=(0.0, 5.0, 0.0))
    refused(INVALID, "singular", horizontal=(0.0, 0.0, 0.0))
    for field in ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v"):
        refused(INVALID, "non-finite", **{field: (1.0, nan, 0.0)})
        refused(INVALID, "non-finite", **{field: (-inf, 0.0, 1.0)})
    for field in ("time0", "time1", "lens_radius"):
        refused(INVALID, "non-finite", **{field: nan})
    # the order: pointers, ns, the camera, the cap of ns, the handle
    refused(INVALID, "NULL argument", cam=False, ns=0)
    refused(INVALID, "ns must be at least 2", ns=1, horizontal=(0.0, 0.0, 0.0))
    refused(INVALID, "non-finite", horizontal=(nan, 0.0, 0.0), vertical=(nan, 0.0, 0.0))  # before the determinant
    refused(INVALID, "singular", ns=2 ** 26, horizontal=(0.0, 0.0, 0.0))


def test_reset_destroy_and_probe_refusals():
    lib = abi.load_rtmi()
    assert lib.rtmi_frame_reset(None) == INVALID and lib.rtmi_last_error().startswith(b"rtmi_frame_reset: ")
    lib.rtmi_frame_destroy(None)  # allowed
    tex = np.zeros((64, 4), np.uint32)
    lin = np.zeros((8, 8, 3), np.float32)

    def probe(nx=8, ny=8, tiled=True, se=False, out_se=False, device=-1):
        n = C.c_uint32(99)
        rc = lib.rtmi_probe_frame_untile(device, nx, ny, tex.ctypes.data if tiled else None, lin.ctypes.data if se else None,
                                         lin.ctypes.data, lin.ctypes.data if out_se else None, C.byref(n))
        assert rc != 0 and n.value == 99 and not lin.any()  # the device index -1 is never valid
        msg = lib.rtmi_last_error().decode()
        assert msg.startswith("rtmi_probe_frame_untile: "), msg
        return rc, msg

    assert probe()[0] == 3 and "device" in probe()[1]
    for nx, ny in ((0, 8), (8, 0), (32769, 8), (8, 32769)):
        rc, msg = probe(nx=nx, ny=ny)
        assert rc == INVALID and "nx and ny" in msg
    assert probe(tiled=False) == (INVALID, "rtmi_probe_frame_untile: NULL argument")
    rc, msg = probe(out_se=True)
    assert rc == INVALID and "out_stderr needs tiled_stderr" in msg
    assert probe(se=True, out_se=True)[0] == 3
    assert probe(nx=0, tiled=False)[1].endswith("nx and ny must be in [1, 32768]")  # the sizes before the pointers
