"""Guided upscaling's public interface (include/rtmi_upscale.h), without a GPU.

* the header compiles as C99 and its five structs have the size and offsets the host reads them with, in the header's
  comments, in ctypes and in sys.rs;
* librtmi.so exports the seven entries and nothing else with the family's word, abi.py and sys.rs declare them, the package
  exports Upscaler and upscale, and no other family's list holds one of them;
* every bad argument that needs no device is refused, with its code and the entry's name, in the documented order.  The
  stateless entries are called with the device index -1, so a valid set of arguments ends at the device check on every
  machine; create is called with a NULL scene and the renders with a NULL handle, which are checked last (the refusals that
  need a live handle: tests/test_gpu_upscale.py)."""
import ctypes as C
import inspect
import math
import re

import numpy as np
import pytest

import temporal_ref
import upscale_ref as ref
import abi_kit as kit
from raytracing_rust_amd import Host, Scene, Upscaler, abi, upscale

ENTRIES = ["rtmi_upscale", "rtmi_upscale_device", "rtmi_upscaler_create", "rtmi_upscaler_destroy", "rtmi_upscaler_render",
           "rtmi_upscaler_render_device", "rtmi_upscaler_reset"]
# struct: (C name, ctypes class, Rust name, size, offsets)
STRUCTS = (
    ("rtmi_upscale_params", abi.UpscaleParams, "RtmiUpscaleParams", 32,
     {"normal_power": 0, "sigma_z": 4, "eps_z": 8, "albedo_min": 12, "w_min": 16, "flags": 20, "reserved": 24}),
    ("rtmi_upscale_in", abi.UpscaleIn, "RtmiUpscaleIn", 64,
     {"linear_lo": 0, "albedo_lo": 8, "normal_lo": 16, "depth_lo": 24, "albedo": 32, "normal": 40, "depth": 48, "reserved": 56}),
    ("rtmi_upscale_out", abi.UpscaleOut, "RtmiUpscaleOut", 32, {"linear": 0, "rgb8": 8, "cls": 16, "reserved": 24}),
    ("rtmi_upscaler_opts", abi.UpscalerOpts, "RtmiUpscalerOpts", 160,
     {"low": 0, "up": 96, "lx": 128, "ly": 132, "guide_ns": 136, "reserved": 140}),
    ("rtmi_upscaler_out", abi.UpscalerOut, "RtmiUpscalerOut", 144,
     {"linear": 0, "rgb8": 8, "cls": 16, "albedo": 24, "normal": 32, "depth": 40, "low": 48}),
)
DEFAULT = dict(normal_power=32, sigma_z=0.05, eps_z=1e-3, albedo_min=1e-3, w_min=1e-3, flags=0, reserved=(0, 0))
INVALID, UNSUPPORTED, DEVICE = 1, 2, 3
FC = abi.RTMI_FLAG_FAST_CULL
nan, inf = math.nan, math.inf


FAMILY = kit.Family("rtmi_upscale.h", ENTRIES, {c: (ct, rust, size, offsets) for c, ct, rust, size, offsets in STRUCTS}, word="upscale",
                    includes=["rtmi.h", "rtmi_math.h", "rtmi_denoise.h", "rtmi_frame.h"], documented=True,
                    host=("rth_upscaler_create", "rth_upscaler_close", "rth_upscaler_render", "rth_upscaler_reset"))


# ---- layout -----------------------------------------------------------------------------------------------------------------
def test_header_is_c99_with_the_documented_layout(tmp_path):
    FAMILY.c99(tmp_path, holds="RTMI_UPSCALE_BACKGROUND == 0u && RTMI_UPSCALE_GUIDED == 1u && RTMI_UPSCALE_NEAREST == 2u && "
               "RTMI_UPSCALE_MISMATCH == 3u && rtmi_expf(0.0f) == 1.0f")


def test_ctypes_and_rust_match_the_header():
    FAMILY.layout()
    kit.assert_plain_repr_c(*[rust for _, _, rust, _, _ in STRUCTS])
    in_abi, in_rust = FAMILY.constants()
    for k, name in enumerate(("BACKGROUND", "GUIDED", "NEAREST", "MISMATCH")):
        assert getattr(abi, "RTMI_UPSCALE_" + name) == k == getattr(ref, name)
        assert "RTMI_UPSCALE_" + name in in_abi and "RTMI_UPSCALE_" + name in in_rust
        kit.assert_rust_const("RTMI_UPSCALE_" + name, "u8", k)


def test_the_defaults_agree():
    text = kit.header_text("rtmi_upscale.h", comments=True)
    sig = inspect.signature(upscale)
    assert sig.parameters["device"].default == 0 and "params" in sig.parameters
    from raytracing_rust_amd import host as H
    kw = {k: v.default for k, v in inspect.signature(H._upscale_params).parameters.items()}
    assert kw == ref.DEFAULTS == {k: DEFAULT[k] for k in ref.DEFAULTS}
    rk = {k: v.default for k, v in inspect.signature(ref.upscale).parameters.items() if k in ref.DEFAULTS}
    assert rk == ref.DEFAULTS
    p = H._upscale_params()
    assert p.flags == 0 and tuple(p.reserved) == (0, 0)
    for field, value in (("normal_power", "32"), ("sigma_z", "0.05"), ("eps_z", "1e-3"), ("albedo_min", "1e-3"), ("w_min", "1e-3"),
                         ("guide_ns", "4")):
        assert re.search(r"\b%s;\s*/\*[^*]*default %s \*/" % (field, value), text), field
    s = inspect.signature(Scene.upscaler)
    assert s.parameters["guide_ns"].default == 4 and s.parameters["scale"].default == 2.0 and s.parameters["low"].default is None
    assert "not been tuned" in text


def test_exports_and_declarations_agree():
    FAMILY.exports()
    assert len(abi.RTMI_UPSCALE_SYMBOLS) == 7
    assert Upscaler.__doc__ and Upscaler.render.__doc__ and upscale.__doc__ and Scene.upscaler.__doc__
    assert all(hasattr(Upscaler, n) for n in ("__enter__", "__exit__", "reset", "close"))
    assert "_upscalers" in Host.free_all.__code__.co_consts or "_upscalers" in Host.free_all.__code__.co_names


def test_nothing_was_added_to_the_other_headers():
    FAMILY.isolation()


# ---- the stateless entries' refusals ------------------------------------------------------------------------------------------
def _call(entry="rtmi_upscale", lx=4, ly=4, nx=8, ny=8, params=True, inp=True, out=True, null_plane=None, outputs=("linear", "rgb8", "cls"),
          in_reserved=False, out_reserved=False, shift=None, device=-1, **fields):
    """A call with 16-byte aligned host buffers standing in for every pointer: the device index -1 is refused before
    anything is dereferenced.  shift = (name, bytes): that pointer moved off its alignment."""
    lib = abi.load_rtmi()
    f = dict(DEFAULT, **fields)
    p = abi.UpscaleParams(f["normal_power"], f["sigma_z"], f["eps_z"], f["albedo_min"], f["w_min"], f["flags"],
                          (C.c_uint32 * 2)(*f["reserved"]))
    names = [n for n, _ in abi.UpscaleIn._fields_[:7]] + ["linear", "rgb8", "cls"]
    buf = {n: np.zeros(64, np.float32) for n in names}
    ptr = {}
    for n, a in buf.items():
        ptr[n] = a.ctypes.data + (-a.ctypes.data) % 16 + (shift[1] if shift and shift[0] == n else 0)
    i = abi.UpscaleIn(*[None if n == null_plane else ptr[n] for n in names[:7]], 0x10 if in_reserved else None)
    o = abi.UpscaleOut(*[ptr[n] if n in outputs else None for n in ("linear", "rgb8", "cls")], 0x10 if out_reserved else None)
    args = [device, lx, ly, nx, ny, C.byref(p) if params else None, C.byref(i) if inp else None, C.byref(o) if out else None]
    rc = getattr(lib, entry)(*(args + ([None] if entry.endswith("_device") else [])))
    assert rc != 0 and all(not a.any() for a in buf.values())
    return rc, (lib.rtmi_last_error() or b"").decode()


ACCEPTED = [dict(normal_power=0), dict(normal_power=1), dict(normal_power=1024), dict(sigma_z=0.0), dict(sigma_z=3e38),
            dict(eps_z=1e-45), dict(eps_z=3e38), dict(albedo_min=1e-45), dict(albedo_min=3e38), dict(w_min=0.0), dict(w_min=3e38)]
REFUSED = [("normal_power", (3, 96, 2048, 2 ** 31, 2 ** 32 - 1)), ("sigma_z", (-1e-6, nan, inf, -inf)), ("eps_z", (0.0, -1.0, nan, inf)),
           ("albedo_min", (0.0, -1.0, nan, inf)), ("w_min", (-1e-6, nan, inf, -inf))]


@pytest.mark.parametrize("entry", ["rtmi_upscale", "rtmi_upscale_device"])
def test_stateless_refusals_before_any_device_work(entry):
    def refused(code, word, **kw):
        rc, msg = _call(entry, **kw)
        assert rc == code and msg.startswith(entry + ": ") and word in msg, (kw, rc, msg)

    refused(DEVICE, "device")  # every value valid: the device index is refused
    for null in ("params", "inp", "out"):
        refused(INVALID, "NULL argument", **{null: False})
    for plane in [n for n, _ in abi.UpscaleIn._fields_[:7]]:
        refused(INVALID, "NULL input plane", null_plane=plane)
    for kw in (dict(lx=0), dict(ly=0), dict(nx=0, lx=0), dict(lx=9), dict(ly=9), dict(nx=32769, lx=32769), dict(ny=32769),
               dict(lx=2 ** 32 - 1, nx=2 ** 32 - 1), dict(lx=32769, nx=32768)):
        refused(INVALID, "sizes", **kw)
    for kw in (dict(lx=1, ly=1, nx=32768, ny=32768), dict(lx=32768, nx=32768), dict(ly=32768, ny=32768), dict(lx=8, ly=8),
               dict(lx=1, ly=1, nx=1, ny=1)):
        refused(DEVICE, "device", **kw)
    for ok in ACCEPTED:
        refused(DEVICE, "device", **ok)
    for field, values in REFUSED:
        for v in values:
            refused(INVALID, field, **{field: v})
    for r in ((1, 0), (0, 7), (2 ** 32 - 1, 0)):
        refused(INVALID, "reserved", reserved=r)
    refused(INVALID, "reserved pointer", in_reserved=True)
    refused(INVALID, "reserved pointer", out_reserved=True)
    refused(INVALID, "every output", outputs=())
    for only in ("linear", "rgb8", "cls"):  # each output alone is enough
        refused(DEVICE, "device", outputs=(only,))
    for bit in (1, 2, 1 << 16, 1 << 31, 3):
        refused(UNSUPPORTED, "flags", flags=bit)
    # the order: pointers, sizes, the fields in the struct's order, the reserved words, the outputs, (the alignment,) the
    # flags, the device
    refused(INVALID, "NULL argument", params=False, lx=0)
    refused(INVALID, "NULL input plane", null_plane="depth", lx=0)
    refused(INVALID, "sizes", lx=0, normal_power=3)
    refused(INVALID, "normal_power", normal_power=3, sigma_z=nan)
    refused(INVALID, "sigma_z", sigma_z=nan, eps_z=0.0)
    refused(INVALID, "eps_z", eps_z=0.0, albedo_min=0.0)
    refused(INVALID, "albedo_min", albedo_min=0.0, w_min=-1.0)
    refused(INVALID, "w_min", w_min=-1.0, reserved=(1, 0))
    refused(INVALID, "reserved", reserved=(1, 0), outputs=())
    refused(INVALID, "every output", outputs=(), flags=1)
    refused(UNSUPPORTED, "flags", flags=2, device=10 ** 6)
    if entry.endswith("_device"):
        for which, by in (("linear_lo", 4), ("albedo_lo", 8), ("normal_lo", 12), ("depth_lo", 4), ("albedo", 4), ("normal", 8),
                          ("depth", 4), ("linear", 4), ("rgb8", 1), ("rgb8", 2), ("cls", 1), ("cls", 2)):
            refused(INVALID, "misaligned", shift=(which, by))
        refused(DEVICE, "device", shift=("rgb8", 4))  # rgb8 and cls need 4 bytes only
        refused(DEVICE, "device", shift=("cls", 12))
        refused(INVALID, "every output", outputs=(), shift=("depth", 4))
        refused(INVALID, "misaligned", shift=("depth", 4), flags=1)
    else:
        refused(DEVICE, "device", shift=("depth", 4))  # the host form takes any alignment
        refused(DEVICE, "device", shift=("rgb8", 1))


# ---- the handle's refusals ----------------------------------------------------------------------------------------------------
def _create(params=True, opts=True, out=True, nx=8, ny=8, lx=4, ly=4, guide_ns=4, render_flags=FC, estimator=0, opt_reserved=(0, 0, 0, 0, 0),
            low_flags=0, denoise_iterations=5, **fields):
    lib = abi.load_rtmi()
    p = abi.RenderParams()
    p.nx, p.ny, p.ns, p.max_depth, p.t_min, p.flags = nx, ny, 0, 50, 0.001, render_flags  # ns is not read
    p.tile_rank, p.tile_world = 0, 1
    f = dict(DEFAULT, **fields)
    fo = abi.FrameOpts(estimator, 0.5, abi.TemporalParams(32, 0.0, 0.05, 0.9, 1e-3, 0),
                       abi.DenoiseParams(denoise_iterations, 128, 4.0, 1.0, 1e-10, 1e-3, 1e-3, 0), low_flags)
    o = abi.UpscalerOpts(fo, abi.UpscaleParams(f["normal_power"], f["sigma_z"], f["eps_z"], f["albedo_min"], f["w_min"], f["flags"],
                                               (C.c_uint32 * 2)(*f["reserved"])), lx, ly, guide_ns, (C.c_uint32 * 5)(*opt_reserved))
    h = C.c_void_p(0x1234)  # a failure must clear it
    rc = lib.rtmi_upscaler_create(None, C.byref(p) if params else None, C.byref(o) if opts else None, C.byref(h) if out else None)
    assert rc != 0  # the scene is NULL
    if out:
        assert h.value is None
    return rc, (lib.rtmi_last_error() or b"").decode()


def test_create_refusals_before_any_device_work():
    def refused(code, word, **kw):
        rc, msg = _create(**kw)
        assert rc == code and msg.startswith("rtmi_upscaler_create: ") and word in msg and "rtmi_frame" not in msg, (kw, rc, msg)

    refused(INVALID, "scene is NULL")  # every value valid: the refusals end at the scene
    for null in ("params", "opts", "out"):
        refused(INVALID, "NULL argument", **{null: False})
    for kw in (dict(lx=0), dict(ly=0), dict(lx=9), dict(ly=9), dict(nx=32769, lx=32769), dict(ny=32769), dict(nx=0, lx=0)):
        refused(INVALID, "sizes", **kw)
    for kw in (dict(lx=8, ly=8), dict(lx=1, ly=1), dict(nx=32768, ny=32768, lx=32768, ly=32768)):
        refused(INVALID, "scene is NULL", **kw)
    for ok in ACCEPTED:
        refused(INVALID, "scene is NULL", **ok)
    for field, values in REFUSED:
        for v in values:
            refused(INVALID, field, **{field: v})
    refused(INVALID, "reserved", reserved=(0, 1))
    refused(INVALID, "guide_ns", guide_ns=0)
    refused(INVALID, "scene is NULL", guide_ns=1)
    refused(INVALID, "scene is NULL", guide_ns=2 ** 26 - 1)
    for k in range(5):
        refused(INVALID, "reserved", opt_reserved=tuple(7 if j == k else 0 for j in range(5)))
    for bit in (1, 2, 1 << 31):
        refused(UNSUPPORTED, "up.flags", flags=bit)
    refused(UNSUPPORTED, "guide_ns", guide_ns=2 ** 26)
    # the low frame's own refusals come back in this entry's name, after the upscaler's own
    refused(INVALID, "estimator", estimator=9)
    refused(INVALID, "iterations", denoise_iterations=11)
    refused(UNSUPPORTED, "frames accept the flags", render_flags=FC | abi.RTMI_FLAG_PATH_SIG)
    refused(UNSUPPORTED, "flags bit of opts", low_flags=64)
    # the order: pointers, sizes, the parameters, guide_ns, the reserved words, the flags, the low frame, the scene
    refused(INVALID, "NULL argument", params=False, opts=False)
    refused(INVALID, "sizes", lx=0, normal_power=3)
    refused(INVALID, "normal_power", normal_power=3, guide_ns=0)
    refused(INVALID, "guide_ns", guide_ns=0, opt_reserved=(1, 0, 0, 0, 0))
    refused(INVALID, "reserved", opt_reserved=(1, 0, 0, 0, 0), guide_ns=2 ** 26)
    refused(UNSUPPORTED, "up.flags", flags=1, guide_ns=2 ** 26)
    refused(UNSUPPORTED, "guide_ns", guide_ns=2 ** 26, estimator=9)
    refused(INVALID, "estimator", estimator=9, render_flags=FC | abi.RTMI_FLAG_PATH_SIG)


def _render(entry, handle=None, cam=True, out=True, ns=4, low_plane=None, **cam_fields):
    lib = abi.load_rtmi()
    c = temporal_ref.pinhole((278.0, 278.0, -800.0), (278.0, 278.0, 0.0))
    for k, v in cam_fields.items():
        setattr(c, k, (C.c_float * 3)(*v) if isinstance(v, tuple) else v)
    lin = np.zeros((4, 4, 3), np.float32)
    o = abi.UpscalerOut()
    o.linear = lin.ctypes.data
    if low_plane:
        setattr(o.low, low_plane, lin.ctypes.data)
    st = abi.Stats()
    rc = getattr(lib, entry)(handle, C.byref(c) if cam else None, ns, 7, C.byref(o) if out else None, C.byref(st))
    assert rc != 0 and not lin.any()
    return rc, (lib.rtmi_last_error() or b"").decode()


@pytest.mark.parametrize("entry", ["rtmi_upscaler_render", "rtmi_upscaler_render_device"])
def test_render_refusals_before_any_device_work(entry):
    def refused(code, word, **kw):
        rc, msg = _render(entry, **kw)
        assert rc == code and msg.startswith(entry + ": ") and word in msg and "rtmi_frame" not in msg, (kw, rc, msg)

    refused(INVALID, "NULL handle")  # every other argument valid: the NULL handle (what destroy leaves a caller with)
    refused(INVALID, "NULL handle", ns=2)
    refused(INVALID, "NULL argument", cam=False)
    refused(INVALID, "NULL argument", out=False)
    for ns in (0, 1):
        refused(INVALID, "ns must be at least 2", ns=ns)
    refused(UNSUPPORTED, "ns must be below 2^26", ns=2 ** 26)
    refused(INVALID, "singular", horizontal=(0.0, 0.0, 0.0))
    refused(INVALID, "non-finite", origin=(1.0, nan, 0.0))
    for plane in ("linear", "albedo", "normal", "depth"):  # the kept planes of the low frame: both forms copy them
        refused(INVALID, "NULL handle", low_plane=plane)
    for plane in ("rgb8", "noisy_linear", "noisy_stderr", "hits", "accum_linear", "accum_stderr", "history", "motion"):
        if entry.endswith("_device"):
            refused(INVALID, "NULL handle", low_plane=plane)
        else:
            refused(INVALID, "host form", low_plane=plane)
    # the order: pointers, (the host form's planes,) ns, the camera, the cap of ns, the handle
    refused(INVALID, "NULL argument", cam=False, ns=0)
    refused(INVALID, "ns must be at least 2", ns=1, horizontal=(0.0, 0.0, 0.0))
    refused(INVALID, "singular", ns=2 ** 26, horizontal=(0.0, 0.0, 0.0))
    if not entry.endswith("_device"):
        refused(INVALID, "host form", low_plane="hits", ns=0)


def test_reset_and_destroy_of_null():
    lib = abi.load_rtmi()
    assert lib.rtmi_upscaler_reset(None) == INVALID and lib.rtmi_last_error().startswith(b"rtmi_upscaler_reset: ")
    lib.rtmi_upscaler_destroy(None)  # allowed


def test_the_python_face_reports_the_refusal():
    z = np.zeros((4, 4), np.float32)
    c = np.zeros((4, 4, 3), np.float32)
    with pytest.raises(ValueError):
        upscale(c, c, c, z, c, c, z.reshape(16))  # depth must be two-dimensional
    with pytest.raises(ValueError):
        upscale(c, c, c, z, c, c[:, :3], z)  # a plane of another size
    with pytest.raises(ValueError):
        upscale(c, c, c, z, c.astype(np.float64), c, z)
    with pytest.raises(TypeError):
        upscale(c, c, c, z, c, c, z, gamma=2.2)  # not a parameter
    with pytest.raises(Exception) as e:
        upscale(c, c, c, z, c, c, z, normal_power=3)
    assert "normal_power" in str(e.value) and "rtmi_upscale:" in str(e.value)
    with pytest.raises(Exception) as e:
        upscale(np.zeros((8, 8, 3), np.float32), np.zeros((8, 8, 3), np.float32), np.zeros((8, 8, 3), np.float32),
                np.zeros((8, 8), np.float32), c, c, z)  # lx > nx
    assert "sizes" in str(e.value)
