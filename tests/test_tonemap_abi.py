"""The tone mapper's public interface (include/rtmi_tonemap.h), without a GPU.

* the header compiles as C99 and its two structs have the size and offsets the host reads them with, in the header's
  comments, in ctypes and in sys.rs;
* librtmi.so exports the six entries and nothing else with the family's word, abi.py and sys.rs declare them, the package
  exports Tonemap and tonemap, and no other family's list holds one of them;
* every bad argument that needs no device is refused, with its code and the entry's name, in the documented order.  create
  and the probe are called with the device index -1, so a valid set of arguments ends at the device check on every machine;
  the applies check their handle last, so a NULL handle shows every other refusal (the refusals that need a live handle:
  tests/test_gpu_tonemap.py)."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import abi_kit as kit
import tonemap_ref as ref
from raytracing_rust_amd import Frame, Host, Tonemap, abi, tonemap

ENTRIES = ["rtmi_probe_tonemap_histogram", "rtmi_tonemap_apply", "rtmi_tonemap_apply_device", "rtmi_tonemap_create",
           "rtmi_tonemap_destroy", "rtmi_tonemap_reset"]
PARAM_OFFSETS = {"op": 0, "oetf": 4, "exposure": 8, "flags": 12, "ev": 16, "white": 20, "key": 24, "log2_min": 28, "log2_max": 32,
                 "p_low": 36, "p_high": 40, "speed_up": 44, "speed_down": 48, "adapt_min": 52, "adapt_max": 56, "reserved": 60}
STATE_OFFSETS = {"exposure": 0, "adapted_log2": 4, "metered_log2": 8, "counted": 12, "kept": 16, "applies": 20, "reserved": 24}
DEFAULT = dict(op=2, oetf=1, exposure=1, flags=0, ev=0.0, white=math.inf, key=0.18, log2_min=-12.0, log2_max=12.0, p_low=0.10,
               p_high=0.95, speed_up=3.0, speed_down=1.0, adapt_min=-12.0, adapt_max=12.0, reserved=0)
INVALID, UNSUPPORTED, DEVICE = 1, 2, 3
FAMILY = kit.Family("rtmi_tonemap.h", ENTRIES, {"rtmi_tonemap_params": (abi.TonemapParams, "RtmiTonemapParams", 64, PARAM_OFFSETS),
                                                "rtmi_tonemap_state": (abi.TonemapState, "RtmiTonemapState", 32, STATE_OFFSETS)},
                    word="tonemap", includes=["rtmi.h", "rtmi_math.h", "rtmi_denoise.h"], documented=True)


# ---- layout -----------------------------------------------------------------------------------------------------------------
def test_header_is_c99_with_the_documented_layout(tmp_path):
    FAMILY.c99(tmp_path, run=True, holds="RTMI_TONEMAP_CLAMP == 0u && RTMI_TONEMAP_REINHARD == 1u && RTMI_TONEMAP_ACES == 2u && "
               "RTMI_TONEMAP_GAMMA2 == 0u && RTMI_TONEMAP_SRGB == 1u && RTMI_TONEMAP_MANUAL == 0u && RTMI_TONEMAP_AUTO == 1u "
               "&& rtmi_logf(1.0f) == 0.0f && rtmi_expf(0.0f) == 1.0f")


def test_ctypes_and_rust_match_the_header():
    FAMILY.layout()
    kit.assert_plain_repr_c("RtmiTonemapParams", "RtmiTonemapState")
    in_abi, in_rust = FAMILY.constants()
    assert in_abi == in_rust and len(in_abi) == 7
    for name, value in (("CLAMP", 0), ("REINHARD", 1), ("ACES", 2), ("GAMMA2", 0), ("SRGB", 1), ("MANUAL", 0), ("AUTO", 1)):
        assert getattr(abi, "RTMI_TONEMAP_" + name) == value and "RTMI_TONEMAP_" + name in in_abi
        kit.assert_rust_const("RTMI_TONEMAP_" + name, "u32", value)
    text = kit.header_text("rtmi_tonemap.h", comments=True)
    # the defaults of the header's comments, of Tonemap and of the restatement agree
    kw = dict(zip(Tonemap.__init__.__code__.co_varnames[1:], (None, None) + Tonemap.__init__.__defaults__))
    assert (kw["op"], kw["oetf"], kw["exposure"]) == ("aces", "srgb", "auto") == tuple(ref.DEFAULTS[k] for k in ("op", "oetf", "exposure"))
    assert kw["ev"] == 0.0 == ref.DEFAULTS["ev"] and kw["white"] == math.inf == ref.DEFAULTS["white"]
    assert kw["key"] == 0.18 == ref.DEFAULTS["key"] and kw["adapt_range"] is None
    assert tuple(kw["log2_range"]) == (-12, 12) == (ref.DEFAULTS["log2_min"], ref.DEFAULTS["log2_max"])
    assert tuple(kw["percentiles"]) == (0.10, 0.95) == (ref.DEFAULTS["p_low"], ref.DEFAULTS["p_high"])
    assert tuple(kw["speed"]) == (3.0, 1.0) == (ref.DEFAULTS["speed_up"], ref.DEFAULTS["speed_down"])
    for field, value in (("op", "_ACES"), ("oetf", "_SRGB"), ("exposure", "_AUTO"), ("ev", "0"), ("white", r"\+inf"),
                         ("key", "0.18"), ("log2_min", "-12"), ("log2_max", "12"), ("p_low", "0.10"), ("p_high", "0.95"),
                         ("speed_up", "3"), ("speed_down", "1"), ("adapt_min", "log2_min"), ("adapt_max", "log2_max")):
        assert re.search(r"\b%s;\s*/\*[^*]*default %s \*/" % (field, value), text), field


def test_exports_and_declarations_agree():
    FAMILY.exports()
    assert len(abi.RTMI_TONEMAP_SYMBOLS) == 6
    assert Tonemap.__doc__ and Tonemap.apply.__doc__ and tonemap.__doc__ and "tonemap" in Frame.render.__doc__
    assert hasattr(Tonemap, "__enter__") and hasattr(Tonemap, "__exit__") and hasattr(Tonemap, "reset") and hasattr(Tonemap, "close")


def test_nothing_was_added_to_the_other_headers():
    FAMILY.isolation()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _params(**fields):
    f = dict(DEFAULT)
    f.update(fields)
    return abi.TonemapParams(*[f[n] for n, _ in abi.TonemapParams._fields_])


def _create(nx=8, ny=8, params=True, out=True, device=-1, **fields):
    lib = abi.load_rtmi()
    p = _params(**fields)
    h = C.c_void_p(0x1234)  # a failure must clear it
    rc = lib.rtmi_tonemap_create(device, nx, ny, C.byref(p) if params else None, C.byref(h) if out else None)
    assert rc != 0  # the device index -1 is never valid
    if out:
        assert h.value is None
    return rc, (lib.rtmi_last_error() or b"").decode()


def _probe(nx=4, ny=4, params=True, linear=True, bins=True, device=-1, **fields):
    lib = abi.load_rtmi()
    p = _params(**fields)
    lin = np.ones((4, 4, 3), np.float32)
    out = np.full(256, 0xdeadbeef, np.uint32)
    rc = lib.rtmi_probe_tonemap_histogram(device, nx, ny, C.byref(p) if params else None, lin.ctypes.data if linear else None,
                                          out.ctypes.data if bins else None)
    assert rc != 0 and (out == 0xdeadbeef).all()
    return rc, (lib.rtmi_last_error() or b"").decode()


# each field's ends (accepted up to the device check) and what lies beyond them (refused)
nan, inf = math.nan, math.inf
ACCEPTED = [dict(op=0), dict(op=1), dict(op=2), dict(oetf=0), dict(oetf=1), dict(exposure=0), dict(exposure=1), dict(ev=-64.0),
            dict(ev=64.0), dict(white=1e-45), dict(white=3e38), dict(white=inf), dict(key=1e-45), dict(key=3e38),
            dict(log2_min=-3e38, adapt_min=0.0), dict(log2_max=3e38, adapt_max=0.0), dict(log2_min=11.0, adapt_min=0.0),
            dict(log2_min=0.0, log2_max=1.0, adapt_min=0.0, adapt_max=0.0), dict(p_low=0.0), dict(p_low=0.94999),
            dict(p_low=0.99999, p_high=1.0), dict(p_high=1.0), dict(p_high=0.10001), dict(speed_up=0.0), dict(speed_up=3e38),
            dict(speed_down=0.0), dict(speed_down=3e38), dict(adapt_min=-3e38), dict(adapt_min=12.0), dict(adapt_max=3e38),
            dict(adapt_max=-12.0), dict(adapt_min=5.0, adapt_max=5.0)]
REFUSED = [("op", (3, 2 ** 32 - 1)), ("oetf", (2, 2 ** 31)), ("exposure", (2, 255)), ("ev", (-64.001, 64.001, nan, inf, -inf)),
           ("white", (0.0, -1.0, nan, -inf)), ("key", (0.0, -0.18, nan, inf)), ("log2_min", (nan, inf, -inf)),
           ("log2_max", (nan, inf, -inf, -11.001, -12.0, -13.0)), ("p_low", (-1e-6, 1.0, 2.0, nan)),
           ("p_high", (0.10, 0.05, 1.000001, nan)), ("speed_up", (-1e-6, nan, inf)), ("speed_down", (-1e-6, nan, inf)),
           ("adapt_min", (nan, inf, -inf)), ("adapt_max", (nan, inf, -inf, -12.001))]


def test_create_refusals_before_any_device_work():
    def refused(code, word, **kw):
        rc, msg = _create(**kw)
        assert rc == code and msg.startswith("rtmi_tonemap_create:") and word in msg, (kw, rc, msg)

    refused(DEVICE, "device")  # every value valid: the device index is refused
    refused(INVALID, "NULL", params=False)
    refused(INVALID, "NULL", out=False)
    for nx, ny in ((0, 8), (8, 0), (32769, 8), (8, 32769), (2 ** 32 - 1, 1)):
        refused(INVALID, "nx and ny", nx=nx, ny=ny)
    refused(DEVICE, "device", nx=32768, ny=1)
    refused(DEVICE, "device", nx=1, ny=32768)
    for ok in ACCEPTED:
        refused(DEVICE, "device", **ok)
    for field, values in REFUSED:
        for v in values:
            refused(INVALID, field, **{field: v})
    for v in (1, 2 ** 31, 2 ** 32 - 1):
        refused(INVALID, "reserved", reserved=v)
    for bit in (1, 2, 1 << 16, 1 << 31, 3):
        refused(UNSUPPORTED, "flags", flags=bit)
    # fields the operator or the mode does not read are checked all the same
    refused(INVALID, "white", op=abi.RTMI_TONEMAP_ACES, white=-1.0)
    refused(INVALID, "key", exposure=abi.RTMI_TONEMAP_MANUAL, key=0.0)
    refused(INVALID, "p_high", exposure=abi.RTMI_TONEMAP_MANUAL, p_high=0.0)
    # the order: the size, the fields in the struct's order, the reserved word, the flags, the device
    refused(INVALID, "nx and ny", nx=0, op=9)
    refused(INVALID, "op", op=9, oetf=9)
    refused(INVALID, "ev", ev=nan, adapt_max=nan)
    refused(INVALID, "adapt_max", adapt_max=nan, reserved=1)
    refused(INVALID, "reserved", reserved=1, flags=1)
    refused(UNSUPPORTED, "flags", flags=2, device=10 ** 6)


def test_probe_refusals_before_any_device_work():
    def refused(code, word, **kw):
        rc, msg = _probe(**kw)
        assert rc == code and msg.startswith("rtmi_probe_tonemap_histogram:") and word in msg, (kw, rc, msg)

    refused(DEVICE, "device")
    for null in ("params", "linear", "bins"):
        refused(INVALID, "NULL", **{null: False})
    refused(INVALID, "nx and ny", nx=0)
    refused(INVALID, "log2_max", log2_max=-12.0)
    refused(INVALID, "reserved", reserved=1)
    refused(UNSUPPORTED, "flags", flags=4)
    refused(INVALID, "NULL", linear=False, flags=4)


def _apply(device_form, handle=None, linear=True, dt=0.0, rgb8=True, display=True, state=True, shift=None):
    """A call with 16-byte aligned host buffers standing in for every pointer: with a NULL handle nothing is dereferenced.
    shift = (name, bytes): that pointer moved off its alignment."""
    lib = abi.load_rtmi()
    buf = {n: np.zeros(64, np.float32) for n in ("linear", "rgb8", "display", "state")}
    ptr = {}
    for n, a in buf.items():
        base = a.ctypes.data + (-a.ctypes.data) % 16
        ptr[n] = base + (shift[1] if shift and shift[0] == n else 0)
    args = [handle, ptr["linear"] if linear else None, dt, ptr["rgb8"] if rgb8 else None, ptr["display"] if display else None]
    if device_form:
        rc = lib.rtmi_tonemap_apply_device(*args, ptr["state"] if state else None, None)
    else:
        rc = lib.rtmi_tonemap_apply(*args, C.cast(ptr["state"], C.POINTER(abi.TonemapState)) if state else None)
    assert all(not a.any() for a in buf.values())
    return rc, (lib.rtmi_last_error() or b"").decode()


@pytest.mark.parametrize("device_form", [False, True])
def test_apply_refusals_before_any_device_work(device_form):
    name = "rtmi_tonemap_apply_device:" if device_form else "rtmi_tonemap_apply:"

    def refused(word, **kw):
        rc, msg = _apply(device_form, **kw)
        assert rc == INVALID and msg.startswith(name) and word in msg, (kw, rc, msg)

    refused("handle")  # every other argument valid: the NULL handle (what destroy leaves a caller with) is refused
    for only in ("rgb8", "display", "state"):  # each output alone is enough
        refused("handle", **{n: n == only for n in ("rgb8", "display", "state")})
    for dt in (0.0, 1 / 60, 10.0, 3e38):
        refused("handle", dt=dt)
    refused("NULL linear", linear=False)
    for dt in (-1e-6, -1.0, nan, inf, -inf):
        refused("dt", dt=dt)
    refused("every output", rgb8=False, display=False, state=False)
    refused("NULL linear", linear=False, dt=nan)  # the order: linear, dt, the outputs, (the alignment,) the handle
    refused("dt", dt=nan, rgb8=False, display=False, state=False)
    if device_form:
        for which, by in (("linear", 4), ("linear", 8), ("display", 4), ("display", 12), ("rgb8", 1), ("rgb8", 2), ("state", 2)):
            refused("misaligned", shift=(which, by))
        refused("handle", shift=("rgb8", 4))  # rgb8 needs 4 bytes only
        refused("every output", rgb8=False, display=False, state=False, shift=("linear", 4))
    else:
        refused("handle", shift=("linear", 4))  # the host form takes any alignment


def test_reset_and_destroy_of_null():
    lib = abi.load_rtmi()
    assert lib.rtmi_tonemap_reset(None) == INVALID and b"rtmi_tonemap_reset" in lib.rtmi_last_error()
    lib.rtmi_tonemap_destroy(None)  # allowed


def test_the_python_face_reports_the_refusal():
    with pytest.raises(Exception) as e:
        Tonemap(8, 8, percentiles=(0.5, 0.5))
    assert "p_high" in str(e.value)
    for kw in (dict(op="filmic"), dict(oetf="rec709"), dict(exposure="spot")):
        with pytest.raises(ValueError):
            Tonemap(8, 8, **kw)
    with pytest.raises(ValueError):
        tonemap(np.zeros((4, 4), np.float32))
    assert Host.free_all.__code__.co_names.count("_tonemaps") == 1
