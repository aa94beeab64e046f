"""The temporal accumulation's public interface (include/rtmi_temporal.h), without a GPU.

* the header compiles as C99 and rtmi_temporal_params has the size and offsets the host reads it with, in the header, in
  ctypes and in sys.rs;
* librtmi.so exports the four entries, abi.py and sys.rs declare them, the package exports Temporal;
* every bad argument that needs no handle is refused before a device is touched, with its code and the entry's name.
  create is called with the device index -1, so a valid set of arguments ends at the device check on every machine; push
  checks its handle last, so a NULL handle shows every other refusal (the refusals that need a live handle:
  tests/test_gpu_temporal.py)."""
import ctypes as C
import re

import numpy as np
import pytest

import temporal_ref as ref
import abi_kit as kit
from raytracing_rust_amd import Temporal, abi

ENTRIES = ["rtmi_temporal_create", "rtmi_temporal_destroy", "rtmi_temporal_push", "rtmi_temporal_reset"]
OFFSETS = {"max_history": 0, "alpha_min": 4, "depth_tol": 8, "normal_min": 12, "albedo_min": 16, "flags": 20, "reserved": 24}
DEFAULT = dict(max_history=32, alpha_min=0.0, depth_tol=0.05, normal_min=0.9, albedo_min=1e-3, flags=0, reserved=(0, 0))


FAMILY = kit.Family("rtmi_temporal.h", ENTRIES, {"rtmi_temporal_params": (abi.TemporalParams, "RtmiTemporalParams", 32, OFFSETS)},
                    word="temporal", word_also_in={"rtmi_frame.h": "embeds rtmi_temporal_params in rtmi_frame_opts",
                                                   "rtmi_denoise.h": "says in a comment which filter input the accumulation feeds"})


def test_header_is_c99_with_the_documented_layout(tmp_path):
    FAMILY.c99(tmp_path, holds="RTMI_TEMPORAL_NO_DEMODULATE == 1u && sizeof(rtmi_camera) == 84")


def test_ctypes_and_rust_match_the_header():
    FAMILY.layout()
    kit.assert_plain_repr_c("RtmiTemporalParams")
    assert C.sizeof(abi.Camera) == 84
    assert FAMILY.constants() == (["RTMI_TEMPORAL_NO_DEMODULATE"], ["RTMI_TEMPORAL_NO_DEMODULATE"]) and abi.RTMI_TEMPORAL_NO_DEMODULATE == 1
    kit.assert_rust_const("RTMI_TEMPORAL_NO_DEMODULATE", "u32", 1)
    # the defaults of the header's comments, of Temporal and of the restatement agree
    text = kit.header_text("rtmi_temporal.h", comments=True)
    for field, value in (("max_history", "32"), ("alpha_min", "0"), ("depth_tol", "0.05"), ("normal_min", "0.9"),
                         ("albedo_min", "1e-3")):
        assert re.search(r"\b%s;\s*/\*[^*]*default %s \*/" % (field, re.escape(value)), text), field
        assert float(value) == ref.DEFAULTS[field] == Temporal.__init__.__defaults__[1 + list(ref.DEFAULTS).index(field)]


def test_exports_and_declarations_agree():
    FAMILY.exports()


def test_the_header_keeps_to_itself():
    FAMILY.isolation()


def _create(nx=8, ny=8, params=True, out=True, device=-1, **fields):
    lib = abi.load_rtmi()
    f = dict(DEFAULT)
    f.update(fields)
    p = abi.TemporalParams(f["max_history"], f["alpha_min"], f["depth_tol"], f["normal_min"], f["albedo_min"], f["flags"],
                           (C.c_uint32 * 2)(*f["reserved"]))
    h = C.c_void_p(0x1234)  # a failure must clear it
    rc = lib.rtmi_temporal_create(device, nx, ny, C.byref(p) if params else None, C.byref(h) if out else None)
    assert rc != 0  # the device index -1 is never valid
    if out:
        assert h.value is None
    return rc, (lib.rtmi_last_error() or b"").decode()


def test_create_refusals_before_any_device_work():
    def refused(code, word, **kw):
        rc, msg = _create(**kw)
        assert rc == code and msg.startswith("rtmi_temporal_create:") and word in msg, (kw, rc, msg)

    nan, inf = float("nan"), float("inf")
    refused(3, "device")  # every value valid: the device index is refused
    refused(1, "NULL", params=False)
    refused(1, "NULL", out=False)
    for nx, ny in ((0, 8), (8, 0), (32769, 8), (8, 32769), (2 ** 32 - 1, 1)):
        refused(1, "nx and ny", nx=nx, ny=ny)
    refused(3, "device", nx=32768, ny=1)
    refused(3, "device", nx=1, ny=32768)
    # each parameter at its range's ends, and beyond them
    for ok in (dict(max_history=1), dict(max_history=65535), dict(alpha_min=0.0), dict(alpha_min=1.0), dict(depth_tol=0.0),
               dict(depth_tol=3e38), dict(normal_min=-1.0), dict(normal_min=1.0), dict(albedo_min=1e-45),
               dict(albedo_min=3e38), dict(flags=abi.RTMI_TEMPORAL_NO_DEMODULATE)):
        refused(3, "device", **ok)
    for field, values in (("max_history", (0, 65536, 2 ** 32 - 1)), ("alpha_min", (-1e-6, 1.000001, nan, inf)),
                          ("depth_tol", (-1e-6, nan, inf)), ("normal_min", (-1.000001, 1.000001, nan, -inf)),
                          ("albedo_min", (0.0, -1.0, nan, inf))):
        for v in values:
            refused(1, field, **{field: v})
    refused(1, "reserved", reserved=(0, 1))
    refused(1, "reserved", reserved=(7, 0))
    for bit in (2, 4, 1 << 16, 1 << 31, 3):
        refused(2, "flags", flags=bit)
    refused(1, "max_history", flags=2, max_history=0)  # argument errors before the flags
    refused(2, "flags", flags=2, device=10 ** 6)  # the flags before the device


def _push(handle=None, cam=True, null=None, se=False, out_se=False, **cam_fields):
    lib = abi.load_rtmi()
    c = ref.pinhole((278.0, 278.0, -800.0), (278.0, 278.0, 0.0))
    for k, v in cam_fields.items():
        setattr(c, k, (C.c_float * 3)(*v) if isinstance(v, tuple) else v)
    planes = {n: np.zeros((4, 4, 3), np.float32) for n in ("linear", "albedo", "normal", "stderr", "out_linear", "out_stderr")}
    planes["depth"] = np.ones((4, 4), np.float32)
    ptr = {n: a.ctypes.data for n, a in planes.items()}
    if null:
        ptr[null] = None
    rc = lib.rtmi_temporal_push(handle, C.byref(c) if cam else None, ptr["linear"], ptr["albedo"], ptr["normal"], ptr["depth"],
                                ptr["stderr"] if se else None, ptr["out_linear"], ptr["out_stderr"] if out_se else None,
                                None, None)
    assert not planes["out_linear"].any() and not planes["out_stderr"].any()
    return rc, (lib.rtmi_last_error() or b"").decode()


def test_push_refusals_before_any_device_work():
    def refused(word, **kw):
        rc, msg = _push(**kw)
        assert rc == 1 and msg.startswith("rtmi_temporal_push:") and word in msg, (kw, rc, msg)

    refused("handle")  # every other argument valid: the NULL handle (what destroy leaves a caller with) is refused
    refused("handle", se=True, out_se=True)
    refused("NULL argument", cam=False)
    for name in ("linear", "albedo", "normal", "depth"):
        refused("NULL argument", null=name)
    # a singular camera: horizontal parallel to vertical, a zero axis, the corner in the plane of the two
    refused("singular", horizontal=(0.0, 2.0, 0.0), vertical=(0.0, 5.0, 0.0))
    refused("singular", horizontal=(0.0, 0.0, 0.0))
    refused("singular", lower_left_corner=(278.0, 278.0, -800.0))
    nan, inf = float("nan"), float("inf")
    for field in ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v"):
        refused("non-finite", **{field: (1.0, nan, 0.0)})
        refused("non-finite", **{field: (-inf, 0.0, 1.0)})
    for field in ("time0", "time1", "lens_radius"):
        refused("non-finite", **{field: nan})
    refused("non-finite", horizontal=(nan, 0.0, 0.0), vertical=(nan, 0.0, 0.0))  # before the determinant
    refused("out_stderr", out_se=True)
    refused("singular", out_se=True, horizontal=(0.0, 0.0, 0.0))  # the camera before the outputs


def test_reset_and_destroy_of_null():
    lib = abi.load_rtmi()
    assert lib.rtmi_temporal_reset(None) == 1 and b"rtmi_temporal_reset" in lib.rtmi_last_error()
    lib.rtmi_temporal_destroy(None)  # allowed


def test_the_python_face_reports_the_refusal():
    with pytest.raises(Exception) as e:
        Temporal(8, 8, max_history=0)
    assert "max_history" in str(e.value)
    assert Temporal.push.__doc__ and Temporal.__doc__
