"""The public interface of RTMI_FLAG_BATCH_COOP (include/rtmi_batch_coop.h): the batch modes on the wave-cooperative
kernel, without a GPU.

* the header compiles as C99 -pedantic next to rtmi.h; the flag is bit 21, apart from every flag and knob bit in use, and
  abi.py and sys.rs say the same (as FLAG_BATCH_COOP: tests/test_abi_signatures.py pins how many constants they restate
  under the headers' names); what the header declares is what abi.py, sys.rs and librtmi.so hold for it;
* each of the six entry pairs accepts the flag: with valid arguments and a NULL scene the call gets as far as the scene
  check (without the feature the flags check answers RTMI_ERR_UNSUPPORTED);
* the two test knobs, bit 11 and TEST_OVERFLOW, stay refused alone and pass the flags check beside the flag;
* every other bit beside the flag is still refused, bit 20 among them;
* the other entries answer the flag as they answer an unknown bit;
* coop=True of the Python methods ORs exactly bit 21 into the flags word."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_kit as kit
from raytracing_rust_amd import abi, host as host_mod
from raytracing_rust_amd.host import RAY_DTYPE, Scene, default_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtmi_batch_coop.h")
FLAG = 2097152
FC = abi.RTMI_FLAG_FAST_CULL
POOL_KNOB = 1 << 11
OVERFLOW = abi.RTMI_FLAG_TEST_OVERFLOW
INVALID, UNSUPPORTED = 1, 2  # RTMI_ERR_INVALID, RTMI_ERR_UNSUPPORTED (include/rtmi.h)
ENTRIES = ["rtmi_radiance", "rtmi_radiance_device", "rtmi_gather", "rtmi_gather_device", "rtmi_sparse_render",
           "rtmi_sparse_render_device", "rtmi_sparse_refine", "rtmi_sparse_refine_device", "rtmi_render_pixelwise",
           "rtmi_render_pixelwise_device", "rtmi_render_window", "rtmi_render_window_device"]
ESTIMATORS = [abi.RTMI_ROULETTE_PLAIN, abi.RTMI_ROULETTE_NEE]

# no entries and no word: the header is one flag of the batch entries
FAMILY = kit.Family("rtmi_batch_coop.h", [])


def _header_define(path, name):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    m = re.search(r"#define\s+%s\s+\(?\s*(0x[0-9a-fA-F]+|\d+)u?" % name, text)
    assert m, name
    return int(m.group(1), 0)


def test_header_is_c99(tmp_path):
    FAMILY.c99(tmp_path, before=("rtmi.h",), body="rtmi_render_params p; p.flags = RTMI_FLAG_FAST_CULL | RTMI_FLAG_BATCH_COOP;",
               holds="p.flags == 2097153u")
    FAMILY.c99(tmp_path, holds="RTMI_FLAG_BATCH_COOP == (1u << 21)")  # the header alone pulls in what it names
    FAMILY.layout()  # no struct
    FAMILY.isolation()


def test_exports_and_declarations_agree():
    FAMILY.exports()
    for m in (Scene.radiance, Scene.irradiance, Scene.gather, Scene.render_pixels, Scene.refine_pixels, Scene.render_pixelwise,
              Scene.render_windowed):
        assert "coop=True" in m.__doc__, m.__name__


def test_flag_value_and_disjointness():
    assert _header_define(HEADER, "RTMI_FLAG_BATCH_COOP") == FLAG == 1 << 21 == abi.FLAG_BATCH_COOP
    assert kit.header_constants("rtmi_batch_coop.h") == {"RTMI_FLAG_BATCH_COOP": FLAG}
    named = [getattr(abi, n) for n in dir(abi) if n.startswith("RTMI_FLAG_")]
    assert len(named) >= 14
    taken = 0
    for v in named:
        taken |= v
    # bits 8-11 are the knobs, bit 19 RTMI_KNOB_REPORT_INST, bit 20 the bit the batch entries' tests pin as unknown
    assert (taken | (0xf << 8) | (1 << 19) | (1 << 20)) & FLAG == 0
    assert "pub const FLAG_BATCH_COOP: u32 = %d;" % FLAG in kit.sys_block("rtmi_batch_coop.h")


def _aligned(words=64):
    a = np.zeros(words + 8, np.uint32)
    return a, a.ctypes.data + (-a.ctypes.data) % 16


def _call(entry, flags, estimator=abi.RTMI_ROULETTE_PLAIN):
    """The entry with valid arguments, a camera and a NULL scene -> (return code, message)."""
    lib = abi.load_rtmi()
    keep = [_aligned() for _ in range(6)]
    a, b, c_, d, e, f = (q for _, q in keep)
    p = default_params(8, 8, 16, flags=flags, seed=7)
    cam = abi.Camera()
    pc, cc = C.byref(p), C.byref(cam)
    sp = abi.SparseParams(1, 2, 0, estimator, 0.5)
    big = 2 ** 40
    if entry.startswith("rtmi_radiance"):
        rays = np.zeros(1, RAY_DTYPE)
        rays["d"] = (0.0, 0.0, 1.0)
        rays["t_max"] = np.inf
        rp = abi.RadianceParams(1, 2, estimator, flags, 50, 0.001, 7, 0, 0, 0, 0.5)
        if entry.endswith("_device"):
            rc = lib.rtmi_radiance_device(None, C.byref(rp), rays.ctypes.data, None, a, None, b, None)
        else:
            rc = lib.rtmi_radiance(None, C.byref(rp), rays.ctypes.data, None, a, None, None, None)
    elif entry.startswith("rtmi_gather"):
        gp = abi.GatherParams(1, 2, abi.GATHER_MODES["sphere"], estimator, flags, 50, 0.001, 7, 0, 0, 0, 0.5)
        if entry.endswith("_device"):
            rc = lib.rtmi_gather_device(None, C.byref(gp), a, None, None, b, None, None, c_, 24, None)
        else:
            rc = lib.rtmi_gather(None, C.byref(gp), a, None, None, b, None, None, None)
    elif entry == "rtmi_sparse_render":
        rc = lib.rtmi_sparse_render(None, pc, cc, C.byref(sp), a, b, None, None, None)
    elif entry == "rtmi_sparse_render_device":
        rc = lib.rtmi_sparse_render_device(None, pc, cc, C.byref(sp), a, None, b, None, c_, d, None)
    elif entry == "rtmi_sparse_refine":
        rc = lib.rtmi_sparse_refine(None, pc, cc, C.byref(sp), 8, 4, a, b, None, None, None)
    elif entry == "rtmi_sparse_refine_device":
        rc = lib.rtmi_sparse_refine_device(None, pc, cc, C.byref(sp), 8, 4, a, b, None, None, c_, big, None, None)
    else:
        window = "window" in entry
        o = abi.WindowOpts(4, 4, estimator, 0, 0.01, 0.0, 0.5, 2) if window else abi.PixelwiseOpts(4, 4, estimator, 0, 0.01, 0.0, 0.5)
        if entry.endswith("_device"):
            rc = getattr(lib, entry)(None, pc, cc, C.byref(o), a, None, b, c_, d, e, big, None)
        else:
            rc = getattr(lib, entry)(None, cc, pc, C.byref(o), a, None, b, c_, d, None)
    assert all(not k.any() for k, _ in keep)  # refused before anything is written
    return rc, (lib.rtmi_last_error() or b"").decode()


@pytest.mark.parametrize("entry", ENTRIES)
def test_batch_entries_accept_the_flag(entry):
    """The flags check passes, so the NULL scene is what is refused (without the feature: RTMI_ERR_UNSUPPORTED, "flags")."""
    for est in ESTIMATORS:
        for base in (FC, 0, FC | abi.RTMI_FLAG_SKY | abi.RTMI_FLAG_FACE_FORWARD | abi.RTMI_FLAG_UV_BOOK):
            rc, msg = _call(entry, FLAG | base, est)
            assert rc == INVALID and "scene is NULL" in msg and msg.startswith(entry + ": "), (entry, est, base, rc, msg)
    rc, msg = _call(entry, FC)  # and the same call without it, as before
    assert rc == INVALID and "scene is NULL" in msg, (entry, rc, msg)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("knob", [POOL_KNOB, OVERFLOW], ids=["pool_knob", "test_overflow"])
def test_knobs_stay_refused_alone_and_pass_beside_the_flag(entry, knob):
    rc, msg = _call(entry, knob | FC)
    assert rc == UNSUPPORTED and "flags" in msg, (rc, msg)
    rc, msg = _call(entry, knob | FLAG | FC)
    assert rc == INVALID and "scene is NULL" in msg, (rc, msg)
    rc, msg = _call(entry, POOL_KNOB | OVERFLOW | FLAG | FC)
    assert rc == INVALID and "scene is NULL" in msg, (rc, msg)


BESIDE = [abi.RTMI_FLAG_REF_TREE, abi.RTMI_FLAG_SYNC, abi.RTMI_FLAG_PATH_SIG, abi.RTMI_FLAG_PROFILE, abi.RTMI_FLAG_LIGHT_COOP, 1 << 20,
          abi.RTMI_FLAG_ROULETTE_COOP, abi.RTMI_FLAG_ASYNC, abi.RTMI_FLAG_BLOCK_COOP, 1 << 19, 3 << 8, 1 << 22]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("extra", BESIDE)
def test_other_bits_beside_the_flag_are_unsupported(entry, extra):
    rc, msg = _call(entry, FLAG | extra | FC)
    assert rc == UNSUPPORTED and "flags" in msg, (rc, msg)
    rc, msg = _call(entry, extra | FC)  # and alone, as before
    assert rc == UNSUPPORTED and "flags" in msg, (rc, msg)


def _other(entry, flags):
    lib = abi.load_rtmi()
    p = default_params(32, 24, 16, flags=flags)
    c = abi.Camera()
    pc, cc = C.byref(p), C.byref(c)
    if entry == "rtmi_render":
        rc = lib.rtmi_render(None, cc, pc, None, None, None, None)
    elif entry == "rtmi_render_nee":
        rc = lib.rtmi_render_nee(None, cc, pc, None, None, None, None, None)
    elif entry == "rtmi_render_features":
        rc = lib.rtmi_render_features(None, cc, pc, None, None, None, None, None, None)
    else:
        rays = np.zeros(1, RAY_DTYPE)
        rays["d"] = (0.0, 0.0, 1.0)
        hits = np.zeros(64, np.uint8)
        q = abi.QueryParams(1, flags, 0, 0)
        rc = lib.rtmi_trace(None, C.byref(q), rays.ctypes.data, None, hits.ctypes.data, None)
    return rc, (lib.rtmi_last_error() or b"").decode()


@pytest.mark.parametrize("entry", ["rtmi_render_nee", "rtmi_render_features", "rtmi_trace"])
def test_other_entries_refuse_the_flag(entry):
    rc, msg = _other(entry, FLAG | FC)
    assert rc == UNSUPPORTED, (entry, rc, msg)
    assert _other(entry, (1 << 20) | FC)[0] == UNSUPPORTED  # as they answer an unknown bit
    rc, msg = _other(entry, FC)  # the same call without it gets as far as the scene
    assert rc == INVALID and "scene" in msg, (entry, rc, msg)


def test_rtmi_render_answers_the_flag_as_an_unknown_bit():
    """rtmi_render names the handle first and reads no unknown bit of flags: the flag changes nothing of its answer."""
    assert _other("rtmi_render", FLAG | FC) == _other("rtmi_render", (1 << 20) | FC) == _other("rtmi_render", FC)
    assert _other("rtmi_render", FLAG | FC)[0] == INVALID


class _Stop(Exception):
    pass


def test_python_coop_ors_exactly_bit_21(monkeypatch):
    """On the params, with no native call: the constructors of the params are watched and the call stopped right there."""
    seen = []

    def spy_params(*a, **kw):
        seen.append(int(kw.get("flags", 0)))
        raise _Stop()

    def spy_struct(*a):
        seen.append(int(a[spy_struct.at]))
        raise _Stop()

    monkeypatch.setattr(host_mod, "default_params", spy_params)
    sc = object.__new__(Scene)
    sc.uploaded = True  # _ready() has nothing to do: no upload, no light table for the plain estimator
    sc.lights_attached = True
    pts = np.zeros((1, 3), np.float32)
    cls = {"cls": np.zeros((2, 2), np.uint8)}
    for base in (0, FC, FC | abi.RTMI_FLAG_SKY):
        for coop in (False, True):
            want = base | (FLAG if coop else 0)
            for call in (lambda: sc.render_pixels(None, 2, 2, [0], 2, flags=base, coop=coop),
                         lambda: sc.refine_pixels(None, cls, flags=base, coop=coop),
                         lambda: sc.render_pixelwise(None, 2, 2, 8, 4, 4, flags=base, coop=coop),
                         lambda: sc.render_windowed(None, 2, 2, 8, 4, 4, flags=base, coop=coop)):
                with pytest.raises(_Stop):
                    call()
                assert seen[-1] == want, (base, coop, seen[-1])
            spy_struct.at = 3
            monkeypatch.setattr(abi, "RadianceParams", spy_struct)
            for call in (lambda: sc.radiance(pts, pts, flags=base, coop=coop), lambda: sc.irradiance(pts, pts + 1.0, 2, flags=base, coop=coop)):
                with pytest.raises(_Stop):
                    call()
                assert seen[-1] == want, (base, coop, seen[-1])
            spy_struct.at = 4
            monkeypatch.setattr(abi, "GatherParams", spy_struct)
            with pytest.raises(_Stop):
                sc.gather(pts, pts + 1.0, spp=2, flags=base, coop=coop)
            assert seen[-1] == want, (base, coop, seen[-1])
