"""The public interface of per-pixel adaptive sampling (include/rtmi_pixelwise.h), without a GPU.

* the header compiles as C99 and rtmi_pixelwise_opts has the size and offsets the entries read it with, in the header's
  comments, in ctypes and in sys.rs;
* librtmi.so exports the five entries and nothing else with the family's word, abi.py and sys.rs declare them, and no other
  family's list holds one of them;
* rtmi_pixelwise_steps and rtmi_pixelwise_scratch_bytes against the stated rule and layout;
* every bad argument that needs no device is refused, with its code and the entry's name, in the documented order.  The
  render entries are called with a NULL scene and the probe with the device index -1, both checked last, so a valid set of
  arguments ends there on every machine (the missing attachments need a live handle: tests/test_gpu_pixelwise.py)."""
import ctypes as C

import numpy as np
import pytest

import abi_kit as kit
from raytracing_rust_amd import Scene, abi

ENTRIES = ["rtmi_pixelwise_scratch_bytes", "rtmi_pixelwise_steps", "rtmi_probe_pixelwise_step", "rtmi_render_pixelwise",
           "rtmi_render_pixelwise_device"]
OFFSETS = {"min_spp": 0, "step_spp": 4, "estimator": 8, "pass_spp": 12, "abs_tol": 16, "rel_tol": 24, "env_select_p": 32, "reserved": 36}
INVALID, UNSUPPORTED, DEVICE = 1, 2, 3
FC = abi.RTMI_FLAG_FAST_CULL


FAMILY = kit.Family("rtmi_pixelwise.h", ENTRIES, {"rtmi_pixelwise_opts": (abi.PixelwiseOpts, "RtmiPixelwiseOpts", 48, OFFSETS)},
                    word="pixelwise", includes=["rtmi.h", "rtmi_adaptive.h", "rtmi_roulette.h"], documented=True,
                    host=("rth_render_pixelwise", "rth_render_pixelwise_device"))


# ---- layout -----------------------------------------------------------------------------------------------------------------
def test_header_is_c99_with_the_documented_layout(tmp_path):
    FAMILY.c99(tmp_path, holds="RTMI_ROULETTE_ENV_NEE == 3u && RTMI_PIXELWISE_MAX_STEPS == 1024u")


def test_ctypes_and_rust_match_the_header():
    FAMILY.layout()
    kit.assert_plain_repr_c("RtmiPixelwiseOpts")


def test_exports_and_declarations_agree():
    FAMILY.exports()
    assert len(abi.RTMI_PIXELWISE_SYMBOLS) == 5 and Scene.render_pixelwise.__doc__


def test_the_header_keeps_to_itself():
    FAMILY.isolation()
    FAMILY.constants()


# ---- the two pure functions ---------------------------------------------------------------------------------------------------
def test_steps():
    f = abi.load_rtmi().rtmi_pixelwise_steps
    assert f(24, 4, 4) == 6 and f(22, 4, 4) == 6 and f(21, 4, 4) == 6 and f(20, 4, 4) == 5
    assert f(4, 4, 4) == 1 and f(5, 4, 100) == 2 and f(1000, 64, 64) == 16 and f(64, 8, 8) == 8
    assert f(2 ** 32 - 1, 2, 1) == 2 ** 32 - 2 and f(2 ** 32 - 1, 2, 2 ** 32 - 1) == 2
    for ns, lo, step in ((24, 1, 4), (24, 0, 4), (24, 25, 4), (24, 4, 0), (1, 2, 1)):
        assert f(ns, lo, step) == 0, (ns, lo, step)
    for lo, step in ((2, 1), (4, 4), (7, 3)):
        got = [f(ns, lo, step) for ns in range(lo, lo + 40)]
        assert got == [1 + -(-(ns - lo) // step) for ns in range(lo, lo + 40)]
        assert all(b - a in (0, 1) for a, b in zip(got, got[1:]))  # monotone in the cap


def _layout(n, pass_spp, steps):
    """the parts of the header's layout, unrounded"""
    return [16, 8 * steps, 4 * ((n + 4095) // 4096), n, 4 * n, 72 * n, 12 * n * pass_spp]


def test_scratch_bytes():
    f = abi.load_rtmi().rtmi_pixelwise_scratch_bytes
    for n, pass_spp, steps in ((1, 1, 1), (19 * 13, 4, 6), (16 * 16, 3, 6), (800 * 800, 64, 16), (1920 * 1080, 8, 8), (32768 ** 2, 1, 1024)):
        b = f(n, pass_spp, steps)
        parts = _layout(n, pass_spp, steps)
        assert b % 16 == 0 and sum(parts) <= b <= sum(parts) + 15 * len(parts), (n, pass_spp, steps, b)
        assert b == sum((x + 15) // 16 * 16 for x in parts)
    assert f(640000, 8, 8) < f(640001, 8, 8) <= f(640016, 8, 8)
    assert f(640000, 8, 8) < f(640000, 9, 8) and f(640000, 8, 2) < f(640000, 8, 4)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _aligned(words=4096):
    a = np.zeros(words + 8, np.uint32)
    return a, a.ctypes.data + (-a.ctypes.data) % 16


def _render(entry, params=True, cam=True, opts=True, outs=(True, True, True, True), counts=True, scratch=True, shift=None,
            scratch_bytes=None, render=None, **fields):
    """the entry with a NULL scene and otherwise valid arguments, except what the keywords change"""
    lib = abi.load_rtmi()
    p = abi.RenderParams()
    p.nx, p.ny, p.ns, p.max_depth, p.t_min, p.flags, p.tile_world, p.seed = 8, 8, 24, 50, 0.001, FC, 1, 7
    for k, v in (render or {}).items():
        setattr(p, k, v)
    f = dict(min_spp=4, step_spp=4, estimator=0, pass_spp=0, abs_tol=0.01, rel_tol=0.0, env_select_p=0.5, reserved=(0, 0, 0))
    f.update(fields)
    o = abi.PixelwiseOpts(f["min_spp"], f["step_spp"], f["estimator"], f["pass_spp"], f["abs_tol"], f["rel_tol"], f["env_select_p"],
                          (C.c_uint32 * 3)(*f["reserved"]))
    c = abi.Camera()
    keep, ptr = [], {}
    for name in ("linear", "rgb8", "stderr", "spp", "counts", "scratch"):
        a, q = _aligned()
        keep.append(a)
        ptr[name] = q + (shift[1] if shift and shift[0] == name else 0)
    planes = [ptr[n] if on else None for n, on in zip(("linear", "rgb8", "stderr", "spp"), outs)] + [ptr["counts"] if counts else None]
    if entry == "rtmi_render_pixelwise":
        args = [None, C.byref(c) if cam else None, C.byref(p) if params else None, C.byref(o) if opts else None] + planes + [None]
    else:
        need = 2 ** 40 if scratch_bytes is None else scratch_bytes
        args = [None, C.byref(p) if params else None, C.byref(c) if cam else None, C.byref(o) if opts else None] + planes + [
            ptr["scratch"] if scratch else None, need, None]
    rc = getattr(lib, entry)(*args)
    assert rc != 0 and all(not a.any() for a in keep)
    return rc, (lib.rtmi_last_error() or b"").decode()


@pytest.mark.parametrize("entry", ["rtmi_render_pixelwise", "rtmi_render_pixelwise_device"])
def test_render_entries_refuse_before_any_device_work(entry):
    def refused(code, word, **kw):
        rc, msg = _render(entry, **kw)
        assert rc == code and msg.startswith(entry + ": ") and word in msg, (kw, rc, msg)

    device = entry.endswith("_device")
    refused(INVALID, "scene is NULL")  # every value valid: the refusals end at the scene
    for null in ("params", "cam", "opts"):
        refused(INVALID, "NULL argument", **{null: False})
    refused(INVALID, "every plane", outs=(False, False, False, False))
    for k in range(4):
        refused(INVALID, "scene is NULL", outs=tuple(j == k for j in range(4)), counts=False)
    refused(INVALID, "ns, the cap", render=dict(ns=0))
    refused(INVALID, "max_depth", render=dict(max_depth=0))
    refused(INVALID, "estimator", estimator=4)
    for bad in (0.0, -0.5, 1.5, float("nan")):
        refused(INVALID, "env_select_p", estimator=abi.RTMI_ROULETTE_ENV_NEE, env_select_p=bad)
    refused(INVALID, "scene is NULL", estimator=abi.RTMI_ROULETTE_ENV, env_select_p=0.0)  # read by ENV_NEE only
    for est in (abi.RTMI_ROULETTE_ENV, abi.RTMI_ROULETTE_ENV_NEE):
        refused(INVALID, "SKY", estimator=est, render=dict(flags=abi.RTMI_FLAG_SKY))
    refused(INVALID, "pixels", render=dict(nx=0))
    refused(INVALID, "pixels", render=dict(nx=32769, ny=32768))
    refused(INVALID, "t_min", render=dict(t_min=float("inf")))
    for flag in (abi.RTMI_FLAG_SYNC, abi.RTMI_FLAG_PATH_SIG, abi.RTMI_FLAG_REF_TREE, abi.RTMI_FLAG_PROFILE, abi.RTMI_FLAG_LIGHT_COOP, 1 << 20):
        refused(UNSUPPORTED, "flags", render=dict(flags=flag | FC))
    accepted = FC | abi.RTMI_FLAG_SKY | abi.RTMI_FLAG_FACE_FORWARD | abi.RTMI_FLAG_UV_BOOK
    refused(INVALID, "scene is NULL", render=dict(flags=accepted))
    # 1. the steps and the tolerances, by the rules of rtmi_adaptive.h
    refused(INVALID, "min_spp must be at least 2", min_spp=1)
    refused(INVALID, "min_spp must not exceed ns", min_spp=25)
    refused(INVALID, "scene is NULL", min_spp=24)
    refused(INVALID, "step_spp", step_spp=0)
    for tol in ("abs_tol", "rel_tol"):
        for bad in (-1e-9, float("inf"), float("nan")):
            refused(INVALID, "finite and non-negative", **{tol: bad})
    refused(INVALID, "scene is NULL", abs_tol=0.0, rel_tol=0.0)
    # 2. the size of a launch
    refused(INVALID, "2^31", render=dict(nx=32768, ny=32768, ns=24))  # 2^30 pixels, 4 samples
    refused(INVALID, "2^31", render=dict(nx=32768, ny=32768, ns=24), pass_spp=2)
    refused(INVALID, "scratch_bytes" if device else "scene is NULL", render=dict(nx=32768, ny=32768, ns=24), pass_spp=1, scratch_bytes=64)
    # 3. the number of steps
    refused(INVALID, "1024 steps", render=dict(ns=2 + 1024), min_spp=2, step_spp=1)
    refused(INVALID, "scene is NULL", render=dict(ns=2 + 1023), min_spp=2, step_spp=1)
    # 6. the reserved words
    for k in range(3):
        refused(INVALID, "reserved", reserved=tuple(5 if j == k else 0 for j in range(3)))
    if device:  # 4. the scratch, 5. the alignments
        lib = abi.load_rtmi()
        need = lib.rtmi_pixelwise_scratch_bytes(64, 4, 6)
        refused(INVALID, "d_scratch", scratch=False)
        refused(INVALID, "scratch_bytes", scratch_bytes=need - 1)
        refused(INVALID, "scene is NULL", scratch_bytes=need)
        refused(INVALID, "scratch_bytes", scratch_bytes=lib.rtmi_pixelwise_scratch_bytes(64, 3, 6), pass_spp=5)  # 5 > a step: a step
        refused(INVALID, "scene is NULL", scratch_bytes=lib.rtmi_pixelwise_scratch_bytes(64, 3, 6), pass_spp=3)
        # a step larger than what the cap leaves is sized by what it leaves: 21 samples
        refused(INVALID, "scene is NULL", scratch_bytes=lib.rtmi_pixelwise_scratch_bytes(64, 21, 2), min_spp=3, step_spp=1000)
        refused(INVALID, "scratch_bytes", scratch_bytes=lib.rtmi_pixelwise_scratch_bytes(64, 21, 2) - 1, min_spp=3, step_spp=1000)
        for which, by in (("linear", 2), ("stderr", 2), ("spp", 2), ("counts", 2), ("scratch", 4), ("scratch", 8)):
            refused(INVALID, "misaligned", shift=(which, by))
        refused(INVALID, "scene is NULL", shift=("rgb8", 1))  # rgb8 takes any alignment
    # the order: pointers, planes, the values of sparse renders' order, the flags, then 1 to 6, the scene
    refused(INVALID, "NULL argument", opts=False, outs=(False, False, False, False))
    refused(INVALID, "every plane", outs=(False, False, False, False), render=dict(ns=0))
    refused(INVALID, "ns, the cap", render=dict(ns=0, max_depth=0))
    refused(INVALID, "max_depth", render=dict(max_depth=0), estimator=9)
    refused(INVALID, "estimator", estimator=9, render=dict(nx=0))
    refused(INVALID, "env_select_p", estimator=3, env_select_p=0.0, render=dict(flags=abi.RTMI_FLAG_SKY))
    refused(INVALID, "SKY", estimator=2, render=dict(flags=abi.RTMI_FLAG_SKY, nx=0))
    refused(INVALID, "pixels", render=dict(nx=0, t_min=float("nan")))
    refused(INVALID, "t_min", render=dict(t_min=float("nan"), flags=1 << 20))
    refused(UNSUPPORTED, "flags", render=dict(flags=1 << 20), min_spp=1)
    refused(INVALID, "min_spp", min_spp=1, render=dict(nx=32768, ny=32768))
    refused(INVALID, "2^31", render=dict(nx=32768, ny=32768, ns=2 + 1024 + 4), min_spp=6, step_spp=1)
    refused(INVALID, "1024 steps", render=dict(ns=2 + 1024), min_spp=2, step_spp=1, scratch=False)
    refused(INVALID, "reserved", reserved=(0, 0, 1))
    if device:
        refused(INVALID, "d_scratch", scratch=False, shift=("linear", 2))
        refused(INVALID, "scratch_bytes", scratch_bytes=16, shift=("linear", 2))
        refused(INVALID, "misaligned", shift=("linear", 2), reserved=(1, 0, 0))


def _probe(n_pixels=8, capacity=4, pass_=2, null=None, device=-1):
    lib = abi.load_rtmi()
    lst, smp, st = np.zeros(64, np.uint32), np.zeros(64 * 3 * 4, np.float32), np.zeros(9 * 64, np.float64)
    rc = lib.rtmi_probe_pixelwise_step(device, n_pixels, capacity, None if null == "list" else lst.ctypes.data, None,
                                       None if null == "samples" else smp.ctypes.data, None if null == "state" else st.ctypes.data,
                                       0, pass_, 1, 24, 0.0, 0.0, None, None, None, None, None)
    assert rc != 0 and not st.any()
    return rc, (lib.rtmi_last_error() or b"").decode()


def test_probe_refusals_before_any_device_work():
    def refused(code, word, **kw):
        rc, msg = _probe(**kw)
        assert rc == code and msg.startswith("rtmi_probe_pixelwise_step: ") and word in msg, (kw, rc, msg)

    refused(DEVICE, "device")
    for null in ("list", "samples", "state"):
        refused(INVALID, "NULL argument", null=null)
    for kw in (dict(n_pixels=0), dict(capacity=0), dict(pass_=0)):
        refused(INVALID, "at least 1", **kw)
    refused(INVALID, "2^31", capacity=2 ** 16, pass_=2 ** 15)
    refused(DEVICE, "device", capacity=2 ** 16, pass_=2 ** 15 - 1)
    refused(INVALID, "NULL argument", null="list", n_pixels=0)
    refused(INVALID, "at least 1", n_pixels=0, capacity=2 ** 16, pass_=2 ** 15)


def test_the_python_face_reports_the_refusal():
    sc = Scene.__new__(Scene)
    with pytest.raises(ValueError, match="estimator"):
        sc.render_pixelwise(None, 8, 8, 24, 4, 4, estimator="roulette")
    with pytest.raises(ValueError, match="out must be"):
        sc.render_pixelwise(None, 8, 8, 24, 4, 4, out="cupy")
