"""The public interface of windowed adaptive sampling (include/rtmi_window.h), without a GPU.

* the header compiles as C99 and rtmi_window_opts has the size and offsets the entries read it with, in the header's
  comments, in ctypes and in sys.rs;
* librtmi.so exports the six entries and nothing else with the family's word, abi.py and sys.rs declare them, and no other
  family's list holds one of them;
* rtmi_window_steps and rtmi_window_scratch_bytes against the per-pixel entries' functions: the same steps, the same layout
  from the front with the fail plane appended;
* every bad argument that needs no device is refused, with its code and the entry's name, in the documented order.  The
  render entries are called with a NULL scene and the probe with the device index -1, both checked last, so a valid set of
  arguments ends there on every machine (the missing attachments need a live handle: tests/test_gpu_window.py)."""
import ctypes as C

import numpy as np
import pytest

import abi_kit as kit
from raytracing_rust_amd import Scene, abi, window_spread

ENTRIES = ["rtmi_probe_window_spread", "rtmi_render_window", "rtmi_render_window_device", "rtmi_window_scratch_bytes",
           "rtmi_window_spread_device", "rtmi_window_steps"]
OFFSETS = {"min_spp": 0, "step_spp": 4, "estimator": 8, "pass_spp": 12, "abs_tol": 16, "rel_tol": 24, "env_select_p": 32, "radius": 36,
           "reserved": 40}
INVALID, UNSUPPORTED, DEVICE = 1, 2, 3
FC = abi.RTMI_FLAG_FAST_CULL
OTHER_WORDS = ("pixelwise", "sparse", "upscale", "tonemap", "rtmi_frame")


FAMILY = kit.Family("rtmi_window.h", ENTRIES, {"rtmi_window_opts": (abi.WindowOpts, "RtmiWindowOpts", 48, OFFSETS)},
                    word="window", includes=["rtmi.h", "rtmi_adaptive.h", "rtmi_roulette.h"], documented=True,
                    host=("rth_render_window", "rth_render_window_device"))


# ---- layout -----------------------------------------------------------------------------------------------------------------
def test_header_is_c99_with_the_documented_layout(tmp_path):
    FAMILY.c99(tmp_path, holds="RTMI_ROULETTE_ENV_NEE == 3u && RTMI_WINDOW_MAX_RADIUS == 16u")


def test_ctypes_and_rust_match_the_header():
    FAMILY.layout()
    kit.assert_plain_repr_c("RtmiWindowOpts")
    assert FAMILY.constants() == (["RTMI_WINDOW_MAX_RADIUS"], ["RTMI_WINDOW_MAX_RADIUS"]) and abi.RTMI_WINDOW_MAX_RADIUS == 16
    kit.assert_rust_const("RTMI_WINDOW_MAX_RADIUS", "u32", 16)
    assert "#define RTMI_WINDOW_MAX_RADIUS 16u" in kit.header_text("rtmi_window.h")


def test_exports_and_declarations_agree():
    FAMILY.exports()
    assert len(abi.RTMI_WINDOW_SYMBOLS) == 6
    for n in ENTRIES:  # none of the new names reads as a member of a neighbouring family
        assert not any(w in n for w in OTHER_WORDS), n
    assert Scene.render_windowed.__doc__ and window_spread.__doc__


def test_the_header_keeps_to_itself():
    FAMILY.isolation()
    text = kit.header_text("rtmi_window.h", comments=True)
    for word in OTHER_WORDS:  # the neighbours are named by their DESIGN.md sections
        assert word not in text.lower(), word
    assert "DESIGN.md §31 / §32" in text


# ---- the two pure functions ---------------------------------------------------------------------------------------------------
def test_steps_are_the_per_pixel_rule():
    lib = abi.load_rtmi()
    f, g = lib.rtmi_window_steps, lib.rtmi_pixelwise_steps
    assert f(24, 4, 4) == 6 and f(22, 4, 4) == 6 and f(20, 4, 4) == 5 and f(4, 4, 4) == 1 and f(1000, 64, 64) == 16
    for ns, lo, step in ((24, 1, 4), (24, 0, 4), (24, 25, 4), (24, 4, 0), (1, 2, 1)):
        assert f(ns, lo, step) == 0, (ns, lo, step)
    for ns in (2, 5, 24, 1000, 2 ** 32 - 1):
        for lo in (0, 1, 2, 4, 24, 25):
            for step in (0, 1, 3, 64, 2 ** 32 - 1):
                assert f(ns, lo, step) == g(ns, lo, step), (ns, lo, step)


def test_scratch_bytes_append_the_fail_plane():
    lib = abi.load_rtmi()
    f, g = lib.rtmi_window_scratch_bytes, lib.rtmi_pixelwise_scratch_bytes
    for n, pass_spp, steps in ((1, 1, 1), (15, 1, 1), (16, 1, 1), (17, 2, 3), (19 * 13, 4, 6), (16 * 16, 3, 6), (800 * 800, 64, 16),
                               (1920 * 1080, 8, 8), (32768 ** 2, 1, 1024)):
        assert f(n, pass_spp, steps) == g(n, pass_spp, steps) + (n + 15) // 16 * 16, (n, pass_spp, steps)
        assert f(n, pass_spp, steps) % 16 == 0


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
    f = dict(min_spp=4, step_spp=4, estimator=0, pass_spp=0, abs_tol=0.01, rel_tol=0.0, env_select_p=0.5, radius=1, reserved=(0, 0))
    f.update(fields)
    o = abi.WindowOpts(f["min_spp"], f["step_spp"], f["estimator"], f["pass_spp"], f["abs_tol"], f["rel_tol"], f["env_select_p"],
                       f["radius"], (C.c_uint32 * 2)(*f["reserved"]))
    c = abi.Camera()
    keep, ptr = [], {}
    for name in ("linear", "rgb8", "stderr", "spp", "counts", "scratch"):
        a, q = _aligned()
        keep.append(a)
        ptr[name] = q + (shift[1] if shift and shift[0] == name else 0)
    planes = [ptr[n] if on else None for n, on in zip(("linear", "rgb8", "stderr", "spp"), outs)] + [ptr["counts"] if counts else None]
    if entry == "rtmi_render_window":
        args = [None, C.byref(c) if cam else None, C.byref(p) if params else None, C.byref(o) if opts else None] + planes + [None]
    else:
        need = 2 ** 40 if scratch_bytes is None else scratch_bytes
        args = [None, C.byref(p) if params else None, C.byref(c) if cam else None, C.byref(o) if opts else None] + planes + [
            ptr["scratch"] if scratch else None, need, None]
    rc = getattr(lib, entry)(*args)
    assert rc != 0 and all(not a.any() for a in keep)
    return rc, (lib.rtmi_last_error() or b"").decode()


@pytest.mark.parametrize("entry", ["rtmi_render_window", "rtmi_render_window_device"])
def test_render_entries_refuse_before_any_device_work(entry):
    def refused(code, word, **kw):
        rc, msg = _render(entry, **kw)
        assert rc == code and msg.startswith(entry + ": ") and word in msg, (kw, rc, msg)

    device = entry.endswith("_device")
    for radius in (0, 1, 16):
        refused(INVALID, "scene is NULL", radius=radius)  # every value valid: the refusals end at the scene
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
    # 1. the steps and the tolerances, by the rules of rtmi_adaptive.h, and the radius
    refused(INVALID, "min_spp must be at least 2", min_spp=1)
    refused(INVALID, "min_spp must not exceed ns", min_spp=25)
    refused(INVALID, "scene is NULL", min_spp=24)
    refused(INVALID, "step_spp", step_spp=0)
    for tol in ("abs_tol", "rel_tol"):
        for bad in (-1e-9, float("inf"), float("nan")):
            refused(INVALID, "finite and non-negative", **{tol: bad})
    refused(INVALID, "scene is NULL", abs_tol=0.0, rel_tol=0.0)
    for bad in (17, 33, 2 ** 32 - 1):
        refused(INVALID, "radius", radius=bad)
    # 2. the size of a launch
    refused(INVALID, "2^31", render=dict(nx=32768, ny=32768, ns=24))  # 2^30 pixels, 4 samples
    refused(INVALID, "2^31", render=dict(nx=32768, ny=32768, ns=24), pass_spp=2)
    refused(INVALID, "scratch_bytes" if device else "scene is NULL", render=dict(nx=32768, ny=32768, ns=24), pass_spp=1, scratch_bytes=64)
    # 3. the number of steps
    refused(INVALID, "1024 steps", render=dict(ns=2 + 1024), min_spp=2, step_spp=1)
    refused(INVALID, "scene is NULL", render=dict(ns=2 + 1023), min_spp=2, step_spp=1)
    # 6. the reserved words
    for k in range(2):
        refused(INVALID, "reserved", reserved=tuple(5 if j == k else 0 for j in range(2)))
    if device:  # 4. the scratch, 5. the alignments
        lib = abi.load_rtmi()
        need = lib.rtmi_window_scratch_bytes(64, 4, 6)
        refused(INVALID, "d_scratch", scratch=False)
        refused(INVALID, "rtmi_window_scratch_bytes", scratch_bytes=need - 1)
        refused(INVALID, "scratch_bytes", scratch_bytes=lib.rtmi_pixelwise_scratch_bytes(64, 4, 6))  # without the fail plane
        refused(INVALID, "scratch_bytes", scratch_bytes=need - 1, radius=0)  # the layout does not depend on the radius
        refused(INVALID, "scene is NULL", scratch_bytes=need)
        refused(INVALID, "scratch_bytes", scratch_bytes=lib.rtmi_window_scratch_bytes(64, 3, 6), pass_spp=5)  # 5 > a step: a step
        refused(INVALID, "scene is NULL", scratch_bytes=lib.rtmi_window_scratch_bytes(64, 3, 6), pass_spp=3)
        refused(INVALID, "scene is NULL", scratch_bytes=lib.rtmi_window_scratch_bytes(64, 21, 2), min_spp=3, step_spp=1000)
        refused(INVALID, "scratch_bytes", scratch_bytes=lib.rtmi_window_scratch_bytes(64, 21, 2) - 1, min_spp=3, step_spp=1000)
        for which, by in (("linear", 2), ("stderr", 2), ("spp", 2), ("counts", 2), ("scratch", 4), ("scratch", 8)):
            refused(INVALID, "misaligned", shift=(which, by))
        refused(INVALID, "scene is NULL", shift=("rgb8", 1))  # rgb8 takes any alignment
    # the order: pointers, planes, the values, the flags, then 1 to 6, the scene
    refused(INVALID, "NULL argument", opts=False, outs=(False, False, False, False))
    refused(INVALID, "every plane", outs=(False, False, False, False), render=dict(ns=0))
    refused(INVALID, "ns, the cap", render=dict(ns=0, max_depth=0))
    refused(INVALID, "max_depth", render=dict(max_depth=0), estimator=9)
    refused(INVALID, "estimator", estimator=9, render=dict(nx=0))
    refused(INVALID, "env_select_p", estimator=3, env_select_p=0.0, render=dict(flags=abi.RTMI_FLAG_SKY))
    refused(INVALID, "SKY", estimator=2, render=dict(flags=abi.RTMI_FLAG_SKY, nx=0))
    refused(INVALID, "pixels", render=dict(nx=0, t_min=float("nan")))
    refused(INVALID, "t_min", render=dict(t_min=float("nan"), flags=1 << 20))
    refused(UNSUPPORTED, "flags", render=dict(flags=1 << 20), min_spp=1, radius=17)
    refused(INVALID, "min_spp", min_spp=1, radius=17)
    refused(INVALID, "finite and non-negative", abs_tol=-1.0, radius=17)  # the radius is the last of group 1
    refused(INVALID, "radius", radius=17, render=dict(nx=32768, ny=32768))
    refused(INVALID, "2^31", render=dict(nx=32768, ny=32768, ns=2 + 1024 + 4), min_spp=6, step_spp=1)
    refused(INVALID, "1024 steps", render=dict(ns=2 + 1024), min_spp=2, step_spp=1, scratch=False)
    refused(INVALID, "reserved", reserved=(0, 1))
    if device:
        refused(INVALID, "d_scratch", scratch=False, shift=("linear", 2))
        refused(INVALID, "scratch_bytes", scratch_bytes=16, shift=("linear", 2))
        refused(INVALID, "misaligned", shift=("linear", 2), reserved=(1, 0))


def _probe(nx=8, ny=4, radius=1, null=None, device=-1):
    lib = abi.load_rtmi()
    a, f = np.full(64, 7, np.uint8), np.ones(64, np.uint8)
    rc = lib.rtmi_probe_window_spread(device, nx, ny, radius, None if null == "active" else a.ctypes.data,
                                      None if null == "fail" else f.ctypes.data)
    assert rc != 0 and (a == 7).all() and (f == 1).all()
    return rc, (lib.rtmi_last_error() or b"").decode()


def test_probe_refusals_before_any_device_work():
    def refused(code, word, **kw):
        rc, msg = _probe(**kw)
        assert rc == code and msg.startswith("rtmi_probe_window_spread: ") and word in msg, (kw, rc, msg)

    refused(DEVICE, "device")
    for radius in (0, 16):
        refused(DEVICE, "device", radius=radius)
    for null in ("active", "fail"):
        refused(INVALID, "NULL argument", null=null)
    for kw in (dict(nx=0), dict(ny=0), dict(nx=0, ny=0), dict(nx=32769, ny=32768), dict(nx=2 ** 32 - 1, ny=2 ** 32 - 1)):
        refused(INVALID, "pixels", **kw)
    refused(INVALID, "radius", radius=17)
    refused(INVALID, "NULL argument", null="fail", nx=0)
    refused(INVALID, "pixels", nx=0, radius=17)


def test_the_device_spread_refuses_the_same_without_a_device():
    lib = abi.load_rtmi()
    a = np.zeros(64, np.uint8)
    for args, word in (((None, a.ctypes.data, 8, 4, 1), "NULL argument"), ((a.ctypes.data, None, 8, 4, 1), "NULL argument"),
                       ((a.ctypes.data, a.ctypes.data, 0, 4, 1), "pixels"), ((a.ctypes.data, a.ctypes.data, 32769, 32768, 1), "pixels"),
                       ((a.ctypes.data, a.ctypes.data, 8, 4, 17), "radius")):
        assert lib.rtmi_window_spread_device(*args, None) == INVALID
        msg = (lib.rtmi_last_error() or b"").decode()
        assert msg.startswith("rtmi_window_spread_device: ") and word in msg, msg


def test_the_python_face_reports_the_refusal():
    sc = Scene.__new__(Scene)
    with pytest.raises(ValueError, match="estimator"):
        sc.render_windowed(None, 8, 8, 24, 4, 4, estimator="roulette")
    with pytest.raises(ValueError, match="out must be"):
        sc.render_windowed(None, 8, 8, 24, 4, 4, out="cupy")
    with pytest.raises(ValueError, match="one shape"):
        window_spread(np.zeros((4, 8), np.uint8), np.zeros((4, 9), np.uint8), 1)
    with pytest.raises(ValueError, match="radius"):
        window_spread(np.zeros((4, 8), np.uint8), np.zeros((4, 8), np.uint8), 17, device=-1)
    import inspect

    assert inspect.signature(Scene.render_windowed).parameters["radius"].default == 1
