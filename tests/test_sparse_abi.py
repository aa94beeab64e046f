"""The sparse renders' public interface (include/rtmi_sparse.h), without a GPU.

* the header compiles as C99 and rtmi_sparse_params has the size and offsets the kernels read it with, in the header's
  comments, in ctypes and in sys.rs;
* librtmi.so exports the seven entries and nothing else with the family's word, abi.py and sys.rs declare them, and no
  other family's list holds one of them;
* every bad argument that needs no device is refused, with its code and the entry's name, in the documented order.  The
  stateless entries are called with the device index -1 and the others with a NULL scene, both checked last, so a valid
  set of arguments ends there on every machine (the missing attachments need a live handle: tests/test_gpu_sparse.py)."""
import ctypes as C

import numpy as np
import pytest

import abi_kit as kit
from raytracing_rust_amd import Scene, abi, sparse_patch, sparse_select

ENTRIES = ["rtmi_sparse_patch_device", "rtmi_sparse_refine", "rtmi_sparse_refine_device", "rtmi_sparse_render",
           "rtmi_sparse_render_device", "rtmi_sparse_scratch_bytes", "rtmi_sparse_select_device"]
OFFSETS = {"n": 0, "ns": 4, "first_sample": 8, "estimator": 12, "env_select_p": 16, "reserved": 20}
FAMILY = kit.Family("rtmi_sparse.h", ENTRIES, {"rtmi_sparse_params": (abi.SparseParams, "RtmiSparseParams", 32, OFFSETS)},
                    word="sparse", includes=["rtmi.h", "rtmi_roulette.h"], documented=True,
                    host=("rth_sparse_render", "rth_sparse_render_device", "rth_sparse_refine"))
INVALID, UNSUPPORTED, DEVICE = 1, 2, 3
FC = abi.RTMI_FLAG_FAST_CULL


# ---- layout -----------------------------------------------------------------------------------------------------------------
def test_header_is_c99_with_the_documented_layout(tmp_path):
    FAMILY.c99(tmp_path, holds="RTMI_ROULETTE_ENV_NEE == 3u")


def test_ctypes_and_rust_match_the_header():
    FAMILY.layout()
    kit.assert_plain_repr_c("RtmiSparseParams")


def test_exports_and_declarations_agree():
    FAMILY.exports()
    assert len(abi.RTMI_SPARSE_SYMBOLS) == 7
    assert Scene.render_pixels.__doc__ and Scene.refine_pixels.__doc__ and sparse_select.__doc__ and sparse_patch.__doc__


def test_the_header_keeps_to_itself():
    FAMILY.isolation()
    FAMILY.constants()
    low = kit.header_text("rtmi_sparse.h", comments=True).lower()
    assert "upscale" not in low and "tonemap" not in low


def test_scratch_bytes():
    f = abi.load_rtmi().rtmi_sparse_scratch_bytes
    assert f(1, 0, 0) == 32 and f(4096, 0, 0) == 32 and f(4097, 0, 0) == 32 and f(4096 * 4 + 1, 0, 0) == 48
    for n, cap, ns in ((64 * 64, 100, 8), (1920 * 1080, 1, 1), (19 * 13, 247, 4), (32768 ** 2, 5, 3)):
        b = f(n, cap, ns)
        assert b % 16 == 0 and b >= 16 + 4 * ((n + 4095) // 4096) + cap * (4 + 24 + 12 * ns)
        assert b <= 16 + 4 * ((n + 4095) // 4096) + cap * (4 + 24 + 12 * ns) + 5 * 16
    assert f(1920 * 1080, 1, 1) < f(1920 * 1080, 2, 1) < f(1920 * 1080, 2, 9)


# ---- the stateless entries' refusals ------------------------------------------------------------------------------------------
def _aligned(words=64):
    a = np.zeros(words + 8, np.uint32)
    return a, a.ctypes.data + (-a.ctypes.data) % 16


def _select(n=100, capacity=10, null=None, shift=None, device=-1):
    lib = abi.load_rtmi()
    keep, ptr = [], {}
    for name in ("bytes", "list", "count", "scratch"):
        a, p = _aligned()
        keep.append(a)
        ptr[name] = None if name == null else p + (shift[1] if shift and shift[0] == name else 0)
    rc = lib.rtmi_sparse_select_device(device, n, ptr["bytes"], 8, capacity, ptr["list"], ptr["count"], ptr["scratch"], None)
    assert rc != 0 and all(not a.any() for a in keep)
    return rc, (lib.rtmi_last_error() or b"").decode()


def test_select_refusals_before_any_device_work():
    def refused(code, word, **kw):
        rc, msg = _select(**kw)
        assert rc == code and msg.startswith("rtmi_sparse_select_device: ") and word in msg, (kw, rc, msg)

    refused(DEVICE, "device")  # every value valid: the device index is refused
    for null in ("bytes", "list", "count", "scratch"):
        refused(INVALID, "NULL argument", null=null)
    for n in (0, 32768 ** 2 + 1, 2 ** 32 - 1):
        refused(INVALID, "n must be", n=n)
    refused(DEVICE, "device", n=32768 ** 2)
    refused(DEVICE, "device", n=1, capacity=2 ** 32 - 1)
    refused(INVALID, "capacity", capacity=0)
    for which, by in (("list", 1), ("list", 2), ("count", 2), ("scratch", 4), ("scratch", 8)):
        refused(INVALID, "misaligned", shift=(which, by))
    refused(DEVICE, "device", shift=("bytes", 1))  # the bytes take any alignment
    refused(DEVICE, "device", shift=("list", 4))
    refused(DEVICE, "device", shift=("count", 4))
    # the order: pointers, n, capacity, the alignment, the device
    refused(INVALID, "NULL argument", null="list", n=0)
    refused(INVALID, "n must be", n=0, capacity=0)
    refused(INVALID, "capacity", capacity=0, shift=("list", 2))
    refused(INVALID, "misaligned", shift=("count", 1), device=10 ** 6)


def _patch(n_pixels=100, capacity=10, null=(), shift=None, mark=4, device=-1):
    lib = abi.load_rtmi()
    keep, ptr = [], {}
    for name in ("list", "count", "mean", "linear", "rgb8", "bytes"):
        a, p = _aligned()
        keep.append(a)
        ptr[name] = None if name in null else p + (shift[1] if shift and shift[0] == name else 0)
    rc = lib.rtmi_sparse_patch_device(device, n_pixels, ptr["list"], ptr["count"], capacity, ptr["mean"], ptr["linear"], ptr["rgb8"],
                                      ptr["bytes"], mark, None)
    assert rc != 0 and all(not a.any() for a in keep)
    return rc, (lib.rtmi_last_error() or b"").decode()


def test_patch_refusals_before_any_device_work():
    def refused(code, word, **kw):
        rc, msg = _patch(**kw)
        assert rc == code and msg.startswith("rtmi_sparse_patch_device: ") and word in msg, (kw, rc, msg)

    refused(DEVICE, "device")
    refused(INVALID, "NULL argument", null=("list",))
    refused(INVALID, "NULL argument", null=("mean",))
    refused(DEVICE, "device", null=("count",))  # no count: every entry of the list
    refused(INVALID, "every plane", null=("linear", "rgb8", "bytes"))
    for only in ("linear", "rgb8", "bytes"):
        refused(DEVICE, "device", null=tuple(n for n in ("linear", "rgb8", "bytes") if n != only))
    for n in (0, 32768 ** 2 + 1):
        refused(INVALID, "n_pixels", n_pixels=n)
    refused(INVALID, "capacity", capacity=0)
    refused(INVALID, "mark", mark=256)
    for which in ("list", "count", "mean", "linear"):
        refused(INVALID, "misaligned", shift=(which, 2))
    refused(DEVICE, "device", shift=("rgb8", 1))
    refused(DEVICE, "device", shift=("bytes", 3))
    refused(INVALID, "NULL argument", null=("list", "linear", "rgb8", "bytes"))
    refused(INVALID, "every plane", null=("linear", "rgb8", "bytes"), n_pixels=0)
    refused(INVALID, "n_pixels", n_pixels=0, capacity=0)
    refused(INVALID, "capacity", capacity=0, mark=999)
    refused(INVALID, "mark", mark=999, shift=("list", 1))


# ---- the entries of a scene ---------------------------------------------------------------------------------------------------
def _render(entry, params=True, cam=True, sp=True, pixels=True, outs=(True, True, True), scratch=True, shift=None, mask=8, mark=4,
            scratch_bytes=None, render=None, **fields):
    """the entry with a NULL scene and otherwise valid arguments, except what the keywords change"""
    lib = abi.load_rtmi()
    p = abi.RenderParams()
    p.nx, p.ny, p.ns, p.max_depth, p.t_min, p.flags, p.tile_world, p.seed = 8, 8, 1, 50, 0.001, FC, 1, 7
    for k, v in (render or {}).items():
        setattr(p, k, v)
    f = dict(n=4, ns=2, first_sample=0, estimator=0, env_select_p=0.5, reserved=(0, 0, 0))
    f.update(fields)
    s = abi.SparseParams(f["n"], f["ns"], f["first_sample"], f["estimator"], f["env_select_p"], (C.c_uint32 * 3)(*f["reserved"]))
    c = abi.Camera()
    keep, ptr = [], {}
    for name in ("pixels", "a", "b", "c", "scratch", "count"):
        a, q = _aligned(256)
        keep.append(a)
        ptr[name] = q + (shift[1] if shift and shift[0] == name else 0)
    head = [None, C.byref(p) if params else None, C.byref(c) if cam else None, C.byref(s) if sp else None]
    o = [ptr[n] if on else None for n, on in zip("abc", outs)]
    if entry == "rtmi_sparse_render":
        args = head + [ptr["pixels"] if pixels else None] + o + [None]
    elif entry == "rtmi_sparse_render_device":
        args = head + [ptr["pixels"] if pixels else None, ptr["count"]] + o + [ptr["scratch"] if scratch else None, None]
    else:
        need = lib.rtmi_sparse_scratch_bytes(p.nx * p.ny, f["n"], f["ns"]) if scratch_bytes is None else scratch_bytes
        args = head + [mask, mark, ptr["pixels"] if pixels else None] + o
        args += [ptr["scratch"] if scratch else None, need, ptr["count"], None] if entry.endswith("_device") else [ptr["count"]]
    rc = getattr(lib, entry)(*args)
    assert rc != 0 and all(not a.any() for a in keep)
    return rc, (lib.rtmi_last_error() or b"").decode()


@pytest.mark.parametrize("entry", ["rtmi_sparse_render", "rtmi_sparse_render_device", "rtmi_sparse_refine", "rtmi_sparse_refine_device"])
def test_scene_entries_refuse_before_any_device_work(entry):
    def refused(code, word, **kw):
        rc, msg = _render(entry, **kw)
        assert rc == code and msg.startswith(entry + ": ") and word in msg, (kw, rc, msg)

    render, device = "render" in entry, entry.endswith("_device")
    refused(INVALID, "scene is NULL")  # every value valid: the refusals end at the scene
    if render:
        refused(INVALID, "scene is NULL", n=0)  # an empty list still needs a handle
    for null in ("params", "cam", "sp"):
        refused(INVALID, "NULL argument", **{null: False})
    refused(INVALID, "is NULL", pixels=False)
    if entry == "rtmi_sparse_render":
        refused(INVALID, "every output", outs=(False, False, False))
        for k in range(3):
            refused(INVALID, "scene is NULL", outs=tuple(j == k for j in range(3)))
    elif entry == "rtmi_sparse_render_device":
        refused(INVALID, "d_samples", outs=(True, True, False))
        refused(INVALID, "scene is NULL", outs=(False, False, True))
    else:
        refused(INVALID, "scene is NULL", outs=(False, False, False))  # the planes besides the bytes are optional
    refused(INVALID, "ns must be", ns=0)
    refused(INVALID, "max_depth", render=dict(max_depth=0))
    refused(INVALID, "estimator", estimator=4)
    refused(INVALID, "first_sample", first_sample=2 ** 32 - 1)
    refused(INVALID, "scene is NULL", first_sample=2 ** 32 - 2)
    refused(INVALID, "n * ns", n=2 ** 16, ns=2 ** 15)
    for bad in (0.0, -0.5, 1.5, float("nan")):
        refused(INVALID, "env_select_p", estimator=abi.RTMI_ROULETTE_ENV_NEE, env_select_p=bad)
    refused(INVALID, "scene is NULL", estimator=abi.RTMI_ROULETTE_ENV, env_select_p=0.0)  # read by ENV_NEE only
    for est in (abi.RTMI_ROULETTE_ENV, abi.RTMI_ROULETTE_ENV_NEE):
        refused(INVALID, "SKY", estimator=est, render=dict(flags=abi.RTMI_FLAG_SKY))
    refused(INVALID, "pixels", render=dict(nx=0))
    refused(INVALID, "pixels", render=dict(nx=2 ** 16, ny=2 ** 16))
    for k in range(3):
        refused(INVALID, "reserved", reserved=tuple(5 if j == k else 0 for j in range(3)))
    for flag in (abi.RTMI_FLAG_SYNC, abi.RTMI_FLAG_PATH_SIG, abi.RTMI_FLAG_REF_TREE, abi.RTMI_FLAG_PROFILE, abi.RTMI_FLAG_LIGHT_COOP, 1 << 20):
        refused(UNSUPPORTED, "flags", render=dict(flags=flag | FC))
    accepted = FC | abi.RTMI_FLAG_SKY | abi.RTMI_FLAG_FACE_FORWARD | abi.RTMI_FLAG_UV_BOOK
    refused(INVALID, "scene is NULL", render=dict(flags=accepted))
    # the order: pointers, outputs, ns, max_depth, the estimator, the two overflow rules, the estimator's own, the image,
    # the reserved words, the flags, the entry's own, the scene
    refused(INVALID, "NULL argument", sp=False, pixels=False)
    refused(INVALID, "ns must be", ns=0, render=dict(max_depth=0))
    refused(INVALID, "max_depth", render=dict(max_depth=0), estimator=9)
    refused(INVALID, "estimator", estimator=9, first_sample=2 ** 32 - 1)
    refused(INVALID, "first_sample", first_sample=2 ** 32 - 1, ns=2 ** 15, n=2 ** 16)
    refused(INVALID, "n * ns", n=2 ** 16, ns=2 ** 15, estimator=3, env_select_p=0.0)
    refused(INVALID, "env_select_p", estimator=3, env_select_p=0.0, render=dict(flags=abi.RTMI_FLAG_SKY))
    refused(INVALID, "SKY", estimator=2, render=dict(flags=abi.RTMI_FLAG_SKY), reserved=(1, 0, 0))
    refused(INVALID, "reserved", reserved=(0, 0, 1), render=dict(flags=1 << 20))
    if entry == "rtmi_sparse_render":
        pass  # a pixel outside the image is named below
    elif entry == "rtmi_sparse_render_device":
        refused(INVALID, "d_scratch", scratch=False)
        for which in ("pixels", "count", "a", "b", "c", "scratch"):
            refused(INVALID, "misaligned", shift=(which, 2))
        refused(UNSUPPORTED, "flags", render=dict(flags=1 << 20), scratch=False)
    else:
        refused(INVALID, "32768^2", render=dict(nx=32769, ny=32768))
        refused(INVALID, "budget", n=0)
        refused(INVALID, "mark", mark=256)
        refused(UNSUPPORTED, "flags", render=dict(flags=1 << 20), mark=256)
        if device:
            refused(INVALID, "d_scratch", scratch=False)
            for which, by in (("a", 2), ("c", 2), ("count", 2), ("scratch", 4), ("scratch", 8)):
                refused(INVALID, "misaligned", shift=(which, by))
            refused(INVALID, "scene is NULL", shift=("pixels", 1))  # the bytes and rgb8 take any alignment
            refused(INVALID, "scene is NULL", shift=("b", 1))
            refused(INVALID, "scratch_bytes", scratch_bytes=abi.load_rtmi().rtmi_sparse_scratch_bytes(64, 4, 2) - 1)
            refused(INVALID, "mark", mark=256, scratch=False)


def test_a_pixel_outside_the_image_is_named():
    lib = abi.load_rtmi()
    p = abi.RenderParams()
    p.nx, p.ny, p.ns, p.max_depth, p.t_min, p.flags, p.tile_world = 8, 8, 1, 50, 0.001, FC, 1
    s = abi.SparseParams(4, 2, 0, 0, 0.5)
    c = abi.Camera()
    out = np.zeros(64, np.float32)
    px = np.array([0, 63, 64, 5], np.uint32)
    rc = lib.rtmi_sparse_render(None, C.byref(p), C.byref(c), C.byref(s), px.ctypes.data, out.ctypes.data, None, None, None)
    assert rc == INVALID and lib.rtmi_last_error() == b"rtmi_sparse_render: pixels[2] = 64 is outside the image"
    px[2] = 9
    rc = lib.rtmi_sparse_render(None, C.byref(p), C.byref(c), C.byref(s), px.ctypes.data, out.ctypes.data, None, None, None)
    assert rc == INVALID and b"scene is NULL" in lib.rtmi_last_error()


def test_the_python_face_reports_the_refusal():
    with pytest.raises(ValueError, match="class"):
        sparse_select(np.zeros(4, np.uint8), (32,))
    with pytest.raises(ValueError, match="class"):
        sparse_select(np.zeros(4, np.uint8), (-1,))
    sc = Scene.__new__(Scene)
    with pytest.raises(ValueError, match="estimator"):
        sc.render_pixels(None, 8, 8, np.zeros(1, np.uint32), 1, estimator="roulette")
    with pytest.raises(ValueError, match="estimator"):
        sc.refine_pixels(None, {}, estimator="roulette")
    with pytest.raises(ValueError, match="class"):
        sc.refine_pixels(None, {}, classes=(40,))
