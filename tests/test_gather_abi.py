"""The hemisphere gathers' public interface (include/rtmi_gather.h), without a GPU.

* the header compiles as C99 and rtmi_gather_params has the size and offsets the kernels read it with, in the header, in
  ctypes and in sys.rs;
* librtmi.so and librt_host.so export the entries, abi.py and sys.rs declare them;
* every bad argument that needs no handle is refused before a device is touched, with its code and the entry's name (the
  missing attachments need a handle: tests/test_gpu_gather.py)."""
import ctypes as C

import numpy as np
import pytest

import abi_kit as kit
from raytracing_rust_amd import abi

ENTRIES = ["rtmi_gather", "rtmi_gather_device", "rtmi_gather_directions"]
OFFSETS = {"n": 0, "spp": 4, "mode": 8, "estimator": 12, "flags": 16, "max_depth": 20, "t_min": 24, "seed": 32,
           "first_point": 40, "first_sample": 48, "slab_points": 52, "env_select_p": 56}


FAMILY = kit.Family("rtmi_gather.h", ENTRIES, {"rtmi_gather_params": (abi.GatherParams, "RtmiGatherParams", 64, OFFSETS)},
                    word="rtmi_gather", includes=["rtmi.h", "rtmi_math.h", "rtmi_radiance.h"], host=("rth_gather", "rth_gather_device"))


def test_header_is_c99_with_the_documented_layout(tmp_path):
    FAMILY.c99(tmp_path, body="float d[3], y[9]; rtmi_gather_sphere(0.25f, 0.5f, d); rtmi_gather_sh9(d, y);",
               holds="RTMI_GATHER_COSINE == 0u && RTMI_GATHER_SPHERE == 1u && y[0] > 0.0f")


def test_ctypes_and_rust_match_the_header():
    FAMILY.layout()
    kit.assert_plain_repr_c("RtmiGatherParams")
    FAMILY.constants()
    assert (abi.RTMI_GATHER_COSINE, abi.RTMI_GATHER_SPHERE) == (0, 1)
    kit.assert_rust_const("RTMI_GATHER_COSINE", "u32", 0)
    kit.assert_rust_const("RTMI_GATHER_SPHERE", "u32", 1)


def test_exports_and_declarations_agree():
    FAMILY.exports()


def test_the_header_keeps_to_itself():
    FAMILY.isolation()


def _call(entry, n=4, params=True, has_points=True, has_normals=True, outs=(True, True, False), points=None, normals=None,
          time=None, scratch=(True, 1 << 20), **fields):
    """the entry with a NULL scene and otherwise valid arguments, except what the keywords change"""
    lib = abi.load_rtmi()
    f = dict(n=n, spp=2, mode=abi.RTMI_GATHER_COSINE, estimator=abi.RTMI_ROULETTE_PLAIN, flags=0, max_depth=50, t_min=0.001, seed=7,
             first_point=0, first_sample=0, slab_points=0, env_select_p=0.5)
    f.update(fields)
    p = abi.GatherParams(*[f[k] for k, _ in abi.GatherParams._fields_])
    m = max(n, 1) if n < 1024 else 1  # the large counts are refused or stop at the NULL scene before a point is read
    pts = np.zeros((m, 3), np.float32) if points is None else points
    nrm = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (m, 1)) if normals is None else normals
    small = np.zeros(128, np.float32)  # never written: every call here is refused
    val, se, sh = (small.ctypes.data if o else None for o in outs)
    args = [None, C.byref(p) if params else None, pts.ctypes.data if has_points else None, nrm.ctypes.data if has_normals else None,
            None if time is None else time.ctypes.data, val, se, sh]
    if entry == "rtmi_gather":
        args.append(None)
    else:
        args += [small.ctypes.data if scratch[0] else None, scratch[1], None]
    rc = getattr(lib, entry)(*args)
    return rc, (lib.rtmi_last_error() or b"").decode()


@pytest.mark.parametrize("entry", ENTRIES[:2])
def test_argument_errors_before_any_device_work(entry):
    def refused(code, word, **kw):
        rc, msg = _call(entry, **kw)
        assert rc == code and msg.startswith(entry + ":") and word in msg, (kw, rc, msg)

    SPH = abi.RTMI_GATHER_SPHERE
    refused(1, "scene")  # every value valid: the NULL scene is refused
    refused(1, "scene", n=0)  # an empty batch still needs a handle
    refused(1, "params", params=False)
    refused(1, "points", has_points=False)
    refused(1, "normals", has_normals=False)
    refused(1, "scene", has_normals=False, mode=SPH)  # SPHERE reads no normals
    for flag in (abi.RTMI_FLAG_SYNC, abi.RTMI_FLAG_PATH_SIG, abi.RTMI_FLAG_REF_TREE, abi.RTMI_FLAG_PROFILE, 1 << 11, 1 << 18, 1 << 20):
        refused(2, "flags", flags=flag | abi.RTMI_FLAG_FAST_CULL)
    accepted = abi.RTMI_FLAG_FAST_CULL | abi.RTMI_FLAG_SKY | abi.RTMI_FLAG_FACE_FORWARD | abi.RTMI_FLAG_UV_BOOK
    refused(1, "scene", flags=accepted)  # the accepted flags reach the scene check
    refused(1, "spp", spp=0)
    refused(1, "spp", spp=2 ** 31)
    refused(1, "max_depth", max_depth=0)
    refused(1, "t_min", t_min=float("nan"))
    refused(1, "mode", mode=2)
    refused(1, "estimator", estimator=4)
    refused(1, "sh output", outs=(True, True, True))  # COSINE has no sh
    refused(1, "scene", outs=(False, False, True), mode=SPH)
    refused(1, "output", outs=(False, False, False))
    refused(1, "scene", outs=(False, True, False))  # any one output is enough
    # the overflow rules: no index may wrap onto another point's or sample's stream
    refused(1, "first_point", first_point=2 ** 32 - 3)
    refused(1, "first_point", first_point=2 ** 32 + 1, n=0)
    refused(1, "first_point", first_point=2 ** 64 - 1)
    refused(1, "scene", first_point=2 ** 32 - 4)  # first_point + n == 2^32 is the last batch that fits
    refused(1, "first_sample", first_sample=2 ** 32 - 1)
    refused(1, "scene", first_sample=2 ** 32 - 2)
    # no n * spp limit: 2^47 paths reach the scene check (the device form reads no point before it)
    if entry == "rtmi_gather_device":
        refused(1, "scene", n=2 ** 32 - 1, spp=2 ** 15, scratch=(True, 12 << 15))
    # the estimator's own
    for bad in (0.0, -0.5, 1.5, float("nan")):
        refused(1, "env_select_p", estimator=abi.RTMI_ROULETTE_ENV_NEE, env_select_p=bad)
    refused(1, "scene", estimator=abi.RTMI_ROULETTE_ENV, env_select_p=0.0)  # read by ENV_NEE only
    for est in (abi.RTMI_ROULETTE_ENV, abi.RTMI_ROULETTE_ENV_NEE):
        refused(1, "SKY", estimator=est, flags=abi.RTMI_FLAG_SKY)
    if entry == "rtmi_gather_device":
        refused(1, "scratch", scratch=(True, 23))  # 12 * spp = 24 bytes hold one point
        refused(1, "scene", scratch=(True, 24))
        refused(1, "scratch", scratch=(False, 1 << 20))
        refused(1, "scene", n=0, scratch=(False, 0))


def test_bad_points_are_named_before_any_device_work():
    """the host form validates every point and normal; the device form takes the caller's word"""
    def pts(i, v):
        a = np.zeros((4, 3), np.float32)
        a[i] = v
        return a

    unit = np.tile(np.array([0.0, 1.0, 0.0], np.float32), (4, 1))
    cases = [(dict(points=pts(2, (0.0, np.inf, 0.0))), "point 2 has a non-finite"),
             (dict(points=pts(3, (np.nan, 0.0, 0.0))), "point 3 has a non-finite"),
             (dict(time=np.array([0.0, np.nan, 0.0, 0.0], np.float32)), "point 1 has a non-finite"),
             (dict(normals=pts(1, (0.0, 0.0, 0.0)) + unit * (np.arange(4) != 1)[:, None].astype(np.float32)), "point 1 has a zero or non-finite normal"),
             (dict(normals=np.where(np.arange(4)[:, None] == 2, np.float32(np.nan), unit)), "point 2 has a zero or non-finite normal"),
             (dict(normals=np.where(np.arange(4)[:, None] == 0, np.float32(1e-30), unit)), "point 0 has a zero or non-finite normal"),
             (dict(normals=np.where(np.arange(4)[:, None] == 3, np.float32(1e30), unit)), "point 3 has a zero or non-finite normal")]
    for kw, word in cases:
        kw = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in kw.items()}
        rc, msg = _call("rtmi_gather", **kw)
        assert rc == 1 and msg.startswith("rtmi_gather: ") and word in msg, (word, msg)
        rc, msg = _call("rtmi_gather_device", **kw)
        assert rc == 1 and "scene" in msg, msg
    # SPHERE reads no normal: a zero one passes
    rc, msg = _call("rtmi_gather", normals=np.zeros((4, 3), np.float32), mode=abi.RTMI_GATHER_SPHERE)
    assert rc == 1 and "scene" in msg, msg


def test_directions_entry_refusals():
    lib = abi.load_rtmi()
    nrm = np.tile(np.array([0.0, 0.0, 2.0], np.float32), (4, 1))
    out = np.zeros((4, 2, 3), np.float32)

    def call(n=4, params=True, normals=nrm, has_out=True, **fields):
        f = dict(n=0, spp=2, mode=0, estimator=0, flags=0, max_depth=1, t_min=0.0, seed=1, first_point=0, first_sample=0,
                 slab_points=0, env_select_p=0.0)
        f.update(fields)
        p = abi.GatherParams(*[f[k] for k, _ in abi.GatherParams._fields_])
        rc = lib.rtmi_gather_directions(C.byref(p) if params else None, None if normals is None else normals.ctypes.data, n,
                                        out.ctypes.data if has_out else None)
        return rc, (lib.rtmi_last_error() or b"").decode()

    assert call()[0] == 0
    assert call(n=0, normals=None, has_out=False)[0] == 0
    assert call(normals=None, mode=1)[0] == 0
    for kw, word in ((dict(params=False), "params"), (dict(normals=None), "normals"), (dict(has_out=False), "out_dirs"),
                     (dict(mode=2), "mode"), (dict(spp=0), "spp"), (dict(first_point=2 ** 32 - 3), "first_point"),
                     (dict(first_sample=2 ** 32 - 1), "first_sample"),
                     (dict(normals=np.zeros((4, 3), np.float32)), "point 0 has a zero or non-finite normal")):
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("rtmi_gather_directions: ") and word in msg, (kw, msg)
