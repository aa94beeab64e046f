"""First-hit features' public interface (include/rtmi_features.h), without a GPU.

* the header compiles as C99;
* librtmi.so and librt_host.so export the functions the header declares, and abi.py and sys.rs declare them;
* every bad argument is refused before any device work: RTMI_ERR_INVALID for bad values and a NULL scene, camera or
  params, RTMI_ERR_UNSUPPORTED for the flags and the tile split the features do not carry;
* pfm_bytes writes the PFM a denoiser reads: header, negative (little-endian) scale, rows bottom to top."""
import ctypes as C

import numpy as np
import pytest

import abi_kit as kit
from raytracing_rust_amd import abi, pfm_bytes
from raytracing_rust_amd.host import default_params


# isolated=False: the denoiser, the frame pipeline and the upscaler all say which first-hit features they read
FAMILY = kit.Family("rtmi_features.h", ["rtmi_render_features"], word="features", isolated=False, host=("rth_render_features",))


def test_header_is_c99(tmp_path):
    FAMILY.c99(tmp_path)


def test_exports_and_declarations_agree():
    FAMILY.exports()
    FAMILY.layout()  # the header defines no struct
    FAMILY.isolation()
    FAMILY.constants()


def _call(params=None, scene=None, cam=True, params_null=False):
    lib = abi.load_rtmi()
    p = default_params(32, 24, 16) if params is None else params
    c = abi.Camera()
    rc = lib.rtmi_render_features(scene, C.byref(c) if cam else None, None if params_null else C.byref(p), None, None, None,
                                  None, None, None)
    return rc, (lib.rtmi_last_error() or b"").decode()


def test_null_arguments_and_bad_params_are_invalid():
    rc, msg = _call()
    assert rc == 1 and "scene" in msg, msg  # every value valid: the NULL scene is what is refused
    rc, msg = _call(cam=False)
    assert rc == 1 and "NULL" in msg, msg
    rc, msg = _call(params_null=True)
    assert rc == 1 and "NULL" in msg, msg
    for bad in (default_params(0, 24, 16), default_params(32, 0, 16), default_params(32, 24, 0)):
        rc, msg = _call(params=bad)
        assert rc == 1 and "positive" in msg, msg
    rc, msg = _call(params=default_params(32, 24, 16, tile_rank=2, tile_world=2))
    assert rc == 1 and "tile_rank" in msg, msg


@pytest.mark.parametrize("flag", [abi.RTMI_FLAG_PROFILE, abi.RTMI_FLAG_ASYNC, abi.RTMI_FLAG_BLOCK_COOP,
                                  abi.RTMI_FLAG_PROGRESSIVE, abi.RTMI_FLAG_TEST_OVERFLOW, 1 << 11, 3 << 8, 1 << 20])
def test_unsupported_flags(flag):
    rc, msg = _call(params=default_params(32, 24, 16, flags=flag | abi.RTMI_FLAG_FAST_CULL))
    assert rc == 2 and "flags" in msg, msg


def test_tile_split_is_unsupported():
    rc, msg = _call(params=default_params(32, 24, 16, tile_rank=1, tile_world=2))
    assert rc == 2 and "tile_world" in msg, msg


def test_accepted_flags_reach_the_scene_check():
    accepted = (abi.RTMI_FLAG_FAST_CULL | abi.RTMI_FLAG_SYNC | abi.RTMI_FLAG_REF_TREE | abi.RTMI_FLAG_SKY |
                abi.RTMI_FLAG_FACE_FORWARD | abi.RTMI_FLAG_UV_BOOK | abi.RTMI_FLAG_PATH_SIG)
    rc, msg = _call(params=default_params(32, 24, 16, flags=accepted))
    assert rc == 1 and "scene" in msg, msg


def _read_pfm(data):
    tag, dims, scale, body = data.split(b"\n", 3)
    nx, ny = map(int, dims.split())
    ch = {b"PF": 3, b"Pf": 1}[tag]
    a = np.frombuffer(body, dtype="<f4" if float(scale) < 0 else ">f4")
    assert a.size == nx * ny * ch
    a = a.reshape((ny, nx, 3) if ch == 3 else (ny, nx))
    return tag, float(scale), a[::-1]  # the file's first row is the bottom one


def test_pfm_round_trip_colour():
    rng = np.random.default_rng(7)
    img = rng.standard_normal((5, 7, 3)).astype(np.float32)
    img[0, 0] = (np.inf, -0.0, np.nan)
    data = pfm_bytes(img)
    assert data.startswith(b"PF\n7 5\n-1.0\n")
    tag, scale, back = _read_pfm(data)
    assert tag == b"PF" and scale < 0
    assert back.tobytes() == img.tobytes()
    # rows bottom to top: the first row in the file is the image's last (bottom) row
    body = data[len(b"PF\n7 5\n-1.0\n"):]
    assert body[:7 * 3 * 4] == img[4].astype("<f4").tobytes()
    assert body[-7 * 3 * 4:] == img[0].astype("<f4").tobytes()


def test_pfm_round_trip_grey_and_dtype():
    plane = np.arange(12, dtype=np.float64).reshape(3, 4)  # converted to float32
    data = pfm_bytes(plane)
    assert data.startswith(b"Pf\n4 3\n-1.0\n") and len(data) == len(b"Pf\n4 3\n-1.0\n") + 12 * 4
    tag, scale, back = _read_pfm(data)
    assert tag == b"Pf" and scale == -1.0
    assert np.array_equal(back, plane.astype(np.float32))


@pytest.mark.parametrize("shape", [(4,), (2, 3, 4), (2, 3, 1), (1, 2, 3, 3)])
def test_pfm_refuses_other_shapes(shape):
    with pytest.raises(ValueError):
        pfm_bytes(np.zeros(shape, np.float32))
