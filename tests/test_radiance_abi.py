"""The radiance queries' public interface (include/rtmi_radiance.h), without a GPU.

* the header compiles as C99 and rtmi_radiance_params has the size and offsets the kernels read it with, in the header,
  in ctypes and in sys.rs;
* librtmi.so and librt_host.so export the entries, abi.py and sys.rs declare them;
* every bad argument that needs no handle is refused before a device is touched, with its code and the entry's name
  (the missing attachments need a handle: tests/test_gpu_radiance.py);
* irradiance's direction generator: unit length, in the normal's hemisphere, cosine-distributed;
* the vectorised Philox of philox.py is the scalar one."""
import ctypes as C

import numpy as np
import pytest

import abi_kit as kit
from raytracing_rust_amd import abi, irradiance_directions, philox
from raytracing_rust_amd.host import RAY_DTYPE

ENTRIES = ["rtmi_radiance", "rtmi_radiance_device"]
OFFSETS = {"n": 0, "spp": 4, "estimator": 8, "flags": 12, "max_depth": 16, "t_min": 20, "seed": 24, "first_ray": 32,
           "first_sample": 40, "stream_skip": 44, "env_select_p": 48}


FAMILY = kit.Family("rtmi_radiance.h", ENTRIES, {"rtmi_radiance_params": (abi.RadianceParams, "RtmiRadianceParams", 56, OFFSETS)},
                    word="rtmi_radiance", includes=["rtmi.h", "rtmi_query.h", "rtmi_roulette.h"], host=("rth_radiance", "rth_radiance_device"),
                    word_also_in={"rtmi_gather.h": "includes the header and takes its estimator rules",
                                  "rtmi_sparse.h": "refers to the header's sample indexing in a comment"})


def test_header_is_c99_with_the_documented_layout(tmp_path):
    FAMILY.c99(tmp_path, holds="RTMI_ROULETTE_ENV_NEE == 3u")


def test_ctypes_and_rust_match_the_header():
    FAMILY.layout()
    kit.assert_plain_repr_c("RtmiRadianceParams")


def test_exports_and_declarations_agree():
    FAMILY.exports()


def test_the_header_keeps_to_itself():
    FAMILY.isolation()
    FAMILY.constants()


def _rays(n):
    r = np.zeros(max(n, 1), RAY_DTYPE)
    r["d"][:, 2] = 1.0
    r["t_min"] = 0.001
    r["t_max"] = np.inf
    return r


def _call(entry, n=4, rays=None, params=True, has_rays=True, outs=(True, True, True), **fields):
    """the entry with a NULL scene and otherwise valid arguments, except what the keywords change"""
    lib = abi.load_rtmi()
    f = dict(n=n, spp=2, estimator=abi.RTMI_ROULETTE_PLAIN, flags=0, max_depth=50, t_min=0.001, seed=7, first_ray=0,
             first_sample=0, stream_skip=0, env_select_p=0.5)
    f.update(fields)
    p = abi.RadianceParams(*[f[k] for k, _ in abi.RadianceParams._fields_])
    r = _rays(n) if rays is None else rays
    small = np.zeros(16, np.float32)  # never written: every call here is refused
    mean, se, smp = (small.ctypes.data if o else None for o in outs)
    args = [None, C.byref(p) if params else None, r.ctypes.data if has_rays else None, None, mean, se, smp, None]
    rc = getattr(lib, entry)(*args)
    return rc, (lib.rtmi_last_error() or b"").decode()


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_before_any_device_work(entry):
    def refused(code, word, **kw):
        rc, msg = _call(entry, **kw)
        assert rc == code and msg.startswith(entry + ":") and word in msg, (kw, rc, msg)

    refused(1, "scene")  # every value valid: the NULL scene is refused
    refused(1, "scene", n=0)  # an empty batch still needs a handle
    refused(1, "params", params=False)
    refused(1, "rays", has_rays=False)
    for flag in (abi.RTMI_FLAG_SYNC, abi.RTMI_FLAG_PATH_SIG, abi.RTMI_FLAG_REF_TREE, abi.RTMI_FLAG_PROFILE, 1 << 11, 1 << 20):
        refused(2, "flags", flags=flag | abi.RTMI_FLAG_FAST_CULL)
    accepted = abi.RTMI_FLAG_FAST_CULL | abi.RTMI_FLAG_SKY | abi.RTMI_FLAG_FACE_FORWARD | abi.RTMI_FLAG_UV_BOOK
    refused(1, "scene", flags=accepted)  # the accepted flags reach the scene check
    refused(1, "spp", spp=0)
    refused(1, "max_depth", max_depth=0)
    refused(1, "estimator", estimator=4)
    # the overflow rules: no index may wrap onto another ray's or sample's stream
    refused(1, "first_ray", first_ray=2 ** 32 - 3)
    refused(1, "first_ray", first_ray=2 ** 32 + 1, n=0)
    refused(1, "first_ray", first_ray=2 ** 64 - 1)
    refused(1, "scene", first_ray=2 ** 32 - 4)  # first_ray + n == 2^32 is the last batch that fits
    refused(1, "first_sample", first_sample=2 ** 32 - 1)
    refused(1, "scene", first_sample=2 ** 32 - 2)
    refused(1, "n * spp", n=2 ** 16, spp=2 ** 15)
    refused(1, "scene", n=2 ** 16, spp=2 ** 15 - 1)  # 2^31 - 2^16 paths: accepted (nothing is written: no handle)
    # the estimator's own
    for bad in (0.0, -0.5, 1.5, float("nan")):
        refused(1, "env_select_p", estimator=abi.RTMI_ROULETTE_ENV_NEE, env_select_p=bad)
    refused(1, "scene", estimator=abi.RTMI_ROULETTE_ENV, env_select_p=0.0)  # read by ENV_NEE only
    for est in (abi.RTMI_ROULETTE_ENV, abi.RTMI_ROULETTE_ENV_NEE):
        refused(1, "SKY", estimator=est, flags=abi.RTMI_FLAG_SKY)
    if entry == "rtmi_radiance":
        refused(1, "output", outs=(False, False, False))
        refused(1, "scene", outs=(False, True, False))  # any one output is enough
    else:
        refused(1, "d_samples", outs=(True, True, False))
        refused(1, "scene", outs=(False, False, True))  # mean and stderr are optional


def test_bad_rays_are_named_before_any_device_work():
    """the host form validates every ray as rtmi_trace does; the device form takes the caller's word"""
    for field, value, word in (("d", (0.0, 0.0, 0.0), "zero direction"), ("d", (0.0, np.nan, 1.0), "non-finite"),
                               ("o", (np.inf, 0.0, 0.0), "non-finite"), ("t_min", np.nan, "non-finite"),
                               ("t_max", np.nan, "non-finite"), ("t_min", 2.0, "t_min > t_max")):
        r = _rays(4)
        if field == "t_min" and value == 2.0:
            r["t_max"][2] = 1.0
        r[field][2] = value
        rc, msg = _call("rtmi_radiance", rays=r)
        assert rc == 1 and msg.startswith("rtmi_radiance: ray 2 ") and word in msg, (field, msg)
        rc, msg = _call("rtmi_radiance_device", rays=r)
        assert rc == 1 and "scene" in msg, msg


def test_irradiance_directions_are_cosine_distributed():
    nrm = np.array([[0.0, 0.0, 1.0], [0.0, -3.0, 0.0], [1.0, 1.0, 1.0], [-0.2, 0.9, -0.4]])
    d = irradiance_directions(nrm, 4096, seed=5)
    assert d.shape == (4, 4096, 3) and d.dtype == np.float32
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=2) - 1.0).max() <= 1e-6
    unit = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    cos = np.einsum("nkc,nc->nk", d.astype(np.float64), unit)
    assert cos.min() >= -1e-7  # in the normal's hemisphere (cos = 0 is the draw u1 = 1 - 2^-24 .. 1, rounded)
    # E[cos] = 2/3 under the density cos / pi; each point's mean within 3 of its own standard errors
    se = cos.std(axis=1, ddof=1) / np.sqrt(cos.shape[1])
    assert np.all(np.abs(cos.mean(axis=1) - 2.0 / 3.0) <= 3.0 * se), (cos.mean(axis=1), se)
    # the azimuth is uniform: no preferred tangent direction
    tangent = d.astype(np.float64) - cos[..., None] * unit[:, None, :]
    assert np.abs(tangent.mean(axis=1)).max() < 0.03
    # another seed, other directions; the same seed, the same
    assert not np.array_equal(d, irradiance_directions(nrm, 4096, seed=6))
    assert np.array_equal(d, irradiance_directions(nrm, 4096, seed=5))
    # point i's directions do not depend on the other points
    assert np.array_equal(d[:2, :7], irradiance_directions(nrm[:2], 7, seed=5))


def test_vectorised_philox_is_the_scalar_one():
    rng = np.random.default_rng(1)
    c = rng.integers(0, 2 ** 32, (4, 50), dtype=np.uint64).astype(np.uint32)
    seed = (0x9E3779B9 << 32) | 0x12345678
    got = philox.philox4x32_10_np(c[0], c[1], c[2], c[3], seed)
    for k in range(50):
        want = philox.philox4x32_10([int(c[j, k]) for j in range(4)], [seed & 0xFFFFFFFF, seed >> 32])
        assert [int(w[k]) for w in got] == want, k
