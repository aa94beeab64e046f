"""The f64 render mode (include/rtmi_f64.h) against the f64 restatement of the reference (oracle, THROUGHPUT_FORM).

The mode traces the reference's paths in double with its literal arithmetic and the same Philox streams.  Beyond
+ - * / and sqrt, which both sides round correctly, only sin (checker, noise), log (media), atan2 and asin (sphere uv)
are evaluated at render time, on the device by the device math library (the sine below 2^40 by csrc/rtmi_sin_f64.hpp, the
correctly rounded one: tests/test_sin_f64.py) and in the oracle by glibc.  Hence:
  * a scene that evaluates none of the four (cornell_box: rects, boxes, rotations, solid Lambertian, a light) is
    bit-identical — double radiance, rgb8 and path signatures;
  * other scenes differ by the ULPs of those four functions: the figures are printed and bounded.
Reference loop: tests/test.rs:62-78, color_throughput of oracle/rt_oracle.c."""
import ctypes as C
import json

import numpy as np
import pytest

from oracle.oracle import THROUGHPUT_FORM, Oracle
from oracle.parallel import render_parallel
from raytracing_rust_amd import abi

import scenes_extra

pytestmark = pytest.mark.gpu


def _probe(op, x, y=None):
    lib = abi.load_rtmi()
    x = np.ascontiguousarray(x, np.float64)
    y = np.ascontiguousarray(x if y is None else y, np.float64)
    out = np.zeros_like(x)
    assert lib.rtmi_probe_math_f64(op, x.ctypes.data, y.ctypes.data, out.ctypes.data, len(x)) == 0, lib.rtmi_last_error()
    return out


def _ulps(a, b):
    """distance in units in the last place (same-sign finite doubles; NaN pairs count 0, a NaN against a number huge)"""
    both_nan = np.isnan(a) & np.isnan(b)
    ia, ib = a.view(np.int64), b.view(np.int64)
    ia = np.where(ia < 0, np.int64(-2**63) - ia, ia)  # monotone integer image of the doubles
    ib = np.where(ib < 0, np.int64(-2**63) - ib, ib)
    with np.errstate(over="ignore"):
        d = np.abs(ia - ib).astype(np.float64)  # exact in int64 for operands of one sign
    d[both_nan] = 0
    d[np.isnan(a) ^ np.isnan(b)] = np.inf
    return d


def _edges():
    tiny = np.finfo(np.float64).tiny
    return np.array([0.0, -0.0, 5e-324, -5e-324, tiny, -tiny, tiny / 3, 1e-300, 1e-16, 0.5, 1.0, -1.0, 1.0 - 2**-53,
                     np.pi, -np.pi, 1e8, 1e15, 1.7e308, -1.7e308, np.inf, -np.inf, np.nan])


def test_math_probe_div_sqrt_exact_and_transcendentals_bounded():
    rng = np.random.default_rng(7)
    n = 1 << 20
    x = np.concatenate([_edges(), rng.standard_normal(n) * 10.0 ** rng.uniform(-300, 300, n)])
    y = np.concatenate([_edges()[::-1], rng.standard_normal(n) * 10.0 ** rng.uniform(-300, 300, n)])
    with np.errstate(all="ignore"):
        assert np.array_equal(_probe(4, x, y), x / y, equal_nan=True)
        assert np.array_equal(_probe(5, x), np.sqrt(x), equal_nan=True)
        # the arguments the render evaluates: sin of 10 p (checker) and of scale*p.x + 5 turb (noise), log of a uniform
        # in (0, 1] (media), atan2 / asin of a unit normal's components (sphere uv)
        xs = np.concatenate([_edges()[:-3], rng.uniform(-2000, 2000, n)])
        xl = np.concatenate([np.array([5e-324, 2.0**-1074 * 3, 2.0**-24, 0.5, 1.0]), rng.uniform(0, 1, n)])
        xa = np.concatenate([np.array([0.0, -0.0, 1.0, -1.0, 5e-324]), rng.uniform(-1, 1, n)])
        ya = np.concatenate([np.array([0.0, -0.0, -1.0, 1.0, -5e-324]), rng.uniform(-1, 1, n)])
        m = {"sin": float(_ulps(_probe(0, xs), np.sin(xs)).max()), "log": float(_ulps(_probe(1, xl), np.log(xl)).max()),
             "atan2": float(_ulps(_probe(2, xa, ya), np.arctan2(xa, ya)).max()),
             "asin": float(_ulps(_probe(3, xa), np.arcsin(xa)).max())}
    print(json.dumps({"max_ulp_vs_numpy": m}))
    # measured (MI355X): sin 1, log 1, atan2 2, asin 1 ULP from numpy (glibc) over these inputs
    for k, v in m.items():
        assert v <= 2, (k, v)


def _f64_render(host, name, nx, ny, ns, **kw):
    cam, world = scenes_extra.build(host, name, nx, ny, seed=1)
    sc = host.lower(world).upload(0, f64=True)
    return sc.render(cam, nx, ny, ns, sig=True, seed=42, precision="f64", **kw)


@pytest.mark.parametrize("budget", [0, 24 * 18 * 32 * 64 * 5])  # default, and five samples per pass (passes)
def test_cornell_box_bit_identical_to_the_f64_oracle(host, budget):
    nx, ny, ns = 256, 144, 56
    got = _f64_render(host, "cornell_box", nx, ny, ns, sample_buffer_bytes=budget)
    ref = render_parallel("scenes_extra", "cornell_box", nx, ny, ns, 42, THROUGHPUT_FORM, precision="f64", timeout=1500)
    assert got["linear"].dtype == np.float64
    assert float(ref["mean"].mean()) > 0.01
    assert np.array_equal(got["linear"], ref["mean"]), np.abs(got["linear"] - ref["mean"]).max()
    assert np.array_equal(got["rgb8"].astype(np.int32), ref["rgb"])
    assert np.array_equal(got["sig"], ref["sig"])


@pytest.mark.parametrize("name", ["two_spheres", "random_spheres", "cornell_smoke", "final_scene", "lit_final_scene", "earth"])
def test_scenes_with_transcendentals_within_ulps_of_the_f64_oracle(host, name):
    nx, ny, ns = 256, 144, 56
    got = _f64_render(host, name, nx, ny, ns)
    ref = render_parallel("scenes_extra", name, nx, ny, ns, 42, THROUGHPUT_FORM, precision="f64", timeout=1500)
    d = np.abs(got["linear"] - ref["mean"])
    res = {"scene": "%s %dx%dx%d" % (name, nx, ny, ns), "sig_mismatch": float((got["sig"] != ref["sig"]).mean()),
           "share_within_1e-12_rel": float((d <= 1e-12 * np.maximum(1.0, np.abs(ref["mean"]))).mean()),
           "rgb8_mismatch": float((got["rgb8"].astype(np.int32) != ref["rgb"]).mean()), "max_abs": float(d.max())}
    print(json.dumps(res))
    # measured (MI355X): signatures differ on 13 / 12 of 36864 pixels of final_scene / lit_final_scene (a t that moves by an
    # ULP rounds to another float), none elsewhere; 99.999 % of the channels within 1e-12 relative (max |d| 1.2e-12, on
    # lit_final_scene), all of them elsewhere; rgb8 identical
    assert res["sig_mismatch"] <= 1e-3
    assert res["share_within_1e-12_rel"] >= 0.9999
    assert res["rgb8_mismatch"] <= 5e-4


def test_c3_cornell_box_fullsize_against_the_f64_literal(host):
    """BASELINE C3 (cornell_box 800x800x1000), 16 evenly spaced rows, against the literal restatement (flags 0: the
    recursive color of src/color.rs:6-23).  The mode sums L = sum T_k e_k iteratively; the recursion nests the same products
    in another order, so the two differ by rounding only — the figures of test_gpu_f64_tolerance.py, for this mode."""
    nx, ny, ns = 800, 800, 1000
    rows = [int((k + 0.5) * ny / 16) for k in range(16)]
    got = _f64_render(host, "cornell_box", nx, ny, ns)
    ref = render_parallel("scenes_extra", "cornell_box", nx, ny, ns, 42, 0, precision="f64", rows=rows, timeout=1500)
    d = np.abs(got["linear"][rows] - ref["mean"][rows])
    lev = np.abs(got["rgb8"][rows].astype(np.int32) - ref["rgb"][rows])
    mean_ref = float(ref["mean"][rows].mean())
    res = {"scene": "cornell_box %dx%dx%d" % (nx, ny, ns), "rows": len(rows), "mean_radiance_f64": mean_ref,
           "image_mean_rel_err": abs(float(got["linear"][rows].mean()) - mean_ref) / mean_ref,
           "share_within_1e-4": float((d <= 1e-4).mean()), "share_within_1e-12": float((d <= 1e-12).mean()),
           "max_abs": float(d.max()), "ppm_values_differing": float((lev > 0).mean()),
           "sig_mismatch": float((got["sig"][rows] != ref["sig"][rows]).mean())}
    print(json.dumps(res))
    assert mean_ref > 0.05
    # measured (MI355X): every channel within 1e-4 (max |d| 1.1e-16), no PPM value and no signature differs
    assert res["share_within_1e-4"] >= 0.9999  # the fp32 path: 0.985 (test_gpu_f64_tolerance.py)
    assert res["sig_mismatch"] == 0.0
    assert res["ppm_values_differing"] <= 1e-4


def test_error_paths_and_isolation(host):
    lib = abi.load_rtmi()
    nx, ny, ns = 32, 24, 4
    cam, world = scenes_extra.build(host, "cornell_box", nx, ny, seed=1)
    sc = host.lower(world).upload(0)
    from raytracing_rust_amd.host import HostError
    a = sc.render(cam, nx, ny, ns, seed=42)
    sc.attach_f64()
    b = sc.render(cam, nx, ny, ns, seed=42)  # an fp32 render is unaffected by attached planes
    assert np.array_equal(a["linear"], b["linear"]) and np.array_equal(a["rgb8"], b["rgb8"])
    for flag in (abi.RTMI_FLAG_PROGRESSIVE, abi.RTMI_FLAG_ASYNC, abi.RTMI_FLAG_BLOCK_COOP, abi.RTMI_FLAG_PROFILE,
                 abi.RTMI_FLAG_TEST_OVERFLOW):
        with pytest.raises(HostError, match="not supported in the f64 mode"):
            sc.render(cam, nx, ny, ns, seed=42, flags=flag, precision="f64")
    # counts that do not match the handle: RTMI_ERR_INVALID, straight through the C ABI
    w = sc.desc_f64()
    w.n_prims += 1
    handle = C.c_void_p()
    d = sc.desc()
    assert lib.rtmi_scene_create(C.byref(d), 0, C.byref(handle)) == 0
    try:
        # a render without attached planes: RTMI_ERR_INVALID
        p = abi.RenderParams()
        p.nx, p.ny, p.ns, p.max_depth, p.tile_world, p.seed = nx, ny, ns, 50, 1, 42
        c64 = cam.lower_f64()
        lin = np.zeros((ny, nx, 3))
        assert lib.rtmi_render_f64(handle, C.byref(c64), C.byref(p), 0.001, lin.ctypes.data, None, None, None) == 1
        assert b"no f64 planes" in lib.rtmi_last_error()
        assert lib.rtmi_scene_attach_f64(handle, C.byref(w)) == 1
        w.n_prims -= 1
        w.prim_a = None
        assert lib.rtmi_scene_attach_f64(handle, C.byref(w)) == 1
    finally:
        lib.rtmi_scene_destroy(handle)


def test_deferred_scene_is_unsupported(host):
    # a ConstantMedium that is a child of a BVHNode becomes a DEFERRED item (rtmi.h)
    red = host.Lambertian(host.SolidTexture(0.5, 0.2, 0.2))
    fog = host.ConstantMedium(host.Sphere((0.0, 0.0, 0.0), 1.0, red), 0.5, host.SolidTexture(1.0, 1.0, 1.0))
    ball = host.Sphere((3.0, 0.0, 0.0), 1.0, red)
    world = host.HittableList()
    world.push(host.BVHNode([fog, ball], 0.0, 1.0))
    cam = host.Camera((0.0, 0.0, 10.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 10.0, 0.0, 1.0)
    sc = host.lower(world).upload(0, f64=True)
    assert any(it.flags & 8 for it in sc.arrays()["items"])
    from raytracing_rust_amd.host import HostError
    with pytest.raises(HostError, match="not supported in the f64 mode"):
        sc.render(cam, 16, 16, 2, precision="f64")


def test_camera_render_f64_ppm_equals_the_oracle(host):
    nx, ny, ns = 48, 32, 8
    cam, world = scenes_extra.build(host, "cornell_box", nx, ny, seed=1)
    got = cam.render(world, nx, ny, ns, seed=42, precision="f64")
    lib = abi.load_rtmi()
    need = lib.rtmi_ppm_p3(nx, ny, got["rgb8"].ctypes.data, None, 0)
    buf = C.create_string_buffer(need)
    n = lib.rtmi_ppm_p3(nx, ny, got["rgb8"].ctypes.data, buf, need)
    orc = Oracle("f64")
    ocam, oworld = scenes_extra.build(orc, "cornell_box", nx, ny, seed=1)
    ref = orc.render(ocam, oworld, nx, ny, ns, seed=42, flags=THROUGHPUT_FORM)
    assert buf.raw[:n] == orc.ppm_text(ref["rgb"])
    orc.free_all()
