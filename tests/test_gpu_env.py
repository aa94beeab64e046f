"""Environment lighting (include/rtmi_env.h) on the device.

1. rtmi_probe_env equals tests/env_ref.py bit for bit (radiance, direction, pdf);
2. reductions: nee=0 has render()'s signatures, an all-zero map is render() (nee=0) and render_nee() (nee=1) bit for bit;
3. env_from_sky is RTMI_FLAG_SKY within its interpolation error;
4. a furnace: a Lambertian sphere under a constant map;
5. a known answer: a Lambertian floor under the sun map;
6. nee=1 has nee=0's expectation;
7. independence from the schedule, no effect on the other renders, render_denoised(env=True)."""
import ctypes as C
import math

import numpy as np
import pytest

import env_ref as ref
import scenes_extra
from test_gpu_nee import _tile_z
from raytracing_rust_amd import abi, env_from_sky, scenes
from raytracing_rust_amd.host import HostError, default_params

FC = abi.RTMI_FLAG_FAST_CULL
SEED = 42


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _build(host, name, nx, ny):
    if name in scenes.SCENES:
        return scenes.build(host, name, nx, ny, seed=1)
    return scenes_extra.build(host, name, nx, ny, seed=7 if name == "lit_random_spheres" else 1)


def _earth_map():
    data, w, h = scenes.earthmap_rgb8()
    return (np.asarray(data, np.float32).reshape(h, w, 3) / np.float32(255.0)).astype(np.float32)


def _maps():
    rng = np.random.default_rng(11)
    return {"1x1": np.float32([[[0.25, 2.0, 0.5]]]), "3x2": rng.random((2, 3, 3)).astype(np.float32),
            "64x32": (rng.random((32, 64, 3)) ** 4 * 10).astype(np.float32), "sun": ref.sun_map(),
            "zero": np.zeros((8, 16, 3), np.float32), "earth": _earth_map()}


# ---- 1. the probe is bit-exact --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_probe_bit_exact(host):
    M = ref.ContractMath()
    cam, world = _build(host, "random_spheres", 16, 16)
    sc = host.lower(world).upload(0)
    rng = np.random.default_rng(9)
    n_total = 0
    for name, m in _maps().items():
        h, w = m.shape[:2]
        T = ref.tables(m)
        p_env = 1.0 if T["total"] > 0 else 0.0
        sc.attach_env(m)
        d = ref.lat_long_dirs(85000, rng)
        got = sc.probe_env(abi.RTMI_ENV_PROBE_LOOKUP, d)
        want = ref.lookup(M, m, T, d, p_env)
        bad = np.nonzero(np.any(got.view(np.uint32) != want.view(np.uint32), axis=1))[0]
        assert bad.size == 0, (name, "lookup", bad.size, d[bad[:3]], got[bad[:3]], want[bad[:3]])
        u = ref.uniforms(85000, rng)
        got = sc.probe_env(abi.RTMI_ENV_PROBE_SAMPLE, u)
        want = ref.sample(M, T, w, h, u[:, 0], u[:, 1], p_env)
        bad = np.nonzero(np.any(got.view(np.uint32) != want.view(np.uint32), axis=1))[0]
        assert bad.size == 0, (name, "sample", bad.size, u[bad[:3]], got[bad[:3]], want[bad[:3]])
        if p_env > 0:
            assert np.mean(want[:, 3] > 0) > 0.999
        n_total += len(d) + len(u)
    assert n_total > 1_000_000


# ---- 2. reductions --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["random_spheres", "cornell_box"])
def test_nee_off_has_render_signatures_and_zero_map_is_render(host, name):
    nx, ny, ns = 48, 32, 8
    cam, world = _build(host, name, nx, ny)
    sc = host.lower(world).upload(0)
    r = sc.render(cam, nx, ny, ns, sig=True, seed=SEED, flags=FC)
    sc.attach_env(ref.sun_map())
    e = sc.render_env(cam, nx, ny, ns, nee=False, sig=True, seed=SEED, flags=FC)
    assert _same(e["sig"], r["sig"])
    sc.attach_env(np.zeros((4, 8, 3), np.float32))
    z = sc.render_env(cam, nx, ny, ns, nee=False, sig=True, seed=SEED, flags=FC)
    for k in ("linear", "rgb8", "sig"):
        assert _same(z[k], r[k]), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_box", "lit_smoke", "lit_random_spheres"])
def test_zero_map_with_nee_is_render_nee(host, name):
    nx, ny, ns = 48, 32, 8
    cam, world = _build(host, name, nx, ny)
    sc = host.lower(world).upload(0, nee=True)
    n = sc.render_nee(cam, nx, ny, ns, sig=True, seed=SEED, flags=FC)
    sc.attach_env(np.zeros((16, 32, 3), np.float32))
    for p in (0.5, 1.0):
        e = sc.render_env(cam, nx, ny, ns, nee=True, env_select_p=p, sig=True, seed=SEED, flags=FC)
        for k in ("linear", "rgb8", "stderr", "sig"):
            assert _same(e[k], n[k]), (name, p, k)


# ---- 3. the sky as a map --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["random_spheres", "two_perlin_spheres"])
def test_sky_map_is_sky(host, name):
    nx, ny, ns = 96, 72, 16
    cam, world = _build(host, name, nx, ny)
    sc = host.lower(world).upload(0)
    r = sc.render(cam, nx, ny, ns, sig=True, seed=SEED, flags=FC | abi.RTMI_FLAG_SKY)
    sc.attach_env(env_from_sky(2048, 1024))
    e = sc.render_env(cam, nx, ny, ns, nee=False, sig=True, seed=SEED, flags=FC)
    assert _same(e["sig"], r["sig"])
    err = float(np.abs(e["linear"].astype(np.float64) - r["linear"]).max())
    print("\nENV-SKY %s max |d linear| %.3g" % (name, err))
    assert err <= 1e-5, err


# ---- 4. furnace -----------------------------------------------------------------------------------------------------------
def _sphere_scene(host, albedo):
    w = host.HittableList()
    w.push(host.Sphere((0.0, 0.0, 0.0), 1.0, host.Lambertian(host.SolidTexture(albedo, albedo, albedo))))
    cam = host.Camera((0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 1.0, 0.0, 1.0)
    return cam, w


@pytest.mark.gpu
def test_furnace(host):
    nx = ny = 64
    ns, a = 16, 0.5
    c = np.float32([0.8, 0.6, 0.4])
    cam, world = _sphere_scene(host, a)
    sc = host.lower(world).upload(0)
    sc.attach_env(np.broadcast_to(c, (32, 64, 3)).astype(np.float32))
    hits = sc.render_features(cam, nx, ny, ns, seed=SEED)["hits"]
    full, none = hits == ns, hits == 0
    assert full.sum() > 500 and none.sum() > 500
    e = sc.render_env(cam, nx, ny, ns, nee=False, seed=SEED)
    assert np.all(e["linear"][full] == np.float32(a) * c) and np.all(e["linear"][none] == c)
    n = sc.render_env(cam, nx, ny, 256, nee=True, seed=SEED)
    tiles = full.reshape(8, 8, 8, 8).all(axis=(1, 3))
    m = n["linear"].astype(np.float64).reshape(8, 8, 8, 8, 3).mean(axis=(1, 3))
    se = np.sqrt((n["stderr"].astype(np.float64) ** 2).reshape(8, 8, 8, 8, 3).sum(axis=(1, 3))) / 64
    z = (m - np.float64(a) * c) / se
    print("\nENV-FURNACE tiles %d max |z| %.2f" % (int(tiles.sum()), float(np.abs(z[tiles]).max())))
    assert tiles.sum() >= 4 and np.all(np.abs(z[tiles]) <= 4)


# ---- 5. sun known answer --------------------------------------------------------------------------------------------------
def _expected_floor(m, albedo, sub=8):
    """albedo * integral of env(w) (2/pi) cos^3 over the upper hemisphere: midpoint quadrature of the f64 bilinear map."""
    h, w = m.shape[:2]
    tex = m.astype(np.float64)
    u = (np.arange(w * sub) + 0.5) / (w * sub)
    v = 0.5 + (np.arange(h * sub // 2) + 0.5) / (h * sub)
    uu, vv = np.meshgrid(u, v)
    x, y = uu * w - 0.5, (1 - vv) * h - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    i0 = np.mod(x0.astype(int), w)
    i1 = np.mod(i0 + 1, w)
    j0, j1 = np.clip(y0.astype(int), 0, h - 1), np.clip(y0.astype(int) + 1, 0, h - 1)
    t0 = tex[j0, i0] + fx * (tex[j0, i1] - tex[j0, i0])
    t1 = tex[j1, i0] + fx * (tex[j1, i1] - tex[j1, i0])
    env = t0 + fy * (t1 - t0)
    lat = vv * math.pi - math.pi / 2
    wgt = (2 / math.pi) * np.sin(lat) ** 3 * 2 * math.pi ** 2 * np.cos(lat) / (w * sub * h * sub)
    return albedo * (env * wgt[..., None]).sum(axis=(0, 1))


@pytest.mark.gpu
def test_sun_known_answer(host):
    nx, ny, a = 32, 32, 0.5
    w = host.HittableList()
    w.push(host.Rect(host.PLANE_ZX, -1e4, -1e4, 1e4, 1e4, 0.0, host.Lambertian(host.SolidTexture(a, a, a))))
    cam = host.Camera((0.0, 1.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 30.0, 1.0, 0.0, 1.0, 0.0, 1.0)
    sc = host.lower(w).upload(0)
    m = ref.sun_map()
    sc.attach_env(m)
    want = _expected_floor(m, a)
    se_med = {}
    for nee, ns in ((False, 2048), (True, 256)):
        out = sc.render_env(cam, nx, ny, ns, nee=nee, seed=SEED)
        mt = out["linear"].astype(np.float64).reshape(4, 8, 4, 8, 3).mean(axis=(1, 3))
        st = np.sqrt((out["stderr"].astype(np.float64) ** 2).reshape(4, 8, 4, 8, 3).sum(axis=(1, 3))) / 64
        z = (mt - want) / st
        se_med[nee] = float(np.median(out["stderr"].mean(-1))) * math.sqrt(ns)  # per-sample sigma
        print("\nENV-SUN nee=%d ns %d want %s mean %s max |z| %.2f sigma/sample %.4g" % (
            nee, ns, np.array2string(want, precision=5), np.array2string(mt.mean((0, 1)), precision=5),
            float(np.abs(z).max()), se_med[nee]))
        assert np.all(np.abs(z) <= 4), (nee, float(np.abs(z).max()))
    # at equal sample counts nee=1's standard error is at most half nee=0's
    assert se_med[True] <= 0.5 * se_med[False], se_med


# ---- 6. same expectation --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,mapname,p", [("random_spheres", "sun", 0.5), ("earth", "earth", 0.5),
                                            ("lit_random_spheres", "sun", 0.5)])
def test_same_expectation(host, name, mapname, p):
    """8x8-tile z-scores of nee=1 at 512 spp against nee=0.  Under the sun map nee=0 finds the sun by rare BSDF hits: at
    512 spp a tile may catch none, and its Welford standard error then misses the sun's share (|z| 13 seen); nee=0 takes
    16x the samples there.  A tile where nee=0's samples have no variance at all (only camera rays that see a uniform
    part of the map) must have nee=1's mean."""
    nx, ny, ns = 64, 48, 512
    cam, world = _build(host, name, nx, ny)
    sc = host.lower(world).upload(0, nee=True)
    sc.attach_env(ref.sun_map() if mapname == "sun" else _earth_map())
    n = sc.render_env(cam, nx, ny, ns, nee=True, env_select_p=p, seed=SEED, flags=FC)
    d = sc.render_env(cam, nx, ny, ns * (16 if mapname == "sun" else 1), nee=False, seed=SEED + 1, flags=FC)
    z, zi, silent, ma = _tile_z(n, d)
    mb = d["linear"].astype(np.float64).reshape(ny // 8, 8, nx // 8, 8, 3).mean((1, 3))
    q = np.percentile(np.abs(z), [50, 90, 99, 100])
    k = np.unravel_index(np.argmax(np.abs(z)), z.shape)
    print("\nENV-Z %s+%s |z| p50 %.2f p90 %.2f p99 %.2f max %.2f (tile %s: %.5g vs %.5g) image-mean z %s silent %d" % (
        name, mapname, q[0], q[1], q[2], q[3], k, ma[k], mb[k], np.array2string(zi, precision=2), int(silent.sum())))
    assert np.all(np.abs(ma[silent] - mb[silent]) <= 1e-6 * np.maximum(mb[silent], 1.0)), name
    assert q[2] <= 5, (name, q[2])
    assert np.all(np.abs(zi) < 4), (name, zi)


# ---- 7. independence ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_deterministic_and_schedule_free(host):
    nx, ny, ns = 40, 24, 20
    cam, world = _build(host, "lit_random_spheres", nx, ny)
    sc = host.lower(world).upload(0, nee=True)
    r0 = sc.render(cam, nx, ny, ns, sig=True, seed=SEED, flags=FC)
    n0 = sc.render_nee(cam, nx, ny, ns, sig=True, seed=SEED, flags=FC)
    sc.attach_env(ref.sun_map())
    for nee in (False, True):
        a = sc.render_env(cam, nx, ny, ns, nee=nee, sig=True, seed=SEED, flags=FC)
        b = sc.render_env(cam, nx, ny, ns, nee=nee, sig=True, seed=SEED, flags=FC)
        for k in ("linear", "rgb8", "stderr", "sig"):
            assert _same(a[k], b[k]), (nee, k)
        others = [dict(flags=0), dict(flags=abi.RTMI_FLAG_REF_TREE | FC), dict(flags=abi.RTMI_FLAG_SYNC | FC),
                  dict(flags=FC, sample_buffer_bytes=nx * ny * 12 * 7)]
        for kw in others:
            c = sc.render_env(cam, nx, ny, ns, nee=nee, sig=True, seed=SEED, **kw)
            for k in ("linear", "rgb8", "stderr", "sig"):
                assert _same(a[k], c[k]), (nee, kw, k)
        assert a["linear"].mean() > r0["linear"].mean()
    for k in ("linear", "rgb8", "sig"):
        assert _same(sc.render(cam, nx, ny, ns, sig=True, seed=SEED, flags=FC)[k], r0[k]), k
        assert _same(sc.render_nee(cam, nx, ny, ns, sig=True, seed=SEED, flags=FC)[k], n0[k]), k
    sc.detach_env()
    with pytest.raises(HostError, match="environment map"):
        sc.render_env(cam, nx, ny, ns, nee=False, seed=SEED)


@pytest.mark.gpu
def test_refusals_on_the_device(host):
    nx, ny = 16, 16
    cam, world = _build(host, "random_spheres", nx, ny)
    sc = host.lower(world).upload(0)
    sc.attach_env(ref.sun_map())
    p = default_params(nx, ny, 2)
    o = abi.EnvRender(1, 0.5)
    rc = host.lib.rth_render_env(sc.h, cam.h, C.byref(p), C.byref(o), None, None, None, None, None)
    with pytest.raises(HostError, match="light table"):
        host._check(rc)
    with pytest.raises(HostError, match="SKY"):
        sc.render_env(cam, nx, ny, 2, nee=False, flags=abi.RTMI_FLAG_SKY)
    with pytest.raises(ValueError):
        sc.attach_env(np.zeros((4, 4), np.float32))


@pytest.mark.gpu
def test_render_denoised_env(host):
    nx, ny, ns = 48, 32, 8
    cam, world = _build(host, "random_spheres", nx, ny)
    sc = host.lower(world).upload(0)
    sc.attach_env(env_from_sky(256, 128))
    out = sc.render_denoised(cam, nx, ny, ns, env=True, nee=True, seed=SEED, flags=FC)
    ref_ = sc.render_env(cam, nx, ny, ns, nee=True, seed=SEED, flags=FC)
    assert _same(out["noisy"]["linear"], ref_["linear"]) and _same(out["noisy"]["stderr"], ref_["stderr"])
    bg = out["features"]["hits"] == 0
    assert bg.sum() > 0 and np.all(np.isfinite(out["linear"]))
    assert out["linear"][bg].tobytes() == ref_["linear"][bg].tobytes()
