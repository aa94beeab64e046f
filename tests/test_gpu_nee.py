"""Next-event estimation (include/rtmi_nee.h) on the device.

NEE is a second estimator of rtmi_render's image on rtmi_render's own paths, so:
1. its path signatures are render()'s bit for bit;
2. without lights it is render() bit for bit;
3. it reproduces known answers a * Le * F (F = the integral of the Lambertian's density (2/pi) cos^3 over the light);
4. it has render()'s expectation on lit scenes (8x8-tile z-scores against render_adaptive's standard errors);
5. it is less noisy;
6. it is deterministic and independent of the schedule."""
import ctypes as C
import math

import numpy as np
import pytest

import nee_ref
import scenes_extra
from raytracing_rust_amd import abi, scenes
from raytracing_rust_amd.host import HostError

FC, SKY = abi.RTMI_FLAG_FAST_CULL, abi.RTMI_FLAG_SKY
SEED = 42
LIT = ["cornell_box", "lit_smoke", "simple_light", "lit_random_spheres", "hollow_glass"]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _build(host, name, nx, ny):
    if name in scenes.SCENES:
        return scenes.build(host, name, nx, ny, seed=1)
    return scenes_extra.build(host, name, nx, ny, seed=7 if name == "lit_random_spheres" else 1)


# ---- 1. same paths --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", LIT)
def test_same_paths(host, name):
    nx, ny = 48, 32
    cam, world = _build(host, name, nx, ny)
    sc = host.lower(world).upload(0, nee=True)
    assert len(sc.lights()) > 0
    for flags in (FC, 0):
        n = sc.render_nee(cam, nx, ny, 8, sig=True, seed=SEED, flags=flags)
        r = sc.render(cam, nx, ny, 8, sig=True, seed=SEED, flags=flags)
        assert _same(n["sig"], r["sig"]), "%s flags %d: %d signatures differ" % (name, flags, int((n["sig"] != r["sig"]).sum()))
        assert n["stats"]["samples"] == nx * ny * 8
        assert np.all(np.isfinite(n["linear"])) and np.all(n["linear"] >= 0)


# ---- 2. no lights, no change ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,flags", [("final_scene", FC), ("random_spheres", FC | SKY), ("two_perlin_spheres", FC | SKY)])
def test_no_lights_is_render(host, name, flags):
    nx, ny = 64, 48
    cam, world = _build(host, name, nx, ny)
    sc = host.lower(world)
    assert len(sc.lights()) == 0
    n = sc.render_nee(cam, nx, ny, 6, sig=True, seed=SEED, flags=flags)
    r = sc.render(cam, nx, ny, 6, sig=True, seed=SEED, flags=flags)
    for k in ("linear", "rgb8", "sig"):
        assert _same(n[k], r[k]), (name, k)
    if name == "final_scene":
        assert not np.any(n["linear"]) and not np.any(n["rgb8"])


@pytest.mark.gpu
def test_missing_light_table_is_refused(host):
    nx, ny = 16, 16
    cam, world = _build(host, "cornell_box", nx, ny)
    sc = host.lower(world).upload(0)
    p = __import__("raytracing_rust_amd.host", fromlist=["default_params"]).default_params(nx, ny, 2)
    lin = np.zeros((ny, nx, 3), np.float32)
    rc = host.lib.rth_render_nee(sc.h, cam.h, C.byref(p), lin.ctypes.data, None, None, None, None)
    assert rc != 0
    with pytest.raises(HostError, match="light table"):
        host._check(rc)


# ---- 3. known answers -----------------------------------------------------------------------------------------------------
NK = 24  # image side of the known-answer renders


def _floor_scene(host, light, albedo=0.5):
    """A Lambertian floor (ZX rect at y = 0, normal +y) seen from y = 1 straight down, and one light above the camera."""
    w = host.HittableList()
    w.push(host.Rect(host.PLANE_ZX, -50.0, -50.0, 50.0, 50.0, 0.0, host.Lambertian(host.SolidTexture(albedo, albedo, albedo))))
    w.push(light)
    cam = host.Camera((0.0, 1.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 30.0, 1.0, 0.0, 1.0, 0.0, 1.0)
    return cam, w


def _footprints(cam, n):
    """Floor points (x, 0, z) of the centre and four corners of every pixel [row (0 = top), col]."""
    c = cam.lower()
    org, llc = np.array(c.origin, np.float64), np.array(c.lower_left_corner, np.float64)
    hor, ver = np.array(c.horizontal, np.float64), np.array(c.vertical, np.float64)
    pts = []
    for du, dv in ((0.5, 0.5), (0, 0), (1, 0), (0, 1), (1, 1)):
        i = np.arange(n)[None, :] + du
        j = (n - 1 - np.arange(n))[:, None] + dv
        d = llc + hor * (i / n)[..., None] + ver * (j / n)[..., None] - org
        t = -org[1] / d[..., 1]
        pts.append(org + d * t[..., None])
    return pts


def _known_answer(sc, cam, f_of, le, albedo, ns_nee=1024, ns_def=4096):
    pts = _footprints(cam, NK)
    f = np.zeros((NK, NK))
    bound = np.zeros((NK, NK))
    for r in range(NK):
        for col in range(NK):
            vals = [f_of(p[r, col]) for p in pts]
            f[r, col] = vals[0][0]
            bound[r, col] = max(v[0] for v in vals) - min(v[0] for v in vals) + vals[0][1]
    want = albedo * le * f
    nee = sc.render_nee(cam, NK, NK, ns_nee, seed=SEED, flags=FC)
    got, se = nee["linear"][..., 0].astype(np.float64), nee["stderr"][..., 0].astype(np.float64)
    z = (got - want) / np.sqrt(se ** 2 + 1e-30)
    assert np.all(np.abs(got - want) <= 5 * se + bound), np.abs(z).max()
    zm = (got.mean() - want.mean()) / (math.sqrt(np.sum(se ** 2)) / (NK * NK))
    assert abs(zm) < 4 + bound.mean() / (math.sqrt(np.sum(se ** 2)) / (NK * NK)), zm
    # the control: the default estimator converges to the same answer
    ref = sc.render_adaptive(cam, NK, NK, ns_def, min_spp=ns_def, step_spp=1, seed=SEED, flags=FC)
    rm, rse = ref["linear"][..., 0].astype(np.float64).mean(), math.sqrt(np.sum(ref["stderr"][..., 0].astype(np.float64) ** 2)) / NK / NK
    assert abs(rm - want.mean()) < 4 * rse + bound.mean(), (rm, want.mean(), rse)
    return got, want, se


@pytest.mark.gpu
def test_known_answer_rect_light(host):
    le, albedo, h = 4.0, 0.5, 3.0
    light = host.Rect(host.PLANE_ZX, -1.0, -2.0, 1.5, 1.0, h, host.DiffuseLight(host.SolidTexture(le, le, le)))
    cam, world = _floor_scene(host, light, albedo)
    sc = host.lower(world).upload(0, nee=True)
    corner, ea, eb = np.array([-2.0, h, -1.0]), np.array([0, 0, 2.5]), np.array([3.0, 0, 0])
    n = np.array([0, 1.0, 0])
    got, want, se = _known_answer(sc, cam, lambda x: nee_ref.f_rect(x, n, corner, ea, eb, 64, 64), le, albedo)
    # a cos/pi lobe would predict a different image: far outside the stderrs
    f_cos = lambda x: nee_ref.f_rect(x, n, corner, ea, eb, 64, 64)[0]  # noqa: E731
    x0 = _footprints(cam, NK)[0][NK // 2, NK // 2]
    w = np.array([[[-2 + 3 * (i + 0.5) / 64, h, -1 + 2.5 * (k + 0.5) / 64] for k in range(64)] for i in range(64)]) - x0
    d2 = np.sum(w * w, -1)
    cos_pi = np.sum((w[..., 1] / np.sqrt(d2)) / np.pi * (w[..., 1] / np.sqrt(d2)) / d2) * 7.5 / 4096
    assert abs(albedo * le * cos_pi - albedo * le * f_cos(x0)) > 20 * se[NK // 2, NK // 2]


@pytest.mark.gpu
def test_known_answer_sphere_light(host):
    le, albedo, r, h = 4.0, 0.5, 0.5, 2.0
    light = host.Sphere((0.0, h, 0.0), r, host.DiffuseLight(host.SolidTexture(le, le, le)))
    cam, world = _floor_scene(host, light, albedo)
    sc = host.lower(world).upload(0, nee=True)
    n = np.array([0, 1.0, 0])
    got, want, se = _known_answer(sc, cam, lambda x: (nee_ref.f_sphere(x, n, [0, h, 0], r, 128), 1e-5), le, albedo)
    # straight below the centre: the closed form
    assert abs(nee_ref.f_sphere(np.zeros(3), n, [0, h, 0], r) - nee_ref.f_sphere_below(r, h)) < 1e-4
    # a cos/pi lobe: F = sin^2(theta_max) instead of 1 - cos^4(theta_max)
    s = (r / h) ** 2
    assert abs(albedo * le * (s - nee_ref.f_sphere_below(r, h))) > 20 * np.median(se)


# ---- 4. same expectation as the default estimator -------------------------------------------------------------------------
def _tile_z(a, b):
    """8x8-tile means of two (linear, stderr) pairs -> z-scores [tiles, 3] and the image-mean z per channel."""
    ny, nx = a["linear"].shape[:2]
    ty, tx = ny // 8, nx // 8

    def tiles(x):
        return x[:ty * 8, :tx * 8].astype(np.float64).reshape(ty, 8, tx, 8, 3)

    ma, mb = tiles(a["linear"]).mean((1, 3)), tiles(b["linear"]).mean((1, 3))
    va, vb = (tiles(a["stderr"]) ** 2).sum((1, 3)) / 64 ** 2, (tiles(b["stderr"]) ** 2).sum((1, 3)) / 64 ** 2
    # a tile where the default's samples have no variance (all equal: typically all 0) carries no standard error to
    # compare with; NEE may legitimately find light there that the default never samples (simple_light's
    # horizon, paths grazing the r = 1000 ground sphere, ~4e-8).  Those tiles are returned apart as `silent`.
    silent = vb == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.where(~silent & (va + vb > 0), (ma - mb) / np.sqrt(va + vb), 0.0)
    npx = ty * tx * 64
    zi = (tiles(a["linear"]).mean((0, 1, 2, 3)) - tiles(b["linear"]).mean((0, 1, 2, 3))) / np.sqrt(
        ((tiles(a["stderr"]) ** 2).sum((0, 1, 2, 3)) + (tiles(b["stderr"]) ** 2).sum((0, 1, 2, 3))) / npx ** 2)
    return z, zi, silent, ma


@pytest.mark.gpu
@pytest.mark.parametrize("name", LIT)
def test_same_expectation(host, name):
    nx, ny, ns = 64, 48, 512
    cam, world = _build(host, name, nx, ny)
    sc = host.lower(world).upload(0, nee=True)
    n = sc.render_nee(cam, nx, ny, ns, seed=SEED, flags=FC)
    d = sc.render_adaptive(cam, nx, ny, ns, min_spp=ns, step_spp=1, seed=SEED + 1, flags=FC)
    z, zi, silent, ma = _tile_z(n, d)
    q = np.percentile(np.abs(z), [50, 90, 99, 100])
    print("\nNEE-Z %s tiles %d |z| p50 %.2f p90 %.2f p99 %.2f max %.2f image-mean z %s; tile-channels without default "
          "variance %d, their NEE mean <= %.3g" % (name, z.size // 3, q[0], q[1], q[2], q[3], np.array2string(zi, precision=2),
                                                   int(silent.sum()), float(ma[silent].max()) if silent.any() else 0.0))
    # where the default saw nothing in ns x 64 paths, NEE's light is negligible against the image
    assert not silent.any() or ma[silent].max() <= 1e-6 * max(float(n["linear"].mean()), 1e-30), name
    assert np.abs(z).max() <= 5, (name, np.abs(z).max())
    assert np.all(np.abs(zi) < 4), (name, zi)


# ---- 5. less noise --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_box", "lit_smoke"])
def test_less_noise(host, name):
    nx, ny, ns = 64, 64, 64
    cam, world = _build(host, name, nx, ny)
    sc = host.lower(world).upload(0, nee=True)
    n = sc.render_nee(cam, nx, ny, ns, seed=SEED, flags=FC)
    d = sc.render_adaptive(cam, nx, ny, ns, min_spp=ns, step_spp=1, seed=SEED, flags=FC)
    lit = d["linear"].sum(-1) > 0
    ratio = np.median(n["stderr"].mean(-1)[lit]) / np.median(d["stderr"].mean(-1)[lit])
    print("\nNEE-NOISE %s median stderr ratio %.3f over %d pixels" % (name, ratio, int(lit.sum())))
    assert ratio <= 0.5, ratio


# ---- 6. determinism and schedule independence -----------------------------------------------------------------------------
@pytest.mark.gpu
def test_deterministic_and_schedule_free(host):
    nx, ny, ns = 40, 24, 20
    cam, world = _build(host, "lit_smoke", nx, ny)
    sc = host.lower(world).upload(0, nee=True)
    a = sc.render_nee(cam, nx, ny, ns, sig=True, seed=SEED, flags=FC)
    b = sc.render_nee(cam, nx, ny, ns, sig=True, seed=SEED, flags=FC)
    for k in ("linear", "rgb8", "stderr", "sig"):
        assert _same(a[k], b[k]), k
    others = [dict(flags=0), dict(flags=abi.RTMI_FLAG_REF_TREE | FC), dict(flags=abi.RTMI_FLAG_SYNC | FC),
              dict(flags=FC, sample_buffer_bytes=nx * ny * 12 * 7), dict(flags=FC, shade_threshold=1)]
    for kw in others:
        c = sc.render_nee(cam, nx, ny, ns, sig=True, seed=SEED, **kw)
        for k in ("linear", "rgb8", "stderr", "sig"):
            assert _same(a[k], c[k]), (kw, k)
    assert not _same(a["linear"], sc.render_nee(cam, nx, ny, ns, seed=SEED + 1, flags=FC)["linear"])


@pytest.mark.gpu
def test_render_denoised_nee(host):
    nx, ny, ns = 48, 32, 8
    cam, world = _build(host, "cornell_box", nx, ny)
    sc = host.lower(world).upload(0)
    out = sc.render_denoised(cam, nx, ny, ns, nee=True, seed=SEED, flags=FC)
    assert np.all(np.isfinite(out["linear"])) and out["rgb8"].dtype == np.uint8
    ref = sc.render_nee(cam, nx, ny, ns, seed=SEED, flags=FC)
    assert _same(out["noisy"]["linear"], ref["linear"]) and _same(out["noisy"]["stderr"], ref["stderr"])
    plain = sc.render_denoised(cam, nx, ny, ns, seed=SEED, flags=FC)
    assert _same(plain["noisy"]["linear"], sc.render(cam, nx, ny, ns, seed=SEED, flags=FC)["linear"])
