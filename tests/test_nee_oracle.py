"""The oracle's restatement of next-event estimation (oracle/rt_oracle.c orc_emitters / orc_render_nee;
include/rtmi_nee.h), checked on the CPU: its light tables are the device's, it is the plain render where it must be,
and the f64 restatement converges to the quadrature known answers of tests/nee_ref.py.  Plus the numpy restatement of
rtmi_adaptive.h's Welford standard error that the GPU tests compare the device's stderr planes with."""
import numpy as np
import pytest

import nee_ref
import scenes_extra
import scenes_random
from nee_oracle_ref import EDGE, device_geometry, light_table, match_emitters, oracle_lights, selection, welford_stderr
from oracle.oracle import ARITH_DEVICE, FACE_FORWARD, LIGHT_DTYPE, SKY, THROUGHPUT_FORM, UV_BOOK
from raytracing_rust_amd import scenes

LIT = ["cornell_box", "lit_smoke", "simple_light", "lit_random_spheres", "hollow_glass", "lit_final_scene"]
DEV = ARITH_DEVICE | THROUGHPUT_FORM


def _world(api, name):
    if name in scenes.SCENES:
        return scenes.SCENES[name][0](api, 1)
    return scenes_extra.EXTRA[name][0](api, 7 if name == "lit_random_spheres" else 1)


def _build(api, name, nx, ny):
    if name in scenes.SCENES:
        return scenes.build(api, name, nx, ny, seed=1)
    return scenes_extra.build(api, name, nx, ny, seed=7 if name == "lit_random_spheres" else 1)


def _tables_agree(host, orc, world_h, world_o):
    sc = host.lower(world_h)
    t, geo = device_geometry(sc)
    em = orc.emitters(world_o)
    idx = match_emitters(em, geo)  # one to one, by kind, plane and geometry
    assert len(idx) == len(t)
    if len(t):
        e = em[idx]
        assert np.array_equal(e["area"], t["area"]) and np.array_equal(e["weight"], t["weight"])
        p, cdf = selection(e["area"], e["weight"])
        assert np.array_equal(t["select_p"], p) and np.array_equal(t["cdf"], cdf)
        assert cdf[-1] == 1.0
    return len(t)


# ---- light tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LIT + ["final_scene", "random_spheres", "cornell_smoke"])
def test_light_tables_agree_named(host, orc32, name):
    n = _tables_agree(host, orc32, _world(host, name), _world(orc32, name))
    assert (n > 0) == (name in LIT or name == "cornell_smoke"), (name, n)
    orc32.free_all()


def _hand_built(api):
    """test_nee_lights.py's emitters that are not lights, the controls that are, and three lights in a row."""
    light = api.DiffuseLight(api.SolidTexture(4.0, 4.0, 4.0))
    w = api.HittableList()
    w.push(api.Rect(api.PLANE_ZX, 0.0, 0.0, 10.0, 10.0, 0.0, api.Lambertian(api.SolidTexture(0.5, 0.5, 0.5))))
    w.push(api.Traslate(api.Sphere((0.0, 5.0, 0.0), 1.0, light), (1.0, 0.0, 0.0)))
    w.push(api.Rotate(api.AXIS_Y, api.Rect(api.PLANE_ZX, 0.0, 0.0, 1.0, 1.0, 5.0, light), 30.0))
    w.push(api.MovingSphere((0.0, 5.0, 0.0), (0.0, 6.0, 0.0), 0.0, 1.0, 1.0, light))
    w.push(api.Cube((0.0, 5.0, 0.0), (1.0, 6.0, 1.0), light))
    w.push(api.Sphere((3.0, 5.0, 0.0), -1.0, light))
    w.push(api.Rect(api.PLANE_ZX, 2.0, 0.0, 1.0, 1.0, 5.0, light))
    w.push(api.ConstantMedium(api.Sphere((0.0, 5.0, 7.0), 1.0, light), 0.1, api.SolidTexture(1.0, 1.0, 1.0)))
    w.push(api.Sphere((0.0, 5.0, -3.0), 1.0, api.DiffuseLight(api.SolidTexture(0.0, 0.0, 0.0))))
    w.push(api.Sphere((0.0, 9.0, 0.0), 1.0, light))
    w.push(api.FlipNormals(api.Rect(api.PLANE_XY, 0.0, 0.0, 1.0, 2.0, 5.0, light)))
    w.push(api.Sphere((0.0, 9.0, 4.0), 0.5, api.DiffuseLight(api.NoiseTexture(1.0))))
    w.push(api.Rect(api.PLANE_YZ, 0.0, 0.0, 4.0, 1.0, 5.0, api.DiffuseLight(api.SolidTexture(1.0, 3.0, 2.0))))
    return w


def test_light_tables_agree_hand_built(host, orc32):
    assert _tables_agree(host, orc32, _hand_built(host), _hand_built(orc32)) == 4
    em = orc32.emitters(_hand_built(orc32))
    not_lights = em[em["eligible"] == 0]
    assert not_lights["under_xform"].sum() == 2 and not_lights["in_medium"].sum() == 1
    orc32.free_all()


@pytest.mark.parametrize("instanced", [False, True], ids=["plain", "instanced"])
@pytest.mark.parametrize("seed", list(range(1, 25)))
def test_light_tables_agree_random(host, orc32, seed, instanced):
    _, wh = scenes_random.build(host, seed, 16, 12, instanced=instanced)
    _, wo = scenes_random.build(orc32, seed, 16, 12, instanced=instanced)
    assert _tables_agree(host, orc32, wh, wo) >= 1  # the sphere light at (0, 7, 0) is always there
    orc32.free_all()


# ---- the restatement is the plain render where it must be -----------------------------------------------------------------
@pytest.mark.parametrize("name,flags", [("cornell_box", 0), ("lit_smoke", FACE_FORWARD), ("simple_light", SKY | UV_BOOK)])
def test_empty_table_is_plain_render(orc32, name, flags):
    nx, ny, ns = 12, 8, 4
    cam, world = _build(orc32, name, nx, ny)
    a = orc32.render_nee(cam, world, np.zeros(0, LIGHT_DTYPE), nx, ny, ns, flags=DEV | flags, samples=True)
    b = orc32.render_samples(cam, world, nx, ny, ns, flags=DEV | flags)
    for k in ("linear", "rgb", "sig", "mean", "samples"):
        assert np.array_equal(a[k], b[k]), (name, k)
    c = orc32.render(cam, world, nx, ny, ns, flags=DEV | flags)
    for k in ("linear", "rgb", "sig", "mean"):
        assert np.array_equal(b[k], c[k]), (name, k)
    assert np.array_equal(b["samples"].astype(np.float64).sum(2) / ns, c["mean"])
    assert np.any(c["linear"] > 0)
    orc32.free_all()


@pytest.mark.parametrize("name", ["cornell_box", "lit_smoke", "simple_light", "hollow_glass"])
def test_lights_keep_the_paths(host, orc32, name):
    nx, ny, ns = 12, 8, 4
    cam, world = _build(orc32, name, nx, ny)
    lights = oracle_lights(orc32, world, host.lower(_world(host, name)))
    assert len(lights) > 0
    a = orc32.render_nee(cam, world, lights, nx, ny, ns, flags=DEV, samples=True)
    b = orc32.render(cam, world, nx, ny, ns, flags=DEV)
    assert np.array_equal(a["sig"], b["sig"])
    assert not np.array_equal(a["linear"], b["linear"])  # the estimator did change
    assert np.all(np.isfinite(a["samples"])) and np.all(a["samples"] >= 0)
    orc32.free_all()


# ---- the f64 restatement converges to the known answers ------------------------------------------------------------------
NK = 8


def _floor_scene(api, light, albedo=0.5):
    """test_gpu_nee.py's: a Lambertian floor (ZX rect at y = 0) seen from y = 1 straight down, one light above."""
    w = api.HittableList()
    w.push(api.Rect(api.PLANE_ZX, -50.0, -50.0, 50.0, 50.0, 0.0, api.Lambertian(api.SolidTexture(albedo, albedo, albedo))))
    w.push(light)
    cam = api.Camera((0.0, 1.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 30.0, 1.0, 0.0, 1.0, 0.0, 1.0)
    return cam, w


def _footprints(orc, cam, n):
    s = orc.camera_state(cam)
    org, llc, hor, ver = s[0:3], s[3:6], s[6:9], s[9:12]
    pts = []
    for du, dv in ((0.5, 0.5), (0, 0), (1, 0), (0, 1), (1, 1)):
        i = np.arange(n)[None, :] + du
        j = (n - 1 - np.arange(n))[:, None] + dv
        d = llc + hor * (i / n)[..., None] + ver * (j / n)[..., None] - org
        t = -org[1] / d[..., 1]
        pts.append(org + d * t[..., None])
    return pts


def _converges(orc, cam, world, f_of, le, albedo, ns, n_lights=1, tree=False):
    """tree=True: the table's lights are selected through the light tree over them (include/rtmi_light_tree.h)"""
    pts = _footprints(orc, cam, NK)
    want, bound = np.zeros((NK, NK)), np.zeros((NK, NK))
    for r in range(NK):
        for c in range(NK):
            vals = [f_of(p[r, c]) for p in pts]
            want[r, c] = albedo * le * vals[0][0]
            bound[r, c] = albedo * le * (max(v[0] for v in vals) - min(v[0] for v in vals) + vals[0][1])
    em = orc.emitters(world)
    idx = np.flatnonzero(em["eligible"])
    assert len(idx) == n_lights
    lights = light_table(em, idx.tolist())
    kw = {}
    if tree:
        from light_tree_oracle_ref import emitter_tree

        kw["tree"] = emitter_tree(em[idx])
    out = orc.render_nee(cam, world, lights, NK, NK, ns, samples=True, **kw)
    got = out["mean"][..., 0]
    se = welford_stderr(out["samples"])[..., 0].astype(np.float64)
    assert np.all(se > 0)
    err = np.abs(got - want)
    assert np.all(err <= 5 * se + bound), float(np.max((err - bound) / se))
    return got, want, se


def test_f64_restatement_converges_rect_light(orc64):
    le, albedo, h = 4.0, 0.5, 3.0
    cam, world = _floor_scene(orc64, orc64.Rect(orc64.PLANE_ZX, -1.0, -2.0, 1.5, 1.0, h,
                                                orc64.DiffuseLight(orc64.SolidTexture(le, le, le))), albedo)
    corner, ea, eb, n = np.array([-2.0, h, -1.0]), np.array([0, 0, 2.5]), np.array([3.0, 0, 0]), np.array([0, 1.0, 0])
    _converges(orc64, cam, world, lambda x: nee_ref.f_rect(x, n, corner, ea, eb, 64, 64), le, albedo, 1024)
    orc64.free_all()


def test_f64_restatement_converges_sphere_light(orc64):
    le, albedo, r, h = 4.0, 0.5, 0.5, 2.0
    cam, world = _floor_scene(orc64, orc64.Sphere((0.0, h, 0.0), r, orc64.DiffuseLight(orc64.SolidTexture(le, le, le))), albedo)
    n = np.array([0, 1.0, 0])
    got, want, se = _converges(orc64, cam, world, lambda x: (nee_ref.f_sphere(x, n, [0, h, 0], r, 128), 1e-5), le,
                               albedo, 1024)
    # a cos/pi lobe (F = sin^2 theta_max below the centre) would be far off
    s = (r / h) ** 2
    assert abs(albedo * le * (s - nee_ref.f_sphere_below(r, h))) > 20 * np.median(se)
    orc64.free_all()


# ---- Welford -------------------------------------------------------------------------------------------------------------
def test_welford_matches_two_pass_variance():
    rng = np.random.default_rng(5)
    for shape, scale in (((7, 5, 64, 3), 1.0), ((3, 4, 2, 3), 1e3), ((2, 2, 300, 3), 1e-6)):
        x = (rng.exponential(size=shape) * scale).astype(np.float32)
        x[0, 0, :, 1] = 0.25  # constant: a zero variance must come out exactly 0
        got = welford_stderr(x).astype(np.float64)
        xd = x.astype(np.float64)
        n = shape[-2]
        var = ((xd - xd.mean(-2, keepdims=True)) ** 2).sum(-2) / (n - 1)
        want = np.sqrt(var / n)
        assert np.allclose(got, want, rtol=2e-6, atol=0), float(np.max(np.abs(got - want) / want.clip(1e-300)))
        assert got[0, 0, 1] == 0.0


@pytest.mark.parametrize("name", sorted(EDGE))
def test_light_tables_agree_edge_scenes(host, orc32, name):
    _, wh = EDGE[name](host, 16, 12)
    _, wo = EDGE[name](orc32, 16, 12)
    assert _tables_agree(host, orc32, wh, wo) >= (1 if name in ("isotropic_rect", "light_in_medium") else 2), name
    orc32.free_all()


def test_cdf_boundaries_are_exact(host):
    t = host.lower(EDGE["cdf_boundaries"](host, 8, 8)[1]).lights()
    assert len(t) == 4096 and np.all(t["select_p"] == 2.0 ** -12)
    assert np.array_equal(t["cdf"], np.arange(1, 4097) / 4096.0)
