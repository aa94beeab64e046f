"""Russian-roulette path termination (include/rtmi_roulette.h) on the device, all four estimators, on the
lit scenes of tests/test_gpu_nee.py and the map scenes of tests/test_gpu_env.py.

1. disabled (min_depth > max_depth, or q_min = 1) it is render_nee / render_env / render_adaptive(min_spp = ns) bit for bit;
2. with roulette disabled the bounce plane adds up to the oracle's scatter counters;
3. a roulette path is a prefix: per pixel it never scatters more often than without roulette;
4. it has the expectation of its non-roulette form (8x8-tile z-scores, the rules and bounds of tests/test_gpu_nee.py) and
   reproduces the known answers a * Le * F of tests/nee_ref.py;
5. it is deterministic and independent of the schedule;
6. the adaptive form stops a tile at the fixed render with that many samples, bounce counts included;
7. a missing light table or map is refused."""
import math

import numpy as np
import pytest

import env_ref
import nee_ref
from nee_oracle_ref import oracle_lights
from oracle.oracle import ARITH_DEVICE, THROUGHPUT_FORM
from raytracing_rust_amd import abi
from raytracing_rust_amd.host import HostError
from test_gpu_env import _earth_map
from test_gpu_nee import LIT, NK, _build, _floor_scene, _footprints, _same, _tile_z

FC = abi.RTMI_FLAG_FAST_CULL
SEED = 42
MAPS = [("random_spheres", "sun"), ("earth", "earth"), ("lit_random_spheres", "sun")]
# (scene, map or None, estimator): the lit scenes under the plain and NEE estimators, the map scenes under the two map ones
CASES = ([(n, None, e) for n in LIT for e in ("plain", "nee")] + [(n, m, e) for n, m in MAPS for e in ("env", "env_nee")])
IDS = ["%s-%s" % (n, e) for n, _, e in CASES]
ON = dict(min_depth=3, q_min=0.05)


def _scene(host, name, mapname, nx, ny):
    cam, world = _build(host, name, nx, ny)
    sc = host.lower(world).upload(0, nee=True)
    if mapname:
        sc.attach_env(env_ref.sun_map() if mapname == "sun" else _earth_map())
    return cam, sc


def _off(sc, cam, nx, ny, ns, est, **kw):
    """The non-roulette form of estimator `est`, with standard errors."""
    if est == "plain":
        return sc.render_adaptive(cam, nx, ny, ns, min_spp=ns, step_spp=1, **kw)
    if est == "nee":
        return sc.render_nee(cam, nx, ny, ns, **kw)
    return sc.render_env(cam, nx, ny, ns, nee=est == "env_nee", env_select_p=0.5, **kw)


# ---- 1. disabled is identical ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,mapname,est", CASES, ids=IDS)
def test_disabled_is_identical_and_prefix(host, name, mapname, est):
    nx, ny, ns = 40, 24, 12
    cam, sc = _scene(host, name, mapname, nx, ny)
    ref = _off(sc, cam, nx, ny, ns, est, seed=SEED, flags=FC)
    a = sc.render_roulette(cam, nx, ny, ns, estimator=est, min_depth=51, q_min=0.05, seed=SEED, flags=FC)
    b = sc.render_roulette(cam, nx, ny, ns, estimator=est, min_depth=1, q_min=1.0, seed=SEED, flags=FC)
    for k in ("linear", "rgb8", "stderr"):
        assert _same(a[k], ref[k]), (name, est, "min_depth > max_depth", k)
        assert _same(b[k], ref[k]), (name, est, "q_min = 1", k)
    # q_min = 1 makes no draw, but a throughput of exactly 0 still ends the continuation (lit_smoke's black fog)
    assert np.all(b["bounces"] <= a["bounces"]) and a["stats"]["samples"] == nx * ny * ns
    if name != "lit_smoke":
        assert _same(a["bounces"], b["bounces"]), (name, est)
    # 3. prefix: with roulette no pixel scatters more often, for the same seed
    for kw in (ON, dict(min_depth=1, q_min=0.2)):
        r = sc.render_roulette(cam, nx, ny, ns, estimator=est, seed=SEED, flags=FC, **kw)
        assert np.all(r["bounces"] <= a["bounces"]), (name, est, kw)
        assert np.all(np.isfinite(r["linear"])) and np.all(r["linear"] >= 0)
        print("\nRR-PREFIX %s %s %s: scatters/sample %.2f -> %.2f" % (name, est, kw, a["bounces"].sum() / (nx * ny * ns),
                                                                      r["bounces"].sum() / (nx * ny * ns)))
        if name == "cornell_box":
            assert r["bounces"].sum() < a["bounces"].sum()


# ---- 2. the bounce count is the oracle's scatter count ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_box", "lit_smoke"])
@pytest.mark.parametrize("est", ["plain", "nee"])
def test_bounce_total_equals_oracle_scatter_counters(host, orc32, name, est):
    """Neither scene holds Metal (the oracle's Metal counter also counts the calls that absorb)."""
    nx, ny, ns = 24, 16, 8
    cam, sc = _scene(host, name, None, nx, ny)
    cam_o, world_o = _build(orc32, name, nx, ny)
    lights = oracle_lights(orc32, world_o, sc)
    orc32.reset_counters()
    if est == "nee":
        ref = orc32.render_nee(cam_o, world_o, lights, nx, ny, ns, seed=SEED, flags=ARITH_DEVICE | THROUGHPUT_FORM)
    else:
        ref = orc32.render_samples(cam_o, world_o, nx, ny, ns, seed=SEED, flags=ARITH_DEVICE | THROUGHPUT_FORM)
    cnt = orc32.counters()
    orc32.free_all()
    assert cnt["sc_metal"] == 0
    want = cnt["sc_lambert"] + cnt["sc_metal"] + cnt["sc_dielectric"] + cnt["sc_isotropic"]
    got = sc.render_roulette(cam, nx, ny, ns, estimator=est, min_depth=51, q_min=0.05, seed=SEED, flags=FC)
    print("\nRR-BOUNCES %s %s: device %d, oracle %d" % (name, est, int(got["bounces"].sum()), want))
    assert np.array_equal(got["linear"].view(np.uint32), ref["linear"].view(np.uint32))
    assert int(got["bounces"].sum(dtype=np.uint64)) == want


# ---- 4. same expectation ----------------------------------------------------------------------------------------------------
# The map estimator without NEE finds the sun map's sun by rare BSDF hits only; tests/test_gpu_env.py records that at 512
# spp a tile may catch none and its standard error then misses the sun's share (|z| 13 seen there), and gives that
# estimator 16x the samples.  Here both sides are that estimator (with and without roulette), so under the sun map both
# take 64x the samples: about 200 sun hits per tile, enough for the tile's Welford standard error to hold its share.
@pytest.mark.gpu
@pytest.mark.parametrize("name,mapname,est", CASES, ids=IDS)
def test_same_expectation(host, name, mapname, est):
    nx, ny, ns = 64, 48, 512 * (64 if (est == "env" and mapname == "sun") else 1)
    cam, sc = _scene(host, name, mapname, nx, ny)
    r = sc.render_roulette(cam, nx, ny, ns, estimator=est, seed=SEED, flags=FC, **ON)
    d = _off(sc, cam, nx, ny, ns, est, seed=SEED + 1, flags=FC)
    z, zi, silent, ma = _tile_z(r, d)
    q = np.percentile(np.abs(z), [50, 90, 99, 100])
    print("\nRR-Z %s %s tiles %d |z| p50 %.2f p90 %.2f p99 %.2f max %.2f image-mean z %s; silent %d; scatters/sample %.2f; "
          "median stderr %.4g vs %.4g" % (name, est, z.size // 3, q[0], q[1], q[2], q[3], np.array2string(zi, precision=2),
                                          int(silent.sum()), r["bounces"].sum() / (nx * ny * ns),
                                          float(np.median(r["stderr"])), float(np.median(d["stderr"]))))
    if mapname:
        # a tile whose non-roulette samples are all equal sees only the map, by camera rays (the sun map's sky is uniform):
        # no scatter, no test, so roulette has that very mean (the rule of tests/test_gpu_env.py for such tiles)
        mb = d["linear"].astype(np.float64).reshape(ny // 8, 8, nx // 8, 8, 3).mean((1, 3))
        assert np.all(np.abs(ma[silent] - mb[silent]) <= 1e-6 * np.maximum(mb[silent], 1.0)), name
    else:
        assert not silent.any() or ma[silent].max() <= 1e-6 * max(float(r["linear"].mean()), 1e-30), name
    assert np.abs(z).max() <= 5, (name, est, np.abs(z).max())
    assert np.all(np.abs(zi) < 4), (name, est, zi)


def _known_answer(sc, cam, f_of, le, albedo, ns=1024, **rr_kw):
    pts = _footprints(cam, NK)
    f = np.zeros((NK, NK))
    bound = np.zeros((NK, NK))
    for r in range(NK):
        for col in range(NK):
            vals = [f_of(p[r, col]) for p in pts]
            f[r, col] = vals[0][0]
            bound[r, col] = max(v[0] for v in vals) - min(v[0] for v in vals) + vals[0][1]
    want = albedo * le * f
    out = sc.render_roulette(cam, NK, NK, ns, estimator="nee", seed=SEED, flags=FC, **rr_kw)
    got, se = out["linear"][..., 0].astype(np.float64), out["stderr"][..., 0].astype(np.float64)
    z = (got - want) / np.sqrt(se ** 2 + 1e-30)
    sem = math.sqrt(np.sum(se ** 2)) / (NK * NK)
    zm = (got.mean() - want.mean()) / sem
    print("\nRR-KNOWN %s: max |z| %.2f image-mean z %.2f scatters/sample %.2f" % (rr_kw, np.abs(z).max(), zm,
                                                                                   out["bounces"].sum() / (NK * NK * ns)))
    assert np.all(np.abs(got - want) <= 5 * se + bound), np.abs(z).max()
    assert abs(zm) < 4 + bound.mean() / sem, zm


@pytest.mark.gpu
@pytest.mark.parametrize("rr_kw", [dict(min_depth=1, q_min=0.2), dict(min_depth=1, q_min=0.8)], ids=["q=m", "q=q_min"])
def test_known_answer_rect_light(host, rr_kw):
    """The floor scene's paths scatter once (a flat floor, then the light or nothing), so only the test at depth 1 is ever
    made: with T = 0.5 it survives with q = 0.5 under q_min 0.2 and with q = q_min under 0.8."""
    le, albedo, h = 4.0, 0.5, 3.0
    light = host.Rect(host.PLANE_ZX, -1.0, -2.0, 1.5, 1.0, h, host.DiffuseLight(host.SolidTexture(le, le, le)))
    cam, world = _floor_scene(host, light, albedo)
    sc = host.lower(world).upload(0, nee=True)
    corner, ea, eb = np.array([-2.0, h, -1.0]), np.array([0, 0, 2.5]), np.array([3.0, 0, 0])
    n = np.array([0, 1.0, 0])
    _known_answer(sc, cam, lambda x: nee_ref.f_rect(x, n, corner, ea, eb, 64, 64), le, albedo, **rr_kw)


@pytest.mark.gpu
def test_known_answer_sphere_light(host):
    le, albedo, r, h = 4.0, 0.5, 0.5, 2.0
    light = host.Sphere((0.0, h, 0.0), r, host.DiffuseLight(host.SolidTexture(le, le, le)))
    cam, world = _floor_scene(host, light, albedo)
    sc = host.lower(world).upload(0, nee=True)
    n = np.array([0, 1.0, 0])
    _known_answer(sc, cam, lambda x: (nee_ref.f_sphere(x, n, [0, h, 0], r, 128), 1e-5), le, albedo, min_depth=1, q_min=0.2)


# ---- 5. determinism and schedule independence -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,mapname,est", [("lit_smoke", None, "plain"), ("lit_smoke", None, "nee"),
                                              ("lit_random_spheres", "sun", "env"), ("lit_random_spheres", "sun", "env_nee")],
                         ids=["plain", "nee", "env", "env_nee"])
def test_deterministic_and_schedule_free(host, name, mapname, est):
    nx, ny, ns = 40, 24, 20
    cam, sc = _scene(host, name, mapname, nx, ny)
    kw0 = dict(estimator=est, seed=SEED, min_depth=2, q_min=0.1)
    a = sc.render_roulette(cam, nx, ny, ns, flags=FC, **kw0)
    b = sc.render_roulette(cam, nx, ny, ns, flags=FC, **kw0)
    keys = ("linear", "rgb8", "stderr", "bounces")
    for k in keys:
        assert _same(a[k], b[k]), k
    others = [dict(flags=0), dict(flags=abi.RTMI_FLAG_REF_TREE | FC), dict(flags=abi.RTMI_FLAG_SYNC | FC),
              dict(flags=FC, sample_buffer_bytes=nx * ny * 12 * 7), dict(flags=FC, shade_threshold=1)]
    for kw in others:
        c = sc.render_roulette(cam, nx, ny, ns, **kw0, **kw)
        for k in keys:
            assert _same(a[k], c[k]), (est, kw, k)
    assert not _same(a["linear"], sc.render_roulette(cam, nx, ny, ns, flags=FC, **dict(kw0, seed=SEED + 1))["linear"])
    assert not _same(a["linear"], _off(sc, cam, nx, ny, ns, est, seed=SEED, flags=FC)["linear"])


# ---- 6. the adaptive form -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,mapname,est", [("cornell_box", None, "plain"), ("cornell_box", None, "nee"),
                                              ("lit_random_spheres", "sun", "env"), ("lit_random_spheres", "sun", "env_nee")],
                         ids=["plain", "nee", "env", "env_nee"])
def test_adaptive_tiles_equal_fixed_renders(host, name, mapname, est):
    nx, ny, cap = 40, 24, 24
    cam, sc = _scene(host, name, mapname, nx, ny)
    kw = dict(estimator=est, seed=SEED, flags=FC, **ON)
    keys = ("linear", "rgb8", "stderr", "bounces")
    full = sc.render_adaptive_roulette(cam, nx, ny, cap, min_spp=cap, step_spp=1, **kw)
    fixed = sc.render_roulette(cam, nx, ny, cap, **kw)
    for k in keys:
        assert _same(full[k], fixed[k]), (est, "min_spp == ns", k)
    assert np.all(full["spp"] == cap)
    # an absolute target that about half the tiles cannot meet at the cap: the median over the tiles of their worst
    # pixel's standard error there (a relative one is met at once by the plain estimator's single-hit pixels, whose
    # stderr equals their mean at any n)
    worst = fixed["stderr"].astype(np.float64).reshape(ny // 8, 8, nx // 8, 8, 3).max((1, 3, 4))
    tol = dict(abs_tol=float(np.median(worst)), rel_tol=0.0)
    ad = sc.render_adaptive_roulette(cam, nx, ny, cap, min_spp=4, step_spp=5, **tol, **kw)
    counts = sorted(set(int(x) for x in np.unique(ad["spp"])))
    print("\nRR-ADAPTIVE %s %s: tile sample counts %s, samples %d of %d" % (name, est, counts, ad["stats"]["samples"], nx * ny * cap))
    assert len(counts) >= 2 and set(counts) <= {4, 9, 14, 19, 24}, counts
    assert ad["stats"]["samples"] == int(ad["spp"].sum(dtype=np.uint64))
    for n in counts:
        ref = sc.render_roulette(cam, nx, ny, n, **kw)
        m = ad["spp"] == n
        for k in keys:
            assert np.array_equal(ad[k][m], ref[k][m]) and ad[k][m].tobytes() == ref[k][m].tobytes(), (est, n, k)
    # and under another schedule
    ad2 = sc.render_adaptive_roulette(cam, nx, ny, cap, min_spp=4, step_spp=5, **tol, **dict(kw, flags=abi.RTMI_FLAG_SYNC),
                                      sample_buffer_bytes=nx * ny * 12 * 3)
    for k in keys + ("spp",):
        assert _same(ad[k], ad2[k]), (est, "schedule", k)


# ---- 7. refusals on the device --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_missing_light_table_or_map_is_refused(host):
    nx, ny = 16, 16
    cam, world = _build(host, "cornell_box", nx, ny)
    sc = host.lower(world).upload(0)
    sc.lights_attached = True  # keep render_roulette from attaching the table
    for est in ("nee", "env_nee"):
        with pytest.raises(HostError, match="light table|environment map"):
            sc.render_roulette(cam, nx, ny, 2, estimator=est, seed=SEED)
    with pytest.raises(HostError, match="environment map"):
        sc.render_roulette(cam, nx, ny, 2, estimator="env", seed=SEED)
    sc.attach_env(np.ones((4, 8, 3), np.float32))
    with pytest.raises(HostError, match="light table"):
        sc.render_roulette(cam, nx, ny, 2, estimator="env_nee", seed=SEED)
    out = sc.render_roulette(cam, nx, ny, 2, estimator="env", seed=SEED)  # the map alone serves the map estimator
    assert np.all(np.isfinite(out["linear"])) and out["bounces"].shape == (ny, nx)
    out = sc.render_roulette(cam, nx, ny, 2, estimator="plain", seed=SEED)
    assert out["stats"]["samples"] == nx * ny * 2
