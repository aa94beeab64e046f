"""The oracle's restatement of the environment estimator (oracle/rt_oracle.c color_env / orc_render_env; include/rtmi_env.h),
checked on the CPU so that it is not a second copy of the device's mistakes:

* its map functions equal tests/env_ref.py's numpy restatement bit for bit, on every map the GPU tests use;
* a zero map reduces it to the oracle's NEE (nee=1) and plain (nee=0) renders bit for bit, nee=0 keeps render's signatures;
* the furnace of tests/test_gpu_env.py has its exact answer with nee=0;
* nee=1 has nee=0's expectation, at the |z| <= 4 per-tile criterion of tests/test_gpu_env.py;
* the appended counters did not move the old ones, and the hand-built maps reach the branches they were built for."""
import numpy as np
import pytest

import env_oracle_ref as eo
import env_ref
from nee_oracle_ref import welford_stderr
from oracle.oracle import (ARITH_DEVICE, COUNTER_NAMES, ENV_COUNTERS, FACE_FORWARD, LIGHT_DTYPE, ROULETTE_COUNTERS, THROUGHPUT_FORM,
                           TREE_COUNTERS)
from test_gpu_nee import _tile_z

SEED = 42
DEV = ARITH_DEVICE | THROUGHPUT_FORM
NO_LIGHTS = np.zeros(0, LIGHT_DTYPE)


@pytest.fixture(scope="module")
def contract():
    return env_ref.ContractMath()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


FIRST_38 = ["samples", "queries", "aabb", "sphere", "msphere", "rect", "xform", "medium", "medium_draw", "mat_fetch", "tex_solid",
            "tex_checker", "tex_noise", "tex_image", "sc_lambert", "sc_metal", "sc_dielectric", "sc_isotropic", "emit", "draws",
            "sphere_trials", "disk_trials", "sphere_accept", "rect_accept", "env_sample", "env_no_sample", "env_occluded",
            "env_unoccluded", "env_miss_mis", "env_miss_one", "env_area_sample", "env_emit_scaled", "rr_test", "rr_draw",
            "rr_end_pending", "rr_end_bare", "rr_floor_survive", "rr_zero"]


def test_counter_indices_are_kept():
    assert COUNTER_NAMES.index("rect_accept") == 23 and COUNTER_NAMES[19] == "draws" and COUNTER_NAMES[0] == "samples"
    assert COUNTER_NAMES[24:38] == ENV_COUNTERS + ROULETTE_COUNTERS and len(set(COUNTER_NAMES[:38])) == 38
    assert COUNTER_NAMES[:38] == FIRST_38  # the 38 indices from before the light tree keep their names ...
    assert COUNTER_NAMES[38:] == TREE_COUNTERS and len(set(COUNTER_NAMES)) == len(COUNTER_NAMES)  # ... and the tail is the tree's


# ---- the map functions against numpy ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(eo.maps()))
def test_map_functions_equal_numpy(orc32, contract, name):
    m = eo.maps()[name]
    h, w = m.shape[:2]
    T = env_ref.tables(m)
    rng = np.random.default_rng(9)
    for p_env in ((1.0, 0.25) if T["total"] > 0 else (0.0,)):
        d = env_ref.lat_long_dirs(10000, rng)
        got, want = orc32.env_lookup(m, T, d, p_env), env_ref.lookup(contract, m, T, d, p_env)
        bad = np.nonzero(np.any(_bits(got) != _bits(want), axis=1))[0]
        assert bad.size == 0, (name, "lookup", bad.size, d[bad[:3]], got[bad[:3]], want[bad[:3]])
        u = env_ref.uniforms(10000, rng)
        got, want = orc32.env_sample(m, T, u, p_env), env_ref.sample(contract, T, w, h, u[:, 0], u[:, 1], p_env)
        bad = np.nonzero(np.any(_bits(got) != _bits(want), axis=1))[0]
        assert bad.size == 0, (name, "sample", bad.size, u[bad[:3]], got[bad[:3]], want[bad[:3]])
        if name == "zero":
            assert not np.any(want[:, 3])
        elif name != "poles":
            assert np.mean(want[:, 3] > 0) > 0.999


def test_lookup_wraps_across_the_seam(orc32):
    """Directions just either side of phi = +-pi (x < 0, z = -+tiny) on the seam map's bright row see a blend of column
    W - 1 and column 0, not one of them alone."""
    m = eo.seam_map()
    T = env_ref.tables(m)
    lat = np.float32(np.pi * (0.5 - 1.5 / 4))  # the centre of row 1
    d = np.float32([[-np.cos(lat), np.sin(lat), 1e-4], [-np.cos(lat), np.sin(lat), -1e-4]])
    got = orc32.env_lookup(m, T, d)[:, :3].astype(np.float64)
    mid = 0.5 * (m[1, 0].astype(np.float64) + m[1, 7])
    assert np.all(np.abs(got - mid) < 1e-2 * mid), (got, mid)


# ---- reductions inside the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,flags", [("cornell_box", 0), ("lit_smoke", FACE_FORWARD), ("lit_random_spheres", 0)])
def test_zero_map_is_nee_and_plain(host, orc32, name, flags):
    nx, ny, ns = 16, 12, 6
    cam_h, world_h = eo.build(host, name, nx, ny)
    cam, world = eo.build(orc32, name, nx, ny)
    lights, _ = eo.lights_for(host, orc32, world_h, world)
    assert len(lights) > 0
    zero = np.zeros((8, 16, 3), np.float32)
    T = env_ref.tables(zero)
    assert T["total"] == 0
    nee = orc32.render_nee(cam, world, lights, nx, ny, ns, seed=SEED, flags=DEV | flags, samples=True)
    plain = orc32.render_samples(cam, world, nx, ny, ns, seed=SEED, flags=DEV | flags)
    for p in (0.5, 1.0):
        e1 = orc32.render_env(cam, world, lights, zero, T, True, p, nx, ny, ns, seed=SEED, flags=DEV | flags, samples=True)
        e0 = orc32.render_env(cam, world, lights, zero, T, False, p, nx, ny, ns, seed=SEED, flags=DEV | flags, samples=True)
        for k in ("linear", "rgb", "sig", "mean", "samples"):
            assert np.array_equal(e1[k], nee[k]), (name, p, k)
            assert np.array_equal(e0[k], plain[k]), (name, p, k)
    assert np.any(nee["samples"] != plain["samples"])
    # under a map that is not zero nee=0 and nee=1 keep render's signatures: the paths are render's
    sun = env_ref.sun_map()
    Ts = env_ref.tables(sun)
    for nee_on in (False, True):
        e = orc32.render_env(cam, world, lights, sun, Ts, nee_on, 0.5, nx, ny, ns, seed=SEED, flags=DEV | flags)
        assert np.array_equal(e["sig"], plain["sig"]) and not np.array_equal(e["linear"], plain["linear"]), (name, nee_on)
    orc32.free_all()


# ---- known answer: the furnace ----------------------------------------------------------------------------------------------
def test_furnace_exact(orc32):
    """tests/test_gpu_env.py's furnace: a Lambertian sphere of albedo a under a constant map c.  With nee=0 a pixel whose
    camera rays all hit the sphere is a * c exactly (the bilinear lookup of a constant map returns the constant, a = 0.5
    scales exactly, and a path leaves the convex sphere after its one scatter), a pixel whose rays all miss is c."""
    nx = ny = 32
    ns, a = 8, 0.5
    c = np.float32([0.8, 0.6, 0.4])
    w = orc32.HittableList()
    w.push(orc32.Sphere((0.0, 0.0, 0.0), 1.0, orc32.Lambertian(orc32.SolidTexture(a, a, a))))
    cam = orc32.Camera((0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 1.0, 0.0, 1.0)
    m = np.broadcast_to(c, (32, 64, 3)).astype(np.float32)
    T = env_ref.tables(m)
    e = orc32.render_env(cam, w, NO_LIGHTS, m, T, False, 0.5, nx, ny, ns, seed=SEED, flags=DEV, samples=True)
    s = e["samples"]
    on = np.all(s == np.float32(a) * c, axis=-1)
    off = np.all(s == c, axis=-1)
    assert np.all(on | off), "a sample is neither a * c nor c"
    full, none = on.all(-1), off.all(-1)
    assert full.sum() > 100 and none.sum() > 100
    assert np.all(e["linear"][full] == np.float32(a) * c) and np.all(e["linear"][none] == c)
    # nee=1 agrees within its standard error on the tiles that lie on the sphere
    n = orc32.render_env(cam, w, NO_LIGHTS, m, T, True, 0.5, nx, ny, 128, seed=SEED, flags=DEV, samples=True)
    se = welford_stderr(n["samples"]).astype(np.float64)
    tiles = full.reshape(4, 8, 4, 8).all(axis=(1, 3))
    mt = n["linear"].astype(np.float64).reshape(4, 8, 4, 8, 3).mean(axis=(1, 3))
    st = np.sqrt((se ** 2).reshape(4, 8, 4, 8, 3).sum(axis=(1, 3))) / 64
    assert tiles.sum() >= 1 and np.all(st[tiles] > 0)
    z = (mt[tiles] - np.float64(a) * c) / st[tiles]
    assert np.all(np.abs(z) <= 4), z
    orc32.free_all()


# ---- expectation ------------------------------------------------------------------------------------------------------------
def test_nee_has_the_bsdf_estimators_expectation(host, orc32):
    """lit_random_spheres under the sun map, env_select_p = 0.5: 8 x 8-tile z-scores of nee=1 against nee=0, |z| <= 4 per
    tile.  nee=0 finds the sun by rare BSDF hits, so it takes 16x the samples (tests/test_gpu_env.py
    test_same_expectation); tiles where its samples have no variance at all are compared for equality of the means."""
    nx, ny, ns = 32, 24, 128
    cam_h, world_h = eo.build(host, "lit_random_spheres", nx, ny)
    cam, world = eo.build(orc32, "lit_random_spheres", nx, ny)
    lights, _ = eo.lights_for(host, orc32, world_h, world)
    sun = env_ref.sun_map()
    T = env_ref.tables(sun)
    orc32.reset_counters()
    a = orc32.render_env(cam, world, lights, sun, T, True, 0.5, nx, ny, ns, seed=SEED, flags=DEV, samples=True)
    cnt = orc32.counters()
    b = orc32.render_env(cam, world, lights, sun, T, False, 0.5, nx, ny, 16 * ns, seed=SEED + 1, flags=DEV, samples=True)
    for r in (a, b):
        r["stderr"] = welford_stderr(r["samples"])
    z, zi, silent, ma = _tile_z(a, b)
    mb = b["linear"].astype(np.float64).reshape(ny // 8, 8, nx // 8, 8, 3).mean((1, 3))
    print("\nENV-ORACLE-Z max |z| %.2f image-mean z %s silent %d" % (float(np.abs(z).max()), np.array2string(zi, precision=2),
                                                                     int(silent.sum())))
    assert np.all(np.abs(ma[silent] - mb[silent]) <= 1e-6 * np.maximum(mb[silent], 1.0))
    assert np.all(np.abs(z) <= 4), float(np.abs(z).max())
    assert np.all(np.abs(zi) < 4), zi
    for k in ("env_sample", "env_unoccluded", "env_occluded", "env_miss_mis", "env_area_sample", "env_emit_scaled"):
        assert cnt[k] >= 100, (k, cnt[k])
    orc32.free_all()


# ---- the hand-built maps reach their branches --------------------------------------------------------------------------------
def test_edge_maps_reach_their_counters(orc32):
    nx, ny, ns = 32, 24, 8
    cam, world = eo.well(orc32, nx, ny)
    m = eo.zero_rows_map()
    orc32.reset_counters()
    orc32.render_env(cam, world, NO_LIGHTS, m, env_ref.tables(m), True, 0.5, nx, ny, ns, seed=SEED, flags=DEV)
    assert orc32.counters()["env_miss_one"] >= 100
    m = eo.poles_map()
    orc32.reset_counters()
    orc32.render_env(cam, world, NO_LIGHTS, m, env_ref.tables(m), True, 0.5, 64, 48, 32, seed=SEED, flags=DEV)
    cnt = orc32.counters()
    assert cnt["env_no_sample"] >= 100 and cnt["env_sample"] > 1000 * cnt["env_no_sample"], cnt
    orc32.free_all()
