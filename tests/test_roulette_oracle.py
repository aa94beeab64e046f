"""The oracle's restatement of Russian roulette (oracle/rt_oracle.c roulette_ends / orc_render_roulette;
include/rtmi_roulette.h), checked on the CPU:

* with no test made (min_depth > max_depth), or no draw made (q_min = 1, on scenes whose throughput never reaches 0), it
  is the named estimator bit for bit, and its bounce plane adds up to the oracle's scatter counters;
* its plain estimator equals tests/roulette_ref.py's numpy restatement, sample for sample and scatter for scatter: two
  restatements of one header that share no code;
* a roulette path is a prefix: every plain roulette sample is 0 or the unrouletted sample scaled by its chain of 1 / q;
* roulette NEE has NEE's expectation, at the |z| <= 4 per-tile criterion of tests/test_gpu_env.py;
* a black surface ends continuations by m == 0, without a draw."""
import numpy as np
import pytest

import env_oracle_ref as eo
import env_ref
import roulette_ref as rr
from nee_oracle_ref import welford_stderr
from oracle.oracle import ARITH_DEVICE, THROUGHPUT_FORM
from test_gpu_nee import _tile_z

SEED = 42
DEV = ARITH_DEVICE | THROUGHPUT_FORM
SCATTERS = ("sc_lambert", "sc_metal", "sc_dielectric", "sc_isotropic")


def _named(orc, est, cam, world, lights, m, T, nx, ny, ns, **kw):
    if est == "plain":
        return orc.render_samples(cam, world, nx, ny, ns, seed=SEED, flags=DEV, **kw)
    if est == "nee":
        return orc.render_nee(cam, world, lights, nx, ny, ns, seed=SEED, flags=DEV, samples=True, **kw)
    return orc.render_env(cam, world, lights, m, T, est == "env_nee", 0.25, nx, ny, ns, seed=SEED, flags=DEV, samples=True, **kw)


# ---- reductions -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("est", ["plain", "nee", "env", "env_nee"])
@pytest.mark.parametrize("name", ["cornell_box", "lit_smoke", "lit_random_spheres"])
def test_disabled_roulette_is_the_named_estimator(host, orc32, name, est):
    """Without a test the bounce plane adds up to the oracle's scatter counters (no Metal here but in lit_random_spheres,
    whose absorbing Metal calls the counter also counts).  With q_min = 1 no draw is made; only lit_smoke's black fog
    brings a throughput to exactly 0, which ends the continuation with nothing left to add: same image, fewer bounces."""
    nx, ny, ns = 16, 12, 4
    cam_h, world_h = eo.build(host, name, nx, ny)
    cam, world = eo.build(orc32, name, nx, ny)
    lights, _ = eo.lights_for(host, orc32, world_h, world)
    m = env_ref.sun_map()
    T = env_ref.tables(m)
    for max_depth, min_depth, q_min in ((50, 2, 1.0), (50, 51, 0.05), (4, 5, 0.05)):
        orc32.reset_counters()
        ref = _named(orc32, est, cam, world, lights, m, T, nx, ny, ns, max_depth=max_depth)
        scat = sum(orc32.counters()[k] for k in SCATTERS)
        orc32.reset_counters()
        got = orc32.render_roulette(cam, world, lights, m, T, est, min_depth, q_min, 0.25, nx, ny, ns, seed=SEED, flags=DEV,
                                    max_depth=max_depth, samples=True)
        cnt = orc32.counters()
        for k in ("linear", "rgb", "mean", "samples"):
            assert np.array_equal(got[k], ref[k]), (name, est, min_depth, q_min, k)
        total = int(got["bounces"].sum())
        assert cnt["rr_draw"] == 0 and (cnt["rr_test"] > 0) == (q_min == 1.0)
        assert (cnt["rr_zero"] > 0) == (q_min == 1.0 and name == "lit_smoke"), cnt["rr_zero"]
        if name == "lit_random_spheres":
            assert 0 < total <= scat
        elif cnt["rr_zero"]:
            assert 0 < total < scat
        else:
            assert total == scat
    orc32.free_all()


# ---- against the numpy restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_depth,q_min", [(1, 0.05), (3, 0.05), (1, 0.5), (1, 0.8), (2, 1.0)])
@pytest.mark.parametrize("name", sorted(rr.BOXES))
def test_plain_roulette_equals_the_numpy_restatement(orc32, name, min_depth, q_min):
    nx, ny, ns = 24, 24, 16
    albedo, closed, max_depth = rr.BOXES[name]
    cam, world = rr.box(orc32, name, nx, ny)
    ref = orc32.render_samples(cam, world, nx, ny, ns, seed=SEED, flags=DEV, max_depth=max_depth)
    k = rr.lookup_k(ref["samples"], albedo, rr.LE, max_depth)
    want, scat, floored = rr.restate(k, albedo, rr.LE, max_depth, min_depth, q_min, SEED, nx, closed)
    orc32.reset_counters()
    got = orc32.render_roulette(cam, world, None, None, None, "plain", min_depth, q_min, 0.5, nx, ny, ns, seed=SEED, flags=DEV,
                                max_depth=max_depth, samples=True)
    cnt = orc32.counters()
    bad = int(np.sum(got["samples"].view(np.uint32) != want.view(np.uint32)))
    assert bad == 0, "%s: %d sample channels differ" % (name, bad)
    lin, rgb = rr.image(want)
    assert lin.tobytes() == got["linear"].tobytes() and np.array_equal(rgb.astype(np.int32), got["rgb"])
    if closed:
        assert np.array_equal(got["bounces"].astype(np.int64), scat.sum(-1))
    # the oracle counts the floor's survivals on every path, the restatement on the lit ones only
    assert cnt["rr_floor_survive"] >= floored and (floored > 0) <= (cnt["rr_floor_survive"] > 0)
    assert cnt["rr_end_pending"] == 0 and (cnt["rr_draw"] > 0) == (q_min < 1.0)
    orc32.free_all()


# ---- a roulette path is a prefix --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_depth,q_min", [(1, 0.05), (3, 0.5)])
def test_plain_roulette_sample_is_zero_or_the_rescaled_sample(orc32, min_depth, q_min):
    """cornell_box (one lamp, so a lit sample is T * Le): a roulette sample is 0 (cut, or unlit anyway) or the
    unrouletted sample times a product of 1 / q >= 1: per channel at least the plain value and at most plain / q_min^d
    (d tests at the most: one per scatter), within the roundings of d divisions."""
    nx, ny, ns, max_depth = 32, 32, 32, 50
    cam, world = eo.build(orc32, "cornell_box", nx, ny)
    ref = orc32.render_samples(cam, world, nx, ny, ns, seed=SEED, flags=DEV, max_depth=max_depth)["samples"]
    got = orc32.render_roulette(cam, world, None, None, None, "plain", min_depth, q_min, 0.5, nx, ny, ns, seed=SEED, flags=DEV,
                                max_depth=max_depth, samples=True)
    smp = got["samples"]
    cut = np.all(smp == 0, axis=-1)
    assert np.all(smp[ref == 0] == 0), "roulette lit a sample the plain path left dark"
    live = ~cut
    assert live.sum() > 100 and (cut & np.any(ref != 0, -1)).sum() > 100
    ratio = smp[live].astype(np.float64) / ref[live]
    assert np.all(ratio >= 1.0 - 1e-5), float(ratio.min())
    # one factor for the three channels: the chain of 1 / q does not depend on the channel
    assert np.all(np.abs(ratio / ratio[:, :1] - 1.0) <= 1e-5)
    assert np.any(ratio > 1.5)
    orc32.free_all()


# ---- expectation ------------------------------------------------------------------------------------------------------------
def test_roulette_nee_has_nees_expectation(host, orc32):
    nx, ny, ns = 32, 24, 256
    cam_h, world_h = eo.build(host, "cornell_box", nx, ny)
    cam, world = eo.build(orc32, "cornell_box", nx, ny)
    lights, _ = eo.lights_for(host, orc32, world_h, world)
    a = orc32.render_roulette(cam, world, lights, None, None, "nee", 1, 0.5, 0.5, nx, ny, ns, seed=SEED, flags=DEV, samples=True)
    b = orc32.render_nee(cam, world, lights, nx, ny, ns, seed=SEED + 1, flags=DEV, samples=True)
    for r in (a, b):
        r["stderr"] = welford_stderr(r["samples"])
    z, zi, silent, _ = _tile_z(a, b)
    print("\nRR-ORACLE-Z max |z| %.2f image-mean z %s silent %d" % (float(np.abs(z).max()), np.array2string(zi, precision=2),
                                                                    int(silent.sum())))
    assert not silent.any()
    assert np.all(np.abs(z) <= 4), float(np.abs(z).max())
    assert np.all(np.abs(zi) < 4), zi
    assert a["bounces"].sum() < 0.5 * nx * ny * ns * 10  # and the paths are short
    orc32.free_all()


# ---- m == 0 -----------------------------------------------------------------------------------------------------------------
def test_black_surfaces_end_paths_without_a_draw(host, orc32):
    nx, ny, ns = 24, 16, 8
    cam_h, world_h = eo.black_room(host, nx, ny)
    cam, world = eo.black_room(orc32, nx, ny)
    lights, _ = eo.lights_for(host, orc32, world_h, world)
    ref = orc32.render_nee(cam, world, lights, nx, ny, ns, seed=SEED, flags=DEV, samples=True)
    orc32.reset_counters()
    got = orc32.render_roulette(cam, world, lights, None, None, "nee", 1, 1.0, 0.5, nx, ny, ns, seed=SEED, flags=DEV, samples=True)
    cnt = orc32.counters()
    assert cnt["rr_zero"] >= 100 and cnt["rr_draw"] == 0
    # a throughput of 0 had nothing left to add: the image is NEE's, the paths are shorter
    assert np.array_equal(got["samples"], ref["samples"])
    assert 0 < got["bounces"].sum()
    orc32.free_all()
