"""The yardstick of tests/test_gpu_roulette_exact.py, checked on the CPU: tests/roulette_ref.py restates Russian roulette
(include/rtmi_roulette.h) for the plain estimator from the unchanged oracle's per-sample radiances.

* on the uniform-albedo scenes every lit sample's scatter count k is found, uniquely, in the fp32 throughput chain;
* in the closed boxes sum(k) + unlit * max_depth equals the oracle's own scatter counters;
* q_min = 1 and min_depth > max_depth return the oracle's samples unchanged (and its image);
* the restated roulette image has the plain image's mean (|z| < 4, the image-mean rule of tests/test_gpu_nee.py), for
  pairs whose floor q_min never binds and pairs where it does (counted on the restated survivors' throughput);
* the stream-4 words are philox.py's."""
import math

import numpy as np
import pytest

import roulette_ref as rr
from oracle.oracle import ARITH_DEVICE, THROUGHPUT_FORM
from raytracing_rust_amd import philox

SEED = 42
OFLAGS = ARITH_DEVICE | THROUGHPUT_FORM
NX, NY, NS = 24, 24, 16


def _oracle(orc32, name):
    albedo, closed, max_depth = rr.BOXES[name]
    cam, world = rr.box(orc32, name, NX, NY)
    orc32.reset_counters()
    ref = orc32.render_samples(cam, world, NX, NY, NS, seed=SEED, flags=OFLAGS, max_depth=max_depth)
    cnt = orc32.counters()
    orc32.free_all()
    return ref, cnt, albedo, closed, max_depth


@pytest.mark.parametrize("name", sorted(rr.BOXES))
def test_lookup_is_total_and_scatters_add_up(orc32, name):
    ref, cnt, albedo, closed, max_depth = _oracle(orc32, name)
    k = rr.lookup_k(ref["samples"], albedo, rr.LE, max_depth)  # asserts: every lit sample matches exactly one row
    lit = k >= 0
    assert lit.sum() > NX * NY * NS // 50, "too few lit samples (%d) to test anything" % int(lit.sum())
    assert cnt["sc_metal"] == cnt["sc_dielectric"] == cnt["sc_isotropic"] == 0
    total = int(k[lit].sum()) + int((~lit).sum()) * max_depth
    print("\nRR-REF %s lit %d of %d, sum k %d, oracle sc_lambert %d, closed-box total %d" % (
        name, int(lit.sum()), k.size, int(k[lit].sum()), cnt["sc_lambert"], total))
    if closed:
        assert total == cnt["sc_lambert"], (total, cnt["sc_lambert"])
    else:
        assert int(k[lit].sum()) <= cnt["sc_lambert"] <= total


@pytest.mark.parametrize("name", sorted(rr.BOXES))
def test_disabled_roulette_is_the_oracle(orc32, name):
    ref, cnt, albedo, closed, max_depth = _oracle(orc32, name)
    k = rr.lookup_k(ref["samples"], albedo, rr.LE, max_depth)
    for min_depth, q_min in ((1, 1.0), (max_depth + 1, 0.05)):
        smp, scat, floored = rr.restate(k, albedo, rr.LE, max_depth, min_depth, q_min, SEED, NX, closed)
        assert smp.tobytes() == ref["samples"].tobytes(), (min_depth, q_min)
        assert floored == 0
        lin, rgb = rr.image(smp)
        assert lin.tobytes() == ref["linear"].tobytes() and np.array_equal(rgb.astype(np.int32), ref["rgb"])
        if closed:
            assert int(scat.sum()) == cnt["sc_lambert"]


@pytest.mark.parametrize("name", sorted(rr.BOXES))
@pytest.mark.parametrize("min_depth,q_min,floor_binds", [(3, 0.05, False), (1, 0.2, False), (3, 0.5, True), (1, 0.8, True)])
def test_restated_roulette_has_the_plain_mean(orc32, name, min_depth, q_min, floor_binds):
    """A survivor is rescaled to a largest channel of about 1, so after the first test m is about max(a): q_min binds only
    where it exceeds max(a)^min_depth (the first test) or max(a) itself (every test).  The last two pairs do, on every
    box, and the count of survivals under q = q_min says so; the first two never reach their floor."""
    ref, cnt, albedo, closed, max_depth = _oracle(orc32, name)
    k = rr.lookup_k(ref["samples"], albedo, rr.LE, max_depth)
    smp, scat, floored = rr.restate(k, albedo, rr.LE, max_depth, min_depth, q_min, SEED, NX, closed)
    assert smp.tobytes() != ref["samples"].tobytes()
    assert (floored > 0) == floor_binds, (floored, floor_binds)
    if floor_binds:  # and the floor decides bits: without it (q = m) the samples differ
        assert rr.restate(k, albedo, rr.LE, max_depth, min_depth, 1e-30, SEED, NX, closed)[0].tobytes() != smp.tobytes()
    # a roulette sample is 0 or its plain sample rescaled upward; a path that survives is never shorter
    assert np.all((smp == 0) | (smp >= ref["samples"]))
    se_r, se_p = rr.welford_stderr(smp).astype(np.float64), rr.welford_stderr(ref["samples"]).astype(np.float64)
    lin_r, lin_p = rr.image(smp)[0].astype(np.float64), ref["linear"].astype(np.float64)
    npx = NX * NY
    z = (lin_r.mean((0, 1)) - lin_p.mean((0, 1))) / np.sqrt(((se_r ** 2).sum((0, 1)) + (se_p ** 2).sum((0, 1))) / npx ** 2)
    per = (float(scat.sum()) / scat.size) if closed else float("nan")
    print("\nRR-REF %s min_depth %d q_min %.2f image-mean z %s scatters/sample %.2f (plain %.2f), %d survivals at q = q_min" % (
        name, min_depth, q_min, np.array2string(z, precision=2), per, cnt["sc_lambert"] / (npx * NS), floored))
    assert np.all(np.abs(z) < 4), z
    if closed:
        assert np.all(scat <= np.where(k >= 0, k, max_depth)) and scat.sum() < cnt["sc_lambert"]


def test_stream_4_words_are_philox_py():
    rng = np.random.default_rng(3)
    d = rng.integers(1, 51, 64)
    s = rng.integers(0, 1 << 20, 64)
    p = rng.integers(0, 1 << 31, 64)
    for seed in (SEED, 0x0123456789ABCDEF):
        w = rr.philox_word0(d, s, p, 4, seed)
        u = rr.roulette_u(d, s, p, seed)
        for i in range(64):
            want = philox.roulette_word(seed, int(d[i]), int(s[i]), int(p[i]))
            assert int(w[i]) == want
            # block d of the sequential stream 4 of (sample, pixel) starts with the same word
            st = philox.Stream(seed, int(s[i]), int(p[i]), 4)
            st.ctr[0] = int(d[i])
            assert st.u32() == want
            assert float(u[i]) == (want >> 8) / 16777216.0 and math.isfinite(float(u[i])) and 0.0 <= u[i] < 1.0
