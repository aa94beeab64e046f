"""rtmi_render_roulette's plain estimator (include/rtmi_roulette.h) against the numpy restatement of
tests/roulette_ref.py, bit for bit: mean radiance, rgb8, the standard-error plane and, in the closed scenes, the bounce
counts.  The restatement needs only the unchanged fp32 oracle's per-sample radiances (tests/test_roulette_ref.py checks
it on the CPU).  Open, closed and coloured boxes; (min_depth, q_min) pairs with min_depth = 1 and 3, two whose floor
never binds and two whose floor does (paths survive tests with q = q_min on every box); FAST_CULL on and off, SYNC,
REF_TREE, a ragged 25 x 17 image and passes forced through sample_buffer_bytes."""
import numpy as np
import pytest

import roulette_ref as rr
from oracle.oracle import ARITH_DEVICE, THROUGHPUT_FORM
from raytracing_rust_amd import abi

SEED = 42
FC = abi.RTMI_FLAG_FAST_CULL
OFLAGS = ARITH_DEVICE | THROUGHPUT_FORM
# (min_depth, q_min, the floor binds).  A survivor is rescaled to a largest channel of about 1, so m < q_min happens only
# where q_min exceeds max(a)^min_depth (at the first test) or max(a) (at every test): the last two pairs, on every box.
PAIRS = [(1, 0.2, False), (3, 0.05, False), (3, 0.5, True), (1, 0.8, True)]
DEVICE_FLAGS = [("fast", dict(flags=FC)), ("exact", dict(flags=0)), ("sync", dict(flags=FC | abi.RTMI_FLAG_SYNC)),
                ("reftree", dict(flags=FC | abi.RTMI_FLAG_REF_TREE))]


def _bits(a, b):
    return int(np.sum(a.view(np.uint32) != b.view(np.uint32)))


def _case(host, orc32, name, nx, ny, ns, variants, pairs=PAIRS):
    albedo, closed, max_depth = rr.BOXES[name]
    cam_o, world_o = rr.box(orc32, name, nx, ny)
    ref = orc32.render_samples(cam_o, world_o, nx, ny, ns, seed=SEED, flags=OFLAGS, max_depth=max_depth)
    orc32.free_all()
    k = rr.lookup_k(ref["samples"], albedo, rr.LE, max_depth)
    cam, world = rr.box(host, name, nx, ny)
    sc = host.lower(world).upload(0)
    plain_scat = np.where(k >= 0, k, max_depth).sum(-1)
    for min_depth, q_min, floor_binds in pairs + [(max_depth + 1, 0.05, False)]:
        smp, scat, floored = rr.restate(k, albedo, rr.LE, max_depth, min_depth, q_min, SEED, nx, closed)
        lin, rgb = rr.image(smp)
        se = rr.welford_stderr(smp)
        if min_depth <= max_depth:
            assert smp.tobytes() != ref["samples"].tobytes()  # the pair does something
        # the floor is reached where it is meant to be: lit paths survived tests with q = q_min, and q = m there would
        # have given other bits
        assert (floored > 0) == floor_binds, (name, min_depth, q_min, floored)
        if floor_binds:
            assert rr.restate(k, albedo, rr.LE, max_depth, min_depth, 1e-30, SEED, nx, closed)[0].tobytes() != smp.tobytes()
        for label, kw in variants:
            got = sc.render_roulette(cam, nx, ny, ns, estimator="plain", min_depth=min_depth, q_min=q_min, seed=SEED,
                                     max_depth=max_depth, **kw)
            what = "%s %s min_depth %d q_min %g" % (name, label, min_depth, q_min)
            bad = _bits(got["linear"], lin)
            print("\nRR-EXACT %s: %d of %d channels differ, %d stderr, bounces/sample %.2f, %d survivals at q = q_min" % (
                what, bad, lin.size, _bits(got["stderr"], se), got["bounces"].sum() / (nx * ny * ns), floored))
            assert bad == 0, "%s: %d channels differ (max |diff| %g)" % (what, bad, float(np.abs(got["linear"].astype(np.float64) - lin).max()))
            assert np.array_equal(got["rgb8"], rgb), what
            assert _bits(got["stderr"], se) == 0, what
            assert got["stats"]["samples"] == nx * ny * ns
            if closed:
                assert np.array_equal(got["bounces"].astype(np.int64), scat.sum(-1)), what
            elif min_depth > max_depth:  # an open scene's unlit paths may leave the world: their length is not restated
                assert np.all(got["bounces"] >= np.where(k >= 0, k, 0).sum(-1)), what
            if min_depth > max_depth and closed:
                assert np.array_equal(got["bounces"].astype(np.int64), plain_scat), what
    return sc, cam


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(rr.BOXES))
def test_boxes_equal_restatement(host, orc32, name):
    _case(host, orc32, name, 32, 32, 16, DEVICE_FLAGS)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["closed", "open"])
def test_ragged_image_and_passes_equal_restatement(host, orc32, name):
    """25 x 17: partial 8 x 8 tiles on both edges; a per-sample buffer of 5 samples: 16 samples in four passes."""
    nx, ny, ns = 25, 17, 16
    tiles = ((nx + 7) // 8) * ((ny + 7) // 8)
    _case(host, orc32, name, nx, ny, ns, [("ragged", dict(flags=FC)), ("ragged-exact", dict(flags=0)),
                                          ("passes", dict(flags=FC, sample_buffer_bytes=tiles * 64 * 12 * 5))])


@pytest.mark.gpu
def test_two_samples_and_shade_threshold(host, orc32):
    _case(host, orc32, "closed", 16, 16, 2, [("ns2", dict(flags=FC)), ("threshold", dict(flags=FC, shade_threshold=1))],
          pairs=[(1, 0.2, False), (1, 0.8, True)])
