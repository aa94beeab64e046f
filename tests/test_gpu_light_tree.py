"""The light tree (include/rtmi_light_tree.h) on the device.

render_nee(light_tree=True) is rtmi_render_nee with another selection probability on the same paths, so:
1. the device's walks are the numpy restatement's bit for bit;
2. with one light it is render_nee() bit for bit;
3. without lights it is render() bit for bit;
4. with many lights its path signatures are render()'s, and it is deterministic and independent of the schedule;
5. it has the table estimator's expectation (8x8-tile z-scores, independent seeds);
6. it reproduces a known answer with four lights;
7. it is less noisy under a grid of lamps, by a pixel's own standard error and across independent seeds;
8. it is refused without an attached tree and on a multi-device handle."""
import ctypes as C

import numpy as np
import pytest

import light_tree_ref as ref
import light_tree_scenes as lts
import nee_ref
from raytracing_rust_amd import abi
from raytracing_rust_amd.host import HostError, Unsupported, default_params
from test_gpu_nee import NK, _floor_scene, _known_answer, _tile_z

FC = abi.RTMI_FLAG_FAST_CULL
SEED = 42
SIZES = [(64, 48), (25, 17)]
PLANES = ("linear", "rgb8", "stderr", "sig")


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the device's walks ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", lts.WITH_LIGHTS)
def test_probe_is_numpy_bit_for_bit(host, name):
    sc = host.lower(lts.build(host, name, 16, 16)[1]).upload(0, light_tree=True)
    nodes, paths = sc.light_tree()
    x, u = lts.probe_points(*ref.light_boxes(sc)[:2])
    light, p = sc.light_pick(x, u)
    want_light, want_p = ref.pick(nodes, x, u)
    assert np.array_equal(light, want_light)
    assert np.array_equal(_bits(p), _bits(want_p))
    assert np.array_equal(_bits(sc.light_pmf(x, light)), _bits(p))  # the reverse walk returns the pick's probability
    other = np.random.default_rng(5).integers(0, len(paths), len(u)).astype(np.uint32)
    assert np.array_equal(_bits(sc.light_pmf(x, other)), _bits(ref.pmf(nodes, paths, x, other)))
    with pytest.raises(HostError, match="outside the table"):
        sc.light_pmf(x[:4], np.array([0, len(paths), 0, 0], np.uint32))


# ---- 2. one light: the table's bits ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_box", "lit_smoke"])
def test_one_light_is_render_nee(host, name):
    for nx, ny in SIZES:
        cam, world = lts.build(host, name, nx, ny)
        sc = host.lower(world).upload(0, light_tree=True)
        assert len(sc.lights()) == 1
        t = sc.render_nee(cam, nx, ny, 8, sig=True, seed=SEED, flags=FC, light_tree=True)
        n = sc.render_nee(cam, nx, ny, 8, sig=True, seed=SEED, flags=FC)
        for k in PLANES:
            assert _same(t[k], n[k]), (name, nx, k)
        assert np.any(t["linear"])


# ---- 3. no light: render()'s bits -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_no_light_is_render(host):
    for nx, ny in SIZES:
        cam, world = lts.build(host, "final_scene", nx, ny)
        sc = host.lower(world)
        assert len(sc.lights()) == 0 and len(sc.light_tree()[0]) == 0
        t = sc.render_nee(cam, nx, ny, 6, sig=True, seed=SEED, flags=FC, light_tree=True)
        r = sc.render(cam, nx, ny, 6, sig=True, seed=SEED, flags=FC)
        for k in ("linear", "rgb8", "sig"):
            assert _same(t[k], r[k]), (nx, k)


# ---- 4. many lights: same paths, no schedule ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lit_random_spheres", "lamp_grid"])
def test_many_lights_same_paths_and_schedule_free(host, name):
    for nx, ny in SIZES:
        ns = 12
        cam, world = lts.build(host, name, nx, ny)
        sc = host.lower(world).upload(0, light_tree=True)
        assert len(sc.lights()) > 1
        a = sc.render_nee(cam, nx, ny, ns, sig=True, seed=SEED, flags=FC, light_tree=True)
        assert _same(a["sig"], sc.render(cam, nx, ny, ns, sig=True, seed=SEED, flags=FC)["sig"])
        assert np.all(np.isfinite(a["linear"])) and np.all(a["linear"] >= 0) and np.any(a["linear"])
        table = sc.render_nee(cam, nx, ny, ns, sig=True, seed=SEED, flags=FC)
        assert _same(a["sig"], table["sig"]) and not _same(a["linear"], table["linear"])  # another estimator on the same paths
        for kw in (dict(flags=FC), dict(flags=0), dict(flags=abi.RTMI_FLAG_REF_TREE | FC), dict(flags=abi.RTMI_FLAG_SYNC | FC),
                   dict(flags=FC, sample_buffer_bytes=nx * ny * 12 * 5)):
            b = sc.render_nee(cam, nx, ny, ns, sig=True, seed=SEED, light_tree=True, **kw)
            for k in PLANES:
                assert _same(a[k], b[k]), (name, nx, kw, k)


# ---- 5. the table estimator's expectation ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lit_random_spheres", "lamp_grid", "lit_final_scene"])
def test_same_expectation_as_the_table(host, name):
    nx, ny, ns = 64, 48, 512
    cam, world = lts.build(host, name, nx, ny)
    sc = host.lower(world).upload(0, light_tree=True)
    t = sc.render_nee(cam, nx, ny, ns, seed=SEED, flags=FC, light_tree=True)
    d = sc.render_nee(cam, nx, ny, ns, seed=SEED + 1, flags=FC)
    z, zi, silent, ma = _tile_z(t, d)
    q = np.percentile(np.abs(z), [50, 90, 99, 100])
    print("\nTREE-Z %s tiles %d |z| p50 %.2f p90 %.2f p99 %.2f max %.2f image-mean z %s; tile-channels without table variance %d"
          % (name, z.size // 3, q[0], q[1], q[2], q[3], np.array2string(zi, precision=2), int(silent.sum())))
    assert not silent.any() or ma[silent].max() <= 1e-6 * max(float(t["linear"].mean()), 1e-30), name
    assert np.abs(z).max() <= 5, (name, np.abs(z).max())
    assert np.all(np.abs(zi) < 4), (name, zi)


# ---- 6. a known answer with four lights -----------------------------------------------------------------------------------
class _WithTree:
    """a Scene whose render_nee selects from the light tree: what _known_answer renders"""

    def __init__(self, sc):
        self.sc = sc

    def render_nee(self, *a, **kw):
        return self.sc.render_nee(*a, light_tree=True, **kw)

    def render_adaptive(self, *a, **kw):
        return self.sc.render_adaptive(*a, **kw)


@pytest.mark.gpu
def test_known_answer_four_rect_lights(host):
    le, albedo = 4.0, 0.5
    world, geo = lts.four_rects(host, le, albedo)
    cam = _floor_scene(host, host.Sphere((0.0, -100.0, 0.0), 1.0, host.Lambertian(host.SolidTexture(0.5, 0.5, 0.5))), albedo)[0]
    sc = host.lower(world).upload(0, light_tree=True)
    assert len(sc.lights()) == 4
    n = np.array([0, 1.0, 0])

    def f_sum(x):
        parts = [nee_ref.f_rect(x, n, corner, ea, eb, 64, 64) for corner, ea, eb in geo]
        return sum(p[0] for p in parts), sum(p[1] for p in parts)

    got, want, se = _known_answer(_WithTree(sc), cam, f_sum, le, albedo)
    # every light matters to the answer: the image mean without the smallest contribution is outside its standard error
    x0 = np.zeros(3)
    smallest = min(nee_ref.f_rect(x0, n, corner, ea, eb, 64, 64)[0] for corner, ea, eb in geo)
    assert albedo * le * smallest > 5 * np.sqrt(np.sum(se ** 2)) / (NK * NK)


# ---- 7. less noise --------------------------------------------------------------------------------------------------------
# r, the median per-pixel stderr with the tree over the same median with the table, measured on an MI355X: 0.795 over 2781
# pixels.  That is above 0.7, the mark of a selection that does its job, so the bound below is not sized from it: it is
# (1 + 0.7) / 2, the most a working selection could be allowed.  Why r reads 0.795 (Noise): lamp_grid has
# direct light only (one planar floor, lamps that do not scatter, a black background), and with the table 79 % of a floor
# point's variance comes from BSDF-sampled hits of the nearest lamps, which MIS weights near 1 because the table's p_l is
# far below p_b there.  Those hits are rare and bright: most pixels see none in 64 samples, so a pixel's own Welford stderr
# under-reports the table's noise (numpy model of the estimator: median Welford 0.161 where the true value is 0.247; the
# tree's 0.118 and 0.125), and the median over pixels under-reports it again.  The model gives r = 0.74 for this statistic
# where the true ratio of standard deviations is 0.51.  The test after this one measures that ratio.
R_MEASURED = 0.795
R_WORKING = 0.7


@pytest.mark.gpu
def test_less_noise_under_a_grid_of_lamps(host):
    nx, ny, ns = 64, 48, 64
    cam, world = lts.build(host, "lamp_grid", nx, ny)
    sc = host.lower(world).upload(0, light_tree=True)
    t = sc.render_nee(cam, nx, ny, ns, seed=SEED, flags=FC, light_tree=True)
    d = sc.render_nee(cam, nx, ny, ns, seed=SEED, flags=FC)
    lit = (t["linear"].sum(-1) > 0) & (d["linear"].sum(-1) > 0)
    r = np.median(t["stderr"].mean(-1)[lit]) / np.median(d["stderr"].mean(-1)[lit])
    print("\nTREE-NOISE lamp_grid median stderr ratio tree / table %.3f over %d pixels" % (r, int(lit.sum())))
    assert r <= (1.0 + min(R_MEASURED, R_WORKING)) / 2.0, r


# The noise itself: the standard deviation of a pixel's 64-spp mean across independent seeds (16 x 64 samples per pixel: the
# rare hits are in it).  r_true = the median of that over the lit pixels with the tree / the same median with the table.
# Measured on an MI355X over 16 seeds: 0.541 (the numpy model of the estimator: 0.51), against 0.795 for the statistic
# above.  The bound is halfway from the measured value to "no gain", and the measured value has to be a working
# selection's.  The root of the MEAN variance over those pixels reads 0.916: a mean of variances is ruled by the few pixels
# that see a lamp's edge (radiance 20 or 100 against a floor of about 0.1), whose noise no light selection changes; the
# test prints it over all lit pixels and over the pixels whose samples all met the floor first (measured: 0.613 over 2348).
R_TRUE_MEASURED = 0.541
SEEDS = 16


@pytest.mark.gpu
def test_less_noise_across_seeds(host):
    nx, ny, ns = 64, 48, 64
    cam, world = lts.build(host, "lamp_grid", nx, ny)
    sc = host.lower(world).upload(0, light_tree=True)
    tree = np.array([sc.render_nee(cam, nx, ny, ns, seed=SEED + k, flags=FC, light_tree=True)["linear"] for k in range(SEEDS)], np.float64)
    table = np.array([sc.render_nee(cam, nx, ny, ns, seed=SEED + k, flags=FC)["linear"] for k in range(SEEDS)], np.float64)
    lit = (tree[0].sum(-1) > 0) & (table[0].sum(-1) > 0)
    vt, vd = tree.var(0, ddof=1).mean(-1), table.var(0, ddof=1).mean(-1)
    r_true = float(np.median(np.sqrt(vt[lit])) / np.median(np.sqrt(vd[lit])))
    # the floor's albedo is 0.7, a lamp's feature albedo min(Le, 1) = 1: a pixel whose mean is above 0.7 saw a lamp directly
    floor = lit & (sc.render_features(cam, nx, ny, 256, seed=SEED, flags=FC)["albedo"].max(-1) < 0.7005)
    print("\nTREE-NOISE lamp_grid across %d seeds: ratio of median standard deviations tree / table %.3f over %d pixels; root of "
          "the mean variance %.3f over them, %.3f over the %d that see the floor only" % (
              SEEDS, r_true, int(lit.sum()), np.sqrt(vt[lit].mean() / vd[lit].mean()),
              np.sqrt(vt[floor].mean() / vd[floor].mean()), int(floor.sum())))
    assert R_TRUE_MEASURED <= R_WORKING
    assert r_true <= (1.0 + R_TRUE_MEASURED) / 2.0, r_true


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(host):
    nx, ny = 16, 16
    cam, world = lts.build(host, "mixed", nx, ny)
    sc = host.lower(world).upload(0, nee=True)  # the table, not the tree
    p = default_params(nx, ny, 2, flags=FC | abi.RTMI_FLAG_LIGHT_TREE)
    lin = np.zeros((ny, nx, 3), np.float32)
    rc = host.lib.rth_render_nee(sc.h, cam.h, C.byref(p), lin.ctypes.data, None, None, None, None)
    assert rc != 0
    with pytest.raises(HostError, match="rtmi_scene_attach_light_tree"):
        host._check(rc)
    assert not lin.any()
    sc.attach_light_tree()
    with pytest.raises(Unsupported, match="LIGHT_COOP"):
        sc.render_nee(cam, nx, ny, 2, flags=FC, light_tree=True, coop=True)
    assert np.any(sc.render_nee(cam, nx, ny, 2, flags=FC, light_tree=True)["linear"])
    sc.attach_lights()  # a new table detaches the tree
    rc = host.lib.rth_render_nee(sc.h, cam.h, C.byref(p), lin.ctypes.data, None, None, None, None)
    with pytest.raises(HostError, match="rtmi_scene_attach_light_tree"):
        host._check(rc)
    multi = host.lower(lts.build(host, "mixed", nx, ny)[1])
    multi.upload_multi([0])
    try:
        with pytest.raises(Unsupported):
            multi.render_nee(cam, nx, ny, 2, light_tree=True)
        with pytest.raises(Unsupported):
            multi.attach_light_tree()
        with pytest.raises(Unsupported):
            multi.light_pick(np.zeros((1, 3), np.float32), np.zeros(1, np.float32))
    finally:
        multi.free_multi()
