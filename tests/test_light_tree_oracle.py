"""The oracle's restatement of the light-tree estimator (include/rtmi_light_tree.h; oracle/rt_oracle.c: tree_pick, tree_pmf,
color_nee with a tree), without a GPU, so that the oracle is not a second copy of the device's mistakes:

* its walks are the numpy restatement's (tests/light_tree_ref.py) and the host's rtmi_light_tree_pick / _pmf bit for bit;
* its tree comes from its own emitters and is the host's byte for byte (tests/light_tree_oracle_ref.py);
* with one light and with none the tree render is the table render and the plain render bit for bit;
* with many lights it keeps the paths and changes the samples;
* a render without a tree touches no tree counter;
* in f64 it converges to a known answer with four lights and has the table estimator's expectation;
* the corpus of tests/test_gpu_light_tree_oracle.py reaches every branch of the tree estimator."""
import ctypes as C

import numpy as np
import pytest

import light_tree_oracle_ref as lto
import light_tree_ref as ref
import light_tree_scenes as lts
import nee_ref
from nee_oracle_ref import light_table, oracle_lights, welford_stderr
from oracle.oracle import ARITH_DEVICE, LIGHT_NODE_DTYPE, LIGHT_PATH_DTYPE, SKY, THROUGHPUT_FORM, TREE_COUNTERS
from raytracing_rust_amd import abi
from raytracing_rust_amd import host as host_mod
from test_gpu_nee import _tile_z
from test_light_tree_ref import _c_pick, _c_pmf
from test_nee_oracle import NK, _converges, _floor_scene

DEV = ARITH_DEVICE | THROUGHPUT_FORM
SEED = 42
PLANES = ("linear", "rgb", "sig", "samples")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _both(host, orc, name, nx, ny):
    """the scene on the oracle and lowered by the host: (cam_o, world_o, sc, lights, tree)"""
    cam_o, world_o = lto.build(orc, name, nx, ny)
    sc = host.lower(lto.build(host, name, nx, ny)[1])
    return cam_o, world_o, sc, oracle_lights(orc, world_o, sc), lto.oracle_tree(orc, world_o, sc)


# ---- the walks ------------------------------------------------------------------------------------------------------------
def test_dtypes_are_the_products():
    for mine, theirs, ct in ((LIGHT_NODE_DTYPE, host_mod.LIGHT_NODE_DTYPE, abi.LightNode),
                             (LIGHT_PATH_DTYPE, host_mod.LIGHT_PATH_DTYPE, abi.LightPath)):
        assert mine.itemsize == theirs.itemsize == C.sizeof(ct)
        assert mine.names == theirs.names
        for k in mine.names:
            assert mine.fields[k][1] == theirs.fields[k][1] and mine.fields[k][0] == theirs.fields[k][0], k
    assert LIGHT_NODE_DTYPE.itemsize == 32 and LIGHT_PATH_DTYPE.itemsize == 8


@pytest.mark.parametrize("name", lts.WITH_LIGHTS + sorted(lto.EXTREME))
def test_walks_equal_numpy_and_host(host, orc32, name):
    _, _, sc, _, (nodes, paths) = _both(host, orc32, name, 16, 16)
    orc32.free_all()
    x, u = lts.probe_points(*ref.light_boxes(sc)[:2])
    assert len(u) >= 10 ** 4
    light, p = orc32.light_tree_pick(nodes, x, u)
    for want_light, want_p in (ref.pick(nodes, x, u), _c_pick(sc.light_tree()[0], x, u)):
        assert np.array_equal(light, want_light)
        assert np.array_equal(_bits(p), _bits(want_p))
    back = orc32.light_tree_pmf(nodes, paths, x, light)
    assert np.array_equal(_bits(back), _bits(p))  # the reverse walk returns the pick's probability
    other = np.random.default_rng(5).integers(0, len(paths), len(u)).astype(np.uint32)
    got = orc32.light_tree_pmf(nodes, paths, x, other)
    assert np.array_equal(_bits(got), _bits(ref.pmf(nodes, paths, x, other)))
    assert np.array_equal(_bits(got), _bits(_c_pmf(*sc.light_tree(), x, other)))
    with pytest.raises(RuntimeError):
        orc32.light_tree_pmf(nodes, paths, x[:2], np.array([0, len(paths)], np.uint32))


@pytest.mark.parametrize("name", sorted(lto.EXTREME))
def test_extreme_powers_round_a_probability_to_one(host, orc32, name):
    """The header's known limit: powers 1e4 and 2.5e-5, pl (the speck on the right) or pr (on the left) exactly 1.0f at
    about 19 760 of 20 000 floor points, and the speck's pmf there positive."""
    _, _, sc, lights, (nodes, paths) = _both(host, orc32, name, 16, 16)
    orc32.free_all()
    em_power = ref.light_boxes(sc)[2]
    # the speck's corners are 8 +- 0.005 rounded to float: its sides are 0.01 within 2^-24 * 8 / 0.01 < 1e-4 of themselves
    assert np.allclose(sorted(em_power.tolist()), [0.01 * 0.01 * 0.25, 100.0 * 100.0], rtol=2e-4, atol=0)
    speck = int(np.argmin(em_power))
    assert paths["trail"][speck] == (1 if name == "extreme_powers" else 0) and paths["depth"][speck] == 1
    rng = np.random.default_rng(1)
    x = np.zeros((20000, 3), np.float32)
    x[:, 0], x[:, 2] = rng.uniform(-20, 20, 20000), rng.uniform(-20, 20, 20000)
    big = orc32.light_tree_pmf(nodes, paths, x, np.full(len(x), 1 - speck, np.uint32))
    small = orc32.light_tree_pmf(nodes, paths, x, np.full(len(x), speck, np.uint32))
    one = big == np.float32(1.0)
    assert one.sum() > 19000, int(one.sum())
    # s = I_big + I_small rounds to I_big once I_small is under half an ulp of it: at most 2^-24 of it
    assert np.all(small[one] > 0) and small[one].max() <= 2.0 ** -24


# ---- the render where the tree must change nothing ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_box", "lit_smoke", "one_light"])
def test_one_light_is_the_table_render(host, orc32, name):
    nx, ny, ns = 16, 12, 4
    cam, world, sc, lights, tree = _both(host, orc32, name, nx, ny)
    assert len(lights) == 1 and len(tree[0]) == 2
    orc32.reset_counters()
    a = orc32.render_nee(cam, world, lights, nx, ny, ns, seed=SEED, flags=DEV, samples=True, tree=tree)
    cnt = orc32.counters()
    assert all(cnt[k] == 0 for k in TREE_COUNTERS)  # today's code path
    b = orc32.render_nee(cam, world, lights, nx, ny, ns, seed=SEED, flags=DEV, samples=True)
    for k in PLANES:
        assert a[k].tobytes() == b[k].tobytes(), (name, k)
    assert np.any(a["linear"] > 0)
    orc32.free_all()


def test_no_light_is_the_plain_render(host, orc32):
    nx, ny, ns = 16, 12, 4
    cam, world, sc, lights, tree = _both(host, orc32, "no_light", nx, ny)
    assert len(lights) == 0 and len(tree[0]) == 0 and len(tree[1]) == 0
    a = orc32.render_nee(cam, world, lights, nx, ny, ns, seed=SEED, flags=DEV | SKY, samples=True, tree=tree)
    b = orc32.render_samples(cam, world, nx, ny, ns, seed=SEED, flags=DEV | SKY)
    for k in PLANES:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.any(a["linear"] > 0)
    with pytest.raises(RuntimeError):  # a tree that is not the table's
        orc32.render_nee(cam, world, lights, nx, ny, ns, tree=(np.zeros(2, LIGHT_NODE_DTYPE), np.zeros(1, LIGHT_PATH_DTYPE)))
    orc32.free_all()


# ---- many lights: the same paths, another estimator -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lamp_grid", "mixed", "lit_random_spheres"])
def test_many_lights_keep_the_paths(host, orc32, name):
    nx, ny, ns = 24, 16, 6
    cam, world, sc, lights, tree = _both(host, orc32, name, nx, ny)
    assert len(lights) > 1
    orc32.reset_counters()
    table = orc32.render_nee(cam, world, lights, nx, ny, ns, seed=SEED, flags=DEV, samples=True)
    plain = orc32.render(cam, world, nx, ny, ns, seed=SEED, flags=DEV)
    cnt = orc32.counters()
    assert all(cnt[k] == 0 for k in TREE_COUNTERS), {k: cnt[k] for k in TREE_COUNTERS}  # no render without a tree counts
    t = orc32.render_nee(cam, world, lights, nx, ny, ns, seed=SEED, flags=DEV, samples=True, tree=tree)
    cnt = orc32.counters()
    assert cnt["tree_walk"] > 0 and cnt["tree_left"] + cnt["tree_right"] >= cnt["tree_walk"]
    assert np.array_equal(t["sig"], table["sig"]) and np.array_equal(t["sig"], plain["sig"])
    assert not np.array_equal(t["samples"], table["samples"])
    assert np.all(np.isfinite(t["samples"])) and np.all(t["samples"] >= 0) and np.any(t["samples"] > 0)
    orc32.free_all()


# ---- f64: a known answer with four lights ---------------------------------------------------------------------------------
def test_f64_tree_converges_four_rect_lights(orc64):
    le, albedo = 4.0, 0.5
    world, geo = lts.four_rects(orc64, le, albedo)
    cam = _floor_scene(orc64, orc64.Sphere((0.0, -100.0, 0.0), 1.0, orc64.Lambertian(orc64.SolidTexture(0.5, 0.5, 0.5))), albedo)[0]
    n = np.array([0, 1.0, 0])

    def f_sum(x):
        parts = [nee_ref.f_rect(x, n, corner, ea, eb, 64, 64) for corner, ea, eb in geo]
        return sum(p[0] for p in parts), sum(p[1] for p in parts)

    orc64.reset_counters()
    got, want, se = _converges(orc64, cam, world, f_sum, le, albedo, 1024, n_lights=4, tree=True)
    cnt = orc64.counters()
    assert cnt["tree_walk"] > 0 and cnt["tree_left"] > 0 and cnt["tree_right"] > 0 and cnt["tree_hit_picked_mismatch"] == 0
    # every light matters to the answer: the image mean without the smallest contribution is outside its standard error
    smallest = min(nee_ref.f_rect(np.zeros(3), n, corner, ea, eb, 64, 64)[0] for corner, ea, eb in geo)
    assert albedo * le * smallest > 5 * np.sqrt(np.sum(se ** 2)) / (NK * NK)
    orc64.free_all()


# ---- f64: the table estimator's expectation -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lamp_grid", "mixed"])
def test_f64_same_expectation_as_the_table(orc64, name):
    """tests/test_gpu_light_tree.py's criterion on the literal restatement: 8 x 8 tiles of a tree render against a table
    render with another seed.  64 x 48 at 256 spp: 48 tiles, a few seconds for both renders on one core."""
    nx, ny, ns = 64, 48, 256
    cam, world = lto.build(orc64, name, nx, ny)
    em = orc64.emitters(world)
    idx = np.flatnonzero(em["eligible"])
    assert len(idx) > 1
    lights, tree = light_table(em, idx.tolist()), lto.emitter_tree(em[idx])

    def planes(out):
        return {"linear": out["mean"], "stderr": welford_stderr(out["samples"])}

    t = planes(orc64.render_nee(cam, world, lights, nx, ny, ns, seed=SEED, samples=True, tree=tree))
    d = planes(orc64.render_nee(cam, world, lights, nx, ny, ns, seed=SEED + 1, samples=True))
    z, zi, silent, ma = _tile_z(t, d)
    q = np.percentile(np.abs(z), [50, 90, 100])
    print("\nTREE-ORACLE-Z %s tiles %d |z| p50 %.2f p90 %.2f max %.2f image-mean z %s; tile-channels without table variance %d"
          % (name, z.size // 3, q[0], q[1], q[2], np.array2string(zi, precision=2), int(silent.sum())))
    assert not silent.any() or ma[silent].max() <= 1e-6 * max(float(t["linear"].mean()), 1e-30), name
    assert np.abs(z).max() <= 5, (name, np.abs(z).max())
    assert np.all(np.abs(zi) < 4), (name, zi)
    orc64.free_all()


# ---- the corpus reaches the branches --------------------------------------------------------------------------------------
def test_corpus_reaches_every_branch(host, orc32):
    """What tests/test_gpu_light_tree_oracle.py asserts of its reference renders, from the oracle alone: a scene that stops
    reaching its branch fails here, without a GPU."""
    print()
    lto.assert_branches_reached(host, orc32)
