"""rtmi_render_env (include/rtmi_env.h) against the fp32 oracle's restatement of it (orc_render_env), bit for bit: mean
radiance, rgb8 and path signatures, and the standard-error plane against rtmi_adaptive.h's Welford recurrence over the
oracle's per-sample radiances.  The oracle gets the map's tables from tests/env_ref.py, not from the product.  No
tolerance anywhere: the planes are compared as bits.

Every case names the oracle counters (oracle.ENV_COUNTERS) it is there to reach and asserts that each reached 100;
test_every_counter_has_a_case checks that no counter is left without one.  Counts seen on the CPU are in the
docstrings."""
import numpy as np
import pytest

import env_oracle_ref as eo
import env_ref
import scenes_random
from nee_oracle_ref import EDGE
from oracle.oracle import ARITH_DEVICE, ENV_COUNTERS, FACE_FORWARD, THROUGHPUT_FORM, UV_BOOK
from raytracing_rust_amd import abi
from test_gpu_nee_oracle import DEVICE_FLAGS, _check, _dev_ext

SEED = 42
FC = abi.RTMI_FLAG_FAST_CULL
DEV = ARITH_DEVICE | THROUGHPUT_FORM
TWO = DEVICE_FLAGS[:2]  # fast, exact
SAMPLED = ("env_sample", "env_unoccluded", "env_miss_mis")
MIXED = SAMPLED + ("env_occluded", "env_area_sample", "env_emit_scaled")

_MAPS = {}


def _map(name):
    if name not in _MAPS:
        m = eo.maps()[name]
        _MAPS[name] = (m, env_ref.tables(m))
    return _MAPS[name]


def _flag_sets(nx, ny, every):
    """fast and exact always; with `every` also reftree, sync and a sample buffer of five samples (several passes)."""
    sets = [(n, f, {}) for n, f in (DEVICE_FLAGS if every else TWO)]
    if every:
        sets.append(("passes", FC, dict(sample_buffer_bytes=nx * ny * 12 * 5)))
    return sets


def _env_case(host, orc32, label, build, nx, ny, ns, mapname, nee, p, oflags=0, every=False, expect=(), absent=()):
    """Renders `build` under the map on the oracle once and on the device under each flag set; returns (the oracle's
    dict, its counters)."""
    cam_h, world_h = build(host, nx, ny)
    cam_o, world_o = build(orc32, nx, ny)
    lights, sc = eo.lights_for(host, orc32, world_h, world_o)
    m, T = _map(mapname)
    orc32.reset_counters()
    ref = orc32.render_env(cam_o, world_o, lights, m, T, nee, p, nx, ny, ns, seed=SEED, flags=DEV | oflags, samples=True)
    cnt = orc32.counters()
    for k in expect:
        assert cnt[k] >= 100, "%s: the case is there for %s, which it reached %d times" % (label, k, cnt[k])
    for k in absent:
        assert cnt[k] == 0, (label, k, cnt[k])
    sc.upload(0, nee=True)
    assert len(sc.lights()) == len(lights)
    sc.attach_env(m)
    for fl, dflags, kw in _flag_sets(nx, ny, every):
        got = sc.render_env(cam_h, nx, ny, ns, nee=nee, env_select_p=p, sig=True, seed=SEED, flags=dflags | _dev_ext(oflags), **kw)
        _check("%s/%s" % (label, fl), got, ref)
    orc32.free_all()
    return ref, cnt


def _named(name):
    return lambda api, nx, ny: eo.build(api, name, nx, ny)


# ---- emitter-less scenes: an empty light table, p_env = 1 -------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mapname", ["sun", "64x32"])
@pytest.mark.parametrize("nee", [False, True], ids=["bsdf", "nee"])
@pytest.mark.parametrize("name", ["random_spheres", "two_perlin_spheres", "earth", "final_scene"])
def test_emitterless_scenes_equal_oracle(host, orc32, name, nee, mapname):
    """40 x 30 x 12 under the sun map, nee=1: env_sample 6118 (earth) .. 46025 (final_scene), env_unoccluded 4858 .. 14619,
    env_miss_mis 6118 .. 13221, env_occluded 0 (earth: one sphere) .. 32470.  nee=0 draws no light sample at all."""
    nx, ny, ns = 40, 30, 12
    expect = SAMPLED + (("env_occluded",) if name != "earth" else ()) if nee else ()
    absent = ("env_area_sample", "env_emit_scaled") + (() if nee else ("env_sample", "env_miss_mis", "env_miss_one"))
    ref, _ = _env_case(host, orc32, "%s %s nee=%d" % (name, mapname, nee), _named(name), nx, ny, ns, mapname, nee, 0.5,
                       oflags=UV_BOOK if name == "earth" else 0, every=(name == "random_spheres" and mapname == "sun"),
                       expect=expect, absent=absent)
    assert np.any(ref["linear"] > 0)


# ---- lit scenes: the map and the area lights share the light samples --------------------------------------------------------
LIT = [("cornell_box", 0), ("lit_smoke", 0), ("lit_smoke", FACE_FORWARD), ("lit_random_spheres", 0), ("hollow_glass", 0),
       ("lit_final_scene", 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.5, 0.25, 1.0])
@pytest.mark.parametrize("name,oflags", LIT, ids=["%s-%d" % c for c in LIT])
def test_lit_scenes_equal_oracle(host, orc32, name, oflags, p):
    """40 x 30 x 12, the sun map (the 64x32 map at p = 0.25).  At p = 0.5: env_sample 5789 (hollow_glass) .. 24078
    (lit_smoke), env_area_sample 5618 .. 23851, env_emit_scaled 254 (cornell_box) .. 2210 (lit_smoke), env_occluded 903
    .. 16620, env_unoccluded 107 (lit_smoke: a closed room) .. 4820.  At p = 1 the area lights are never sampled, their
    density is 0 and an emitter hit has weight 1: both area counters stay 0 and env_sample doubles."""
    nx, ny, ns = 40, 30, 12
    if p < 1.0:
        expect = MIXED
        absent = ()
    else:
        expect, absent = SAMPLED + ("env_occluded",), ("env_area_sample", "env_emit_scaled")
    ref, _ = _env_case(host, orc32, "%s p=%g" % (name, p), _named(name), nx, ny, ns, "64x32" if p == 0.25 else "sun", True, p,
                       oflags=oflags, every=(name == "lit_random_spheres" and p == 0.5), expect=expect, absent=absent)
    assert np.any(ref["linear"] > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_box", "lit_smoke", "lit_random_spheres"])
def test_lit_scenes_without_nee_equal_oracle(host, orc32, name):
    """nee=0 on a scene that has lights: the table is not read and env_select_p does not matter."""
    nx, ny, ns = 40, 30, 12
    _env_case(host, orc32, "%s nee=0" % name, _named(name), nx, ny, ns, "sun", False, 0.25,
              absent=("env_sample", "env_area_sample", "env_emit_scaled", "env_miss_mis"))


# ---- map edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mapname", ["1x1", "3x2", "zero_rows", "seam", "poles"])
@pytest.mark.parametrize("name", ["random_spheres", "lit_random_spheres"])
def test_map_edges_equal_oracle(host, orc32, name, mapname):
    """32 x 24 x 16.  1x1 and 3x2: every index is an edge index.  zero_rows: BSDF rays leave through texels of pdf 0
    (env_miss_one 2945 on random_spheres).  seam: the lookup wraps across phi = +-pi.  poles: ct -> 0."""
    nx, ny, ns = 32, 24, 16
    expect = SAMPLED + (("env_miss_one",) if mapname == "zero_rows" else ())
    _env_case(host, orc32, "%s %s" % (name, mapname), _named(name), nx, ny, ns, mapname, True, 0.5, expect=expect)


@pytest.mark.gpu
def test_poles_map_has_light_samples_without_a_sample(host, orc32):
    """The shaft under the poles map, 64 x 48 x 32 (a cheap scene: 1 s on the oracle): 2.2 million light samples aim within
    4e-4 of the poles, and for 175 of them ct <= 0: no sample."""
    nx, ny, ns = 64, 48, 32
    _env_case(host, orc32, "well poles", eo.well, nx, ny, ns, "poles", True, 0.5,
              expect=SAMPLED + ("env_no_sample", "env_occluded"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_box", "lit_random_spheres"])
def test_map_that_cannot_be_sampled_is_nee(host, orc32, name):
    """total == 0: p_env = 0, no light sample aims at the map and the result is the oracle's NEE render."""
    nx, ny, ns = 32, 24, 16
    ref, _ = _env_case(host, orc32, "%s zero" % name, _named(name), nx, ny, ns, "zero", True, 0.5,
                       absent=("env_sample", "env_miss_mis", "env_area_sample", "env_emit_scaled"))
    cam_h, world_h = eo.build(host, name, nx, ny)
    cam_o, world_o = eo.build(orc32, name, nx, ny)
    lights, _ = eo.lights_for(host, orc32, world_h, world_o)
    nee = orc32.render_nee(cam_o, world_o, lights, nx, ny, ns, seed=SEED, flags=DEV, samples=True)
    for k in ("linear", "rgb", "sig", "samples"):
        assert np.array_equal(ref[k], nee[k]), k
    assert np.any(nee["linear"] > 0)
    orc32.free_all()


# ---- scene edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(EDGE))
def test_edge_scenes_equal_oracle(host, orc32, name):
    """tests/nee_oracle_ref.py's hand-built scenes under the sun map, 32 x 24 x 16, env_select_p = 0.5: light_in_medium's
    shadow rays toward the map draw free flights from stream 3, isotropic_rect's vertices have p_b = 1 / (4 pi)."""
    nx, ny, ns = 32, 24, 16
    ref, cnt = _env_case(host, orc32, name, EDGE[name], nx, ny, ns, "sun", True, 0.5, expect=("env_sample", "env_area_sample"))
    assert np.any(ref["linear"] > 0), name
    if name == "light_in_medium":
        assert cnt["medium_draw"] > 1000
    if name == "isotropic_rect":
        assert cnt["sc_isotropic"] > 100


@pytest.mark.gpu
def test_closed_box_equals_oracle(host, orc32):
    """The shaft with its lid on: 611938 light samples, 305866 shadow rays toward the map, all occluded but the 54 that
    slip through a corner within t_min, and all but about a hundred camera paths end inside, at the depth limit."""
    nx, ny, ns = 32, 24, 16
    ref, cnt = _env_case(host, orc32, "closed box", lambda api, nx, ny: eo.well(api, nx, ny, lid=True), nx, ny, ns, "sun",
                         True, 0.5, expect=("env_sample", "env_occluded"))
    assert cnt["env_unoccluded"] * 1000 < cnt["env_occluded"] and cnt["sc_lambert"] > 45 * nx * ny * ns


@pytest.mark.gpu
@pytest.mark.parametrize("nee", [False, True], ids=["bsdf", "nee"])
def test_ragged_image_equals_oracle(host, orc32, nee):
    """25 x 17: partial 8 x 8 tiles on both edges."""
    _env_case(host, orc32, "ragged nee=%d" % nee, _named("lit_random_spheres"), 25, 17, 16, "sun", nee, 0.5, every=True,
              expect=MIXED if nee else ())


# ---- random compositions ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("instanced", [False, True], ids=["plain", "instanced"])
@pytest.mark.parametrize("seed", range(1, 9))
def test_random_scenes_equal_oracle(host, orc32, seed, instanced):
    nx, ny, ns = 24, 16, 6

    def build(api, nx, ny):
        return scenes_random.build(api, seed, nx, ny, instanced=instanced)

    _env_case(host, orc32, "random %d" % seed, build, nx, ny, ns, "64x32", True, 0.5, oflags=FACE_FORWARD if seed % 3 == 1 else 0,
              expect=("env_sample", "env_area_sample"))


# ---- coverage ---------------------------------------------------------------------------------------------------------------
def test_every_counter_has_a_case():
    """Each counter of the environment estimator is named by a case above that asserts it reached 100."""
    named = set(MIXED) | {"env_miss_one", "env_no_sample"}
    assert named == set(ENV_COUNTERS)
