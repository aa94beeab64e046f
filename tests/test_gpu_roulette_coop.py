"""RTMI_FLAG_ROULETTE_COOP (include/rtmi_roulette_coop.h) on the device: the four roulette estimators,
fixed and adaptive, on the wave-cooperative kernel.

The claim is "the same bits, another kernel": every comparison is on the raw bits of every output plane (linear, rgb8,
stderr, bounces, spp), and stats["kernel"] is asserted on both sides of every pair.

1. the plain estimator against the numpy restatement of tests/roulette_ref.py over the unchanged oracle, so that the claim
   does not rest on the per-lane kernel alone (the boxes have no tree: the lean pool form with the ring RNG);
2. all four estimators against the per-lane kernel, with and without REF_TREE, and the guard that roulette fires;
3. disabled (min_depth > max_depth and q_min = 1) it is the cooperative lighting entry;
4. the 256-entry pool, shade_threshold = 1 and a 7-sample per-sample buffer;
5. a ragged image, two samples per pixel, and a repeat of the same call;
6. the adaptive form;
7. the fallbacks to the per-lane kernel;
8. a missing light table or map is refused as without the flag."""
import numpy as np
import pytest

import env_ref
import roulette_ref as rr
import scenes_extra
import scenes_random
from oracle.oracle import ARITH_DEVICE, THROUGHPUT_FORM
from raytracing_rust_amd import abi, scenes
from raytracing_rust_amd.host import HostError

SEED = 42
FC = abi.RTMI_FLAG_FAST_CULL
COOP, PERLANE = abi.RTMI_KERNEL_WAVE_COOP, abi.RTMI_KERNEL_PERLANE
POOL_KNOB = 1 << 11
PLANES = ("linear", "rgb8", "stderr", "bounces")
ON = [dict(min_depth=3, q_min=0.05), dict(min_depth=1, q_min=0.2)]
OFF = dict(min_depth=51, q_min=0.05)  # max_depth is 50: no scatter reaches the first test


def _build(api, name, nx, ny):
    if name in scenes.SCENES:
        return scenes.build(api, name, nx, ny, seed=1)
    return scenes_extra.build(api, name, nx, ny, seed=7 if name == "lit_random_spheres" else 1)


def _earth_map():
    data, w, h = scenes.earthmap_rgb8()
    return (np.asarray(data, np.float32).reshape(h, w, 3) / np.float32(255.0)).astype(np.float32)


def _scene(host, name, mapname, nx, ny):
    cam, world = _build(host, name, nx, ny)
    sc = host.lower(world).upload(0, nee=True)
    if mapname:
        sc.attach_env(env_ref.sun_map() if mapname == "sun" else _earth_map())
    return cam, sc


def _level0(sc):
    """The selection rule's scene part: neither instanced primitives nor media under outer transforms / among a BVHNode's
    children (has_prim_xf, has_medium_outer of the device scene), from the description."""
    d = sc.desc()
    for i in range(d.n_prims):
        if (d.prim_meta[i].flags >> abi.RTMI_PRIMFLAG_XF_COUNT_SHIFT) & 15:
            return False
    for i in range(d.n_items):
        f = d.items[i].flags
        if (f >> abi.RTMI_ITEMFLAG_MEDIUM_OUTER_SHIFT) & 15 or f & (abi.ITEMFLAG_SAVE_T0 | abi.ITEMFLAG_DEFERRED |
                                                                    abi.ITEMFLAG_NESTED_MEDIUM):
            return False
    return True


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_planes(label, got, ref, planes=PLANES):
    """Bit for bit, plane by plane; counts the differing words first so that a failure says how much differs."""
    for key in planes:
        a, b = got[key], ref[key]
        assert a.shape == b.shape and a.dtype == b.dtype, (label, key)
        bad = int(np.sum(_bits(a) != _bits(b)))
        assert bad == 0, "%s: %d of %d words of %s differ" % (label, bad, a.size, key)
        assert np.array_equal(_bits(a), _bits(b)), (label, key)


def _pair(label, render, flags, want_kernel=COOP, planes=PLANES, **kw):
    """render(flags=..., coop=...) without and with the flag: the same bits, the expected kernels.  Returns the flagged dict."""
    ref = render(flags=flags, coop=False, **kw)
    got = render(flags=flags, coop=True, **kw)
    assert ref["stats"]["kernel"] == PERLANE, label
    assert got["stats"]["kernel"] == want_kernel, (label, got["stats"]["kernel"])
    _same_planes(label, got, ref, planes)
    return got


def _rr(sc, cam, nx, ny, ns, est, **opts):
    return lambda **kw: sc.render_roulette(cam, nx, ny, ns, estimator=est, env_select_p=0.5, seed=SEED, **opts, **kw)


# ---- 1. the restatement -------------------------------------------------------------------------------------------------------
# (min_depth, q_min, the floor binds): the pairs of tests/test_gpu_roulette_exact.py, and roulette off
PAIRS = [(1, 0.2, False), (3, 0.05, False), (3, 0.5, True), (1, 0.8, True), (51, 0.05, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(rr.BOXES))
def test_plain_boxes_equal_restatement(host, orc32, name):
    nx, ny, ns = 32, 32, 16
    albedo, closed, max_depth = rr.BOXES[name]
    cam_o, world_o = rr.box(orc32, name, nx, ny)
    ref = orc32.render_samples(cam_o, world_o, nx, ny, ns, seed=SEED, flags=ARITH_DEVICE | THROUGHPUT_FORM, max_depth=max_depth)
    orc32.free_all()
    k = rr.lookup_k(ref["samples"], albedo, rr.LE, max_depth)  # asserts the method's condition: no sample left out
    cam, world = rr.box(host, name, nx, ny)
    sc = host.lower(world).upload(0)
    assert _level0(sc) and sc.desc().n_nodes == 0  # no tree: the lean pool form, RngRing
    for min_depth, q_min, floor_binds in PAIRS:
        smp, scat, floored = rr.restate(k, albedo, rr.LE, max_depth, min_depth, q_min, SEED, nx, closed)
        lin, rgb = rr.image(smp)
        se = rr.welford_stderr(smp)
        assert (floored > 0) == floor_binds, (name, min_depth, q_min, floored)
        if min_depth <= max_depth:
            assert smp.tobytes() != ref["samples"].tobytes()  # the pair does something
        got = sc.render_roulette(cam, nx, ny, ns, estimator="plain", min_depth=min_depth, q_min=q_min, seed=SEED,
                                 max_depth=max_depth, flags=FC, coop=True)
        what = "%s min_depth %d q_min %g" % (name, min_depth, q_min)
        assert got["stats"]["kernel"] == COOP, what
        bad = int(np.sum(_bits(got["linear"]) != _bits(lin)))
        bad_se = int(np.sum(_bits(got["stderr"]) != _bits(se)))
        print("\nRR-COOP-EXACT %s: %d of %d channels differ, %d stderr, bounces/sample %.2f, %d survivals at q = q_min" % (
            what, bad, lin.size, bad_se, got["bounces"].sum() / (nx * ny * ns), floored))
        assert bad == 0, "%s: %d channels differ" % (what, bad)
        assert np.array_equal(got["rgb8"], rgb), what
        assert bad_se == 0, what
        assert got["stats"]["samples"] == nx * ny * ns
        if closed:
            assert np.array_equal(got["bounces"].astype(np.int64), scat.sum(-1)), what


# ---- 2. all four estimators against the per-lane kernel -----------------------------------------------------------------------
LIT_NAMES = ["cornell_box", "lit_smoke", "simple_light", "hollow_glass", "lit_random_spheres", "lit_final_scene"]
MAPS = [("random_spheres", "sun"), ("lit_random_spheres", "sun"), ("earth", "earth")]
CASES = [(n, None, ("plain", "nee")) for n in LIT_NAMES] + [(n, m, ("env", "env_nee")) for n, m in MAPS]
GUARDED = {("cornell_box", None), ("lit_random_spheres", None), ("random_spheres", "sun")}  # roulette must be seen to fire


@pytest.mark.gpu
@pytest.mark.parametrize("name,mapname,ests", CASES, ids=["%s-%s" % (n, m or "lights") for n, m, _ in CASES])
def test_estimators_equal_the_perlane_kernel(host, name, mapname, ests):
    nx, ny, ns = 40, 30, 12
    cam, sc = _scene(host, name, mapname, nx, ny)
    assert _level0(sc)
    tree = sc.desc().n_nodes > 0
    for est in ests:
        for fl in (FC, FC | abi.RTMI_FLAG_REF_TREE) if tree else (FC,):
            total = {}
            for opts in ON:
                got = _pair("%s/%s/%d/%s" % (name, est, fl, opts), _rr(sc, cam, nx, ny, ns, est, **opts), fl)
                assert np.any(got["linear"] > 0) and np.all(np.isfinite(got["linear"]))
                total[opts["min_depth"]] = int(got["bounces"].sum(dtype=np.uint64))
            if (name, mapname) in GUARDED and fl == FC:
                off = sc.render_roulette(cam, nx, ny, ns, estimator=est, env_select_p=0.5, seed=SEED, flags=fl, coop=True, **OFF)
                assert off["stats"]["kernel"] == COOP
                assert total[1] < int(off["bounces"].sum(dtype=np.uint64)), (name, est, total)


def test_cases_cover_both_pool_forms(host):
    """The lean pool form serves scenes without any BVH item, the extended one the others (plan_traversal); each of the
    four estimators meets both."""
    nodes = {}
    for name in sorted(set(LIT_NAMES) | set(n for n, _ in MAPS)):
        _, world = _build(host, name, 40, 30)
        nodes[name] = host.lower(world).desc().n_nodes
    assert nodes["cornell_box"] == 0 and nodes["lit_smoke"] == 0            # plain, nee: lean
    assert nodes["lit_final_scene"] > 0 and nodes["lit_random_spheres"] > 0  # plain, nee (and env, env_nee): ext
    assert nodes["earth"] == 0 and nodes["random_spheres"] > 0               # env, env_nee: lean / ext
    assert GUARDED <= set((n, m) for n, m, _ in CASES)


# ---- 3. disabled is the lighting entry ----------------------------------------------------------------------------------------
OFF_CASES = [("cornell_box", None, ("plain", "nee")), ("lit_random_spheres", None, ("plain", "nee")),
             ("random_spheres", "sun", ("env", "env_nee"))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,mapname,ests", OFF_CASES, ids=["%s-%s" % (n, m or "lights") for n, m, _ in OFF_CASES])
def test_disabled_is_the_cooperative_lighting_entry(host, name, mapname, ests):
    nx, ny, ns = 40, 30, 12
    cam, sc = _scene(host, name, mapname, nx, ny)
    for est in ests:
        if est == "plain":
            ref = sc.render_adaptive(cam, nx, ny, ns, min_spp=ns, step_spp=1, seed=SEED, flags=FC)
        elif est == "nee":
            ref = sc.render_nee(cam, nx, ny, ns, seed=SEED, flags=FC, coop=True)
        else:
            ref = sc.render_env(cam, nx, ny, ns, nee=est == "env_nee", env_select_p=0.5, seed=SEED, flags=FC, coop=True)
        assert ref["stats"]["kernel"] == COOP, (name, est)
        for label, opts in (("min_depth 51", OFF), ("q_min 1", dict(min_depth=1, q_min=1.0))):
            got = sc.render_roulette(cam, nx, ny, ns, estimator=est, env_select_p=0.5, seed=SEED, flags=FC, coop=True, **opts)
            assert got["stats"]["kernel"] == COOP, (name, est, label)
            _same_planes("%s/%s/%s" % (name, est, label), got, ref, ("linear", "rgb8", "stderr"))


# ---- 4. pool spill and schedule -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lit_final_scene", "lit_random_spheres"])
def test_small_pool_threshold_and_passes_keep_the_bits(host, name):
    nx, ny, ns = 40, 30, 12
    cam, sc = _scene(host, name, None, nx, ny)
    per_sample = ((nx + 7) // 8) * ((ny + 7) // 8) * 64 * abi.RTMI_SAMPLE_SLOT_BYTES
    for est in ("nee", "plain"):
        render = _rr(sc, cam, nx, ny, ns, est, **ON[0])
        ref = render(flags=FC, coop=False)
        assert ref["stats"]["kernel"] == PERLANE
        for label, fl, kw in (("pool knob", FC | POOL_KNOB, {}), ("threshold 1", FC, {"shade_threshold": 1}),
                              ("7-sample buffer", FC, {"sample_buffer_bytes": per_sample * 7}),
                              ("pool knob, threshold 1, 5-sample buffer", FC | POOL_KNOB,
                               {"shade_threshold": 1, "sample_buffer_bytes": per_sample * 5})):
            got = render(flags=fl, coop=True, **kw)
            assert got["stats"]["kernel"] == COOP, label
            _same_planes("%s/%s/%s" % (name, est, label), got, ref)


# ---- 5. ragged image, tiny sample count, repetition ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_box", "lit_random_spheres"])
def test_ragged_image_two_samples_and_repetition(host, name):
    """25 x 17: partial 8 x 8 tiles on both edges.  The repeat checks that the bounce plane is zeroed per call."""
    nx, ny = 25, 17
    cam, sc = _scene(host, name, None, nx, ny)
    for est in ("nee", "plain"):
        first = _pair("ragged %s/%s" % (name, est), _rr(sc, cam, nx, ny, 16, est, **ON[1]), FC)
        assert first["bounces"].sum() > 0
        again = _rr(sc, cam, nx, ny, 16, est, **ON[1])(flags=FC, coop=True)
        assert again["stats"]["kernel"] == COOP
        _same_planes("repeat %s/%s" % (name, est), again, first)
        _pair("2 spp %s/%s" % (name, est), _rr(sc, cam, nx, ny, 2, est, **ON[1]), FC, shade_threshold=1)


# ---- 6. adaptive --------------------------------------------------------------------------------------------------------------
AD_NX, AD_NY, AD_NS, AD_MIN, AD_STEP = 96, 72, 48, 16, 16
AD_CASES = [("cornell_box", None, "nee"), ("lit_random_spheres", None, "plain"), ("random_spheres", "sun", "env_nee")]
AD_PLANES = ("linear", "rgb8", "stderr", "spp", "bounces")


def _tile_max(a, nx, ny):
    ty, tx = (ny + 7) // 8, (nx + 7) // 8
    pad = np.full((ty * 8, tx * 8, 3), -np.inf)
    pad[:ny, :nx] = a
    return pad.reshape(ty, 8, tx, 8, 3).max(axis=(1, 3, 4))


@pytest.mark.gpu
@pytest.mark.parametrize("name,mapname,est", AD_CASES, ids=["%s-%s" % (n, e) for n, _, e in AD_CASES])
def test_adaptive_form_equals_the_perlane_kernel(host, name, mapname, est):
    nx, ny = AD_NX, AD_NY
    cam, sc = _scene(host, name, mapname, nx, ny)

    def adaptive(ns, mn, step, tol, **kw):
        return sc.render_adaptive_roulette(cam, nx, ny, ns, mn, step, abs_tol=tol, estimator=est, env_select_p=0.5, seed=SEED,
                                           **ON[0], **kw)

    # abs_tol = the median over tiles of the per-tile max stderr after the first step of the unflagged form: about half
    # the tiles cannot meet it there (the rule of tests/test_gpu_light_coop.py)
    st = adaptive(AD_MIN, AD_MIN, AD_STEP, 0.0, flags=FC)
    tol = float(np.median(_tile_max(st["stderr"].astype(np.float64), nx, ny)))
    ref = adaptive(AD_NS, AD_MIN, AD_STEP, tol, flags=FC)
    assert ref["stats"]["kernel"] == PERLANE
    spp = ref["spp"]
    tiles = _tile_max(np.repeat(spp[..., None].astype(np.float64), 3, -1), nx, ny)
    share = float(np.mean(tiles > AD_MIN))
    print(name, est, "abs_tol %.4g" % tol, "tiles past min_spp: %.2f" % share, {int(k): int((spp == k).sum()) for k in np.unique(spp)})
    assert 0.25 <= share <= 0.75, share  # the condition, on the unflagged result
    got = adaptive(AD_NS, AD_MIN, AD_STEP, tol, flags=FC, coop=True)
    assert got["stats"]["kernel"] == COOP
    _same_planes("adaptive %s/%s" % (name, est), got, ref, AD_PLANES)
    assert got["stats"]["samples"] == int(got["spp"].astype(np.uint64).sum())
    # the small pool and sub-passes, in the step loop
    per_sample = ((nx + 7) // 8) * ((ny + 7) // 8) * 64 * abi.RTMI_SAMPLE_SLOT_BYTES
    small = adaptive(AD_NS, AD_MIN, AD_STEP, tol, flags=FC | POOL_KNOB, coop=True, sample_buffer_bytes=per_sample * 7)
    assert small["stats"]["kernel"] == COOP
    _same_planes("adaptive small pool %s/%s" % (name, est), small, got, AD_PLANES)
    # min_spp == ns: the flagged fixed render
    ns = 24
    stat = adaptive(ns, ns, 1, 1e9, flags=FC, coop=True)
    fixed = _rr(sc, cam, nx, ny, ns, est, **ON[0])(flags=FC, coop=True)
    assert stat["stats"]["kernel"] == COOP and fixed["stats"]["kernel"] == COOP
    _same_planes("min_spp == ns %s/%s" % (name, est), stat, fixed)
    assert np.all(stat["spp"] == ns)


# ---- 7. fallbacks -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fallbacks_run_the_perlane_kernel_with_the_same_bits(host):
    nx, ny, ns = 40, 30, 12
    cam, sc = _scene(host, "lit_random_spheres", None, nx, ny)
    for est in ("nee", "plain"):
        render = _rr(sc, cam, nx, ny, ns, est, **ON[0])
        base = _pair("selected " + est, render, FC)  # the guard: this scene and camera do select the cooperative kernel
        for label, fl in (("no fast-cull", 0), ("sync", FC | abi.RTMI_FLAG_SYNC), ("sync+pool knob", FC | abi.RTMI_FLAG_SYNC | POOL_KNOB)):
            got = render(flags=fl, coop=True)
            assert got["stats"]["kernel"] == PERLANE, label
            _same_planes("%s/%s" % (label, est), got, base)
    # a shutter that leaves the BVH's time range (the spheres move during [0, 1]): fast-cull is not valid, per-lane exact walk
    d = sc.desc()
    assert d.bvh_time_lo <= 0.0 and d.bvh_time_hi >= 1.0 and d.bvh_time_hi < 3.0
    _, look_from, look_at, vfov = scenes_extra.EXTRA["lit_random_spheres"]
    cam2 = scenes.set_camera(host, nx, ny, look_from, look_at, vertical_fov=vfov, time0=0.0, time1=3.0)
    _pair("shutter outside", _rr(sc, cam2, nx, ny, ns, "nee", **ON[0]), FC, want_kernel=PERLANE)
    # an instanced random composition
    cam3, world3 = scenes_random.build(host, 4, 24, 16, instanced=True)
    sc3 = host.lower(world3).upload(0, nee=True)
    assert not _level0(sc3) and len(sc3.lights()) > 0
    for est in ("nee", "plain"):
        _pair("instanced " + est, _rr(sc3, cam3, 24, 16, 6, est, **ON[1]), FC, want_kernel=PERLANE)


# ---- 8. errors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_missing_light_table_or_map_is_refused_as_without_the_flag(host):
    nx, ny, ns = 16, 16, 4
    cam, world = _build(host, "cornell_box", nx, ny)
    sc = host.lower(world).upload(0)  # no light table, no map
    sc.lights_attached = True          # keep the wrapper from attaching it on first use
    for est, word in (("nee", "light table"), ("env", "environment map")):
        msgs = []
        for coop in (False, True):
            with pytest.raises(HostError) as e:
                sc.render_roulette(cam, nx, ny, ns, estimator=est, seed=SEED, flags=FC, coop=coop)
            msgs.append(str(e.value))
            assert type(e.value) is HostError  # RTMI_ERR_INVALID: RTMI_ERR_UNSUPPORTED would raise Unsupported
            assert "rtmi_render_roulette" in msgs[-1] and word in msgs[-1], msgs[-1]
        assert msgs[0] == msgs[1]
