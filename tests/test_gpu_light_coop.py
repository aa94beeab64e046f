"""RTMI_FLAG_LIGHT_COOP (include/rtmi_light_coop.h) on the device: next-event estimation, environment
lighting and their adaptive forms on the wave-cooperative kernel.

The claim is "the same bits, another kernel": every comparison is on the raw bits of every output plane (linear, rgb8,
stderr, path signatures, spp) of the flagged call against the unflagged one, and on three scenes also against the fp32
oracle's restatement of NEE, so that the claim does not rest on the per-lane kernel alone.  stats["kernel"] tells which
kernel ran; the selection rule is restated here from the scene description (_level0).

 1. named lit scenes, NEE, with and without REF_TREE (scenes without a tree: lean pool form; with trees: the other);
 2. the flagged render against the oracle;
 3. environment maps, with and without light sampling;
 4. the hand-built rare-branch scenes of the NEE oracle test;
 5. the fallbacks to the per-lane kernel;
 6. the 256-entry pool, shade_threshold = 1 and a 7-sample per-sample buffer;
 7. a ragged image, and a repeat of the same call;
 8. the adaptive forms;
 9. the random compositions;
10. render_denoised."""
import numpy as np
import pytest

import env_ref
import scenes_extra
import scenes_random
from nee_oracle_ref import EDGE, oracle_lights, welford_stderr
from oracle.oracle import ARITH_DEVICE, FACE_FORWARD, SKY, THROUGHPUT_FORM, UV_BOOK
from raytracing_rust_amd import abi, env_from_sky, scenes

SEED = 42
FC = abi.RTMI_FLAG_FAST_CULL
COOP, PERLANE = abi.RTMI_KERNEL_WAVE_COOP, abi.RTMI_KERNEL_PERLANE
POOL_KNOB = 1 << 11
EXT = {SKY: abi.RTMI_FLAG_SKY, FACE_FORWARD: abi.RTMI_FLAG_FACE_FORWARD, UV_BOOK: abi.RTMI_FLAG_UV_BOOK}
PLANES = ("linear", "rgb8", "stderr", "sig")


def _dev_ext(oflags):
    return sum(d for o, d in EXT.items() if oflags & o)


def _build(api, name, nx, ny):
    if name in scenes.SCENES:
        return scenes.build(api, name, nx, ny, seed=1)
    return scenes_extra.build(api, name, nx, ny, seed=7 if name == "lit_random_spheres" else 1)


def _earth_map():
    data, w, h = scenes.earthmap_rgb8()
    return (np.asarray(data, np.float32).reshape(h, w, 3) / np.float32(255.0)).astype(np.float32)


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


def _nee(sc, cam, nx, ny, ns):
    return lambda **kw: sc.render_nee(cam, nx, ny, ns, sig=True, seed=SEED, **kw)


# ---- 1. named scenes, NEE ---------------------------------------------------------------------------------------------------
NAMED = [("cornell_box", 0), ("lit_smoke", 0), ("lit_smoke", FACE_FORWARD), ("simple_light", 0), ("simple_light", SKY),
         ("lit_random_spheres", 0), ("lit_random_spheres", UV_BOOK | SKY), ("hollow_glass", 0), ("hollow_glass", FACE_FORWARD | UV_BOOK),
         ("lit_final_scene", 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,oflags", NAMED, ids=["%s-%d" % c for c in NAMED])
def test_named_scenes_equal_the_perlane_kernel(host, name, oflags):
    nx, ny, ns = 40, 30, 12
    cam, world = _build(host, name, nx, ny)
    sc = host.lower(world).upload(0, nee=True)
    assert _level0(sc) and len(sc.lights()) > 0
    for fl in (FC, FC | abi.RTMI_FLAG_REF_TREE):
        got = _pair("%s/%d" % (name, fl), _nee(sc, cam, nx, ny, ns), fl | _dev_ext(oflags))
        assert np.any(got["linear"] > 0) and np.any(got["sig"] != 0)


def test_named_scenes_cover_both_pool_forms(host):
    """The lean pool form serves scenes without any BVH item, the extended one the others (plan_traversal)."""
    nodes = {}
    for name in sorted(set(n for n, _ in NAMED)):
        _, world = _build(host, name, 40, 30)
        nodes[name] = host.lower(world).desc().n_nodes
    assert nodes["cornell_box"] == 0 and nodes["lit_smoke"] == 0
    assert nodes["lit_final_scene"] > 0 and nodes["lit_random_spheres"] > 0


# ---- 2. the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_box", "lit_random_spheres", "lit_final_scene"])
def test_flagged_render_equals_oracle(host, orc32, name):
    nx, ny, ns = 40, 30, 12
    cam_h, world_h = _build(host, name, nx, ny)
    cam_o, world_o = _build(orc32, name, nx, ny)
    sc = host.lower(world_h).upload(0, nee=True)
    lights = oracle_lights(orc32, world_o, sc)
    assert len(lights) == len(sc.lights()) > 0
    ref = orc32.render_nee(cam_o, world_o, lights, nx, ny, ns, seed=SEED, flags=ARITH_DEVICE | THROUGHPUT_FORM, samples=True)
    for fl in (FC, FC | abi.RTMI_FLAG_REF_TREE):
        got = sc.render_nee(cam_h, nx, ny, ns, sig=True, seed=SEED, flags=fl, coop=True)
        assert got["stats"]["kernel"] == COOP
        lin, rlin = got["linear"], ref["linear"]
        bad = int(np.sum(lin.view(np.uint32) != rlin.view(np.uint32)))
        bad_sig = int(np.sum(got["sig"] != ref["sig"]))
        assert bad == 0 and bad_sig == 0, "%s/%d: %d channels and %d signatures differ" % (name, fl, bad, bad_sig)
        assert np.array_equal(got["rgb8"].astype(np.int32), ref["rgb"]), name
        se = welford_stderr(ref["samples"])
        bad_se = int(np.sum(got["stderr"].view(np.uint32) != se.view(np.uint32)))
        assert bad_se == 0, "%s/%d: %d stderr channels differ" % (name, fl, bad_se)
    assert np.any(ref["linear"] > 0)
    orc32.free_all()


# ---- 3. environment maps ------------------------------------------------------------------------------------------------------
ENV_CASES = [("random_spheres", "sun"), ("random_spheres", "sky"), ("lit_random_spheres", "sun"), ("lit_random_spheres", "sky"),
             ("earth", "earth")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,mapname", ENV_CASES, ids=["%s-%s" % c for c in ENV_CASES])
def test_environment_renders_equal_the_perlane_kernel(host, name, mapname):
    nx, ny, ns = 40, 30, 12
    cam, world = _build(host, name, nx, ny)
    sc = host.lower(world).upload(0, nee=True)
    sc.attach_env({"sun": env_ref.sun_map, "sky": lambda: env_from_sky(256, 128), "earth": _earth_map}[mapname]())
    assert _level0(sc)
    for nee in (False, True):
        got = _pair("%s/%s/nee%d" % (name, mapname, nee),
                    lambda **kw: sc.render_env(cam, nx, ny, ns, nee=nee, env_select_p=0.5, sig=True, seed=SEED, **kw), FC)
        assert np.any(got["linear"] > 0)


# ---- 4. hand-built rare-branch scenes -----------------------------------------------------------------------------------------
EDGE_SIZES = {"cdf_boundaries": (64, 64, 48)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(EDGE))
def test_edge_scenes_equal_the_perlane_kernel(host, name):
    assert len(EDGE) == 10
    nx, ny, ns = EDGE_SIZES.get(name, (32, 24, 16))
    cam, world = EDGE[name](host, nx, ny)
    sc = host.lower(world).upload(0, nee=True)
    want = COOP if _level0(sc) else PERLANE
    assert (want == PERLANE) == (name in ("deferred_lights", "listscan_light"))  # the two with media among a BVHNode's children
    got = _pair(name, _nee(sc, cam, nx, ny, ns), FC, want_kernel=want)
    assert np.any(got["linear"] > 0), name


# ---- 5. fallbacks -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fallbacks_run_the_perlane_kernel_with_the_same_bits(host):
    nx, ny, ns = 40, 30, 12
    cam, world = _build(host, "lit_random_spheres", nx, ny)
    sc = host.lower(world).upload(0, nee=True)
    render = _nee(sc, cam, nx, ny, ns)
    base = _pair("selected", render, FC)  # the guard: this scene and camera do select the cooperative kernel
    for label, fl in (("no fast-cull", 0), ("sync", FC | abi.RTMI_FLAG_SYNC), ("sync+pool knob", FC | abi.RTMI_FLAG_SYNC | POOL_KNOB)):
        got = render(flags=fl, coop=True)
        assert got["stats"]["kernel"] == PERLANE, label
        _same_planes(label, got, base)
    # a shutter that leaves the BVH's time range (the spheres move during [0, 1]): fast-cull is not valid, per-lane exact walk
    d = sc.desc()
    assert d.bvh_time_lo <= 0.0 and d.bvh_time_hi >= 1.0 and d.bvh_time_hi < 3.0
    _, look_from, look_at, vfov = scenes_extra.EXTRA["lit_random_spheres"]
    cam2 = scenes.set_camera(host, nx, ny, look_from, look_at, vertical_fov=vfov, time0=0.0, time1=3.0)
    _pair("shutter outside", _nee(sc, cam2, nx, ny, ns), FC, want_kernel=PERLANE)
    # an instanced random composition
    cam3, world3 = scenes_random.build(host, 4, 24, 16, instanced=True)
    sc3 = host.lower(world3).upload(0, nee=True)
    assert not _level0(sc3) and len(sc3.lights()) > 0
    _pair("instanced", _nee(sc3, cam3, 24, 16, 6), FC, want_kernel=PERLANE)


# ---- 6. pool spill and schedule -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lit_final_scene", "lit_random_spheres"])
def test_small_pool_threshold_and_passes_keep_the_bits(host, name):
    nx, ny, ns = 40, 30, 12
    cam, world = _build(host, name, nx, ny)
    sc = host.lower(world).upload(0, nee=True)
    render = _nee(sc, cam, nx, ny, ns)
    ref = render(flags=FC, coop=False)
    per_sample = ((nx + 7) // 8) * ((ny + 7) // 8) * 64 * abi.RTMI_SAMPLE_SLOT_BYTES
    for label, fl, kw in (("pool knob", FC | POOL_KNOB, {}), ("threshold 1", FC, {"shade_threshold": 1}),
                          ("7-sample buffer", FC, {"sample_buffer_bytes": per_sample * 7}),
                          ("pool knob, threshold 1, 5-sample buffer", FC | POOL_KNOB,
                           {"shade_threshold": 1, "sample_buffer_bytes": per_sample * 5})):
        got = render(flags=fl, coop=True, **kw)
        assert got["stats"]["kernel"] == COOP, label
        _same_planes("%s/%s" % (name, label), got, ref)


# ---- 7. ragged image, repetition ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_box", "lit_random_spheres"])
def test_ragged_image_and_repetition(host, name):
    """25 x 17: partial 8 x 8 tiles on both edges."""
    nx, ny, ns = 25, 17, 16
    cam, world = _build(host, name, nx, ny)
    sc = host.lower(world).upload(0, nee=True)
    first = _pair("ragged " + name, _nee(sc, cam, nx, ny, ns), FC)
    again = sc.render_nee(cam, nx, ny, ns, sig=True, seed=SEED, flags=FC, coop=True)
    _same_planes("repeat " + name, again, first)


# ---- 8. adaptive --------------------------------------------------------------------------------------------------------------
AD_NX, AD_NY, AD_NS, AD_MIN, AD_STEP = 160, 120, 64, 16, 16
AD_CASES = [("cornell_box", None), ("lit_random_spheres", None), ("random_spheres", "sun")]


def _tile_max(a, nx, ny):
    ty, tx = (ny + 7) // 8, (nx + 7) // 8
    pad = np.full((ty * 8, tx * 8, 3), -np.inf)
    pad[:ny, :nx] = a
    return pad.reshape(ty, 8, tx, 8, 3).max(axis=(1, 3, 4))


@pytest.mark.gpu
@pytest.mark.parametrize("name,mapname", AD_CASES, ids=["%s-%s" % (n, m or "lights") for n, m in AD_CASES])
def test_adaptive_forms_equal_the_perlane_kernel(host, name, mapname):
    nx, ny = AD_NX, AD_NY
    cam, world = _build(host, name, nx, ny)
    sc = host.lower(world).upload(0, nee=True)
    env = mapname is not None
    if env:
        sc.attach_env(env_ref.sun_map())

    def adaptive(ns, mn, step, tol, **kw):
        return sc.render_adaptive(cam, nx, ny, ns, mn, step, abs_tol=tol, nee=True, env=env, env_select_p=0.5, seed=SEED, **kw)

    # abs_tol at the median tile noise after the first step of the unflagged estimator: about half the tiles cannot meet it
    # there (tests/test_gpu_adaptive_nee.py's _mixed_tolerance, at the median itself)
    st = adaptive(AD_MIN, AD_MIN, AD_STEP, 0.0, flags=FC)
    tol = float(np.median(_tile_max(st["stderr"].astype(np.float64), nx, ny)))
    ad_planes = ("linear", "rgb8", "stderr", "spp")
    got = _pair("adaptive " + name, lambda **kw: adaptive(AD_NS, AD_MIN, AD_STEP, tol, **kw), FC, planes=ad_planes)
    spp = got["spp"]
    tiles = _tile_max(np.repeat(spp[..., None].astype(np.float64), 3, -1), nx, ny)
    share = float(np.mean(tiles > AD_MIN))
    print(name, mapname, "abs_tol %.4g" % tol, "tiles past min_spp: %.2f" % share,
          {int(k): int((spp == k).sum()) for k in np.unique(spp)})
    assert 0.25 <= share <= 0.75, share  # "about half"
    assert got["stats"]["samples"] == int(spp.astype(np.uint64).sum())
    # the small pool and sub-passes, in the step loop
    per_sample = ((nx + 7) // 8) * ((ny + 7) // 8) * 64 * abi.RTMI_SAMPLE_SLOT_BYTES
    small = adaptive(AD_NS, AD_MIN, AD_STEP, tol, flags=FC | POOL_KNOB, coop=True, sample_buffer_bytes=per_sample * 7)
    assert small["stats"]["kernel"] == COOP
    _same_planes("adaptive small pool " + name, small, got, ad_planes)
    # statistics only: the flagged fixed render
    ns = 24
    stat = adaptive(ns, ns, 1, 1e9, flags=FC, coop=True)
    if env:
        fixed = sc.render_env(cam, nx, ny, ns, nee=True, env_select_p=0.5, seed=SEED, flags=FC, coop=True)
    else:
        fixed = sc.render_nee(cam, nx, ny, ns, seed=SEED, flags=FC, coop=True)
    assert stat["stats"]["kernel"] == COOP and fixed["stats"]["kernel"] == COOP
    _same_planes("statistics only " + name, stat, fixed, ("linear", "rgb8", "stderr"))
    assert np.all(stat["spp"] == ns)


# ---- 9. random compositions ---------------------------------------------------------------------------------------------------
PLACEMENTS = [("unit", 1.0, (0.0, 0.0, 0.0)), ("scale1_64", 1.0 / 64.0, (0.0, 0.0, 0.0)), ("scale300", 300.0, (0.0, 0.0, 0.0)),
              ("offset700", 1.0, (700.0, 0.0, -700.0))]
RANDOM = [(s, p) for p in PLACEMENTS for s in (range(1, 25) if p[0] == "unit" else range(1, 5))]


def test_random_compositions_all_have_lights_and_select_the_cooperative_kernel(host):
    """On the CPU: none of the 36 cases below has to be skipped for want of an eligible light, and every one is a scene
    the selection rule sends to the cooperative kernel."""
    assert len(RANDOM) >= 24
    for seed, (_, scale, off) in RANDOM:
        _, world = scenes_random.build(host, seed, 24, 16, instanced=False, scale=scale, offset=off)
        sc = host.lower(world)
        assert len(sc.lights()) > 0 and _level0(sc), seed


@pytest.mark.gpu
@pytest.mark.parametrize("seed,placement", [pytest.param(s, p, id="%d-%s" % (s, p[0])) for s, p in RANDOM])
def test_random_scenes_equal_the_perlane_kernel(host, seed, placement):
    nx, ny, ns = 24, 16, 6
    _, scale, off = placement
    cam, world = scenes_random.build(host, seed, nx, ny, instanced=False, scale=scale, offset=off)
    sc = host.lower(world).upload(0, nee=True)
    ext = abi.RTMI_FLAG_SKY if seed % 3 == 0 else (abi.RTMI_FLAG_FACE_FORWARD if seed % 3 == 1 else 0)
    fl = FC | ext | (abi.RTMI_FLAG_REF_TREE if seed % 2 else 0)
    _pair("random %d %s" % (seed, placement[0]), _nee(sc, cam, nx, ny, ns), fl)


# ---- 10. render_denoised ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_render_denoised_passes_the_flag_to_the_lit_render_only(host):
    nx, ny, ns = 64, 48, 8
    cam, world = _build(host, "cornell_box", nx, ny)
    sc = host.lower(world).upload(0, nee=True)
    ref = sc.render_denoised(cam, nx, ny, ns, nee=True, seed=SEED, flags=FC)
    got = sc.render_denoised(cam, nx, ny, ns, nee=True, coop=True, seed=SEED, flags=FC)  # (features would refuse the flag)
    assert ref["noisy"]["stats"]["kernel"] == PERLANE and got["noisy"]["stats"]["kernel"] == COOP
    _same_planes("denoised", got, ref, ("linear", "rgb8"))
    _same_planes("noisy", got["noisy"], ref["noisy"], ("linear", "rgb8", "stderr"))
    for key in ("albedo", "normal", "depth", "hits"):
        assert np.array_equal(_bits(got["features"][key]), _bits(ref["features"][key])), key
