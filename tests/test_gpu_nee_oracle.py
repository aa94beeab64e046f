"""rtmi_render_nee (include/rtmi_nee.h) against the fp32 oracle's restatement of it (orc_render_nee), bit for bit: mean
radiance, rgb8 and path signatures, and the standard-error plane against rtmi_adaptive.h's Welford recurrence over the
oracle's per-sample radiances (tests/nee_oracle_ref.py).  Named lit scenes under every accepted flag, the random
compositions of tests/scenes_random.py, and hand-built scenes that make NEE's rarely taken branches happen.  Also
render_adaptive's stderr plane against the same recurrence over the plain render's samples."""
import numpy as np
import pytest

import scenes_extra
import scenes_random
from nee_oracle_ref import EDGE, oracle_lights, welford_stderr
from oracle.oracle import ARITH_DEVICE, FACE_FORWARD, SKY, THROUGHPUT_FORM, UV_BOOK
from raytracing_rust_amd import abi, scenes

SEED = 42
FC = abi.RTMI_FLAG_FAST_CULL
DEVICE_FLAGS = [("fast", FC), ("exact", 0), ("reftree", FC | abi.RTMI_FLAG_REF_TREE), ("sync", FC | abi.RTMI_FLAG_SYNC)]
EXT = {SKY: abi.RTMI_FLAG_SKY, FACE_FORWARD: abi.RTMI_FLAG_FACE_FORWARD, UV_BOOK: abi.RTMI_FLAG_UV_BOOK}


def _dev_ext(oflags):
    return sum(d for o, d in EXT.items() if oflags & o)


def _build(api, name, nx, ny):
    if name in scenes.SCENES:
        return scenes.build(api, name, nx, ny, seed=1)
    return scenes_extra.build(api, name, nx, ny, seed=7 if name == "lit_random_spheres" else 1)


def _check(label, got, ref):
    """got: render_nee's dict, ref: the oracle's (samples=True).  Counts differing channels / signatures first, so that
    a failure says how much differs."""
    lin, rlin = got["linear"], ref["linear"]
    bad = int(np.sum(lin.view(np.uint32) != rlin.view(np.uint32)))
    bad_sig = int(np.sum(got["sig"] != ref["sig"]))
    assert bad == 0 and bad_sig == 0, "%s: %d channels and %d signatures differ (max |diff| %g)" % (
        label, bad, bad_sig, float(np.nanmax(np.abs(lin.astype(np.float64) - rlin))))
    assert np.array_equal(got["rgb8"].astype(np.int32), ref["rgb"]), label
    se = welford_stderr(ref["samples"])
    bad_se = int(np.sum(got["stderr"].view(np.uint32) != se.view(np.uint32)))
    assert bad_se == 0, "%s: %d stderr channels differ" % (label, bad_se)


def _nee_case(host, orc32, label, cam_h, world_h, cam_o, world_o, nx, ny, ns, oflags=0, flag_sets=DEVICE_FLAGS):
    sc = host.lower(world_h).upload(0, nee=True)
    lights = oracle_lights(orc32, world_o, sc)
    assert len(lights) == len(sc.lights()) > 0
    ref = orc32.render_nee(cam_o, world_o, lights, nx, ny, ns, seed=SEED, flags=ARITH_DEVICE | THROUGHPUT_FORM | oflags,
                           samples=True)
    for fl, dflags in flag_sets:
        got = sc.render_nee(cam_h, nx, ny, ns, sig=True, seed=SEED, flags=dflags | _dev_ext(oflags))
        _check("%s/%s" % (label, fl), got, ref)
    orc32.free_all()
    return ref


# ---- named scenes ---------------------------------------------------------------------------------------------------------
NAMED = [("cornell_box", 0), ("lit_smoke", 0), ("lit_smoke", FACE_FORWARD), ("simple_light", 0), ("simple_light", SKY),
         ("lit_random_spheres", 0), ("lit_random_spheres", UV_BOOK | SKY), ("hollow_glass", 0), ("hollow_glass", FACE_FORWARD | UV_BOOK),
         ("lit_final_scene", 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,oflags", NAMED, ids=["%s-%d" % c for c in NAMED])
def test_named_scenes_equal_oracle(host, orc32, name, oflags):
    nx, ny, ns = 40, 30, 12
    cam_h, world_h = _build(host, name, nx, ny)
    cam_o, world_o = _build(orc32, name, nx, ny)
    ref = _nee_case(host, orc32, name, cam_h, world_h, cam_o, world_o, nx, ny, ns, oflags)
    assert np.any(ref["linear"] > 0)


@pytest.mark.gpu
def test_ragged_image_equals_oracle(host, orc32):
    """25 x 17: partial 8 x 8 tiles on both edges."""
    nx, ny, ns = 25, 17, 16
    cam_h, world_h = _build(host, "cornell_box", nx, ny)
    cam_o, world_o = _build(orc32, "cornell_box", nx, ny)
    _nee_case(host, orc32, "ragged", cam_h, world_h, cam_o, world_o, nx, ny, ns)


# ---- random compositions ----------------------------------------------------------------------------------------------------
PLACEMENTS = [("unit", 1.0, (0.0, 0.0, 0.0)), ("scale1_64", 1.0 / 64.0, (0.0, 0.0, 0.0)), ("scale300", 300.0, (0.0, 0.0, 0.0)),
              ("offset700", 1.0, (700.0, 0.0, -700.0))]
RANDOM = [pytest.param(s, p, id="%d-%s" % (s, p[0])) for p in PLACEMENTS for s in (range(1, 25) if p[0] == "unit" else range(1, 5))]


@pytest.mark.gpu
@pytest.mark.parametrize("instanced", [False, True], ids=["plain", "instanced"])
@pytest.mark.parametrize("seed,placement", RANDOM)
def test_random_scenes_equal_oracle(host, orc32, seed, placement, instanced):
    nx, ny, ns = 24, 16, 6
    _, scale, off = placement
    cam_h, world_h = scenes_random.build(host, seed, nx, ny, instanced=instanced, scale=scale, offset=off)
    cam_o, world_o = scenes_random.build(orc32, seed, nx, ny, instanced=instanced, scale=scale, offset=off)
    oflags = SKY if seed % 3 == 0 else (FACE_FORWARD if seed % 3 == 1 else 0)
    flag_sets = DEVICE_FLAGS[:2] if seed % 2 else [DEVICE_FLAGS[0], DEVICE_FLAGS[3]]
    _nee_case(host, orc32, "random %d %s" % (seed, placement[0]), cam_h, world_h, cam_o, world_o, nx, ny, ns, oflags, flag_sets)


# ---- hand-built edge scenes ------------------------------------------------------------------------------------------------
EDGE_SIZES = {"cdf_boundaries": (64, 64, 48)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(EDGE))
def test_edge_scenes_equal_oracle(host, orc32, name):
    nx, ny, ns = EDGE_SIZES.get(name, (32, 24, 16))
    cam_h, world_h = EDGE[name](host, nx, ny)
    cam_o, world_o = EDGE[name](orc32, nx, ny)
    ref = _nee_case(host, orc32, name, cam_h, world_h, cam_o, world_o, nx, ny, ns, flag_sets=DEVICE_FLAGS[:2])
    assert np.any(ref["linear"] > 0), name


# ---- render_adaptive's standard errors -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_box", "lit_smoke", "simple_light"])
def test_adaptive_stderr_equals_welford(host, orc32, name):
    """render_adaptive(min_spp = ns): render()'s image plus the standard error of rtmi_adaptive.h, against the plain
    oracle's per-sample radiances (lit_smoke: media)."""
    nx, ny, ns = 32, 24, 10
    cam_h, world_h = _build(host, name, nx, ny)
    cam_o, world_o = _build(orc32, name, nx, ny)
    ref = orc32.render_samples(cam_o, world_o, nx, ny, ns, seed=SEED, flags=ARITH_DEVICE | THROUGHPUT_FORM)
    got = host.lower(world_h).render_adaptive(cam_h, nx, ny, ns, min_spp=ns, step_spp=1, seed=SEED, flags=FC)
    assert np.array_equal(got["linear"].view(np.uint32), ref["linear"].view(np.uint32)), name
    assert np.array_equal(got["rgb8"].astype(np.int32), ref["rgb"]), name
    se = welford_stderr(ref["samples"])
    bad = int(np.sum(got["stderr"].view(np.uint32) != se.view(np.uint32)))
    assert bad == 0, "%s: %d stderr channels differ" % (name, bad)
    assert np.all(got["spp"] == ns) and np.any(se > 0)
    orc32.free_all()


# ---- the contract cosine on the device --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_probe_cos_equals_host(orc32):
    lib = abi.load_rtmi()
    rng = np.random.default_rng(4)
    n = 1 << 16
    x = np.concatenate([np.float32(2.0 * np.pi) * rng.uniform(0.0, 1.0, n // 2).astype(np.float32),
                        rng.uniform(-1e6, 1e6, n // 2).astype(np.float32)]).astype(np.float32)
    out = np.zeros(n, np.float32)
    assert lib.rtmi_probe_math(7, x.ctypes.data, None, out.ctypes.data, n) == 0, lib.rtmi_last_error()
    ref = np.array([orc32.lib.orc_rtmi_cosf(float(v)) for v in x], np.float32)
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), int(np.sum(out.view(np.uint32) != ref.view(np.uint32)))
