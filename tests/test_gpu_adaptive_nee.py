"""Adaptive sampling with next-event estimation or environment lighting (include/rtmi_adaptive_nee.h) on
the device.

The core property is §11's with another estimator: both Philox streams of a path (stream 0 for the path, stream 3 for its
light samples) are keyed by (seed, sample, pixel) and a pixel's samples are summed in sample order, so a tile that
retires with n samples is bit for bit, stderr included, the tile of render_nee / render_env with ns = n.  The decisions
are pinned through the API, as in test_gpu_adaptive.py.

1. tile equivalence with the decisions pinned (three NEE scenes, four environment cases);
2. statistics only (min_spp == ns) is the fixed render;
3. reductions: no lights -> render_adaptive; an all-zero map -> adaptive NEE (nee=1) or render_adaptive (nee=0);
4. the zero-variance trap of the plain estimator, against a known answer;
5. fewer camera paths than the plain estimator for the same tolerance;
6. independence from the schedule;
7. progress, cancellation and the handle's state."""
import math

import numpy as np
import pytest

import env_ref
import nee_ref
import scenes_extra
from test_gpu_nee import _floor_scene, _footprints
from raytracing_rust_amd import abi, scenes
from raytracing_rust_amd.host import HostError

NX, NY, NS, MIN, STEP = 160, 120, 128, 16, 16
FC = abi.RTMI_FLAG_FAST_CULL
SEED = 42


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _earth_map():
    data, w, h = scenes.earthmap_rgb8()
    return (np.asarray(data, np.float32).reshape(h, w, 3) / np.float32(255.0)).astype(np.float32)


def _build(host, name, nx, ny):
    if name in scenes.SCENES:
        return scenes.build(host, name, nx, ny, seed=1)
    return scenes_extra.build(host, name, nx, ny, seed=7 if name == "lit_random_spheres" else 1)


class Case:
    """One estimator on one scene: mapname None = the NEE form, else the env form with that map, nee and env_select_p."""

    def __init__(self, host, name, mapname=None, nee=True, p=0.5, nx=NX, ny=NY, flags=FC):
        self.name, self.mapname, self.nee, self.p, self.nx, self.ny, self.flags = name, mapname, nee, p, nx, ny, flags
        self.cam, world = _build(host, name, nx, ny)
        self.sc = host.lower(world).upload(0, nee=True)
        if mapname is not None:
            m = {"sun": env_ref.sun_map, "earth": _earth_map,
                 "zero": lambda: np.zeros((16, 32, 3), np.float32)}[mapname]()
            self.sc.attach_env(m)

    def adaptive(self, ns, mn, step, tol=0.0, rel=0.0, env=None, **kw):
        """env=False: the NEE form on this handle even when a map is attached"""
        kw.setdefault("flags", self.flags)
        if self.mapname is None or env is False:
            return self.sc.render_adaptive(self.cam, self.nx, self.ny, ns, mn, step, abs_tol=tol, rel_tol=rel, nee=True,
                                           seed=SEED, **kw)
        return self.sc.render_adaptive(self.cam, self.nx, self.ny, ns, mn, step, abs_tol=tol, rel_tol=rel, nee=self.nee,
                                       env=True, env_select_p=self.p, seed=SEED, **kw)

    def fixed(self, ns, **kw):
        kw.setdefault("flags", self.flags)
        if self.mapname is None:
            return self.sc.render_nee(self.cam, self.nx, self.ny, ns, seed=SEED, **kw)
        return self.sc.render_env(self.cam, self.nx, self.ny, ns, nee=self.nee, env_select_p=self.p, seed=SEED, **kw)

    def plain(self, ns, mn, step, tol=0.0, rel=0.0, **kw):
        kw.setdefault("flags", self.flags)
        return self.sc.render_adaptive(self.cam, self.nx, self.ny, ns, mn, step, abs_tol=tol, rel_tol=rel, seed=SEED, **kw)


def _tile_max(a, nx, ny):
    """per 8x8 tile, the maximum of a [ny,nx,3] plane over its pixels and channels (row 0 = top row, as the outputs)"""
    ty, tx = (ny + 7) // 8, (nx + 7) // 8
    pad = np.full((ty * 8, tx * 8, 3), -np.inf)
    pad[:ny, :nx] = a
    return pad.reshape(ty, 8, tx, 8, 3).max(axis=(1, 3, 4))


def _mixed_tolerance(case):
    """abs_tol at half the median tile noise after MIN samples of the case's own estimator"""
    st = case.adaptive(MIN, MIN, STEP)
    return 0.5 * float(np.median(_tile_max(st["stderr"].astype(np.float64), case.nx, case.ny)))


CASES = [("cornell_box", None, True, 0.5), ("lit_smoke", None, True, 0.5), ("lit_final_scene", None, True, 0.5),
         ("random_spheres", "sun", False, 0.5), ("random_spheres", "sun", True, 0.5), ("earth", "earth", True, 0.5),
         ("lit_random_spheres", "sun", True, 0.5)]
IDS = ["%s-%s-nee%d" % (n, m or "lights", e) for n, m, e, _ in CASES]


# ---- 1. tile equivalence, decisions pinned ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,mapname,nee,p", CASES, ids=IDS)
def test_tiles_equal_fixed_renders_and_decisions_are_pinned(host, name, mapname, nee, p):
    case = Case(host, name, mapname, nee, p)
    tol = _mixed_tolerance(case)
    ad = case.adaptive(NS, MIN, STEP, tol)
    spp = ad["spp"]
    counts = sorted(set(int(k) for k in np.unique(spp)))
    print(name, mapname, nee, "abs_tol %.4g" % tol, "counts", {k: int((spp == k).sum()) for k in counts},
          "samples", ad["stats"]["samples"])
    assert len(counts) >= 3, counts
    assert all(k in range(MIN, NS + 1, STEP) for k in counts), counts
    assert ad["stats"]["kernel"] == abi.RTMI_KERNEL_PERLANE
    for k in counts:
        m = spp == k
        ref = case.fixed(k)
        for key in ("linear", "rgb8", "stderr"):
            assert _same(ad[key][m], ref[key][m]), (name, k, key)
        if k < NS:  # converged at k: a run that starts at k stops those tiles there
            at_k = case.adaptive(NS, k, STEP, tol)
            assert np.all(at_k["spp"][m] == k), (name, k)
        if k > MIN:  # not converged at k - step: a run that starts there goes on with those tiles
            before = case.adaptive(NS, k - STEP, STEP, tol)
            assert np.all(before["spp"][m] > k - STEP), (name, k)
    assert ad["stats"]["samples"] == int(spp.astype(np.uint64).sum())
    assert ad["stats"]["samples"] < NX * NY * NS


# ---- 2. statistics only ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,mapname,nee,p", [CASES[0], CASES[4], CASES[6]], ids=[IDS[0], IDS[4], IDS[6]])
def test_statistics_only_is_the_fixed_render(host, name, mapname, nee, p):
    case = Case(host, name, mapname, nee, p)
    ns = 40
    fixed = case.fixed(ns)
    out = case.adaptive(ns, ns, 1, 1e9, 1e9)  # every tile retires at min_spp = ns whatever the tolerance
    for key in ("linear", "rgb8", "stderr"):
        assert _same(out[key], fixed[key]), key
    assert np.all(out["spp"] == ns) and out["stats"]["samples"] == NX * NY * ns
    assert np.all(np.isfinite(out["stderr"])) and out["stderr"].max() > 0


# ---- 3. reductions across estimators ----------------------------------------------------------------------------------------
def _all_equal(a, b):
    for key in ("linear", "rgb8", "stderr", "spp"):
        assert _same(a[key], b[key]), key
    assert a["stats"]["samples"] == b["stats"]["samples"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["final_scene", "random_spheres"])
def test_without_lights_adaptive_nee_is_render_adaptive(host, name):
    case = Case(host, name, flags=FC | (abi.RTMI_FLAG_SKY if name == "random_spheres" else 0))
    assert len(case.sc.lights()) == 0
    tol = _mixed_tolerance(case)
    a = case.adaptive(NS, MIN, STEP, tol, 0.01)
    b = case.plain(NS, MIN, STEP, tol, 0.01)
    _all_equal(a, b)
    if name == "random_spheres":
        assert len(np.unique(a["spp"])) >= 2


@pytest.mark.gpu
def test_zero_map_reduces_to_adaptive_nee_and_to_render_adaptive(host):
    zero = Case(host, "cornell_box", "zero", True, 0.5)
    lights = Case(host, "cornell_box")
    tol = _mixed_tolerance(lights)
    _all_equal(zero.adaptive(NS, MIN, STEP, tol), lights.adaptive(NS, MIN, STEP, tol))
    zero.nee = False
    tol = 0.5 * tol
    a, b = zero.adaptive(NS, MIN, STEP, tol), lights.plain(NS, MIN, STEP, tol)
    _all_equal(a, b)
    assert len(np.unique(a["spp"])) >= 2


# ---- 4. the zero-variance trap, against a known answer -------------------------------------------------------------------
# A Lambertian floor under a small sphere light (test_gpu_nee.py's known-answer scene).  The plain estimator reaches the
# light by BSDF sampling only, so most 16-sample tiles never see it: every pixel has mean 0 and stderr 0 and the tile
# retires at min_spp as "converged" although it is lit.  Radius, height, min_spp and the tolerance were set by measuring
# on an MI355X.
TRAP_N, TRAP_NS, TRAP_MIN, TRAP_REL = 64, 64, 16, 0.05
TRAP_LE, TRAP_ALBEDO, TRAP_R, TRAP_H = 4.0, 0.5, 0.05, 2.0


@pytest.mark.gpu
def test_zero_variance_trap_against_a_known_answer(host):
    n = TRAP_N
    light = host.Sphere((0.0, TRAP_H, 0.0), TRAP_R, host.DiffuseLight(host.SolidTexture(TRAP_LE, TRAP_LE, TRAP_LE)))
    cam, world = _floor_scene(host, light, TRAP_ALBEDO)
    sc = host.lower(world).upload(0, nee=True)
    nrm = np.array([0, 1.0, 0])
    pts = _footprints(cam, n)
    f = np.zeros((n, n))
    bound = np.zeros((n, n))
    for r in range(n):
        for c in range(n):
            vals = [nee_ref.f_sphere(p[r, c], nrm, [0, TRAP_H, 0], TRAP_R, 64) for p in pts]
            f[r, c] = vals[0]
            bound[r, c] = max(vals) - min(vals) + 1e-5
    want = TRAP_ALBEDO * TRAP_LE * f
    assert want.min() > 0
    tiles_lit = _tile_max(np.repeat(want[..., None], 3, -1), n, n) > 0

    plain = sc.render_adaptive(cam, n, n, TRAP_NS, TRAP_MIN, TRAP_MIN, rel_tol=TRAP_REL, seed=SEED, flags=FC)
    black = (_tile_max(plain["linear"].astype(np.float64), n, n) == 0) & (_tile_max(plain["stderr"].astype(np.float64), n, n) == 0)
    at_min = _tile_max(np.repeat(plain["spp"][..., None].astype(np.float64), 3, -1), n, n) == TRAP_MIN
    trapped = black & at_min & tiles_lit
    print("plain: %d of %d tiles retired black at min_spp, samples %d" % (trapped.sum(), trapped.size, plain["stats"]["samples"]))
    assert trapped.sum() >= 1  # the guard: this scene is one where the plain estimator is fooled

    ad = sc.render_adaptive(cam, n, n, TRAP_NS, TRAP_MIN, TRAP_MIN, rel_tol=TRAP_REL, nee=True, seed=SEED, flags=FC)
    zero_se = _tile_max(-ad["stderr"].astype(np.float64), n, n) == 0  # some pixel and channel has stderr 0
    print("adaptive NEE: counts", {int(k): int((ad["spp"] == k).sum()) for k in np.unique(ad["spp"])},
          "samples", ad["stats"]["samples"])
    assert not np.any(zero_se & tiles_lit)
    got, se = ad["linear"][..., 0].astype(np.float64), ad["stderr"][..., 0].astype(np.float64)
    z = (got - want) / np.sqrt(se ** 2 + 1e-30)
    assert np.all(np.abs(got - want) <= 5 * se + bound), np.abs(z).max()
    # the plain estimator's black tiles are the trap: the answer there is far from 0 in NEE's standard errors
    assert np.all(want[np.repeat(np.repeat(trapped, 8, 0), 8, 1)] > 5 * se[np.repeat(np.repeat(trapped, 8, 0), 8, 1)])


# ---- 5. fewer paths for the same tolerance ----------------------------------------------------------------------------------
# rel_tol alone is not reachable within 512 samples by either estimator on most tiles (NEE's median pixel needs about 3.6x
# the cap, the plain estimator's about 140x), so both run to the cap and the ratio measures the cap: 0.978 on an
# MI355X.  With abs_tol 0.02 beside it the tolerance is reachable for NEE: measured ratio 0.171.
FEWER_NX, FEWER_NY, FEWER_NS, FEWER_STEP, FEWER_REL, FEWER_ABS = 96, 72, 512, 32, 0.05, 0.02
FEWER_R = 0.25  # bound on samples(adaptive NEE) / samples(plain adaptive)


@pytest.mark.gpu
def test_fewer_paths_for_the_same_tolerance(host):
    case = Case(host, "cornell_box", nx=FEWER_NX, ny=FEWER_NY)
    nee = case.adaptive(FEWER_NS, FEWER_STEP, FEWER_STEP, FEWER_ABS, FEWER_REL)
    plain = case.plain(FEWER_NS, FEWER_STEP, FEWER_STEP, FEWER_ABS, FEWER_REL)
    ratio = nee["stats"]["samples"] / plain["stats"]["samples"]
    print("cornell_box %dx%d abs_tol %.3f rel_tol %.2f: samples nee %d plain %d ratio %.4f" % (
        FEWER_NX, FEWER_NY, FEWER_ABS, FEWER_REL, nee["stats"]["samples"], plain["stats"]["samples"], ratio))
    assert nee["stats"]["samples"] <= FEWER_R * plain["stats"]["samples"]


# ---- 6. schedule independence -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,mapname,nee,p", [CASES[0], CASES[6]], ids=[IDS[0], IDS[6]])
def test_independent_of_culling_kernel_passes_and_repetition(host, name, mapname, nee, p):
    case = Case(host, name, mapname, nee, p)
    tol = _mixed_tolerance(case)
    per_sample = ((NX + 7) // 8) * ((NY + 7) // 8) * 64 * abi.RTMI_SAMPLE_SLOT_BYTES
    runs = [case.adaptive(96, 8, 8, tol, 0.01, flags=f, **kw) for f, kw in (
        (FC, {}), (FC, {}), (0, {}), (FC | abi.RTMI_FLAG_SYNC, {}), (FC | abi.RTMI_FLAG_REF_TREE, {}),
        (FC, {"sample_buffer_bytes": per_sample * 3}))]
    for r in runs[1:]:
        for key in ("linear", "rgb8", "stderr", "spp"):
            assert _same(r[key], runs[0][key]), key
    assert all(r["stats"]["kernel"] == abi.RTMI_KERNEL_PERLANE for r in runs)
    assert len(np.unique(runs[0]["spp"])) >= 2


# ---- 7. progress, cancellation, handle state --------------------------------------------------------------------------------
@pytest.mark.gpu
def test_progress_cancellation_and_handle_state(host):
    case = Case(host, "lit_random_spheres", "sun", True, 0.5)
    sc, cam = case.sc, case.cam

    def others():
        return (sc.render_adaptive(cam, NX, NY, 48, 16, 16, abs_tol=0.01, seed=SEED, flags=FC),
                sc.render_nee(cam, NX, NY, 24, seed=SEED, flags=FC),
                sc.render_env(cam, NX, NY, 24, nee=True, seed=SEED, flags=FC))

    def same_others(a, b):
        for x, y in zip(a, b):
            for key in ("linear", "rgb8", "stderr"):
                assert _same(x[key], y[key]), key

    before = others()
    tol = _mixed_tolerance(case)
    for env in (False, True):
        form = "env" if env else "nee"
        seen = []
        out = case.adaptive(NS, MIN, STEP, tol, env=env, progress=lambda d, t: seen.append((d, t)) and False)
        tiles = ((NX + 7) // 8) * ((NY + 7) // 8)
        assert seen and seen[-1] == (tiles * NS, tiles * NS), (form, seen[-3:])
        assert [d for d, _ in seen] == sorted(d for d, _ in seen) and all(d <= t for d, t in seen)
        assert out["stats"]["samples"] == int(out["spp"].astype(np.uint64).sum())
        same_others(before, others())
        with pytest.raises(HostError, match="cancelled"):
            case.adaptive(NS, MIN, STEP, tol, env=env, progress=lambda d, t: True)
        same_others(before, others())
        again = case.adaptive(NS, MIN, STEP, tol, env=env)
        for key in ("linear", "rgb8", "stderr", "spp"):
            assert _same(again[key], out[key]), (form, key)


@pytest.mark.gpu
def test_refusals_on_the_device(host):
    cam, world = _build(host, "cornell_box", 32, 24)
    sc = host.lower(world).upload(0)
    with pytest.raises(HostError, match="env"):  # no map attached
        sc.render_adaptive(cam, 32, 24, 16, 4, 4, env=True, nee=False, seed=SEED)
    # the defaults are today's call: no light table is attached by a plain adaptive render
    sc.render_adaptive(cam, 32, 24, 16, 4, 4, seed=SEED)
    assert not sc.lights_attached
    out = sc.render_adaptive(cam, 32, 24, 16, 4, 4, nee=True, seed=SEED)
    assert sc.lights_attached and out["stats"]["kernel"] == abi.RTMI_KERNEL_PERLANE
    assert math.isfinite(float(out["linear"].sum()))
