"""RTMI_FLAG_BATCH_COOP (include/rtmi_batch_coop.h) on the device: radiance queries, gathers, sparse renders
and the per-pixel adaptive renders on the wave-cooperative kernel.

The claim is "the same bits, another kernel": every comparison is on the raw bits of every output of the flagged call
against the unflagged one (_pair: first without the flag, then with it, and the expected kernel each time), and for the
radiance queries under NEE also against the fp32 oracle's per-sample radiance, so that the claim does not rest on the
per-lane kernel alone.  Scenes: cornell_box and lit_smoke (no BVH item: the lean pool form with the LDS word ring, a
top-level medium), lit_random_spheres and lit_final_scene (alternative trees, a deep tree, a medium beside a tree),
random_spheres under a map, and an instanced random composition for the fallback.

 1. radiance, camera rays (2160 items: no multiple of 64, several chunks), all four estimators; the oracle;
 2. radiance, caller rays with their own first-segment intervals; batch sizes 1, 65 and 300 x 7; a split batch; n = 0;
 3. gathers, cosine and sphere, NEE and plain;
 4. sparse renders: a list, the device form with a device-side count, a refine;
 5. per-pixel and windowed adaptive renders;
 6. the fallbacks to the per-lane kernel;
 7. the two test knobs;
 8. repeatability, and the device form after a blocking call has reserved the kernel's scratch.

Which kernel ran: these entries have no rtmi_stats (the per-pixel renders have, and it is read too), so _kernel asks
through the public interface: the same call with RTMI_FLAG_TEST_OVERFLOW beside the flag fails with the overflow report if
and only if the cooperative kernel ran; the per-lane kernel never reads the knob."""
import numpy as np
import pytest

import scenes_extra
import scenes_random
import test_gpu_radiance as R
from nee_oracle_ref import oracle_lights
from oracle.oracle import ARITH_DEVICE, THROUGHPUT_FORM
from raytracing_rust_amd import abi, env_from_sky, scenes
from raytracing_rust_amd.host import HostError

SEED = 42
FC = abi.RTMI_FLAG_FAST_CULL
COOP, PERLANE = abi.RTMI_KERNEL_WAVE_COOP, abi.RTMI_KERNEL_PERLANE
POOL_KNOB = 1 << 11
FLT_MAX = float(np.finfo(np.float32).max)
ESTIMATORS = ["plain", "nee", "env", "env_nee"]
f32 = np.float32


def _world(api, name, nx, ny):
    if name in scenes.SCENES:
        return scenes.build(api, name, nx, ny, seed=1)
    return scenes_extra.build(api, name, nx, ny, seed=7 if name == "lit_random_spheres" else 1)


def _pinhole(api, name, nx, ny):
    _, look_from, look_at, vfov = (scenes.SCENES if name in scenes.SCENES else scenes_extra.EXTRA)[name]
    return scenes.set_camera(api, nx, ny, look_from, look_at, vertical_fov=vfov, aperture=0.0)


def _scene(host, name, nx, ny, env=True, nee=True):
    cam, world = _world(host, name, nx, ny)
    sc = host.lower(world).upload(0, nee=nee)
    if env:
        sc.attach_env(env_from_sky(64, 32))
    return sc, cam


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(label, got, ref, keys):
    """Bit for bit, output by output; counts the differing words first so that a failure says how much differs."""
    for key in keys:
        a, b = np.asarray(got[key]), np.asarray(ref[key])
        assert a.shape == b.shape and a.dtype == b.dtype, (label, key)
        bad = int(np.sum(_bits(a) != _bits(b)))
        assert bad == 0, "%s: %d of %d words of %s differ" % (label, bad, a.size, key)


OVERFLOW = abi.RTMI_FLAG_TEST_OVERFLOW


def _kernel(call, flags=FC, status=None):
    """The kernel the flagged call(flags=..., coop=True) runs.  status: the scene, for a device form, whose report comes
    through rtmi_scene_status."""
    try:
        call(flags=flags | OVERFLOW, coop=True)
        if status is not None:
            status.check_status()
    except HostError as e:
        assert "overflow" in str(e), e
        return COOP
    return PERLANE


def _pair(label, call, keys, want=COOP, flags=FC, status=None):
    """call(flags=..., coop=...) without and with the flag: the same bits, the expected kernel.  Returns the flagged dict."""
    ref = call(flags=flags, coop=False)
    assert "kernel" not in ref, label
    got = call(flags=flags, coop=True)
    assert got.get("kernel", want) == want, (label, got["kernel"])  # rtmi_stats.kernel, where the entry has stats
    assert _kernel(call, flags, status) == want, label
    _same(label, got, ref, keys)
    return got


RAD = ("mean", "stderr", "samples")


# ---- 1. radiance, camera rays -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_box", "lit_smoke", "lit_random_spheres", "lit_final_scene"])
def test_radiance_camera_rays_all_estimators(host, name):
    nx, ny, spp = 24, 18, 5
    sc, _ = _scene(host, name, nx, ny)
    o, d, t = R._camera_rays(_pinhole(host, name, nx, ny).lower(), 0, nx, ny, SEED)
    # a time plane sends a scene whose BVH time range is bounded to the exact traversal (case 6): rays at time 0 there
    times = t if sc.desc().bvh_time_lo <= -FLT_MAX else None
    assert o.shape[0] * spp == 2160 and 2160 % 64 != 0
    for est in ESTIMATORS:
        got = _pair("%s/%s" % (name, est), lambda **kw: sc.radiance(o, d, times, spp=spp, estimator=est, seed=SEED, stream_skip=3,
                                                                      samples=True, **kw), RAD)
        assert np.any(got["samples"] > 0), (name, est)
    # the seek of the stream: inside block 0, at the start of block 1 (the ring's other half, nothing generated), inside
    # block 1, and inside block 2 (the first half again); plain: the lean pool form's LDS ring where the scene has no tree
    for skip in (1, 4, 6, 9):
        _pair("%s/skip %d" % (name, skip), lambda **kw: sc.radiance(o, d, times, spp=2, estimator="plain", seed=SEED, stream_skip=skip,
                                                                     samples=True, **kw), RAD)


@pytest.mark.gpu
def test_random_spheres_under_a_map(host):
    """random_spheres (no emitter, one deep tree of static and moving spheres) under env_from_sky: PLAIN, ENV and ENV_NEE,
    radiance along the camera's rays at time 0, a gather and a pixel list."""
    nx, ny, spp = 24, 18, 5
    sc, cam = _scene(host, "random_spheres", nx, ny, nee=False)
    o, d, _ = R._camera_rays(_pinhole(host, "random_spheres", nx, ny).lower(), 0, nx, ny, SEED)
    first = sc.trace(o, d, flags=FC)
    at = np.flatnonzero(first["hit"])[:100]
    nrm = np.ascontiguousarray(first["normal"][at], dtype=f32)
    pts = (first["p"][at] + f32(0.01) * nrm).astype(f32)
    px = np.random.default_rng(3).permutation(nx * ny)[:37].astype(np.uint32)
    for est in ("plain", "env", "env_nee"):
        got = _pair("radiance/" + est, lambda **kw: sc.radiance(o, d, spp=spp, estimator=est, seed=SEED, stream_skip=3, samples=True,
                                                                **kw), RAD)
        assert np.any(got["samples"] > 0) == (est != "plain"), est  # without the map, and without the sky, nothing emits
        _pair("gather/" + est, lambda **kw: sc.gather(pts, spp=7, mode="sphere", estimator=est, seed=SEED, **kw), ("value", "stderr", "sh"))
        _pair("pixels/" + est, lambda **kw: sc.render_pixels(cam, nx, ny, px, 6, estimator=est, seed=SEED, samples=True, **kw), RAD)
    got = _pair("radiance/plain under the sky", lambda **kw: sc.radiance(o, d, spp=spp, estimator="plain", seed=SEED, stream_skip=3,
                                                                        samples=True, **kw), RAD, flags=FC | abi.RTMI_FLAG_SKY)
    assert np.any(got["samples"] > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_box", "lit_final_scene"])
def test_flagged_radiance_equals_oracle(host, orc32, name):
    """The way tests/test_gpu_radiance.py reaches the oracle: one call per sample of the pinhole camera's rays."""
    nx, ny, ns = 24, 18, 5
    sc, _ = _scene(host, name, nx, ny, env=False)
    cam_o, world_o = _pinhole(orc32, name, nx, ny), _world(orc32, name, nx, ny)[1]
    lights = oracle_lights(orc32, world_o, sc)
    assert len(lights) == len(sc.lights()) > 0
    ref = orc32.render_nee(cam_o, world_o, lights, nx, ny, ns, seed=SEED, flags=ARITH_DEVICE | THROUGHPUT_FORM, samples=True)["samples"]
    orc32.free_all()
    assert float(np.mean(np.any(ref != 0.0, axis=-1))) >= 0.4  # not a vacuous pass
    c = _pinhole(host, name, nx, ny).lower()
    o, d, t = R._camera_rays(c, 0, nx, ny, SEED)
    assert _kernel(lambda **kw: sc.radiance(o, d, t, spp=1, estimator="nee", seed=SEED, stream_skip=3, **kw)) == COOP
    got = np.zeros((ny, nx, ns, 3), f32)
    for s in range(ns):
        o, d, t = R._camera_rays(c, s, nx, ny, SEED)
        r = sc.radiance(o, d, t, spp=1, estimator="nee", seed=SEED, first_sample=s, stream_skip=3, flags=FC, samples=True, coop=True)
        got[:, :, s] = r["samples"][:, 0].reshape(ny, nx, 3)[::-1]
    bad = int(np.sum(_bits(got) != _bits(ref)))
    assert bad == 0, "%s: %d of %d channels differ from the oracle" % (name, bad, ref.size)


# ---- 2. radiance, caller rays -------------------------------------------------------------------------------------------------
def _caller_rays(sc, host, name, n):
    """n incoherent rays only a caller sends: origins at the hit points of the camera's rays, seeded directions with every
    component non-zero.  A quarter of them end at half their known first-hit distance, a quarter start just beyond it, the
    rest are unbounded: the two quarters are drawn from the candidates that hit something, the rest from all of them."""
    nx, ny = 32, 24
    o, d, _ = R._camera_rays(_pinhole(host, name, nx, ny).lower(), 0, nx, ny, SEED)
    first = sc.trace(o, d, flags=FC)
    at = np.flatnonzero(first["hit"])
    m = at.size
    rng = np.random.default_rng(5)
    dirs = rng.uniform(0.05, 1.0, (m, 3)).astype(f32) * rng.choice(np.array([-1.0, 1.0], f32), (m, 3))
    assert np.all(dirs != 0.0)
    org = np.ascontiguousarray(first["p"][at], dtype=f32)
    hit = sc.trace(org, dirs, t_min=0.001, flags=FC)
    t1 = np.where(hit["hit"], hit["t"], f32(1.0)).astype(f32)
    far = np.flatnonzero(hit["hit"] & (t1 > f32(0.01)))  # (half the distance stays above the ray's t_min)
    q = n // 4
    assert far.size >= 2 * q and m >= n, (far.size, m)
    bounded = far[:2 * q]
    rest = np.setdiff1d(np.arange(m), bounded)[:n - 2 * q]
    pick = np.concatenate([bounded, rest])
    kind = np.concatenate([np.zeros(q, int), np.ones(q, int), np.full(n - 2 * q, 2)])
    order = rng.permutation(n)  # the three kinds mixed within every wavefront
    pick, kind = pick[order], kind[order]
    t_min = np.full(n, 0.001, f32)
    t_max = np.full(n, np.inf, f32)
    short, late = kind == 0, kind == 1
    t_max[short] = (f32(0.5) * t1[pick])[short]
    t_min[late] = np.nextafter(t1[pick], f32(np.inf))[late]
    return org[pick], dirs[pick], t_min, t_max, short


@pytest.mark.gpu
@pytest.mark.parametrize("name,est", [("cornell_box", "plain"), ("lit_final_scene", "nee"), ("lit_random_spheres", "env_nee")])
def test_radiance_caller_rays(host, name, est):
    sc, _ = _scene(host, name, 24, 18)
    o, d, t_min, t_max, short = _caller_rays(sc, host, name, 300)

    def call(n, spp, lo=0, first_ray=0, **kw):
        s = slice(lo, lo + n)
        return sc.radiance(o[s], d[s], t_min=t_min[s], t_max=t_max[s], spp=spp, estimator=est, seed=SEED, first_ray=first_ray,
                           samples=True, **kw)

    for n, spp in ((1, 1), (65, 1), (300, 7)):
        got = _pair("%s/%d x %d" % (name, n, spp), lambda **kw: call(n, spp, **kw), RAD)
    if name == "cornell_box":  # no medium, no map: a first segment that ends before the first hit misses, and the path ends black
        assert np.all(got["samples"][short] == 0.0) and np.any(got["samples"][~short] > 0.0)
    # the same batch in two calls
    a, b = call(130, 7, flags=FC, coop=True), call(170, 7, lo=130, first_ray=130, flags=FC, coop=True)
    assert _kernel(lambda **kw: call(170, 7, lo=130, first_ray=130, **kw)) == COOP
    _same(name + "/split", {k: np.concatenate([a[k], b[k]]) for k in RAD}, got, RAD)
    # an empty batch launches nothing: RTMI_OK, and not even the overflow knob has anything to report
    r = sc.radiance(o[:0], d[:0], spp=3, estimator=est, flags=FC | OVERFLOW, coop=True)
    assert r["mean"].shape == (0, 3)
    sc.check_status()


# ---- 3. gathers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_box", "lit_final_scene"])
def test_gathers(host, name):
    nx, ny, n, spp = 24, 18, 100, 7
    sc, _ = _scene(host, name, nx, ny)
    o, d, _ = R._camera_rays(_pinhole(host, name, nx, ny).lower(), 0, nx, ny, SEED)
    first = sc.trace(o, d, flags=FC)
    at = np.flatnonzero(first["hit"])[:n]
    assert at.size == n
    nrm = np.ascontiguousarray(first["normal"][at], dtype=f32)
    pts = (first["p"][at] + f32(0.01) * nrm).astype(f32)
    for est in ("nee", "plain"):
        for mode, keys in (("cosine", ("value", "stderr")), ("sphere", ("value", "stderr", "sh"))):
            got = _pair("%s/%s/%s" % (name, est, mode), lambda **kw: sc.gather(pts, nrm, spp=spp, mode=mode, estimator=est,
                                                                                seed=SEED, **kw), keys)
            assert np.any(got["value"] > 0), (name, est, mode)
    got = _pair(name + "/irradiance", lambda **kw: sc.irradiance(pts, nrm, spp, seed=SEED, estimator="nee", **kw),
                ("irradiance", "stderr"))


# ---- 4. sparse renders --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,est", [("cornell_box", "nee"), ("lit_final_scene", "nee"), ("lit_random_spheres", "env")])
def test_sparse_renders(host, name, est):
    import torch

    nx, ny, ns = 40, 30, 6
    sc, cam = _scene(host, name, nx, ny)
    px = np.random.default_rng(3).permutation(nx * ny)[:37].astype(np.uint32)
    _pair(name + "/list", lambda **kw: sc.render_pixels(cam, nx, ny, px, ns, estimator=est, seed=SEED, samples=True, **kw), RAD)
    # the device form, with a device-side count below the list's capacity: the first 20 entries are traced
    dev = torch.device("cuda", sc.device)
    lst = torch.from_numpy(px.astype(np.int32)).to(dev)
    cnt = torch.tensor([20, 12345], dtype=torch.int32, device=dev)

    def device_form(**kw):
        r = sc.render_pixels(cam, nx, ny, lst, ns, estimator=est, seed=SEED, count=cnt, **kw)
        torch.cuda.synchronize(dev)
        return {k: r[k][:20].cpu().numpy() for k in RAD}

    got = _pair(name + "/device", device_form, RAD, status=sc)
    host_form = sc.render_pixels(cam, nx, ny, px[:20], ns, estimator=est, seed=SEED, samples=True, flags=FC)
    _same(name + "/device == blocking", got, host_form, RAD)
    sc.check_status()


@pytest.mark.gpu
def test_sparse_refine(host):
    nx, ny = 40, 30
    sc, cam = _scene(host, "lit_final_scene", nx, ny, env=False)
    with sc.upscaler(nx, ny, low=(20, 15), estimator="nee", flags=FC) as ups:
        planes = ups.render(cam, 4, seed=1, aux=True, out="numpy")
    classes = tuple(int(c) for c in np.unique(planes["cls"]))[-2:]
    got = _pair("refine", lambda **kw: sc.refine_pixels(cam, planes, classes=classes, ns=6, estimator="nee", seed=9, **kw),
                ("linear", "rgb8", "cls"))
    assert got["refined"][0] > 0 and np.any(got["cls"] == 4)


# ---- 5. per-pixel and windowed adaptive renders -------------------------------------------------------------------------------
ADAPTIVE = ("linear", "rgb8", "stderr", "spp", "counts")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_box", "lit_final_scene"])
def test_pixelwise_and_windowed(host, name):
    nx, ny = 40, 30
    sc, cam = _scene(host, name, nx, ny, env=False)
    kw0 = dict(abs_tol=0.02, estimator="nee", seed=SEED)
    got = _pair(name + "/pixelwise", lambda **kw: sc.render_pixelwise(cam, nx, ny, 16, 4, 4, **kw0, **kw), ADAPTIVE)
    assert got["kernel"] == COOP  # rtmi_stats.kernel
    assert got["spp"].min() >= 4 and got["spp"].max() == 16 and got["samples"] == int(got["spp"].sum())  # every step ran
    for radius in (0, 2):
        win = _pair("%s/window %d" % (name, radius), lambda **kw: sc.render_windowed(cam, nx, ny, 16, 4, 4, radius=radius, **kw0, **kw),
                    ADAPTIVE)
        if radius == 0:
            _same(name + "/radius 0 is pixelwise", win, got, ADAPTIVE)
        assert win["kernel"] == COOP


# ---- 6. fallbacks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fallbacks_run_the_perlane_kernel_with_the_same_bits(host):
    nx, ny = 24, 18
    sc, cam = _scene(host, "random_spheres", nx, ny, nee=False)  # no emitter: the map alone
    o, d, t = R._camera_rays(_pinhole(host, "random_spheres", nx, ny).lower(), 0, nx, ny, SEED)

    def rad(times, **kw):
        return sc.radiance(o, d, times, spp=5, estimator="env", seed=SEED, stream_skip=3, samples=True, **kw)

    _pair("flagged, for contrast", lambda **kw: rad(None, **kw), RAD, want=COOP)
    _pair("no FAST_CULL", lambda **kw: rad(None, **kw), RAD, want=PERLANE, flags=0)
    # a time plane, and the scene's BVH time range is bounded: the existing rule picks the exact traversal
    dsc = sc.desc()
    assert dsc.bvh_time_lo > -FLT_MAX and dsc.bvh_time_hi < FLT_MAX
    _pair("time plane", lambda **kw: rad(t, **kw), RAD, want=PERLANE)
    px = np.arange(0, nx * ny, 13, dtype=np.uint32)
    _pair("no FAST_CULL, sparse", lambda **kw: sc.render_pixels(cam, nx, ny, px, 5, estimator="env", seed=SEED, samples=True, **kw),
          RAD, want=PERLANE, flags=0)
    # an instanced random composition
    cam3, world3 = scenes_random.build(host, 4, 24, 16, instanced=True)
    sc3 = host.lower(world3).upload(0, nee=True)
    d3 = sc3.desc()
    assert any((d3.prim_meta[i].flags >> abi.RTMI_PRIMFLAG_XF_COUNT_SHIFT) & 15 for i in range(d3.n_prims))
    px3 = np.arange(0, 24 * 16, 7, dtype=np.uint32)
    got = _pair("instanced", lambda **kw: sc3.render_pixels(cam3, 24, 16, px3, 6, estimator="nee", seed=SEED, samples=True, **kw),
                RAD, want=PERLANE)
    assert np.any(got["samples"] > 0)
    _pair("instanced, pixelwise", lambda **kw: sc3.render_pixelwise(cam3, 24, 16, 8, 4, 4, abs_tol=0.05, estimator="nee", seed=SEED,
                                                                     **kw), ADAPTIVE, want=PERLANE)


# ---- 7. the knobs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_small_pool_knob(host):
    nx, ny = 24, 18
    sc, _ = _scene(host, "lit_final_scene", nx, ny, env=False)
    o, d, t = R._camera_rays(_pinhole(host, "lit_final_scene", nx, ny).lower(), 0, nx, ny, SEED)
    ref = sc.radiance(o, d, t, spp=5, estimator="nee", seed=SEED, stream_skip=3, samples=True, flags=FC)
    knob = lambda **kw: sc.radiance(o, d, t, spp=5, estimator="nee", seed=SEED, stream_skip=3, samples=True, **kw)  # noqa: E731
    got = knob(flags=FC | POOL_KNOB, coop=True)
    assert _kernel(knob, FC | POOL_KNOB) == COOP
    _same("256-entry pool", got, ref, RAD)
    with pytest.raises(HostError, match="flags"):
        sc.radiance(o, d, t, spp=5, estimator="nee", flags=FC | POOL_KNOB)


@pytest.mark.gpu
def test_overflow_report(host):
    """The overflow report is a status word: the blocking form returns RTMI_ERR_DEVICE, rtmi_scene_status reports a device
    form's overflow once and then clears, and a following plain call succeeds."""
    import torch

    nx, ny = 24, 18
    sc, _ = _scene(host, "lit_final_scene", nx, ny, env=False)
    o, d, t = R._camera_rays(_pinhole(host, "lit_final_scene", nx, ny).lower(), 0, nx, ny, SEED)
    ref = sc.radiance(o, d, t, spp=2, estimator="nee", seed=SEED, samples=True, flags=FC)
    with pytest.raises(HostError, match="flags"):
        sc.radiance(o, d, t, spp=2, estimator="nee", flags=FC | abi.RTMI_FLAG_TEST_OVERFLOW)
    with pytest.raises(HostError, match="overflow"):
        sc.radiance(o, d, t, spp=2, estimator="nee", seed=SEED, flags=FC | abi.RTMI_FLAG_TEST_OVERFLOW, coop=True)
    sc.check_status()  # reported by the blocking call: not again
    dev = torch.device("cuda", sc.device)
    r = sc.radiance(torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev), torch.from_numpy(t).to(dev), spp=2, estimator="nee",
                    seed=SEED, flags=FC | abi.RTMI_FLAG_TEST_OVERFLOW, coop=True)
    torch.cuda.synchronize(dev)
    assert r["mean"].shape == (o.shape[0], 3)
    # a blocking call in between reads its own word: it succeeds, and leaves the device form's report where it is
    between = sc.radiance(o, d, t, spp=2, estimator="nee", seed=SEED, samples=True, flags=FC, coop=True)
    _same("between", between, ref, RAD)
    with pytest.raises(HostError, match="overflow"):
        sc.check_status()
    sc.check_status()  # once
    again = sc.radiance(o, d, t, spp=2, estimator="nee", seed=SEED, samples=True, flags=FC, coop=True)
    _same("after the report", again, ref, RAD)
    sc.check_status()


# ---- 8. repeatability -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_repeat_and_device_form_after_a_blocking_call(host):
    import torch

    nx, ny = 24, 18
    sc, _ = _scene(host, "lit_random_spheres", nx, ny)
    o, d, _ = R._camera_rays(_pinhole(host, "lit_random_spheres", nx, ny).lower(), 0, nx, ny, SEED)
    kw = dict(spp=5, estimator="env_nee", seed=SEED, stream_skip=3, flags=FC, coop=True)
    sc.radiance(o[:1], d[:1], **kw)  # any cooperative call reserves the kernel's spill buffer (include/rtmi_batch_coop.h)
    dev = torch.device("cuda", sc.device)
    od, dd = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    torch.cuda.synchronize(dev)
    free_before = torch.cuda.mem_get_info(dev)[0]
    r = sc.radiance(od, dd, **kw)
    torch.cuda.synchronize(dev)
    assert _kernel(lambda **k2: sc.radiance(o, d, spp=5, estimator="env_nee", seed=SEED, stream_skip=3, **k2)) == COOP
    a = sc.radiance(o, d, samples=True, **kw)
    b = sc.radiance(o, d, samples=True, **kw)
    _same("repeat", b, a, RAD)
    _same("device form", {k: r[k].cpu().numpy() for k in RAD}, a, RAD)
    # the enqueue took nothing from the device beyond torch's own tensors (3 outputs and the packed rays, < 1 MiB)
    del r
    assert free_before - torch.cuda.mem_get_info(dev)[0] <= 64 << 20
    sc.check_status()
