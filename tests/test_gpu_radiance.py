"""Radiance queries (include/rtmi_radiance.h) on the device.

The feature is defined by its equivalence with the render: the radiance query of a render's camera rays is that render's
per-sample radiance, bit for bit.  The test restates camera_sample in float32 (pinhole cameras: aperture 0 on both sides,
shutter [0, 1]) for every sample s — direction from words 0 and 1 of stream (seed, s, j*nx + i), time from word 2 — and
makes one radiance call per s with first_sample = s, spp = 1, stream_skip = 3 and the rays in pixel-index order.
1. plain == the fp32 oracle's render_samples, both flag settings, byte-identical between them;
2. NEE == the oracle's render_nee(samples=True);
3. ENV and ENV_NEE == the device's own render_env, through the numpy restatements of the resolve, and == the oracle's
   render_env(samples=True), sample for sample;
4. mean and stderr are the two numpy restatements of the returned samples; spp = 1 gives stderr = +inf;
5. the result does not depend on how samples or rays are split into calls; the device form writes nothing beyond;
6. the first segment's interval follows trace / occluded;
7. the device form on a non-default stream equals the host form and leaves the handle's renders unchanged;
8. irradiance: a known answer inside a closed emitter, and NEE against plain on cornell_box's floor;
9. what needs a handle among the refusals: a missing map, a missing light table, a multi-GPU scene."""
import ctypes as C

import numpy as np
import pytest

import env_ref
import query_ref as Q
import scenes_extra
from nee_oracle_ref import oracle_lights, welford_stderr
from oracle.oracle import ARITH_DEVICE, LIGHT_DTYPE, SKY, THROUGHPUT_FORM
from raytracing_rust_amd import abi, env_from_sky, philox, scenes
from raytracing_rust_amd.host import RAY_DTYPE, HostError, Unsupported
from roulette_ref import image

NX, NY, NS, SEED = 32, 24, 8, 42
FC = abi.RTMI_FLAG_FAST_CULL
DSKY = abi.RTMI_FLAG_SKY
f32 = np.float32


def _build(api, name):
    """(pinhole camera, world) of a named scene"""
    fn, look_from, look_at, vfov = (scenes.SCENES if name in scenes.SCENES else scenes_extra.EXTRA)[name]
    world = scenes_extra.build(api, name, NX, NY, seed=7 if name == "lit_random_spheres" else 1)[1]
    return scenes.set_camera(api, NX, NY, look_from, look_at, vertical_fov=vfov, aperture=0.0), world


def _camera_rays(c, s, nx=NX, ny=NY, seed=SEED):
    """camera_sample restated in float32 for sample s of every pixel, in pixel-index order (index = j * nx + i, j = 0 the
    bottom row): origins [n, 3], directions [n, 3], times [n]"""
    assert c.lens_radius == 0.0
    llc, hor, ver, org = (np.array(list(x), f32) for x in (c.lower_left_corner, c.horizontal, c.vertical, c.origin))
    j, i = np.meshgrid(np.arange(ny, dtype=np.uint32), np.arange(nx, dtype=np.uint32), indexing="ij")
    pix = j * np.uint32(nx) + i
    w = philox.philox4x32_10_np(np.zeros_like(pix), np.full_like(pix, s), pix, np.zeros_like(pix), seed)
    u01 = [((x >> np.uint32(8)).astype(np.float64) * (1.0 / 16777216.0)).astype(f32) for x in w[:3]]
    u = ((i.astype(f32) + u01[0]) / f32(nx)).astype(f32)
    v = ((j.astype(f32) + u01[1]) / f32(ny)).astype(f32)
    d = (((llc + hor * u[..., None]).astype(f32) + (ver * v[..., None]).astype(f32)).astype(f32) - org).astype(f32)
    t = (f32(c.time0) + (u01[2] * (f32(c.time1) - f32(c.time0))).astype(f32)).astype(f32)
    n = nx * ny
    return np.ascontiguousarray(np.broadcast_to(org, (n, 3))), d.reshape(n, 3), t.reshape(n)


def _gather(sc, cam, estimator, flags, **kw):
    """one radiance call per sample -> samples [ny, nx, ns, 3], row 0 the top row, as the oracle lays them out"""
    c = cam.lower()
    out = np.zeros((NY, NX, NS, 3), f32)
    for s in range(NS):
        o, d, t = _camera_rays(c, s)
        r = sc.radiance(o, d, t, spp=1, estimator=estimator, seed=SEED, first_sample=s, stream_skip=3, flags=flags,
                        samples=True, **kw)
        assert r["samples"].shape == (NX * NY, 1, 3)
        out[:, :, s] = r["samples"][:, 0].reshape(NY, NX, 3)[::-1]
        assert r["mean"].tobytes() == r["samples"][:, 0].tobytes() and np.all(np.isposinf(r["stderr"]))
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _differing(a, b):
    return int(np.sum(_bits(a) != _bits(b)))


# ---- 1. plain == oracle ---------------------------------------------------------------------------------------------------
PLAIN = [("random_spheres", SKY), ("hollow_glass", SKY), ("final_scene", SKY), ("two_perlin_spheres", SKY), ("cornell_box", 0),
         ("lit_smoke", 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,oflags", PLAIN, ids=[c[0] for c in PLAIN])
def test_plain_equals_oracle_samples(host, orc32, name, oflags):
    cam_o, world_o = _build(orc32, name)
    ref = orc32.render_samples(cam_o, world_o, NX, NY, NS, seed=SEED, flags=ARITH_DEVICE | THROUGHPUT_FORM | oflags)["samples"]
    orc32.free_all()
    nonzero = float(np.mean(np.any(ref != 0.0, axis=-1)))
    print("%s: %.1f %% of the oracle's samples are non-zero" % (name, 100.0 * nonzero))
    if oflags & SKY:
        assert nonzero >= 0.9, nonzero  # not a vacuous pass
    cam_h, world_h = _build(host, name)
    sc = host.lower(world_h).upload(0)
    dflags = DSKY if oflags & SKY else 0
    exact, fast = _gather(sc, cam_h, "plain", dflags), _gather(sc, cam_h, "plain", dflags | FC)
    assert exact.tobytes() == fast.tobytes(), "%s: %d channels differ between the flags" % (name, _differing(exact, fast))
    bad = _differing(fast, ref)
    assert bad == 0, "%s: %d of %d channels differ from the oracle" % (name, bad, ref.size)


# ---- 2. NEE == oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_box", "lit_smoke", "lit_random_spheres", "lit_final_scene", "hollow_glass"])
def test_nee_equals_oracle_samples(host, orc32, name):
    cam_h, world_h = _build(host, name)
    sc = host.lower(world_h).upload(0, nee=True)
    cam_o, world_o = _build(orc32, name)
    lights = oracle_lights(orc32, world_o, sc)
    assert len(lights) == len(sc.lights()) > 0
    ref = orc32.render_nee(cam_o, world_o, lights, NX, NY, NS, seed=SEED, flags=ARITH_DEVICE | THROUGHPUT_FORM, samples=True)["samples"]
    orc32.free_all()
    nonzero = float(np.mean(np.any(ref != 0.0, axis=-1)))
    print("%s: %.1f %% of the oracle's samples are non-zero" % (name, 100.0 * nonzero))
    assert nonzero >= 0.4, nonzero
    exact, fast = _gather(sc, cam_h, "nee", 0), _gather(sc, cam_h, "nee", FC)
    assert exact.tobytes() == fast.tobytes(), "%s: %d channels differ between the flags" % (name, _differing(exact, fast))
    bad = _differing(fast, ref)
    assert bad == 0, "%s: %d of %d channels differ from the oracle" % (name, bad, ref.size)


# ---- 3. ENV and ENV_NEE == the device's own render ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["random_spheres", "lit_random_spheres"])
@pytest.mark.parametrize("nee", [False, True], ids=["env", "env_nee"])
def test_env_equals_the_devices_render(host, name, nee):
    cam_h, world_h = _build(host, name)
    sc = host.lower(world_h).upload(0)
    sc.attach_env(env_from_sky(256, 128))
    ref = sc.render_env(cam_h, NX, NY, NS, nee=nee, env_select_p=0.5, seed=SEED)
    assert np.any(ref["linear"] > 0)
    got = _gather(sc, cam_h, "env_nee" if nee else "env", FC, env_select_p=0.5)
    assert len(np.unique(got.reshape(-1, 3), axis=0)) > NX * NY  # samples, not one value per pixel
    lin = image(got)[0]
    assert _differing(lin, ref["linear"]) == 0, "%d channels of linear differ" % _differing(lin, ref["linear"])
    se = welford_stderr(got)
    assert _differing(se, ref["stderr"]) == 0, "%d channels of stderr differ" % _differing(se, ref["stderr"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["random_spheres", "lit_random_spheres", "lit_smoke"])
@pytest.mark.parametrize("nee", [False, True], ids=["env", "env_nee"])
def test_env_equals_oracle_samples(host, orc32, name, nee):
    """The sun map, env_select_p = 0.25, the tables from tests/env_ref.py: random_spheres has no light (p_env = 1), the
    other two share the light samples between the map and their lamps."""
    cam_h, world_h = _build(host, name)
    cam_o, world_o = _build(orc32, name)
    sc = host.lower(world_h).upload(0, nee=True)
    lights = oracle_lights(orc32, world_o, sc) if len(sc.lights()) else np.zeros(0, LIGHT_DTYPE)
    assert (len(lights) > 0) == (name != "random_spheres")
    m = env_ref.sun_map()
    orc32.reset_counters()
    ref = orc32.render_env(cam_o, world_o, lights, m, env_ref.tables(m), nee, 0.25, NX, NY, NS, seed=SEED,
                           flags=ARITH_DEVICE | THROUGHPUT_FORM, samples=True)["samples"]
    cnt = orc32.counters()
    orc32.free_all()
    assert (cnt["env_sample"] >= 100) == nee and (cnt["env_area_sample"] >= 100) == (nee and len(lights) > 0)
    nonzero = float(np.mean(np.any(ref != 0.0, axis=-1)))
    print("%s: %.1f %% of the oracle's samples are non-zero" % (name, 100.0 * nonzero))
    assert nonzero >= 0.4, nonzero
    sc.attach_env(m)
    est = "env_nee" if nee else "env"
    exact, fast = _gather(sc, cam_h, est, 0, env_select_p=0.25), _gather(sc, cam_h, est, FC, env_select_p=0.25)
    assert exact.tobytes() == fast.tobytes(), "%s: %d channels differ between the flags" % (name, _differing(exact, fast))
    bad = _differing(fast, ref)
    assert bad == 0, "%s: %d of %d channels differ from the oracle" % (name, bad, ref.size)


# ---- 4. / 5. mean, stderr and independence of splitting --------------------------------------------------------------------
def _fan(name, n=1024):
    look_from, look_at = Q.scene_camera(name)
    return Q.fan(np.random.default_rng(7), look_from, look_at, n)


def _mean_restated(x):
    """[n, spp, 3] float32 -> the f64 sum in sample order / spp, rounded once"""
    s = np.zeros((x.shape[0], 3), np.float64)
    for k in range(x.shape[1]):
        s = s + x[:, k].astype(np.float64)
    return (s / float(x.shape[1])).astype(f32)


@pytest.fixture
def spheres(host):
    """random_spheres (moving spheres, a BVH) with its light table and a 1000-ray fan with times"""
    sc = host.lower(_build(host, "random_spheres")[1]).upload(0)
    o, d = _fan("random_spheres", 1000)
    t = np.random.default_rng(3).uniform(0.0, 1.0, 1000).astype(f32)
    return sc, o, d, t


@pytest.mark.gpu
def test_mean_and_stderr_restate_the_samples(spheres):
    sc, o, d, t = spheres
    r = sc.radiance(o, d, t, spp=8, seed=SEED, flags=FC | DSKY, samples=True)
    x = r["samples"]
    assert x.shape == (1000, 8, 3) and len(np.unique(x.reshape(-1, 3), axis=0)) > 4000
    assert r["mean"].tobytes() == _mean_restated(x).tobytes()
    assert r["stderr"].tobytes() == welford_stderr(x).tobytes()
    assert np.all(np.isfinite(r["stderr"])) and np.any(r["stderr"] > 0)
    one = sc.radiance(o, d, t, spp=1, seed=SEED, flags=FC | DSKY, samples=True)
    assert np.all(np.isposinf(one["stderr"])) and one["mean"].tobytes() == one["samples"].tobytes()
    assert one["samples"][:, 0].tobytes() == np.ascontiguousarray(x[:, 0]).tobytes()


@pytest.mark.gpu
def test_independent_of_splitting(spheres):
    sc, o, d, t = spheres
    kw = dict(seed=SEED, flags=FC | DSKY, samples=True)
    whole = sc.radiance(o, d, t, spp=8, **kw)
    # samples: eight spp = 1 calls
    for s in range(8):
        r = sc.radiance(o, d, t, spp=1, first_sample=s, **kw)
        assert r["samples"][:, 0].tobytes() == np.ascontiguousarray(whole["samples"][:, s]).tobytes(), s
    # rays: two calls split at k, the second with first_ray = k
    for k in (1, 63, 64, 65, 999):
        a = sc.radiance(o[:k], d[:k], t[:k], spp=8, **kw)
        b = sc.radiance(o[k:], d[k:], t[k:], spp=8, first_ray=k, **kw)
        for key in ("samples", "mean", "stderr"):
            assert np.concatenate([a[key], b[key]]).tobytes() == whole[key].tobytes(), (k, key)
    # prefixes (an empty batch among them)
    for k in (0, 1, 63, 65):
        a = sc.radiance(o[:k], d[:k], t[:k], spp=8, **kw)
        for key in ("samples", "mean", "stderr"):
            assert a[key].shape[0] == k and a[key].tobytes() == whole[key][:k].tobytes(), (k, key)


@pytest.mark.gpu
def test_device_form_writes_nothing_beyond_its_records(host, spheres):
    import torch

    sc, o, d, t = spheres
    n, spp, pad = 65, 3, 16
    dev = torch.device("cuda", sc.device)
    rays = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    rays[:, 0:3], rays[:, 4:7] = torch.from_numpy(o[:n]).to(dev), torch.from_numpy(d[:n]).to(dev)
    rays[:, 3], rays[:, 7] = 0.001, float("inf")
    tm = torch.from_numpy(t[:n]).to(dev)
    sentinel = -12345.5
    bufs = {k: torch.full((m * 3 + pad,), sentinel, dtype=torch.float32, device=dev) for k, m in (("mean", n), ("stderr", n), ("samples", n * spp))}
    p = abi.RadianceParams(n, spp, abi.RTMI_ROULETTE_PLAIN, FC | DSKY, 50, 0.001, SEED, 0, 0, 0, 0.5)
    host._check(host.lib.rth_radiance_device(sc.h, C.byref(p), C.c_void_p(rays.data_ptr()), C.c_void_p(tm.data_ptr()),
                                             C.c_void_p(bufs["mean"].data_ptr()), C.c_void_p(bufs["stderr"].data_ptr()),
                                             C.c_void_p(bufs["samples"].data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    torch.cuda.synchronize(dev)
    ref = sc.radiance(o[:n], d[:n], t[:n], spp=spp, seed=SEED, flags=FC | DSKY, samples=True)
    for k, m in (("mean", n), ("stderr", n), ("samples", n * spp)):
        got = bufs[k].cpu().numpy()
        assert got[:m * 3].tobytes() == ref[k].tobytes(), k
        assert np.all(got[m * 3:] == f32(sentinel)), k


# ---- 6. the first segment's interval follows trace -------------------------------------------------------------------------
def _sky_color(d):
    """RTMI_FLAG_SKY's gradient of a direction, in float32 without fused operations: what a path that leaves the world at
    once returns"""
    x, y, z = (d[:, k].astype(f32) for k in range(3))
    nrm = np.sqrt(((x * x + y * y).astype(f32) + z * z).astype(f32)).astype(f32)
    t = (f32(0.5) * ((y / nrm).astype(f32) + f32(1.0))).astype(f32)
    a = (f32(1.0) - t).astype(f32)
    return np.stack([(a + (t * f32(c)).astype(f32)).astype(f32) for c in (0.5, 0.7, 1.0)], axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("name,sky", [("cornell_box", False), ("final_scene", True)])
def test_first_segment_interval_follows_trace(host, name, sky):
    """trace and occluded decide every case.  They draw a medium's free path from the stream keyed seed + i of ray i, a
    radiance path from stream (seed, sample, first_ray + i): for final_scene, whose rays all cross the fog, each ray is
    therefore its own radiance call with seed + i, first_ray = 0 and stream_skip = 0, which is trace's stream of ray i."""
    sc = host.lower(_build(host, name)[1]).upload(0)
    o, d = _fan(name)
    n = o.shape[0]
    flags = FC | (DSKY if sky else 0)
    media = name == "final_scene"

    def rad(t_min, t_max):
        t_min, t_max = (np.broadcast_to(np.asarray(x, f32), (n,)) for x in (t_min, t_max))
        if not media:
            return sc.radiance(o, d, spp=1, seed=Q.SEED, flags=flags, t_min=t_min, t_max=t_max)["mean"]
        return np.concatenate([sc.radiance(o[i:i + 1], d[i:i + 1], spp=1, seed=Q.SEED + i, flags=flags, t_min=t_min[i:i + 1],
                                           t_max=t_max[i:i + 1])["mean"] for i in range(n)])

    full_hit = sc.trace(o, d, t_min=Q.T_MIN, seed=Q.SEED, flags=FC)
    full = rad(Q.T_MIN, np.inf)
    miss = _sky_color(d) if sky else np.zeros((n, 3), f32)
    hits = full_hit["hit"]
    assert 0.5 * n < hits.sum()
    t = full_hit["t"]
    big = f32(3.0e38)
    cases = [(Q.T_MIN, np.where(hits, t, big)), (Q.T_MIN, np.where(hits, np.nextafter(t, f32(np.inf)), big)),
             (Q.T_MIN, np.where(hits, np.nextafter(t, f32(0.0)), big)), (np.where(hits, np.nextafter(t, f32(np.inf)), Q.T_MIN), np.inf)]
    n_miss = n_same = 0
    for t_min, t_max in cases:
        occ = sc.occluded(o, d, t_min=t_min, t_max=t_max, seed=Q.SEED, flags=FC)
        got = rad(t_min, t_max)
        tmn, tmx = (np.broadcast_to(np.asarray(x, f32), (n,)) for x in (t_min, t_max))
        free = ~occ
        assert got[free].tobytes() == miss[free].tobytes()
        inside = occ & hits & (tmn < t) & (t < tmx)
        assert got[inside].tobytes() == full[inside].tobytes()
        n_miss += int(free.sum())
        n_same += int(inside.sum())
    assert n_miss > n // 2 and n_same > n // 2, (n_miss, n_same)  # both branches were exercised


# ---- 7. the device form ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_form_on_a_side_stream(host):
    import torch

    cam_h, world_h = _build(host, "cornell_box")
    sc = host.lower(world_h).upload(0)
    before = sc.render_nee(cam_h, NX, NY, 4, seed=SEED)
    o, d = _fan("cornell_box", 999)
    ref = sc.radiance(o, d, spp=4, estimator="nee", seed=SEED, samples=True)
    dev = torch.device("cuda", sc.device)
    side = torch.cuda.Stream(device=dev)
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        got = sc.radiance(to, td, spp=4, estimator="nee", seed=SEED, samples=True)
    side.synchronize()
    for k in ("mean", "stderr", "samples"):
        assert isinstance(got[k], torch.Tensor) and got[k].device == dev
        assert got[k].cpu().numpy().tobytes() == ref[k].tobytes(), k
    after = sc.render_nee(cam_h, NX, NY, 4, seed=SEED)
    for k in ("linear", "rgb8", "stderr"):
        assert before[k].tobytes() == after[k].tobytes(), k


# ---- 8. irradiance --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_irradiance_inside_a_closed_emitter(host):
    le = (2.0, 3.0, 4.0)
    w = host.HittableList()
    w.push(host.Sphere((0.0, 0.0, 0.0), 10.0, host.DiffuseLight(host.SolidTexture(*le))))
    sc = host.lower(w).upload(0)
    rng = np.random.default_rng(5)
    pts = rng.uniform(-4.0, 4.0, (16, 3)).astype(f32)
    nrm = rng.standard_normal((16, 3)).astype(f32)
    r = sc.irradiance(pts, nrm, 12, seed=9)
    want = (np.pi * np.array(le, np.float64)).astype(f32)
    ulp = np.abs(_bits(r["irradiance"]).astype(np.int64) - _bits(np.broadcast_to(want, (16, 3))).astype(np.int64))
    assert ulp.max() <= 1, ulp.max()
    assert np.all(r["stderr"] == 0.0)


@pytest.mark.gpu
def test_irradiance_nee_agrees_with_plain_on_cornells_floor(host):
    """Both estimate the same integral: at 256 directions and the fixed seed their difference is within 4 combined
    standard errors in every channel — a statistical tolerance, fixed by the seed.  The point lies under the lamp
    (x 213..343, z 227..332 at y = 554) on the strip of floor between the two boxes: the short one's footprint ends at its
    corner (236, 273), the tall one's begins at its corner (265, 295)."""
    sc = host.lower(_build(host, "cornell_box")[1]).upload(0, nee=True)
    pts = np.array([[250.0, 0.0, 285.0]], f32)
    nrm = np.array([[0.0, 1.0, 0.0]], f32)
    a = sc.irradiance(pts, nrm, 256, seed=11, estimator="plain", t_min=0.01)
    b = sc.irradiance(pts, nrm, 256, seed=11, estimator="nee", t_min=0.01)
    print("plain", a["irradiance"], a["stderr"], "nee", b["irradiance"], b["stderr"])
    assert np.all(a["irradiance"] > 0) and np.all(b["irradiance"] > 0)
    comb = np.sqrt(a["stderr"].astype(np.float64) ** 2 + b["stderr"].astype(np.float64) ** 2)
    assert np.all(np.abs(a["irradiance"].astype(np.float64) - b["irradiance"]) <= 4.0 * comb)
    assert np.all(b["stderr"] < a["stderr"])  # the light sample is what NEE is for


# ---- 9. the refusals that need a handle -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_missing_attachments_are_refused(host):
    cam_h, world_h = _build(host, "cornell_box")
    sc = host.lower(world_h).upload(0)
    o, d = _fan("cornell_box", 8)
    for est in ("env", "env_nee"):
        with pytest.raises(HostError, match="rtmi_radiance: no environment map attached"):
            sc.radiance(o, d, estimator=est)
    rays = np.zeros(8, RAY_DTYPE)
    rays["o"], rays["d"], rays["t_min"], rays["t_max"] = o, d, 0.001, np.inf
    out = np.zeros((8, 3), f32)
    sc2 = host.lower(_build(host, "cornell_box")[1]).upload(0)  # no light table
    p = abi.RadianceParams(8, 1, abi.RTMI_ROULETTE_NEE, 0, 50, 0.001, 1, 0, 0, 0, 0.5)
    rc = host.lib.rth_radiance(sc2.h, C.byref(p), rays.ctypes.data, None, out.ctypes.data, None, None, None)
    assert rc != 0 and b"rtmi_radiance: no light table attached" in host.lib.rth_last_error()
    sc2.attach_env(env_from_sky(16, 8))
    p.estimator = abi.RTMI_ROULETTE_ENV_NEE
    rc = host.lib.rth_radiance(sc2.h, C.byref(p), rays.ctypes.data, None, out.ctypes.data, None, None, None)
    assert rc != 0 and b"rtmi_radiance: no light table attached" in host.lib.rth_last_error()
    with pytest.raises(HostError, match="RTMI_FLAG_SKY is refused"):
        sc2.radiance(o, d, estimator="env", flags=FC | DSKY)
    assert sc2.radiance(o, d, estimator="env")["mean"].shape == (8, 3)
    sc3 = host.lower(_build(host, "cornell_box")[1])
    sc3.upload_multi([0])
    try:
        with pytest.raises(Unsupported):
            sc3.radiance(o, d)
    finally:
        sc3.free_multi()
