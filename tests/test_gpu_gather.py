"""Hemisphere gathers (include/rtmi_gather.h) on the device.

The feature is defined by its equivalence with the radiance query: path (i, s) of a gather is the path rtmi_radiance traces
along direction s of point i, bit for bit, and value, stderr and sh are tests/gather_ref.py's reduction of those samples.
Points and normals are the first hits of 16 x 12 primary rays, the normals turned against the ray.
1. path parity: the per-sample values, read from the device form's scratch, equal Scene.radiance along
   gather_directions, both flag settings byte-identical; 2. reduction parity on the same samples;
3. shapes around the 128-item chunk, slab sizes, point and sample splits, sentinels behind every buffer;
4. the device form on a side stream, with scratch for 1 and for 5 points;
5. known answers: a closed emitter, and cornell_box's floor against Scene.irradiance;
6. the refusals that need a handle."""
import ctypes as C

import numpy as np
import pytest

import env_ref
import gather_ref as G
import scenes_extra
from raytracing_rust_amd import abi, gather_directions, primary_rays, scenes, sh_irradiance
from raytracing_rust_amd.host import HostError, Unsupported, sh_basis

NX, NY, SEED, T_MIN = 16, 12, 42, 0.001
FC = abi.RTMI_FLAG_FAST_CULL
DSKY = abi.RTMI_FLAG_SKY
f32 = np.float32
SENTINEL = f32(-12345.5)
PAD = 16


def _build(api, name):
    """(pinhole camera, world) of a named scene"""
    fn, look_from, look_at, vfov = (scenes.SCENES if name in scenes.SCENES else scenes_extra.EXTRA)[name]
    world = scenes_extra.build(api, name, NX, NY, seed=1)[1]
    return scenes.set_camera(api, NX, NY, look_from, look_at, vertical_fov=vfov, aperture=0.0), world


def _surface(sc, cam, n=NX * NY):
    """n surface points with their normals turned against the primary ray that found them (media events, which have no
    normal, and misses dropped; the rest repeated cyclically up to n)"""
    o, d = (a.reshape(-1, 3) for a in primary_rays(cam, NX, NY))
    h = sc.trace(o, d, t_min=T_MIN, seed=SEED)
    nrm = h["normal"].copy()
    back = np.einsum("nc,nc->n", nrm.astype(np.float64), d.astype(np.float64)) > 0.0
    nrm[back] = -nrm[back]
    keep = h["hit"] & np.any(nrm != 0.0, axis=1)
    assert keep.sum() >= n // 4, keep.sum()
    idx = np.resize(np.flatnonzero(keep), n)
    return np.ascontiguousarray(h["p"][idx]), np.ascontiguousarray(nrm[idx])


def _dev(host, sc, pts, nrm, spp, mode="cosine", estimator="plain", flags=FC, times=None, scratch_points=None, first_point=0,
         first_sample=0, slab_points=0, env_select_p=0.5, stream=None):
    """rtmi_gather_device with sentinels behind the three outputs and the scratch -> dict(value, stderr[, sh], scratch
    float32 [scratch_points, spp, 3]); asserts that the sentinels are untouched"""
    import torch

    dev = torch.device("cuda", sc.device)
    n = pts.shape[0]
    cap = n if scratch_points is None else scratch_points
    sphere = mode == "sphere"
    sizes = {"value": n * 3, "stderr": n * 3, "scratch": cap * spp * 3}
    if sphere:
        sizes["sh"] = n * 27
    bufs = {k: torch.full((m + PAD,), float(SENTINEL), dtype=torch.float32, device=dev) for k, m in sizes.items()}
    tp = torch.from_numpy(pts).to(dev)
    tn = None if sphere else torch.from_numpy(nrm).to(dev)
    tt = None if times is None else torch.from_numpy(times).to(dev)
    p = abi.GatherParams(n, spp, abi.GATHER_MODES[mode], abi.ROULETTE_ESTIMATORS[estimator], flags, 50, T_MIN, SEED, first_point,
                         first_sample, slab_points, env_select_p)
    st = torch.cuda.current_stream(dev) if stream is None else stream
    torch.cuda.synchronize(dev)
    host._check(host.lib.rth_gather_device(
        sc.h, C.byref(p), C.c_void_p(tp.data_ptr()), C.c_void_p(tn.data_ptr()) if tn is not None else None,
        C.c_void_p(tt.data_ptr()) if tt is not None else None, C.c_void_p(bufs["value"].data_ptr()),
        C.c_void_p(bufs["stderr"].data_ptr()), C.c_void_p(bufs["sh"].data_ptr()) if sphere else None,
        C.c_void_p(bufs["scratch"].data_ptr()), C.c_uint64(cap * spp * 12), C.c_void_p(st.cuda_stream)))
    st.synchronize()
    res = {}
    for k, m in sizes.items():
        a = bufs[k].cpu().numpy()
        assert np.all(a[m:] == SENTINEL), k
        res[k] = a[:m]
    res["value"], res["stderr"] = res["value"].reshape(n, 3), res["stderr"].reshape(n, 3)
    res["scratch"] = res["scratch"].reshape(cap, spp, 3)
    if sphere:
        res["sh"] = res["sh"].reshape(n, 9, 3)
    return res


def _radiance_samples(sc, pts, dirs, estimator, flags, times=None, first_point=0, first_sample=0, env_select_p=0.5):
    """the radiance query along every direction -> float32 [n, spp, 3]: the gather's definition"""
    out = np.zeros(dirs.shape, f32)
    for s in range(dirs.shape[1]):
        r = sc.radiance(pts, np.ascontiguousarray(dirs[:, s]), times, spp=1, estimator=estimator, t_min=T_MIN, path_t_min=T_MIN,
                        seed=SEED, first_ray=first_point, first_sample=first_sample + s, stream_skip=0, flags=flags, samples=True,
                        env_select_p=env_select_p)
        out[:, s] = r["samples"][:, 0]
    return out


def _same(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=f32), np.ascontiguousarray(b, dtype=f32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), "%s: %d of %d values differ" % (what, int(np.sum(a.view(np.uint32) != b.view(np.uint32))), a.size)


# ---- 1. / 2. path and reduction parity --------------------------------------------------------------------------------------
PARITY = [("cornell_box", "plain", 0, False), ("cornell_box", "nee", 0, False), ("lit_smoke", "nee", 0, False),
          ("random_spheres", "env_nee", 0, True), ("final_scene", "plain", DSKY, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,estimator,sky,sun", PARITY, ids=["%s-%s" % c[:2] for c in PARITY])
def test_paths_are_the_radiance_querys_and_the_reduction_is_the_headers(host, name, estimator, sky, sun):
    cam, world = _build(host, name)
    sc = host.lower(world).upload(0, nee=estimator in ("nee", "env_nee"))
    if sun:
        sc.attach_env(env_ref.sun_map())
    pts, nrm = _surface(sc, cam)
    n, spp, fp, fs, sel = pts.shape[0], 5, 1000, 3, 0.25
    # random_spheres has moving spheres: its points get times, the others the time-0 plane
    times = np.random.default_rng(3).uniform(0.0, 1.0, n).astype(f32) if name == "random_spheres" else None
    for mode in ("cosine", "sphere"):
        dirs = gather_directions(nrm, spp, seed=SEED, mode=mode, first_point=fp, first_sample=fs, n=n)
        ref = _radiance_samples(sc, pts, dirs, estimator, FC | sky, times, fp, fs, sel)
        nonzero = float(np.mean(np.any(ref != 0.0, axis=-1)))
        print("%s %s %s: %.1f %% of the samples are non-zero" % (name, estimator, mode, 100.0 * nonzero))
        # Not a vacuous pass.  A light sample or the sky lights nearly every vertex (the radiance tests see 50 % and more).
        # The plain estimator in cornell_box has to find the lamp by chance: its form factor is 130 * 105 / (pi * 555^2) =
        # 1.4 % from the floor beneath it and less elsewhere, and a path leaves through the open front after a few bounces.
        lit = np.any(ref != 0.0, axis=-1)
        assert nonzero >= (0.005 if (name, estimator) == ("cornell_box", "plain") else 0.3), nonzero
        # samples, not one value repeated (paths that end on the lamp or in the map's uniform sky at once do share theirs)
        assert len(np.unique(ref[lit], axis=0)) > 4
        got = {}
        for flags in (sky, FC | sky):
            got[flags] = _dev(host, sc, pts, nrm, spp, mode, estimator, flags, times, first_point=fp, first_sample=fs, env_select_p=sel)
            _same(got[flags]["scratch"], ref, "%s samples, flags %d" % (mode, flags))
        want = G.reduce(ref, mode, dirs if mode == "sphere" else None)
        for k in want:
            _same(got[sky][k], got[FC | sky][k], k + " between the flags")
            _same(got[FC | sky][k], want[k], "%s %s" % (mode, k))
        assert np.all(np.isfinite(want["stderr"])) and np.any(want["stderr"] > 0)


# ---- 3. shapes, slabs, splits -----------------------------------------------------------------------------------------------
@pytest.fixture
def cornell(host):
    cam, world = _build(host, "cornell_box")
    sc = host.lower(world).upload(0, nee=True)
    pts, nrm = _surface(sc, cam)
    return sc, pts, nrm


SHAPES = [(1, 1), (3, 43), (65, 2), (192, 8)]  # 129 and 130 items around the 128-item chunk, a partial last chunk


@pytest.mark.gpu
@pytest.mark.parametrize("n,spp", SHAPES)
def test_shapes_slabs_and_splits(host, cornell, n, spp):
    sc, pts, nrm = cornell
    pts, nrm = pts[:n], nrm[:n]
    kw = dict(spp=spp, estimator="nee", seed=SEED, t_min=T_MIN)
    whole = {m: _dev(host, sc, pts, nrm, spp, m, "nee") for m in ("cosine", "sphere")}
    for mode in ("cosine", "sphere"):
        w = whole[mode]
        keys = ("value", "stderr") + (("sh",) if mode == "sphere" else ())
        if spp == 1:
            assert np.all(np.isposinf(w["stderr"]))
        for slab in (0, 1, 7, n):
            r = sc.gather(pts, nrm, mode=mode, slab_points=slab, **kw)
            for k in keys:
                _same(r[k], w[k], "%s %s, host form, slab %d" % (mode, k, slab))
            r = _dev(host, sc, pts, nrm, spp, mode, "nee", slab_points=slab)
            for k in keys:
                _same(r[k], w[k], "%s %s, device form, slab %d" % (mode, k, slab))
        # the host form equals the restatement of the whole's samples
        want = G.reduce(w["scratch"], mode, gather_directions(nrm, spp, seed=SEED, mode=mode, n=n) if mode == "sphere" else None)
        for k in keys:
            _same(w[k], want[k], "%s %s against the restatement" % (mode, k))
        # points split at k, the second call with first_point = k
        for k in (1, 63):
            if k < n:
                a = _dev(host, sc, pts[:k], nrm[:k], spp, mode, "nee")
                b = _dev(host, sc, pts[k:], nrm[k:], spp, mode, "nee", first_point=k)
                _same(np.concatenate([a["scratch"], b["scratch"]]), w["scratch"], "%s samples, points split at %d" % (mode, k))
                for key in keys:
                    _same(np.concatenate([a[key], b[key]]), w[key], "%s %s, points split at %d" % (mode, key, k))
        # samples split at k, the second call with first_sample = k
        for k in (1, spp // 2):
            if 0 < k < spp:
                a = _dev(host, sc, pts, nrm, k, mode, "nee")
                b = _dev(host, sc, pts, nrm, spp - k, mode, "nee", first_sample=k)
                _same(np.concatenate([a["scratch"], b["scratch"]], axis=1), w["scratch"], "%s samples split at %d" % (mode, k))


@pytest.mark.gpu
def test_empty_batch_and_optional_outputs(host, cornell):
    sc, pts, nrm = cornell
    r = sc.gather(pts[:0], nrm[:0], spp=4, estimator="nee")
    assert r["value"].shape == (0, 3) and r["stderr"].shape == (0, 3)
    r = sc.gather(pts[:5], mode="sphere", spp=4, estimator="nee", seed=SEED, sh=False)
    assert "sh" not in r
    _same(r["value"], _dev(host, sc, pts[:5], nrm[:5], 4, "sphere", "nee")["value"], "value without sh")


# ---- 4. the device form -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_form_on_a_side_stream(host):
    import torch

    cam, world = _build(host, "cornell_box")
    sc = host.lower(world).upload(0, nee=True)
    pts, nrm = _surface(sc, cam, 67)
    before = sc.render_nee(cam, NX, NY, 4, seed=SEED)
    dev = torch.device("cuda", sc.device)
    side = torch.cuda.Stream(device=dev)
    for mode in ("cosine", "sphere"):
        ref = sc.gather(pts, nrm, spp=6, mode=mode, estimator="nee", seed=SEED, t_min=T_MIN)
        for cap in (1, 5):
            got = _dev(host, sc, pts, nrm, 6, mode, "nee", scratch_points=cap, stream=side)
            for k in ("value", "stderr") + (("sh",) if mode == "sphere" else ()):
                _same(got[k], ref[k], "%s %s with scratch for %d points" % (mode, k, cap))
        # the Python face: torch tensors in, torch tensors out, on torch's current stream
        tp, tn = torch.from_numpy(pts).to(dev), torch.from_numpy(nrm).to(dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(side):
            got = sc.gather(tp, tn, spp=6, mode=mode, estimator="nee", seed=SEED, t_min=T_MIN, scratch_bytes=12 * 6 * 5)
        side.synchronize()
        for k in ref:
            if k != "kernel_ms":
                assert isinstance(got[k], torch.Tensor) and got[k].device == dev
                _same(got[k].cpu().numpy(), ref[k], "%s %s through torch" % (mode, k))
    after = sc.render_nee(cam, NX, NY, 4, seed=SEED)
    for k in ("linear", "rgb8", "stderr"):
        assert before[k].tobytes() == after[k].tobytes(), k


# ---- 5. known answers -------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    a, b = (np.ascontiguousarray(np.broadcast_to(x, np.broadcast(a, b).shape), dtype=f32).view(np.uint32).astype(np.int64) for x in (a, b))
    return np.abs(a - b)


@pytest.mark.gpu
def test_inside_a_closed_emitter(host):
    le = np.array([2.0, 3.0, 4.0])
    w = host.HittableList()
    w.push(host.Sphere((0.0, 0.0, 0.0), 10.0, host.DiffuseLight(host.SolidTexture(*le))))
    sc = host.lower(w).upload(0)
    rng = np.random.default_rng(5)
    n, spp = 16, 256
    pts = rng.uniform(-4.0, 4.0, (n, 3)).astype(f32)
    nrm = rng.standard_normal((n, 3)).astype(f32)
    r = sc.gather(pts, nrm, spp=spp, mode="cosine", seed=9)
    assert _ulps(r["value"], (np.pi * le).astype(f32)).max() <= 1
    assert np.all(r["stderr"] == 0.0)
    r = sc.gather(pts, mode="sphere", spp=spp, seed=9)
    assert _ulps(r["value"], le.astype(f32)).max() <= 1 and np.all(r["stderr"] == 0.0)
    y0 = float(f32(0.2820947917738781))
    assert _ulps(r["sh"][:, 0], (4.0 * np.pi * le * y0).astype(f32)).max() <= 1
    # The probe's irradiance: E(n) = (4 pi / spp) sum_s Le f(d_s) with f(d) = sum_k A_k Y_k(n) Y_k(d).  Band 0 of f is the
    # constant 1/4; the estimate's error is that of the band-1 and band-2 sums, from the sample variance of f.
    got = sh_irradiance(r["sh"], nrm)
    d = gather_directions(None, spp, seed=9, mode="sphere", n=n).astype(np.float64)
    unit = nrm.astype(np.float64) / np.linalg.norm(nrm.astype(np.float64), axis=1, keepdims=True)
    a = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)
    f = np.einsum("nk,nsk->ns", sh_basis(unit) * a, sh_basis(d))
    se = 4.0 * np.pi * f.std(axis=1, ddof=1) / np.sqrt(spp)  # per unit of Le
    z = (got - np.pi * le) / (se[:, None] * le)
    print("sh_irradiance inside the emitter: largest |z| %.2f, relative standard error %.3f" % (np.abs(z).max(), (se / np.pi).max()))
    assert np.all(se > 0) and np.abs(z).max() <= 5.0


@pytest.mark.gpu
def test_cornell_floor_agrees_with_scene_irradiance(host):
    """cornell_box's open-floor point under the lamp (the point of tests/test_gpu_radiance.py's floor test), NEE, 256
    directions: the gather against Scene.irradiance, whose directions come from another frame and another seed, so the two
    estimates are independent: |z| <= 5 per channel."""
    sc = host.lower(_build(host, "cornell_box")[1]).upload(0, nee=True)
    pts = np.array([[250.0, 0.0, 285.0]], f32)
    nrm = np.array([[0.0, 1.0, 0.0]], f32)
    a = sc.gather(pts, nrm, spp=256, mode="cosine", estimator="nee", seed=11)
    b = sc.irradiance(pts, nrm, 256, seed=12, estimator="nee")
    comb = np.sqrt(a["stderr"].astype(np.float64) ** 2 + b["stderr"].astype(np.float64) ** 2)
    z = (a["value"].astype(np.float64) - b["irradiance"]) / comb
    print("gather", a["value"], a["stderr"], "irradiance", b["irradiance"], b["stderr"], "z", z)
    assert np.all(a["value"] > 0) and np.all(np.isfinite(z)) and np.abs(z).max() <= 5.0


# ---- 6. the refusals that need a handle -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_missing_attachments_and_multi_device_are_refused(host):
    cam, world = _build(host, "cornell_box")
    sc = host.lower(world).upload(0)
    pts, nrm = _surface(sc, cam, 8)
    for est in ("env", "env_nee"):
        with pytest.raises(HostError, match="rtmi_gather: no environment map attached"):
            sc.gather(pts, nrm, spp=2, estimator=est)
    out = np.zeros((8, 3), f32)
    sc2 = host.lower(_build(host, "cornell_box")[1]).upload(0)  # no light table
    p = abi.GatherParams(8, 1, abi.RTMI_GATHER_COSINE, abi.RTMI_ROULETTE_NEE, 0, 50, 0.001, 1, 0, 0, 0, 0.5)
    call = lambda: host.lib.rth_gather(sc2.h, C.byref(p), pts.ctypes.data, nrm.ctypes.data, None, out.ctypes.data, None, None, None)
    assert call() != 0 and b"rtmi_gather: no light table attached" in host.lib.rth_last_error()
    sc2.attach_env(env_ref.sun_map(16, 8))
    p.estimator = abi.RTMI_ROULETTE_ENV_NEE
    assert call() != 0 and b"rtmi_gather: no light table attached" in host.lib.rth_last_error()
    with pytest.raises(HostError, match="RTMI_FLAG_SKY is refused"):
        sc2.gather(pts, nrm, spp=2, estimator="env", flags=FC | DSKY)
    assert sc2.gather(pts, nrm, spp=2, estimator="env")["value"].shape == (8, 3)
    import torch

    dev = torch.device("cuda", sc2.device)
    with pytest.raises(HostError, match="rtmi_gather_device: no light table attached"):
        sc2_p = abi.GatherParams(8, 1, 0, abi.RTMI_ROULETTE_NEE, 0, 50, 0.001, 1, 0, 0, 0, 0.5)
        buf = torch.zeros((8 * 3 * 4,), dtype=torch.float32, device=dev)
        host._check(host.lib.rth_gather_device(sc2.h, C.byref(sc2_p), C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr()), None,
                                               C.c_void_p(buf.data_ptr()), None, None, C.c_void_p(buf.data_ptr()), C.c_uint64(96), None))
    sc3 = host.lower(_build(host, "cornell_box")[1])
    sc3.upload_multi([0])
    try:
        with pytest.raises(Unsupported):
            sc3.gather(pts, nrm, spp=2)
    finally:
        sc3.free_multi()
