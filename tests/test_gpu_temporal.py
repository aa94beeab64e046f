"""Temporal accumulation (include/rtmi_temporal.h) on the device.

* bit for bit the numpy restatement (tests/temporal_ref.py) in every output plane after every push, on synthetic planes
  (odd sizes, non-finite depths, zero normals, zero and tiny albedos, fireflies) under cameras that stand, translate,
  rotate and jump, with and without standard errors and demodulation and with every parameter off its default, with
  sentinels behind every output; and on renders, media included;
* a standing camera accumulates the mean of its frames, reproducibly;
* a push sequence leaves renders and other handles alone, and render_temporal is its four calls;
* on a moving camera over cornell_box, temporal + a-trous is closer to a converged render than a-trous alone;
* the refusals that need a live handle."""
import ctypes as C

import numpy as np
import pytest

import scenes_extra
import temporal_ref as ref
from raytracing_rust_amd import Temporal, abi, denoise, scenes
from test_gpu_denoise import _synthetic, display_rmse

FC = abi.RTMI_FLAG_FAST_CULL
SEED = 42
F = np.float32
SENTINEL = 0x7FC0BEEF  # a NaN pattern no arithmetic here produces
TAIL = 64
PLANES = (("linear", 3), ("stderr", 3), ("history", 1), ("motion", 2))


def _raw_push(t, cam, lin, alb, nrm, dep, se):
    """rtmi_temporal_push through ctypes with TAIL sentinel words behind every output plane, which must come back
    untouched.  Returns the dict Temporal.push(motion=True) returns."""
    n = t.nx * t.ny
    bufs = {name: np.full(n * k + TAIL, SENTINEL, np.uint32) for name, k in PLANES if se is not None or name != "stderr"}
    c = cam.lower() if hasattr(cam, "lower") else cam
    arrs = [np.ascontiguousarray(a, F) for a in (lin, alb, nrm, dep)] + [None if se is None else np.ascontiguousarray(se, F)]
    rc = t.lib.rtmi_temporal_push(t.h, C.byref(c), *[None if a is None else a.ctypes.data for a in arrs],
                                  bufs["linear"].ctypes.data, bufs["stderr"].ctypes.data if se is not None else None,
                                  bufs["history"].ctypes.data, bufs["motion"].ctypes.data)
    assert rc == 0, t.lib.rtmi_last_error()
    out = {"stderr": None}
    for name, k in PLANES:
        if name in bufs:
            assert np.all(bufs[name][n * k:] == SENTINEL), "%s: written past its end" % name
            assert not np.any(bufs[name][:n * k] == SENTINEL), "%s: not every value written" % name
            out[name] = bufs[name][:n * k].view(F).reshape((t.ny, t.nx) + ((k,) if k > 1 else ())).copy()
    return out


def _assert_same(got, want, depth, what):
    surf = np.isfinite(depth)
    for name, _ in PLANES:
        g, w = got[name], want[name]
        if w is None:
            assert g is None
            continue
        assert np.all(np.isfinite(w[surf])), "%s: the restatement produced non-finite %s on a surface pixel: not comparable" % (what, name)
        diff = g.view(np.uint32) != w.view(np.uint32)
        assert not diff.any(), "%s, %s: %d of %d values differ, e.g. at %s: %r vs %r" % (
            what, name, diff.sum(), diff.size, np.argwhere(diff)[0], g[diff][:4], w[diff][:4])


def _cameras(kind, nx, ny, n=4):
    """n cameras about depths of 2..3 units (what _synthetic makes): a pixel is about 1.8/nx units wide there"""
    lf, la = np.array([0.0, 0.0, 0.0]), np.array([0.0, 0.0, -10.0])
    px = 1.82 / nx
    out = []
    for j in range(n):
        if kind == "stand":
            f, a = lf, la
        elif kind == "translate":  # 1.7 px per frame sideways, 1.4 px up
            f = lf + j * np.array([1.7 * px, 1.4 * px, 0.0])
            a = la + j * np.array([1.7 * px, 1.4 * px, 0.0])
        elif kind == "rotate":  # 1 degree per frame about the up axis
            th = np.radians(float(j))
            f, a = lf, lf + 10.0 * np.array([-np.sin(th), 0.0, -np.cos(th)])
        else:  # jump: every other frame from far away, so that nothing reprojects
            f = lf + (j % 2) * np.array([500.0, 0.0, 0.0])
            a = la + (j % 2) * np.array([500.0, 0.0, 0.0])
        out.append(ref.pinhole(tuple(f), tuple(a), aspect=nx / ny))
    return out


def _sequence(nx, ny, kind, with_se, frames=4, **kw):
    """pushes `frames` synthetic frames through a handle and the restatement; returns the last restated output"""
    cams = _cameras(kind, nx, ny, frames)
    _, alb, nrm, dep, _ = _synthetic(nx, ny)
    t, want_t = Temporal(nx, ny, **kw), ref.Temporal(nx, ny, **kw)
    try:
        for j, cam in enumerate(cams):
            lin, _, _, _, se = _synthetic(nx, ny, seed=10 + j)
            se = se if with_se else None
            got = _raw_push(t, cam, lin, alb, nrm, dep, se)
            want = want_t.push(cam, lin, alb, nrm, dep, stderr=se)
            _assert_same(got, want, dep, "%dx%d %s push %d %r" % (nx, ny, kind, j, kw))
    finally:
        t.close()
    return want, dep


SIZES = [(1, 1), (1, 17), (37, 23), (130, 67)]


# ---- 1. bit for bit the restatement ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny", SIZES)
@pytest.mark.parametrize("kind", ["stand", "translate", "rotate", "jump"])
def test_synthetic_parity(nx, ny, kind):
    for with_se in (True, False):
        for demodulate in (True, False):
            want, dep = _sequence(nx, ny, kind, with_se, demodulate=demodulate)
            surf = np.isfinite(dep)
            if kind == "stand":
                assert np.all(want["history"][surf] == 4)
            if kind == "jump":
                assert np.all(want["history"][surf] == 1)
            if kind in ("translate", "rotate") and nx * ny > 500:  # the case reprojects, and the translation also rejects
                h = want["history"][surf]
                assert (h > 1.5).mean() > 0.5 and (kind == "rotate" or (h == 1).any()), ((h > 1.5).mean(), (h == 1).mean())


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(max_history=2), dict(alpha_min=0.3), dict(alpha_min=1.0), dict(depth_tol=0.0),
                                dict(depth_tol=0.5, normal_min=-1.0), dict(normal_min=0.999), dict(albedo_min=0.5),
                                dict(max_history=65535, alpha_min=0.01, depth_tol=0.01, normal_min=0.5, albedo_min=0.02,
                                     demodulate=False)])
def test_synthetic_parity_parameters(kw):
    for kind in ("stand", "translate"):
        _sequence(37, 23, kind, True, **kw)
        _sequence(37, 23, kind, False, **kw)


def _frame(sc, cam, nx, ny, ns, seed, nee=False):
    if nee:
        noisy = sc.render_nee(cam, nx, ny, ns, seed=seed, flags=FC)
    else:
        noisy = sc.render_adaptive(cam, nx, ny, ns, min_spp=ns, step_spp=1, seed=seed, flags=FC)
    return noisy, sc.render_features(cam, nx, ny, ns, seed=seed, flags=FC)


def _moving_camera(host, nx, ny, j, step=2.0):
    return scenes.set_camera(host, nx, ny, (278.0 + step * j, 278.0, -800.0), (278.0, 278.0, 0.0), vertical_fov=40.0)


@pytest.mark.gpu
def test_render_parity_on_a_moving_camera(host):
    """cornell_box, 64x64, 4 spp, six frames, look_from.x + 2 per frame with look_at fixed.  A pixel spans
    2 tan(20 deg) / 64 = 0.0114 rad.  Per frame the camera turns 2/800 = 0.0025 rad (0.22 px) about the look-at point, which
    undoes the parallax 2/D of a point at distance D exactly at D = 800 (the box's opening) and leaves 0.22 (1 - 800/D) px
    beyond it: 0.09 px at the back wall (D = 1355), less on everything nearer.  Every surface pixel therefore looks up
    its own position to within a tenth of a pixel, each frame, and only the pixels on a depth or normal edge (a few
    hundred of 4096) can lose their history; so at least half of the surface pixels must have history >= 3 after
    six frames."""
    nx = ny = 64
    _, world = scenes.build(host, "cornell_box", nx, ny, seed=1)
    sc = host.lower(world).upload(0)
    t, want_t = Temporal(nx, ny), ref.Temporal(nx, ny)
    for j in range(6):
        cam = _moving_camera(host, nx, ny, j)
        noisy, ft = _frame(sc, cam, nx, ny, 4, SEED + j)
        got = _raw_push(t, cam, noisy["linear"], ft["albedo"], ft["normal"], ft["depth"], noisy["stderr"])
        want = want_t.push(cam, noisy["linear"], ft["albedo"], ft["normal"], ft["depth"], stderr=noisy["stderr"])
        _assert_same(got, want, ft["depth"], "cornell_box frame %d" % j)
        if j > 0:
            m = got["motion"][np.isfinite(ft["depth"])]
            assert np.abs(m).max() < 0.5, np.abs(m).max()
    surf = np.isfinite(ft["depth"])
    share = float((got["history"][surf] >= 3).mean())
    print("cornell_box 64x64: %d surface pixels, %.1f %% with history >= 3, mean history %.2f" % (
        surf.sum(), 100 * share, got["history"][surf].mean()))
    assert surf.sum() > 2000 and share >= 0.5


@pytest.mark.gpu
def test_render_parity_through_a_medium(host):
    """lit_smoke with NEE: the smoke's scattering events have zero normals, which pass the normal test and reproject"""
    nx, ny = 64, 48
    _, world = scenes_extra.build(host, "lit_smoke", nx, ny, seed=1)
    sc = host.lower(world).upload(0, nee=True)
    t, want_t = Temporal(nx, ny), ref.Temporal(nx, ny)
    for j in range(3):
        cam = _moving_camera(host, nx, ny, j)
        noisy, ft = _frame(sc, cam, nx, ny, 4, SEED + j, nee=True)
        got = _raw_push(t, cam, noisy["linear"], ft["albedo"], ft["normal"], ft["depth"], noisy["stderr"])
        want = want_t.push(cam, noisy["linear"], ft["albedo"], ft["normal"], ft["depth"], stderr=noisy["stderr"])
        _assert_same(got, want, ft["depth"], "lit_smoke frame %d" % j)
    # A zero normal passes the normal test, so what can reject a medium pixel is its depth: the mean of 4 scattering
    # distances spread over the smoke's ~165 units at ~1000 from the camera differs between two frames by about 3.4 %
    # (one sigma) against the 5 % tolerance, so one tap is accepted about 6 times in 7 and a pixel has up to four.
    medium = np.isfinite(ft["depth"]) & ~ft["normal"].any(axis=2)
    share = float((got["history"][medium] >= 2).mean())
    print("lit_smoke: %d pixels with a zero normal, %.1f %% reprojected, mean history %.2f" % (
        medium.sum(), 100 * share, got["history"][medium].mean()))
    assert medium.sum() > 20 and share > 0.5


# ---- 2. a standing camera ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_standing_camera_accumulates_the_mean(host):
    nx = ny = 64
    K = 8
    cam, world = scenes.build(host, "cornell_box", nx, ny, seed=1)
    sc = host.lower(world).upload(0)
    frames = [_frame(sc, cam, nx, ny, 4, SEED + j) for j in range(K)]
    ft = frames[0][1]
    surf = np.isfinite(ft["depth"])
    runs = []
    for _ in range(2):
        t = Temporal(nx, ny)
        for noisy, _ in frames:  # the features of one frame throughout: a standing camera's features differ only by noise
            out = t.push(cam, noisy["linear"], ft["albedo"], ft["normal"], ft["depth"], stderr=noisy["stderr"], motion=True)
        t.close()
        runs.append(out)
    out = runs[0]
    assert all(runs[0][k].tobytes() == runs[1][k].tobytes() for k in ("linear", "stderr", "history", "motion"))
    assert np.all(out["history"][surf] == K) and np.all(out["history"][~surf] == 0) and not out["motion"].any()
    a = np.fmax(ft["albedo"], F(1e-3)).astype(np.float64)
    xs = np.stack([n["linear"].astype(np.float64) / a for n, _ in frames])
    es = np.stack([n["stderr"].astype(np.float64) / a for n, _ in frames])
    s3 = np.broadcast_to(surf[..., None], xs[0].shape)
    scale_x, scale_e = np.abs(xs).max(axis=0), es.max(axis=0)
    live = s3 & (scale_x > 0)
    err_x = np.abs(out["linear"].astype(np.float64) / a - xs.mean(axis=0))[live] / scale_x[live]
    live_e = s3 & (scale_e > 0)
    err_e = np.abs(out["stderr"].astype(np.float64) / a - np.sqrt((es * es).sum(axis=0)) / K)[live_e] / scale_e[live_e]
    print("8 frames: mean within %.3g, stderr within %.3g of the largest frame value (bound %.3g)" % (
        err_x.max(), err_e.max(), ref.mean_bound(K)))
    assert err_x.max() <= ref.mean_bound(K) and err_e.max() <= ref.mean_bound(K)
    assert np.all(out["linear"][s3 & (scale_x == 0)] == 0)


# ---- 3. it leaves its neighbours alone --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_render_is_unchanged_by_pushes_and_handles_are_independent(host):
    cam, world = scenes.build(host, "cornell_smoke", 64, 48, seed=1)
    sc = host.lower(world).upload(0)
    before = sc.render(cam, 64, 48, 8, seed=SEED, flags=FC)
    nx, ny = 37, 23
    cams = _cameras("translate", nx, ny, 4)
    _, alb, nrm, dep, _ = _synthetic(nx, ny)
    frames = [_synthetic(nx, ny, seed=20 + j) for j in range(4)]
    a, b, alone = Temporal(nx, ny), Temporal(nx, ny, max_history=2), Temporal(nx, ny)
    for j in range(4):  # a and b interleaved, b one frame behind and with other settings
        oa = a.push(cams[j], frames[j][0], alb, nrm, dep, stderr=frames[j][4], motion=True)
        if j > 0:
            b.push(cams[j - 1], frames[j - 1][0], alb, nrm, dep, motion=True)
        oo = alone.push(cams[j], frames[j][0], alb, nrm, dep, stderr=frames[j][4], motion=True)
        assert all(oa[k].tobytes() == oo[k].tobytes() for k in ("linear", "stderr", "history", "motion"))
    after = sc.render(cam, 64, 48, 8, seed=SEED, flags=FC)
    assert before["linear"].tobytes() == after["linear"].tobytes() and before["rgb8"].tobytes() == after["rgb8"].tobytes()
    host.free_all()  # closes the open handles
    assert a.h is None and b.h is None and alone.h is None
    with pytest.raises(Exception, match="closed"):
        a.push(cams[0], frames[0][0], alb, nrm, dep)


@pytest.mark.gpu
def test_render_temporal_is_its_four_calls(host):
    nx, ny = 64, 48
    _, world = scenes.build(host, "cornell_box", nx, ny, seed=1)
    sc = host.lower(world).upload(0)
    t, mine = Temporal(nx, ny), Temporal(nx, ny)
    for j in range(3):
        cam = _moving_camera(host, nx, ny, j)
        opts = dict(iterations=4, sigma_l=2.0)
        got = sc.render_temporal(t, cam, nx, ny, 4, denoise=opts if j < 2 else False, seed=SEED + j, flags=FC)
        noisy, ft = _frame(sc, cam, nx, ny, 4, SEED + j)
        acc = mine.push(cam, noisy["linear"], ft["albedo"], ft["normal"], ft["depth"], stderr=noisy["stderr"])
        want = denoise(acc["linear"], ft["albedo"], ft["normal"], ft["depth"], stderr=acc["stderr"],
                       **(opts if j < 2 else dict(iterations=0)))
        assert got["linear"].tobytes() == want["linear"].tobytes() and got["rgb8"].tobytes() == want["rgb8"].tobytes()
        assert all(got["accumulated"][k].tobytes() == acc[k].tobytes() for k in ("linear", "stderr", "history"))
        assert got["noisy"]["linear"].tobytes() == noisy["linear"].tobytes()
        assert got["features"]["depth"].tobytes() == ft["depth"].tobytes()
    assert got["linear"].tobytes() == acc["linear"].tobytes()  # denoise=False: the accumulated image itself
    with pytest.raises(ValueError):
        sc.render_temporal(t, cam, nx, ny, 1)


# ---- 4. quality -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_temporal_and_atrous_beat_atrous_alone_on_a_moving_camera(host):
    """cornell_box 128x128, eight frames of 4 spp, look_from.x + 2 per frame; truth = 4096 spp from the last camera.
    Measured on an MI355X: noisy 0.2900, a-trous alone 0.1833, temporal + a-trous 0.0861, ratio 0.469."""
    nx = ny = 128
    _, world = scenes.build(host, "cornell_box", nx, ny, seed=1)
    sc = host.lower(world).upload(0)
    t = Temporal(nx, ny)
    for j in range(8):
        cam = _moving_camera(host, nx, ny, j)
        got = sc.render_temporal(t, cam, nx, ny, 4, seed=SEED + j, flags=FC)
    truth = sc.render(cam, nx, ny, 4096, seed=7, flags=FC)["linear"]
    alone = sc.render_denoised(cam, nx, ny, 4, seed=SEED + 7, flags=FC)
    assert alone["noisy"]["linear"].tobytes() == got["noisy"]["linear"].tobytes()  # the same last frame
    r_t, r_a, r_n = (display_rmse(x, truth) for x in (got["linear"], alone["linear"], got["noisy"]["linear"]))
    print("cornell_box 128x128, 8 x 4 spp: noisy RMSE %.5f, a-trous alone %.5f, temporal + a-trous %.5f, ratio %.3f; "
          "accumulated before the filter %.5f" % (r_n, r_a, r_t, r_t / r_a, display_rmse(got["accumulated"]["linear"], truth)))
    assert r_t < r_a, (r_t, r_a)


# ---- 5. the refusals that need a handle -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_with_a_live_handle():
    nx, ny = 5, 3
    cam = ref.pinhole((0.0, 0.0, 0.0), (0.0, 0.0, -10.0), aspect=nx / ny)
    lin, alb, nrm, dep, se = _synthetic(nx, ny)
    lib = abi.load_rtmi()
    t = Temporal(nx, ny)
    first = t.push(cam, lin, alb, nrm, dep, stderr=se)
    with pytest.raises(Exception, match="stderr_rgb must be supplied"):
        t.push(cam, lin, alb, nrm, dep)
    again = t.push(cam, lin, alb, nrm, dep, stderr=se)  # the refused push left the history as it was
    surf = np.isfinite(dep)
    assert np.all(again["history"][surf] == 2) and np.all(first["history"][surf] == 1)
    singular = ref.pinhole((0.0, 0.0, 0.0), (0.0, 0.0, -10.0))
    singular.vertical = singular.horizontal
    with pytest.raises(Exception, match="singular"):
        t.push(singular, lin, alb, nrm, dep, stderr=se)
    assert np.all(t.push(cam, lin, alb, nrm, dep, stderr=se)["history"][surf] == 3)
    t.reset()
    assert t.push(cam, lin, alb, nrm, dep)["stderr"] is None  # after a reset the choice is open again
    with pytest.raises(Exception, match="stderr_rgb must be supplied"):
        t.push(cam, lin, alb, nrm, dep, stderr=se)
    with pytest.raises(ValueError):
        t.push(cam, lin[:, :4], alb, nrm, dep)
    with pytest.raises(ValueError):
        t.push(cam, lin.astype(np.float64), alb, nrm, dep)
    t.close()
    t.close()  # twice is allowed
    with pytest.raises(Exception, match="closed"):
        t.reset()
    # what destroy leaves a caller with: NULL
    out = np.zeros_like(lin)
    rc = lib.rtmi_temporal_push(None, C.byref(cam), lin.ctypes.data, alb.ctypes.data, nrm.ctypes.data, dep.ctypes.data, None,
                                out.ctypes.data, None, None, None)
    assert rc == 1 and b"NULL handle" in lib.rtmi_last_error()
    h = C.c_void_p()
    p = abi.TemporalParams(32, 0.0, 0.05, 0.9, 1e-3, 0)
    assert lib.rtmi_temporal_create(lib.rtmi_device_count(), nx, ny, C.byref(p), C.byref(h)) == 3 and h.value is None
    assert b"device index out of range" in lib.rtmi_last_error()
