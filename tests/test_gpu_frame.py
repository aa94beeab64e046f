"""The frame pipeline (include/rtmi_frame.h) on the device.  Its yardstick is the chain it replaces:
Scene.render_temporal (and render_denoised) over host planes.

* the un-tiling kernel is bit for bit the numpy restatement (tests/frame_ref.py), writes nothing past its planes and counts
  the poisoned texels of the image, not of the padding;
* every plane of every frame of a camera path has the bits of render_temporal's, for every estimator, under the
  cooperative flag, through a medium, under a map, with parameters off their defaults, without the filter and without
  the history;
* a standing camera, reset, the torch form, two frames on one scene, the neighbours, a changing ns, stable memory;
* the refusals that need a live handle."""
import ctypes as C

import numpy as np
import pytest

import frame_ref as ref
import scenes_extra
from raytracing_rust_amd import Temporal, abi, env_from_sky, scenes

FC = abi.RTMI_FLAG_FAST_CULL
F = np.float32
SENTINEL = 0x7FC0BEEF  # a NaN pattern the inputs do not hold
TAIL = 64
CORNELL = ((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), 40.0, 2.0)
SPHERES = ((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 20.0, 0.05)
GROUPS = (("noisy", ("linear", "stderr")), ("features", ("albedo", "normal", "depth", "hits")),
          ("accumulated", ("linear", "stderr", "history", "motion")))


# ---- 1. the probe -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny", [(1, 1), (1, 17), (8, 8), (37, 23), (130, 67)])
def test_untile_probe_is_the_restatement(nx, ny):
    lib = abi.load_rtmi()
    rng = np.random.default_rng(1000 * nx + ny)
    ntex, n = ref.texel_count(nx, ny), nx * ny
    tex = np.zeros((ntex, 4), np.uint32)
    tex[:, :3] = rng.standard_normal((ntex, 3)).astype(F).view(np.uint32)  # finite floats
    tex[:, 3] = rng.integers(0, 1 << 24, ntex, dtype=np.uint32)
    se = rng.random((ntex, 3)).astype(F)

    def probe(tex, with_se=True, want_lin=True):
        lin, ose = (np.full(n * 3 + TAIL, SENTINEL, np.uint32) for _ in range(2))
        count = C.c_uint32(12345)
        rc = lib.rtmi_probe_frame_untile(0, nx, ny, tex.ctypes.data, se.ctypes.data if with_se else None,
                                         lin.ctypes.data if want_lin else None, ose.ctypes.data if with_se else None, C.byref(count))
        assert rc == 0, lib.rtmi_last_error()
        for buf, written in ((lin, want_lin), (ose, with_se)):
            assert np.all(buf[n * 3:] == SENTINEL), "written past its end"
            assert np.all(buf[:n * 3] == SENTINEL) != written
        return lin[:n * 3], ose[:n * 3], count.value

    want_lin, want_se, _ = ref.untile(nx, ny, tex, se)
    lin, ose, count = probe(tex)
    assert lin.tobytes() == want_lin.tobytes() and ose.tobytes() == want_se.tobytes() and count == 0
    assert probe(tex, with_se=False)[0].tobytes() == want_lin.tobytes()  # each plane is optional
    assert probe(tex, want_lin=False)[1].tobytes() == want_se.tobytes()
    # poisoned texels: counted inside the image, never in the padding of the edge tiles
    pad = ref.padding_texels(nx, ny)
    poisoned = tex.copy()
    poisoned[pad, 3] |= ref.POISON
    poisoned[pad, :3] = 0x7FC00000
    lin, ose, count = probe(poisoned)
    assert count == 0 and lin.tobytes() == want_lin.tobytes() and ose.tobytes() == want_se.tobytes()
    inside = ref.tiled_index(nx, ny)
    hit = {int(inside[0, 0]), int(inside[ny - 1, nx - 1]), int(inside[ny // 2, nx // 3])}
    poisoned[sorted(hit), 3] |= ref.POISON
    lin, _, count = probe(poisoned)
    assert count == len(hit) == ref.untile(nx, ny, poisoned)[2]
    assert lin.tobytes() == want_lin.tobytes()  # the colour words are copied whatever the mark says


# ---- 2. the sequence --------------------------------------------------------------------------------------------------------
def _scene(host, name, nx, ny, env=False, nee=False):
    build = scenes_extra.build if name.startswith("lit_") else scenes.build
    _, world = build(host, name, nx, ny, seed=1)
    sc = host.lower(world).upload(0, nee=nee)
    if env:
        sc.attach_env(env_from_sky(64, 32))
    return sc


def _camera(host, nx, ny, j, path=CORNELL):
    look_from, look_at, vfov, step = path
    return scenes.set_camera(host, nx, ny, (look_from[0] + step * j,) + look_from[1:], look_at, vertical_fov=vfov)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        diff = got.view(np.uint8).reshape(-1) != want.view(np.uint8).reshape(-1)
        raise AssertionError("%s: %d of %d bytes differ" % (what, diff.sum(), diff.size))


class _Chain:
    """render_temporal over host planes (the yardstick), with a second history pushed alongside for the motion plane,
    which render_temporal does not return; temporal=None: render_denoised."""

    def __init__(self, sc, nx, ny, temporal=(), **opts):
        self.sc, self.nx, self.ny, self.opts = sc, nx, ny, opts
        self.t = None if temporal is None else (Temporal(nx, ny, **dict(temporal)), Temporal(nx, ny, **dict(temporal)))

    def render(self, cam, ns, seed):
        if self.t is None:  # render_denoised has no denoise=False: the filter with 0 iterations is what it means
            opts = dict(self.opts, denoise=dict(iterations=0)) if self.opts.get("denoise") is False else self.opts
            return self.sc.render_denoised(cam, self.nx, self.ny, ns, seed=seed, flags=FC, **opts)
        out = self.sc.render_temporal(self.t[0], cam, self.nx, self.ny, ns, seed=seed, flags=FC, **self.opts)
        ft, noisy = out["features"], out["noisy"]
        again = self.t[1].push(cam, noisy["linear"], ft["albedo"], ft["normal"], ft["depth"], stderr=noisy["stderr"], motion=True)
        assert all(again[k].tobytes() == out["accumulated"][k].tobytes() for k in ("linear", "stderr", "history"))
        out["accumulated"] = again
        return out


def _compare(got, want, what, temporal=True):
    for name in ("linear", "rgb8"):
        _same(got[name], want[name], "%s, %s" % (what, name))
    for group, names in GROUPS:
        if group == "accumulated" and not temporal:
            assert group not in got
            continue
        for name in names:
            _same(got[group][name], want[group][name], "%s, %s.%s" % (what, group, name))


def _sequence(host, name, nx, ny, estimator, frames, path=CORNELL, temporal=(), denoise=(), coop=False):
    nee, env = estimator in ("nee", "env_nee"), estimator in ("env", "env_nee")
    sc = _scene(host, name, nx, ny, env=env, nee=nee)
    chain = _Chain(sc, nx, ny, temporal=temporal, denoise=False if denoise is False else dict(denoise), nee=nee, env=env,
                   **(dict(coop=True) if coop else {}))
    frame = sc.frame(nx, ny, estimator=estimator, temporal=temporal, denoise=denoise, coop=coop, flags=FC)
    last = None
    for k in range(frames):
        cam = _camera(host, nx, ny, k, path)
        got = frame.render(cam, 4, seed=k, aux=True)
        want = chain.render(cam, 4, k)
        _compare(got, want, "%s %s frame %d" % (name, estimator, k), temporal is not None)
        last = got
    if coop:
        assert last["stats"]["kernel"] == abi.RTMI_KERNEL_WAVE_COOP
    return last


@pytest.mark.gpu
@pytest.mark.parametrize("estimator", ["plain", "nee"])
def test_cornell_box_sequence(host, estimator):
    """the sequence of test_gpu_temporal.py: 64x64, six frames, look_from.x + 2 per frame"""
    last = _sequence(host, "cornell_box", 64, 64, estimator, 6)
    surf = np.isfinite(last["features"]["depth"])
    hist = last["accumulated"]["history"]
    assert surf.sum() > 2000 and (hist[surf] >= 3).mean() >= 0.5 and np.all(hist[~surf] == 0)
    assert np.abs(last["accumulated"]["motion"]).max() < 0.5 and last["accumulated"]["motion"].any()


@pytest.mark.gpu
def test_cornell_box_odd_size_under_the_cooperative_flag(host):
    _sequence(host, "cornell_box", 37, 23, "nee", 3, coop=True)


@pytest.mark.gpu
def test_sequence_through_a_medium(host):
    """lit_smoke: the smoke's scattering events have zero normals, which must reproject"""
    last = _sequence(host, "lit_smoke", 64, 48, "nee", 3)
    medium = np.isfinite(last["features"]["depth"]) & ~last["features"]["normal"].any(axis=2)
    assert medium.sum() > 20 and (last["accumulated"]["history"][medium] >= 2).mean() > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("estimator", ["env", "env_nee"])
def test_sequence_under_a_map(host, estimator):
    last = _sequence(host, "random_spheres", 48, 32, estimator, 3, path=SPHERES)
    assert not np.isfinite(last["features"]["depth"]).all()  # the map is seen directly somewhere


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(temporal=dict(max_history=3, alpha_min=0.1, depth_tol=0.02, normal_min=0.5, albedo_min=0.02)),
                                dict(temporal=dict(demodulate=False)),
                                dict(denoise=dict(iterations=3, normal_power=32, sigma_l=2.0, sigma_z=0.5, albedo_min=0.01)),
                                dict(denoise=dict(iterations=0)),
                                dict(denoise=False),
                                dict(temporal=None),
                                dict(temporal=None, denoise=False)])
def test_options_off_their_defaults(host, kw):
    last = _sequence(host, "cornell_box", 37, 23, "nee", 3, **kw)
    if kw.get("denoise") is False and kw.get("temporal", ()) is not None:
        assert last["linear"].tobytes() == last["accumulated"]["linear"].tobytes()
    if kw.get("denoise") is False and kw.get("temporal", ()) is None:
        assert last["linear"].tobytes() == last["noisy"]["linear"].tobytes()


# ---- 3. the handle ----------------------------------------------------------------------------------------------------------
PLAIN_PLANES = ("linear", "rgb8")


def _bytes(out):
    return b"".join(out[n].tobytes() for n in PLAIN_PLANES) + b"".join(out[g][n].tobytes() for g, names in GROUPS for n in names)


@pytest.mark.gpu
def test_standing_camera_reaches_full_history(host):
    """A standing camera with seeds 0..7 reaches history == 8 on every surface pixel.

    The view is cornell_box's back wall alone: from (278, 278, -800) towards (278, 450, 555) with a 4 degree field, the
    image spans 48 units about that point at a distance of 1366, so it stays 55 units below the ceiling, 120 above the tall
    box and inside the side walls, and the lens (radius 0.05, focus 10) blurs by 7 units at that distance.  Every sample
    of every frame then hits the one plane: the depth of a pixel differs between two frames by the lens jitter (far below
    the 5 % tolerance) and every normal is the wall's, so under the same-camera rule no tap can be rejected and each of
    the eight frames adds one to every pixel's history.  The view is chosen because the property cannot hold on an image
    with silhouettes: a frame renders its own features, as render_temporal does, and the mean depth and normal of an edge
    pixel's four samples change with the seed, so the push rejects its history there.  On the whole box (the camera of
    test_cornell_box_sequence, standing) an MI355X gave 2886 of 3251 surface pixels (88.77 %) with history == 8, the
    least 1, the mean 7.41, bit for bit what render_temporal gives: that run is kept below as a comparison with the
    yardstick, with its figures printed."""
    nx = ny = 64
    sc = _scene(host, "cornell_box", nx, ny)
    wall = scenes.set_camera(host, nx, ny, (278.0, 278.0, -800.0), (278.0, 450.0, 555.0), vertical_fov=4.0)
    with sc.frame(nx, ny, flags=FC) as frame:
        for k in range(8):
            got = frame.render(wall, 4, seed=k, aux=True)
            assert np.all(got["accumulated"]["history"] == k + 1), "frame %d" % k
    surf = np.isfinite(got["features"]["depth"])
    assert surf.all() and np.all(got["features"]["hits"] == 4) and got["linear"].any()
    assert np.all(got["accumulated"]["history"][surf] == 8) and not got["accumulated"]["motion"].any()
    # the whole box: the history is the yardstick's on every pixel, and full wherever no silhouette crosses the pixel
    cam = _camera(host, nx, ny, 0)
    chain = _Chain(sc, nx, ny)
    with sc.frame(nx, ny, flags=FC) as frame:
        for k in range(8):
            got = frame.render(cam, 4, seed=k, aux=True)
            _compare(got, chain.render(cam, 4, k), "standing camera, frame %d" % k)
    surf = np.isfinite(got["features"]["depth"])
    hist = got["accumulated"]["history"]
    print("standing camera on the whole box, 8 frames of 4 spp, seeds 0..7: %d surface pixels, %d with history == 8 (%.2f %%), "
          "least %g, mean %.3f" % (surf.sum(), (hist[surf] == 8).sum(), 100.0 * (hist[surf] == 8).mean(), hist[surf].min(),
                                   hist[surf].mean()))
    assert not got["accumulated"]["motion"].any() and np.all(hist[~surf] == 0) and surf.sum() > 2000 and hist.max() == 8


@pytest.mark.gpu
def test_reset_and_torch(host):
    import torch

    nx = ny = 64
    sc = _scene(host, "cornell_box", nx, ny)
    cam = _camera(host, nx, ny, 0)
    with sc.frame(nx, ny, flags=FC) as frame:
        first = [frame.render(cam if k < 2 else _camera(host, nx, ny, k), 4, seed=k, aux=True) for k in range(4)]
        assert first[-1]["accumulated"]["history"].max() > 3.5  # four frames deep (a resampled length is not an integer)
        frame.reset()
        again = [frame.render(cam if k < 2 else _camera(host, nx, ny, k), 4, seed=k, aux=True) for k in range(4)]
        assert [_bytes(a) for a in again] == [_bytes(a) for a in first]
        frame.reset()
        for k in range(3):  # the device form: tensors on the scene's device with the numpy form's bits
            t = frame.render(cam if k < 2 else _camera(host, nx, ny, k), 4, seed=k, aux=True, out="torch")
            for name in PLAIN_PLANES:
                assert t[name].device == torch.device("cuda", sc.device)
                _same(t[name].cpu().numpy(), first[k][name], "torch frame %d, %s" % (k, name))
            for group, names in GROUPS:
                for name in names:
                    assert t[group][name].is_cuda
                    _same(t[group][name].cpu().numpy(), first[k][group][name], "torch frame %d, %s.%s" % (k, group, name))
        assert sorted(frame.render(cam, 4, seed=3)) == ["linear", "rgb8", "stats"]  # aux=False: the image only
        assert sorted(frame.render(cam, 4, seed=4, out="torch")) == ["linear", "rgb8", "stats"]
        with pytest.raises(ValueError):
            frame.render(cam, 4, out="cupy")
    assert frame.h is None  # the context manager closed it


@pytest.mark.gpu
def test_two_frames_on_one_scene_and_the_neighbours(host):
    nx, ny = 64, 48
    sc = _scene(host, "cornell_box", nx, ny, nee=True)
    cams = [_camera(host, nx, ny, k) for k in range(4)]
    t = Temporal(nx, ny)
    before = (sc.render(cams[0], nx, ny, 8, seed=5, flags=FC), sc.render_nee(cams[0], nx, ny, 8, seed=5, flags=FC),
              sc.render_temporal(t, cams[0], nx, ny, 4, seed=5, flags=FC))
    t.reset()
    a = sc.frame(nx, ny, estimator="nee", flags=FC)
    b = sc.frame(nx, ny, estimator="plain", temporal=dict(max_history=2), denoise=dict(iterations=2), flags=FC)
    alone = sc.frame(nx, ny, estimator="nee", flags=FC)
    want = [alone.render(cams[k], 4, seed=k, aux=True) for k in range(4)]
    alone.close()
    for k in range(4):  # a and b in turn, b one frame behind and with other settings
        got = a.render(cams[k], 4, seed=k, aux=True)
        if k > 0:
            b.render(cams[k - 1], 4, seed=k - 1)
        assert _bytes(got) == _bytes(want[k])
    after = (sc.render(cams[0], nx, ny, 8, seed=5, flags=FC), sc.render_nee(cams[0], nx, ny, 8, seed=5, flags=FC),
             sc.render_temporal(t, cams[0], nx, ny, 4, seed=5, flags=FC))
    for x, y in zip(before, after):
        assert x["linear"].tobytes() == y["linear"].tobytes() and x["rgb8"].tobytes() == y["rgb8"].tobytes()
    assert before[1]["stderr"].tobytes() == after[1]["stderr"].tobytes()
    assert all(before[2]["accumulated"][n].tobytes() == after[2]["accumulated"][n].tobytes() for n in ("linear", "stderr", "history"))
    host.free_all()  # closes the open frames before their scene
    assert a.h is None and b.h is None
    with pytest.raises(Exception, match="closed"):
        a.render(cams[0], 4)


@pytest.mark.gpu
def test_ns_may_change_and_memory_is_stable(host):
    import torch

    nx, ny = 64, 48
    sc = _scene(host, "cornell_box", nx, ny, nee=True)
    chain = _Chain(sc, nx, ny, nee=True)
    frame = sc.frame(nx, ny, estimator="nee", flags=FC)
    for k, ns in enumerate((4, 9, 2, 4)):  # the yardstick's scratch grows first, so it does not disturb the count below
        cam = _camera(host, nx, ny, k)
        want = chain.render(cam, ns, k)
        _compare(frame.render(cam, ns, seed=k, aux=True), want, "ns = %d" % ns)
    frame.reset()
    outs = []
    for k in range(5):
        if k == 2:
            free_before = torch.cuda.mem_get_info(sc.device)[0]
        outs.append(frame.render(_camera(host, nx, ny, k), 4, seed=k, aux=True))
    free_after = torch.cuda.mem_get_info(sc.device)[0]
    assert free_before == free_after, "a frame call allocated: %d bytes free before frame 2, %d after frame 4" % (free_before, free_after)


# ---- 4. the refusals that need a handle -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_with_a_scene(host):
    nx, ny = 16, 16
    _, world = scenes.build(host, "cornell_box", nx, ny, seed=1)
    sc = host.lower(world).upload(0)
    cam = _camera(host, nx, ny, 0)
    lib, hlib = abi.load_rtmi(), host.lib
    p = abi.RenderParams()
    p.nx, p.ny, p.ns, p.max_depth, p.t_min, p.flags, p.tile_world = nx, ny, 1, 50, 0.001, FC, 1
    t = abi.TemporalParams(32, 0.0, 0.05, 0.9, 1e-3, 0)
    d = abi.DenoiseParams(5, 128, 4.0, 1.0, 1e-10, 1e-3, 1e-3, 0)

    def create(estimator):
        h = hlib.rth_frame_create(sc.h, C.byref(p), C.byref(abi.FrameOpts(estimator, 0.5, t, d, 0)))
        return h, (hlib.rth_last_error() or b"").decode()

    # what the estimator needs attached, in begin_call's words, with the entry's name
    for estimator, word in ((1, "no light table attached (rtmi_scene_attach_lights)"),
                            (2, "no environment map attached (rtmi_scene_attach_env)"),
                            (3, "no environment map attached (rtmi_scene_attach_env)")):
        h, msg = create(estimator)
        assert not h and "rtmi_frame_create: " in msg and word in msg, msg
    sc.attach_env(env_from_sky(16, 8))
    h, msg = create(3)
    assert not h and "no light table attached" in msg, msg
    h, _ = create(2)
    assert h and hlib.rth_frame_close(h) == 0
    # the Python face
    with pytest.raises(ValueError, match="estimator"):
        sc.frame(nx, ny, estimator="roulette")
    with pytest.raises(ValueError, match="coop"):
        sc.frame(nx, ny, coop=True)
    with pytest.raises(TypeError):
        sc.frame(nx, ny, temporal=dict(iterations=3))  # a filter keyword is not a history keyword
    with pytest.raises(Exception, match="max_history"):
        sc.frame(nx, ny, temporal=dict(max_history=0))
    with pytest.raises(Exception, match="frames accept the flags"):
        sc.frame(nx, ny, flags=FC | abi.RTMI_FLAG_PATH_SIG)
    # a map detached under a live frame: the call is refused and the history stays
    frame = sc.frame(nx, ny, estimator="env", flags=FC)
    first = frame.render(cam, 4, seed=0, aux=True)
    saved = env_from_sky(16, 8)
    sc.detach_env()
    with pytest.raises(Exception, match="rtmi_frame_render: no environment map attached"):
        frame.render(cam, 4, seed=1)
    sc.attach_env(saved)
    second = frame.render(cam, 4, seed=1, aux=True)
    with sc.frame(nx, ny, estimator="env", flags=FC) as fresh:  # the same two frames without the refused call between them
        assert _bytes(fresh.render(cam, 4, seed=0, aux=True)) == _bytes(first)
        assert _bytes(fresh.render(cam, 4, seed=1, aux=True)) == _bytes(second)
    surf = np.isfinite(first["features"]["depth"])
    assert surf.any() and np.all(first["accumulated"]["history"][surf] == 1) and second["accumulated"]["history"].max() == 2
    with pytest.raises(Exception, match="ns must be at least 2"):
        frame.render(cam, 1)
    frame.close()
    frame.close()  # twice is allowed
    with pytest.raises(Exception, match="closed"):
        frame.render(cam, 4)
    with pytest.raises(Exception, match="closed"):
        frame.reset()
    # what destroy leaves a caller with: NULL
    c = cam.lower()
    o = abi.FrameOut()
    assert lib.rtmi_frame_render(None, C.byref(c), 4, 0, C.byref(o), None) == 1 and b"NULL handle" in lib.rtmi_last_error()
