"""Guided upscaling on the device (include/rtmi_upscale.h).

1. the kernel against the numpy restatement (tests/upscale_ref.py), every bit of linear, rgb8 and cls, on the synthetic inputs
   that tests/test_upscale_ref.py shows to reach all four classes at every size; each output alone; sentinels behind every
   plane;
2. the device form: torch tensors on the current stream and on another, a misaligned view, no allocation;
3. the handle against the composition it stands for, every bit: Scene.frame at the low size, render_features at the full
   size, upscale();
4. the one statistical test: the guided reconstruction is nearer a converged full-resolution render than blind bilinear
   interpolation of the same low image."""
import ctypes as C

import numpy as np
import pytest

import upscale_ref as ref
from raytracing_rust_amd import Tonemap, abi, env_from_sky, scenes, upscale

FC = abi.RTMI_FLAG_FAST_CULL
F = np.float32
SENTINEL = 0x7FC0BEEF  # a NaN pattern no output holds
TAIL = 64
CORNELL = ((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), 40.0, 2.0)
SPHERES = ((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 20.0, 0.05)
NAMES = ("linear_lo", "albedo_lo", "normal_lo", "depth_lo", "albedo", "normal", "depth")
_REF = {}


def _want(size, variant):
    """The restatement's planes of one synthetic case, computed once."""
    if (size, variant) not in _REF:
        planes, params = ref.synthetic(size, variant)
        _REF[size, variant] = (planes, params, ref.upscale(**planes, **params))
    return _REF[size, variant]


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        diff = got.view(np.uint8).reshape(-1) != want.view(np.uint8).reshape(-1)
        raise AssertionError("%s: %d of %d bytes differ" % (what, diff.sum(), diff.size))


def _params(params):
    f = dict(ref.DEFAULTS, **params)
    return abi.UpscaleParams(f["normal_power"], f["sigma_z"], f["eps_z"], f["albedo_min"], f["w_min"], 0)


def _raw(planes, params, outputs=("linear", "rgb8", "cls")):
    """rtmi_upscale through ctypes, each output plane followed by TAIL sentinel words: dict of the planes asked for."""
    (ly, lx), (ny, nx) = planes["depth_lo"].shape, planes["depth"].shape
    words = {"linear": ny * nx * 3, "rgb8": (ny * nx * 3 + 3) // 4, "cls": (ny * nx + 3) // 4}
    buf = {n: np.full(words[n] + TAIL, SENTINEL, np.uint32) for n in outputs}
    i = abi.UpscaleIn(*[planes[n].ctypes.data for n in NAMES])
    o = abi.UpscaleOut(*[buf[n].ctypes.data if n in buf else None for n in ("linear", "rgb8", "cls")])
    p = _params(params)
    lib = abi.load_rtmi()
    rc = lib.rtmi_upscale(0, lx, ly, nx, ny, C.byref(p), C.byref(i), C.byref(o))
    assert rc == 0, lib.rtmi_last_error()
    out = {}
    for n, b in buf.items():
        raw = b.view(np.uint8)
        size = {"linear": ny * nx * 12, "rgb8": ny * nx * 3, "cls": ny * nx}[n]
        assert (raw[size:] == np.full(words[n] + TAIL, SENTINEL, np.uint32).view(np.uint8)[size:]).all(), "%s: written past its end" % n
        out[n] = raw[:size].view(F).reshape(ny, nx, 3) if n == "linear" else raw[:size].reshape((ny, nx, 3) if n == "rgb8" else (ny, nx))
    return out


# ---- 1. the kernel against the restatement ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["default", "direct", "staged"])
@pytest.mark.parametrize("size", ref.SIZES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_kernel_is_the_restatement(size, kernel, monkeypatch):
    """Both variants of the kernel (the taps gathered from global memory, or staged in LDS per workgroup;
    RTMI_UPSCALE_VARIANT picks one, and a footprint too large for LDS, as at a ratio of 1, goes to the direct one) and
    whichever is the default."""
    if kernel == "default":
        monkeypatch.delenv("RTMI_UPSCALE_VARIANT", raising=False)
    else:
        monkeypatch.setenv("RTMI_UPSCALE_VARIANT", kernel)
    seen = set()
    for variant in range(4):
        planes, params, want = _want(size, variant)
        got = _raw(planes, params)
        for n in ("cls", "linear", "rgb8"):
            _same(got[n], want[n], "%r variant %d %s, %s" % (size, variant, kernel, n))
        seen |= set(np.unique(got["cls"]).tolist())
    assert seen == {0, 1, 2, 3}


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["direct", "staged"])
def test_kernel_variants_beyond_one_tile(kernel, monkeypatch):
    """260x9 -> 520x18 and 173x7 -> 259x10: more than one 256 x 4 tile of the staged variant in both directions, a last
    tile three pixels wide, nx a multiple of four and not."""
    monkeypatch.setenv("RTMI_UPSCALE_VARIANT", kernel)
    for size in ((260, 9, 520, 18), (173, 7, 259, 10)):
        for variant in (0, 3):
            planes, params, want = _want(size, variant)
            got = _raw(planes, params)
            for n in ("cls", "linear", "rgb8"):
                _same(got[n], want[n], "%r variant %d %s, %s" % (size, variant, kernel, n))


@pytest.mark.gpu
def test_each_output_alone_and_the_python_face():
    size = (19, 12, 37, 23)
    planes, params, want = _want(size, 0)
    for only in ("linear", "rgb8", "cls"):
        got = _raw(planes, params, outputs=(only,))
        assert list(got) == [only]
        _same(got[only], want[only], "%s alone" % only)
    got = upscale(*[planes[n] for n in NAMES], **params)
    assert sorted(got) == ["cls", "linear", "rgb8"]
    for n in got:
        _same(got[n], want[n], "upscale(), %s" % n)


# ---- 2. the device form -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_form_on_torch_tensors():
    import torch

    dev = torch.device("cuda", 0)
    size = (65, 34, 130, 67)
    lx, ly, nx, ny = size
    lib = abi.load_rtmi()
    cases = [_want(size, v) for v in (0, 3)]
    side = torch.cuda.Stream(dev)
    free_before = None
    for call in range(5):
        planes, params, want = cases[call % 2]
        if call == 2:
            free_before = torch.cuda.mem_get_info(dev)[0]
        t = [torch.from_numpy(planes[n]).to(dev) for n in NAMES]
        if call in (1, 3):  # on another stream than the current one's default
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                got = upscale(*t, **params)
            side.synchronize()
        else:
            got = upscale(*t, **params)
            torch.cuda.current_stream(dev).synchronize()
        for n in ("cls", "linear", "rgb8"):
            assert got[n].device == dev
            _same(got[n].cpu().numpy(), want[n], "device form call %d, %s" % (call, n))
        del t, got
    # torch's caching allocator serves the tensors of calls 2 to 4 from what calls 0 and 1 returned to it
    free_after = torch.cuda.mem_get_info(dev)[0]
    assert free_before == free_after, "the device form allocated: %d bytes free before call 2, %d after call 4" % (free_before, free_after)

    # the raw entry: sentinels behind each plane, and a misaligned view is refused before anything is written
    planes, params, want = cases[0]
    t = {n: torch.from_numpy(planes[n]).to(dev) for n in NAMES}
    words = {"linear": ny * nx * 3, "rgb8": (ny * nx * 3 + 3) // 4, "cls": (ny * nx + 3) // 4}
    buf = {n: torch.full((words[n] + TAIL,), SENTINEL, dtype=torch.int32, device=dev) for n in words}
    p = _params(params)
    i = abi.UpscaleIn(*[t[n].data_ptr() for n in NAMES])
    o = abi.UpscaleOut(*[buf[n].data_ptr() for n in ("linear", "rgb8", "cls")])
    stream = torch.cuda.current_stream(dev)
    off = torch.zeros(ny * nx + 4, dtype=torch.float32, device=dev)[1:1 + ny * nx]  # a view 4 bytes off a 16-byte boundary
    off.copy_(t["depth"].reshape(-1))
    bad = abi.UpscaleIn(*[off.data_ptr() if n == "depth" else t[n].data_ptr() for n in NAMES])
    assert off.data_ptr() % 16 == 4
    rc = lib.rtmi_upscale_device(0, lx, ly, nx, ny, C.byref(p), C.byref(bad), C.byref(o), stream.cuda_stream)
    assert rc == 1 and lib.rtmi_last_error().startswith(b"rtmi_upscale_device: misaligned")
    stream.synchronize()
    assert all((b == SENTINEL).all().item() for b in buf.values())
    rc = lib.rtmi_upscale_device(0, lx, ly, nx, ny, C.byref(p), C.byref(i), C.byref(o), stream.cuda_stream)
    assert rc == 0, lib.rtmi_last_error()
    stream.synchronize()
    sentinel = np.full(max(words.values()) + TAIL, SENTINEL, np.uint32).view(np.uint8)
    for n, size_b in (("linear", ny * nx * 12), ("rgb8", ny * nx * 3), ("cls", ny * nx)):
        raw = buf[n].cpu().numpy().view(np.uint8)
        assert (raw[size_b:] == sentinel[size_b:raw.size]).all(), "%s: written past its end" % n
        assert raw[:size_b].tobytes() == want[n].tobytes(), n
    for only in ("linear", "rgb8", "cls"):  # each output alone: the kernel's uniform branch on each pointer
        for b in buf.values():
            b.fill_(SENTINEL)
        one = abi.UpscaleOut(*[buf[n].data_ptr() if n == only else None for n in ("linear", "rgb8", "cls")])
        rc = lib.rtmi_upscale_device(0, lx, ly, nx, ny, C.byref(p), C.byref(i), C.byref(one), stream.cuda_stream)
        assert rc == 0, lib.rtmi_last_error()
        stream.synchronize()
        for n, size_b in (("linear", ny * nx * 12), ("rgb8", ny * nx * 3), ("cls", ny * nx)):
            raw = buf[n].cpu().numpy().view(np.uint8)
            if n == only:
                assert raw[:size_b].tobytes() == want[n].tobytes() and (raw[size_b:] == sentinel[size_b:raw.size]).all(), n
            else:
                assert (raw == sentinel[:raw.size]).all(), "%s written when only %s was asked for" % (n, only)
    with pytest.raises(ValueError, match="device"):
        upscale(*[t[n] if n != "depth" else t[n].cpu() for n in NAMES])
    with pytest.raises(ValueError, match="contiguous"):
        upscale(*[t[n] if n != "albedo" else torch.zeros((ny, nx, 6), device=dev)[:, :, ::2] for n in NAMES])


# ---- 3. the handle against the composition ------------------------------------------------------------------------------------
def _scene(host, name, nx, ny, env=False, nee=False):
    _, world = scenes.build(host, name, nx, ny, seed=1)
    sc = host.lower(world).upload(0, nee=nee)
    if env:
        sc.attach_env(env_from_sky(64, 32))
    return sc


def _camera(host, nx, ny, j, path=CORNELL):
    look_from, look_at, vfov, step = path
    return scenes.set_camera(host, nx, ny, (look_from[0] + step * j,) + look_from[1:], look_at, vertical_fov=vfov)


def _composition(sc, frame, cam, low, full, ns, seed, guide_ns, up, feature_kw):
    """What one Upscaler.render stands for: the low frame, the full-resolution features, upscale()."""
    lo = frame.render(cam, ns, seed=seed, aux=True)
    ft = sc.render_features(cam, full[0], full[1], guide_ns, seed=seed, **feature_kw)
    out = upscale(lo["linear"], lo["features"]["albedo"], lo["features"]["normal"], lo["features"]["depth"], ft["albedo"], ft["normal"],
                  ft["depth"], **up)
    out["guide"] = {n: ft[n] for n in ("albedo", "normal", "depth")}
    out["low"] = {"linear": lo["linear"], "albedo": lo["features"]["albedo"], "normal": lo["features"]["normal"],
                  "depth": lo["features"]["depth"]}
    return out


def _compare(got, want, what):
    for n in ("cls", "linear", "rgb8"):
        _same(got[n], want[n], "%s, %s" % (what, n))
    for group in ("guide", "low"):
        for n in want[group]:
            _same(got[group][n], want[group][n], "%s, %s.%s" % (what, group, n))


def _bytes(out):
    return b"".join(out[n].tobytes() for n in ("linear", "rgb8", "cls")) + b"".join(
        out[g][n].tobytes() for g in ("guide", "low") for n in sorted(out[g]))


def _sequence(host, name, low, full, estimator, frames=4, path=CORNELL, guide_ns=4, up=None, **kw):
    nee, env = estimator in ("nee", "env_nee"), estimator in ("env", "env_nee")
    sc = _scene(host, name, full[0], full[1], env=env, nee=nee)
    frame = sc.frame(low[0], low[1], estimator=estimator, flags=FC, **kw)
    ups = sc.upscaler(full[0], full[1], low=low, guide_ns=guide_ns, estimator=estimator, upscale=up, flags=FC, **kw)
    assert (ups.lx, ups.ly, ups.nx, ups.ny) == low + full
    last = None
    for k in range(frames):
        cam = _camera(host, full[0], full[1], k, path)
        want = _composition(sc, frame, cam, low, full, 4, k, guide_ns, up or {}, dict(flags=FC))
        last = ups.render(cam, 4, seed=k, aux=True)
        _compare(last, want, "%s %s frame %d" % (name, estimator, k))
    return sc, ups, last


@pytest.mark.gpu
def test_cornell_box_sequence(host):
    _, _, last = _sequence(host, "cornell_box", (32, 32), (64, 64), "nee")
    counts = np.bincount(last["cls"].reshape(-1), minlength=4)
    print("cornell_box 32x32 -> 64x64, classes 0..3:", counts.tolist())
    assert counts.sum() == 64 * 64 and counts[1] > 0 and len(counts) == 4


@pytest.mark.gpu
def test_cornell_box_odd_sizes_under_the_cooperative_flag(host):
    """37 x 23 = 851 pixels: not a multiple of four, so the scene's guide planes are not 16-byte aligned and the kernel reads
    them dword by dword; and the tail."""
    _, _, last = _sequence(host, "cornell_box", (25, 16), (37, 23), "nee", coop=True)
    assert last["stats"]["kernel"] == abi.RTMI_KERNEL_WAVE_COOP


@pytest.mark.gpu
def test_sequence_under_a_map(host):
    _, _, last = _sequence(host, "random_spheres", (24, 16), (48, 32), "env_nee", path=SPHERES)
    assert (last["cls"] == 0).any() and (last["cls"] == 1).any()  # the map is seen directly somewhere


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(temporal=None), dict(denoise=False)], ids=["no-history", "no-filter"])
def test_options_of_the_low_frame(host, kw):
    _sequence(host, "cornell_box", (32, 32), (64, 64), "nee", frames=3, guide_ns=2,
              up=dict(normal_power=8, sigma_z=0.1, w_min=0.01), **kw)


@pytest.mark.gpu
def test_reset_torch_and_tonemap(host):
    import torch

    low, full = (32, 32), (64, 64)
    sc = _scene(host, "cornell_box", 64, 64, nee=True)
    cams = [_camera(host, 64, 64, k) for k in range(4)]
    with sc.upscaler(64, 64, scale=2.0, estimator="nee", flags=FC) as ups:
        assert (ups.lx, ups.ly) == low
        first = [ups.render(cams[k], 4, seed=k, aux=True) for k in range(4)]
        assert first[0]["linear"].tobytes() != first[3]["linear"].tobytes()
        ups.reset()
        again = [ups.render(cams[k], 4, seed=k, aux=True) for k in range(4)]
        assert [_bytes(a) for a in again] == [_bytes(a) for a in first]
        ups.reset()
        for k in range(4):  # the device form: tensors on the scene's device with the numpy form's bits
            t = ups.render(cams[k], 4, seed=k, aux=True, out="torch")
            assert t["linear"].device == torch.device("cuda", sc.device) and t["low"]["depth"].is_cuda and t["guide"]["albedo"].is_cuda
            host_side = {n: t[n].cpu().numpy() for n in ("linear", "rgb8", "cls")}
            host_side.update({g: {n: a.cpu().numpy() for n, a in t[g].items()} for g in ("guide", "low")})
            assert _bytes(host_side) == _bytes(first[k]), "torch frame %d" % k
        assert sorted(ups.render(cams[0], 4, seed=3)) == ["cls", "linear", "rgb8", "stats"]  # aux=False: the image only
        assert sorted(ups.render(cams[0], 4, seed=4, out="torch")) == ["cls", "linear", "rgb8", "stats"]
        with pytest.raises(ValueError):
            ups.render(cams[0], 4, out="cupy")
        # tonemap= is Tonemap.apply afterwards, in both forms
        ups.reset()
        with Tonemap(64, 64, op="reinhard", white=4.0) as tm, Tonemap(64, 64, op="reinhard", white=4.0) as tm2:
            for k, out in ((0, "numpy"), (1, "torch")):
                got = ups.render(cams[k], 4, seed=k, out=out, tonemap=tm, dt=0.1)
                lin = got["linear"] if out == "numpy" else got["linear"].cpu().numpy()
                _same(lin, first[k]["linear"], "tonemap frame %d, linear" % k)
                want = tm2.apply(first[k]["linear"], dt=0.1)
                rgb = got["rgb8"] if out == "numpy" else got["rgb8"].cpu().numpy()
                _same(rgb, want["rgb8"], "tonemap frame %d, rgb8" % k)
                assert got["exposure"] == want["exposure"]
            with Tonemap(32, 32) as small, pytest.raises(ValueError, match="full size"):
                ups.render(cams[0], 4, tonemap=small)
    assert ups.h is None  # the context manager closed it


@pytest.mark.gpu
def test_neighbours_memory_and_closing(host):
    import torch

    low, full = (32, 24), (64, 48)
    sc = _scene(host, "cornell_box", 64, 48, nee=True)
    cams = [_camera(host, 64, 48, k) for k in range(5)]
    before = (sc.render_nee(cams[0], 64, 48, 8, seed=5, flags=FC), sc.render_features(cams[0], 64, 48, 4, seed=5, flags=FC))
    alone = sc.upscaler(64, 48, low=low, estimator="nee", flags=FC)
    want = [alone.render(cams[k], 4, seed=k, aux=True) for k in range(5)]
    alone.close()
    ups = sc.upscaler(64, 48, low=low, estimator="nee", flags=FC)
    frame = sc.frame(64, 48, estimator="nee", flags=FC)  # a full-size frame on the same scene, rendered in turn
    solo = sc.frame(64, 48, estimator="nee", flags=FC)
    frames_alone = [solo.render(cams[k], 4, seed=k) for k in range(5)]
    solo.close()
    for k in range(5):
        if k == 2:
            free_before = torch.cuda.mem_get_info(sc.device)[0]
        got = ups.render(cams[k], 4, seed=k, aux=True)
        f = frame.render(cams[k], 4, seed=k)
        assert _bytes(got) == _bytes(want[k]), "frame %d beside a Frame" % k
        assert f["linear"].tobytes() == frames_alone[k]["linear"].tobytes() and f["rgb8"].tobytes() == frames_alone[k]["rgb8"].tobytes()
    free_after = torch.cuda.mem_get_info(sc.device)[0]
    assert free_before == free_after, "a render call allocated: %d bytes free before frame 2, %d after frame 4" % (free_before, free_after)
    after = (sc.render_nee(cams[0], 64, 48, 8, seed=5, flags=FC), sc.render_features(cams[0], 64, 48, 4, seed=5, flags=FC))
    for n in ("linear", "rgb8", "stderr"):
        assert before[0][n].tobytes() == after[0][n].tobytes(), n
    for n in ("albedo", "normal", "depth", "hits"):
        assert before[1][n].tobytes() == after[1][n].tobytes(), n
    second = sc.upscaler(64, 48, scale=1.5, estimator="nee", flags=FC)
    assert (second.lx, second.ly) == (43, 32)
    second.render(cams[0], 4)
    second.close()
    with pytest.raises(Exception, match="closed"):
        second.render(cams[0], 4)
    host.free_all()  # closes the open upscaler and frame before their scene
    assert ups.h is None and frame.h is None
    with pytest.raises(Exception, match="closed"):
        ups.render(cams[0], 4)


@pytest.mark.gpu
def test_refusals_with_a_scene(host):
    nx, ny = 16, 16
    _, world = scenes.build(host, "cornell_box", nx, ny, seed=1)
    sc = host.lower(world).upload(0)
    p = abi.RenderParams()
    p.nx, p.ny, p.ns, p.max_depth, p.t_min, p.flags, p.tile_world = nx, ny, 1, 50, 0.001, FC, 1
    t = abi.TemporalParams(32, 0.0, 0.05, 0.9, 1e-3, 0)
    d = abi.DenoiseParams(5, 128, 4.0, 1.0, 1e-10, 1e-3, 1e-3, 0)

    def create(estimator):
        o = abi.UpscalerOpts(abi.FrameOpts(estimator, 0.5, t, d, 0), abi.UpscaleParams(32, 0.05, 1e-3, 1e-3, 1e-3, 0), 8, 8, 4)
        h = host.lib.rth_upscaler_create(sc.h, C.byref(p), C.byref(o))
        return h, (host.lib.rth_last_error() or b"").decode()

    for estimator, word in ((1, "no light table attached"), (2, "no environment map attached"), (3, "no environment map attached")):
        h, msg = create(estimator)
        assert not h and "rtmi_upscaler_create: " in msg and word in msg and "rtmi_frame" not in msg, msg
    h, _ = create(0)
    assert h and host.lib.rth_upscaler_close(h) == 0
    with pytest.raises(ValueError, match="estimator"):
        sc.upscaler(nx, ny, estimator="roulette")
    with pytest.raises(ValueError, match="coop"):
        sc.upscaler(nx, ny, coop=True)
    with pytest.raises(ValueError, match="scale"):
        sc.upscaler(nx, ny, scale=0.5)
    with pytest.raises(TypeError):
        sc.upscaler(nx, ny, upscale=dict(iterations=3))  # a filter keyword is not a reconstruction keyword
    with pytest.raises(Exception, match="sizes"):
        sc.upscaler(nx, ny, low=(17, 8))
    with pytest.raises(Exception, match="guide_ns"):
        sc.upscaler(nx, ny, guide_ns=0)
    with pytest.raises(Exception, match="normal_power"):
        sc.upscaler(nx, ny, upscale=dict(normal_power=5))
    ups = sc.upscaler(nx, ny, flags=FC)
    with pytest.raises(Exception, match="rtmi_upscaler_render: ns must be at least 2"):
        ups.render(_camera(host, nx, ny, 0), 1)
    ups.render(_camera(host, nx, ny, 0), 2)  # a refused call leaves the handle usable


# ---- 4. quality -----------------------------------------------------------------------------------------------------------
def _rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


# r = rmse_guided / rmse_bilinear measured on an MI355X (the renders are deterministic: no run-to-run variation), DESIGN.md §30
R_MEASURED = {"cornell_box": 0.8498, "random_spheres": 0.9790}


@pytest.mark.gpu
@pytest.mark.parametrize("name,low,full,path,estimator,flags", [("cornell_box", (32, 32), (64, 64), CORNELL, "nee", FC),
                                                               ("random_spheres", (48, 32), (96, 64), SPHERES, "plain", FC | abi.RTMI_FLAG_SKY)])
def test_guided_beats_bilinear(host, name, low, full, path, estimator, flags):
    """The reference is render_nee at the full size and 4096 spp (an existing entry; on random_spheres, which has no lamp, it
    is the plain render under the sky).  The low frame has 256 spp, no history and no filter, so that the reconstruction is
    what is compared: r = RMSE(guided) / RMSE(bilinear of the same low image, same taps, no guide) must be below 1, and no
    more than half-way from the measured value to 1 (the margin rule of DESIGN.md §25)."""
    sc = _scene(host, name, full[0], full[1], nee=estimator == "nee")
    cam = _camera(host, full[0], full[1], 0, path)
    truth = sc.render_nee(cam, full[0], full[1], 4096, seed=99, flags=flags)["linear"]
    with sc.upscaler(full[0], full[1], low=low, estimator=estimator, temporal=None, denoise=False, flags=flags) as ups:
        out = ups.render(cam, 256, seed=1, aux=True)
    blind = ref.bilinear(out["low"]["linear"], full[1], full[0])
    guided, plain = _rmse(out["linear"], truth), _rmse(blind, truth)
    r = guided / plain
    print("%s: rmse guided %.6f, bilinear %.6f, r = %.4f, classes %s" % (name, guided, plain, r,
                                                                        np.bincount(out["cls"].reshape(-1), minlength=4).tolist()))
    assert r < 1.0
    assert r <= (1.0 + R_MEASURED[name]) / 2
