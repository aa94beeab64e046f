"""The tone mapper (include/rtmi_tonemap.h) on the device, bit for bit against tests/tonemap_ref.py.

* the metering kernel's bins are numpy's, at sizes that take the tail, several workgroups and a second trip of the
  grid-stride loop;
* every plane and every word of the state of an apply equal the restatement, for every operator, transfer function and
  exposure mode, with each output optional and nothing written past a plane;
* sequences on one handle: adaptation up and down, black frames, reset, two handles in turn;
* the identity setting is the project's own quantiser, on rendered images;
* the device form on torch tensors and streams, its refusal of a misaligned tensor, and that it allocates nothing;
* Frame.render(tonemap=...) is Frame.render followed by Tonemap.apply;
* the refusals that need a live handle."""
import ctypes as C
import itertools

import numpy as np
import pytest

import tonemap_ref as ref
from raytracing_rust_amd import HostError, Tonemap, abi, denoise, env_from_sky, scenes, tonemap

FC = abi.RTMI_FLAG_FAST_CULL
F = np.float32
SENTINEL = 0x7FC0BEEF  # a NaN pattern the outputs do not hold
TAIL = 64  # sentinel words behind each plane
METER_CAP, METER_BLOCK, METER_PIXELS = 256, 1024, 4  # kMeterCap, kMeterBlock and the pixels per lane of rtmi_tonemap.hip
SIZES = [(1, 1), (1, 17), (8, 8), (37, 23), (130, 67)]
SECOND_TRIP = (1031, 1019)  # more pixels than one trip of the capped meter grid covers
assert SECOND_TRIP[0] * SECOND_TRIP[1] > METER_CAP * METER_BLOCK * METER_PIXELS
APPLY_SIZES = [(1, 1), (37, 23), (130, 67)]  # pixel counts that are no multiple of four: the tail runs
assert all((nx * ny) % 4 for nx, ny in APPLY_SIZES)


def _kw(p):
    """Tonemap's keywords of the restatement's keywords."""
    p = dict(ref.DEFAULTS, **p)
    kw = dict(op=p["op"], oetf=p["oetf"], exposure=p["exposure"], ev=p["ev"], white=p["white"], key=p["key"],
              log2_range=(p["log2_min"], p["log2_max"]), percentiles=(p["p_low"], p["p_high"]), speed=(p["speed_up"], p["speed_down"]))
    if p["adapt_min"] is not None:
        kw["adapt_range"] = (p["adapt_min"], p["adapt_max"])
    return kw


def _params(p):
    from raytracing_rust_amd.host import _tonemap_params

    return _tonemap_params(**_kw(p))


# ---- 1. the probe -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny", SIZES + [SECOND_TRIP])
def test_probe_histogram_is_the_restatement(nx, ny):
    lib = abi.load_rtmi()
    img = ref.sample_image(ny, nx, 1000 * nx + ny)  # 2^-30 .. 2^30, zeros, negatives, NaN, +-inf, denormals, bin edges
    for p in (dict(), dict(log2_min=-3.0, log2_max=5.0), dict(log2_min=-40.0, log2_max=40.0, exposure="manual")):
        bins = np.full(256 + TAIL, SENTINEL, np.uint32)
        rc = lib.rtmi_probe_tonemap_histogram(0, nx, ny, C.byref(_params(p)), img.ctypes.data, bins.ctypes.data)
        assert rc == 0, lib.rtmi_last_error()
        want = ref.histogram(img, ref.params(**p))
        assert (bins[256:] == SENTINEL).all()
        assert (bins[:256] == want).all(), (p, np.flatnonzero(bins[:256] != want))
        if nx * ny > 100 and not p:
            assert 0 < want.sum() < nx * ny and want[0] > 0 and want[255] > 0 and np.count_nonzero(want) > 100


# ---- 2. one apply -----------------------------------------------------------------------------------------------------------
def _host_apply(tm, img, dt=0.0, rgb8=True, display=True, state=True):
    """rtmi_tonemap_apply with sentinel words behind each plane -> (rgb8 or None, display or None, state words or None)."""
    n = img.shape[0] * img.shape[1] * 3
    o_rgb = np.full(n + 4 * TAIL, 0xA5, np.uint8)
    o_dis = np.full(n + TAIL, SENTINEL, np.uint32)
    o_st = np.full(8 + TAIL, SENTINEL, np.uint32)
    rc = tm.lib.rtmi_tonemap_apply(tm.h, img.ctypes.data, dt, o_rgb.ctypes.data if rgb8 else None,
                                   o_dis.ctypes.data if display else None,
                                   C.cast(o_st.ctypes.data, C.POINTER(abi.TonemapState)) if state else None)
    assert rc == 0, tm.lib.rtmi_last_error()
    assert (o_rgb[n:] == 0xA5).all() and (o_dis[n:] == SENTINEL).all() and (o_st[8:] == SENTINEL).all(), "written past its end"
    assert rgb8 or (o_rgb == 0xA5).all()
    assert display or (o_dis == SENTINEL).all()
    assert state or (o_st == SENTINEL).all()
    return (o_rgb[:n].reshape(img.shape) if rgb8 else None, o_dis[:n].reshape(img.shape) if display else None,
            o_st[:8] if state else None)


def _check(got, want, what):
    rgb8, display, words = got
    w_rgb8, w_display, w_state = want
    if words is not None:
        assert (words == ref.state_words(w_state)).all(), (what, words, ref.state_words(w_state), w_state)
    if rgb8 is not None and not (rgb8 == w_rgb8).all():
        raise AssertionError("%s: %d of %d bytes of rgb8 differ" % (what, (rgb8 != w_rgb8).sum(), rgb8.size))
    if display is not None and not (display == w_display.view(np.uint32)).all():
        raise AssertionError("%s: %d of %d words of display differ" % (what, (display != w_display.view(np.uint32)).sum(), display.size))


def _image(ny, nx, seed, scale=1.0):
    """Radiances around `scale` over sixteen stops with the odd pixels of sample_image among them."""
    img = ref.sample_image(ny, nx, seed, lo=-8.0, hi=8.0)
    with np.errstate(all="ignore"):
        return (img * F(scale)).astype(F)


@pytest.mark.gpu
@pytest.mark.parametrize("op,oetf,exposure", list(itertools.product(ref.OPS, ref.OETFS, ref.EXPOSURES)))
def test_apply_is_the_restatement(op, oetf, exposure):
    p = dict(op=op, oetf=oetf, exposure=exposure, ev=0.75, white=3.0 if op == "reinhard" else float("inf"))
    for nx, ny in APPLY_SIZES:
        what = "%s %s %s %dx%d" % (op, oetf, exposure, nx, ny)
        imgs = [_image(ny, nx, 7 * nx + k, 2.0 ** (3 * k - 3)) for k in range(4)]
        with Tonemap(nx, ny, **_kw(p)) as tm:
            want = ref.Tonemap(**p)
            _check(_host_apply(tm, imgs[0]), want.apply(imgs[0]), what)
            # each output alone, on the same handle: the state goes on whichever is asked for
            for k, only in enumerate(("rgb8", "display", "state")):
                got = _host_apply(tm, imgs[k + 1], dt=0.25, **{n: n == only for n in ("rgb8", "display", "state")})
                _check(got, want.apply(imgs[k + 1], dt=0.25), "%s, %s alone" % (what, only))
            got = tm.apply(imgs[0], dt=0.1, display=True)  # the Python face
            w = want.apply(imgs[0], dt=0.1)
            _check((got["rgb8"], got["display"].view(np.uint32), None), w, what + ", python")
            assert got["exposure"]["applies"] == 5 and got["exposure"]["counted"] == w[2]["counted"]
            assert F(got["exposure"]["exposure"]) == w[2]["exposure"]


# ---- 3. sequences -----------------------------------------------------------------------------------------------------------
P_A = dict()
P_B = dict(op="reinhard", oetf="gamma2", white=8.0, ev=-1.0, key=0.25, log2_min=-6.0, log2_max=10.0, p_low=0.0, p_high=1.0,
           speed_up=0.5, speed_down=20.0, adapt_min=-2.0, adapt_max=3.0)


def _sequence(ny, nx):
    base = _image(ny, nx, 99)
    black = np.zeros_like(base)
    up, down = _image(ny, nx, 98, 16.0), _image(ny, nx, 97, 1 / 16.0)
    return [(black, 0.0), (base, 1 / 60), (up, 10.0), (black, 1 / 60), (base, 0.0), (down, 10.0)]


def _run(tm, seq):
    return [_host_apply(tm, img, dt) for img, dt in seq]


@pytest.mark.gpu
def test_sequences_adapt_reset_and_do_not_mix():
    nx, ny = 37, 23
    seq = _sequence(ny, nx)
    want = {}
    for name, p in (("a", P_A), ("b", P_B)):
        r = ref.Tonemap(**p)
        want[name] = [r.apply(img, dt) for img, dt in seq]
    st = [w[2] for w in want["a"]]
    assert [s["counted"] == 0 for s in st] == [True, False, False, True, False, False]
    assert st[1]["adapted_log2"] == st[1]["metered_log2"]  # adopted after the black first frame
    assert st[1]["adapted_log2"] < st[2]["adapted_log2"] <= st[2]["metered_log2"]  # up, dt = 10
    assert st[3]["adapted_log2"] == st[2]["adapted_log2"] == st[4]["adapted_log2"]  # black, then dt = 0
    assert st[5]["metered_log2"] < st[5]["adapted_log2"] < st[4]["adapted_log2"]  # down
    with Tonemap(nx, ny, **_kw(P_A)) as a, Tonemap(nx, ny, **_kw(P_B)) as b:
        first = _run(a, seq)
        for k, (got, w) in enumerate(zip(first, want["a"])):
            _check(got, w, "step %d" % k)  # a step equals the restatement only over bins the step before left zero
        a.reset()
        again = _run(a, seq)
        for k, (g0, g1) in enumerate(zip(first, again)):
            assert all((x == y).all() for x, y in zip(g0, g1)), "reset, step %d" % k
        # two handles in turn equal each handle alone
        a.reset()
        for k, (img, dt) in enumerate(seq):
            _check(_host_apply(a, img, dt), want["a"][k], "a in turn, step %d" % k)
            _check(_host_apply(b, img, dt), want["b"][k], "b in turn, step %d" % k)
        # a metered first frame, and a reset in the middle of a sequence
        a.reset()
        r = ref.Tonemap(**P_A)
        for img, dt in seq[1:3]:
            _check(_host_apply(a, img, dt), r.apply(img, dt), "metered first frame")
        a.reset(), r.reset()
        _check(_host_apply(a, seq[5][0], 1.0), r.apply(seq[5][0], 1.0), "after a reset")


# ---- 4. the project's own yardstick -----------------------------------------------------------------------------------------
IDENTITY = dict(exposure="manual", ev=0.0, op="clamp", oetf="gamma2")


def _cornell(host, nx, ny, nee=True):
    cam, world = scenes.build(host, "cornell_box", nx, ny, seed=1)
    return cam, host.lower(world).upload(0, nee=nee)


@pytest.mark.gpu
def test_the_identity_setting_is_the_projects_quantiser(host):
    nx = ny = 64
    cam, sc = _cornell(host, nx, ny)
    img = sc.render(cam, nx, ny, 8, flags=FC)
    zeros = np.zeros((ny, nx, 3), F)
    dn = denoise(img["linear"], zeros, zeros, np.zeros((ny, nx), F), iterations=0)
    got = tonemap(img["linear"], **IDENTITY)
    assert (got["rgb8"] == dn["rgb8"]).all() and (dn["linear"] == img["linear"]).all()
    assert 50 < len(np.unique(got["rgb8"])) and got["exposure"]["exposure"] == 1.0 and got["exposure"]["applies"] == 1
    # ... and the rgb8 a Frame returned with its linear
    nx, ny = 37, 23
    cam, sc = _cornell(host, nx, ny)
    with sc.frame(nx, ny, estimator="nee", flags=FC) as frame:
        fr = frame.render(cam, 4, seed=3)
    got = tonemap(fr["linear"], **IDENTITY)
    assert (got["rgb8"] == fr["rgb8"]).all() and len(np.unique(got["rgb8"])) > 20


# ---- 5. the device form -----------------------------------------------------------------------------------------------------
def _padded(torch, words, dtype, fill):
    """A tensor of `words` elements followed by sentinel elements, and the view of the elements."""
    t = torch.full((words + 4 * TAIL,), fill, dtype=dtype, device="cuda:0")
    return t, t[:words]


@pytest.mark.gpu
def test_device_form_on_torch_tensors_and_streams():
    import torch

    nx, ny = 37, 23
    n = nx * ny * 3
    seq = _sequence(ny, nx)
    r = ref.Tonemap(**P_A)
    want = [r.apply(img, dt) for img, dt in seq]
    lib = abi.load_rtmi()
    side = torch.cuda.Stream(device=0)
    with Tonemap(nx, ny, **_kw(P_A)) as tm:
        # the Python face: tensors in, tensors out, on the current stream and on a stream of torch's
        for k, (img, dt) in enumerate(seq):
            lin = torch.from_numpy(img).to("cuda:0")
            if k % 2:
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    out = tm.apply(lin, dt=dt, display=True, sync=True)
                torch.cuda.current_stream().wait_stream(side)
            else:
                out = tm.apply(lin, dt=dt, display=True, sync=True)
            assert out["rgb8"].is_cuda and out["display"].dtype == torch.float32 and out["state"].numel() == 32
            words = out["state"].cpu().numpy().view(np.uint32)
            _check((out["rgb8"].cpu().numpy(), out["display"].cpu().numpy().view(np.uint32), words), want[k], "torch, step %d" % k)
            assert out["exposure"]["applies"] == k + 1 and F(out["exposure"]["exposure"]) == want[k][2]["exposure"]
        out = tm.apply(lin, dt=0.0)  # without sync: no decoded dict, no display
        assert "exposure" not in out and "display" not in out and out["state"].numel() == 32
        # the native entry with sentinels behind each plane, each output optional, and no allocation
        tm.reset()
        lins = [torch.from_numpy(img).to("cuda:0") for img, _ in seq]
        bufs = {"rgb8": _padded(torch, n, torch.uint8, 0xA5), "display": _padded(torch, n, torch.int32, SENTINEL),
                "state": _padded(torch, 8, torch.int32, SENTINEL)}
        stream = torch.cuda.current_stream().cuda_stream
        free = None
        for k, (img, dt) in enumerate(seq):
            asked = [("rgb8", "display", "state"), ("rgb8",), ("display",), ("state",), ("rgb8", "state"), ("rgb8", "display", "state")][k]
            for name, (whole, _) in bufs.items():
                whole.fill_(0xA5 if name == "rgb8" else SENTINEL)
            torch.cuda.synchronize()
            if k == 1:
                free = torch.cuda.mem_get_info(0)[0]  # before apply 2
            rc = lib.rtmi_tonemap_apply_device(tm.h, lins[k].data_ptr(), dt, *[bufs[name][1].data_ptr() if name in asked else None
                                                                              for name in ("rgb8", "display", "state")], stream)
            assert rc == 0, lib.rtmi_last_error()
            torch.cuda.synchronize()
            if k == 3:
                assert torch.cuda.mem_get_info(0)[0] == free  # after apply 4
            host = {name: whole.cpu().numpy() for name, (whole, _) in bufs.items()}
            for name, words in (("rgb8", n), ("display", n), ("state", 8)):
                fill = 0xA5 if name == "rgb8" else SENTINEL
                assert (host[name][words:] == fill).all(), "%s written past its end" % name
                assert name in asked or (host[name] == fill).all(), "%s written unasked" % name
            _check((host["rgb8"][:n].reshape(ny, nx, 3) if "rgb8" in asked else None,
                    host["display"][:n].view(np.uint32).reshape(ny, nx, 3) if "display" in asked else None,
                    host["state"][:8].view(np.uint32) if "state" in asked else None), want[k], "native, step %d" % k)
        # a misaligned view is refused by the entry, and the refusal leaves the state as it was
        off = torch.zeros(n + 4, dtype=torch.float32, device="cuda:0")[1:n + 1].view(ny, nx, 3)
        assert off.is_contiguous() and off.data_ptr() % 16 == 4
        with pytest.raises(HostError) as e:
            tm.apply(off)
        assert "(1)" in str(e.value) and "rtmi_tonemap_apply_device" in str(e.value) and "misaligned" in str(e.value)
        for bad in (torch.zeros(ny, nx, 4, device="cuda:0")[:, :, :3], lins[0].double(), lins[0].cpu(), lins[0].permute(1, 0, 2), lins[0][:, :-1].contiguous()):
            with pytest.raises(ValueError):
                tm.apply(bad)
        more = r.apply(seq[1][0], 0.5)
        out = tm.apply(lins[1], dt=0.5, sync=True)
        _check((out["rgb8"].cpu().numpy(), None, out["state"].cpu().numpy().view(np.uint32)), more, "after the refusals")


# ---- 6. Frame.render(tonemap=...) -------------------------------------------------------------------------------------------
def _frames(host, name, nx, ny, estimator, path):
    """Four frames of a moving camera, three ways: frame handles that never saw the keyword, out="numpy" and out="torch"
    with it, against Frame.render followed by Tonemap.apply."""
    _, world = scenes.build(host, name, nx, ny, seed=1)
    sc = host.lower(world).upload(0, nee=estimator in ("nee", "env_nee"))
    if estimator.startswith("env"):
        sc.attach_env(env_from_sky(64, 32))
    look_from, look_at, vfov, step = path
    plain, none, with_np, with_t = (sc.frame(nx, ny, estimator=estimator, flags=FC) for _ in range(4))
    with Tonemap(nx, ny) as after, Tonemap(nx, ny) as tm_np, Tonemap(nx, ny) as tm_t:
        for k in range(4):
            cam = scenes.set_camera(host, nx, ny, (look_from[0] + step * k,) + look_from[1:], look_at, vertical_fov=vfov)
            base = plain.render(cam, 4, seed=k)
            same = none.render(cam, 4, seed=k, tonemap=None)
            assert sorted(same) == sorted(base) == ["linear", "rgb8", "stats"]
            assert all(same[n].tobytes() == base[n].tobytes() for n in ("linear", "rgb8"))
            want = after.apply(base["linear"], dt=1 / 30)
            got = with_np.render(cam, 4, seed=k, tonemap=tm_np, dt=1 / 30)
            assert got["linear"].tobytes() == base["linear"].tobytes()
            assert got["rgb8"].tobytes() == want["rgb8"].tobytes() and got["exposure"] == want["exposure"], k
            got = with_t.render(cam, 4, seed=k, out="torch", tonemap=tm_t, dt=1 / 30)
            assert got["rgb8"].is_cuda and got["linear"].cpu().numpy().tobytes() == base["linear"].tobytes()
            assert got["rgb8"].cpu().numpy().tobytes() == want["rgb8"].tobytes() and got["exposure"] == want["exposure"], k
            assert want["exposure"]["applies"] == k + 1 and want["exposure"]["counted"] > 0
        assert (want["rgb8"] != base["rgb8"]).any()  # the tone-mapped image is another one
    return plain


@pytest.mark.gpu
def test_frame_render_with_a_tonemap_cornell_nee(host):
    nx, ny = 64, 64
    frame = _frames(host, "cornell_box", nx, ny, "nee", ((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), 40.0, 2.0))
    cam, _ = scenes.build(host, "cornell_box", nx, ny, seed=1)
    with Tonemap(32, 64) as other:
        with pytest.raises(ValueError):
            frame.render(cam, 4, tonemap=other)
    with pytest.raises(ValueError):
        frame.render(cam, 4, tonemap="aces")
    import torch

    if torch.cuda.device_count() > 1:
        with Tonemap(nx, ny, device=1) as elsewhere:
            with pytest.raises(ValueError):
                frame.render(cam, 4, tonemap=elsewhere)
    else:
        wrong = Tonemap(nx, ny)
        wrong.device = 1  # a handle that says it lives elsewhere
        with pytest.raises(ValueError):
            frame.render(cam, 4, tonemap=wrong)
        wrong.device = 0
        wrong.close()


@pytest.mark.gpu
def test_frame_render_with_a_tonemap_spheres_under_a_map(host):
    _frames(host, "random_spheres", 48, 32, "env_nee", ((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 20.0, 0.05))


# ---- 7. refusals that need a handle -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_with_a_live_handle(host):
    from raytracing_rust_amd.host import _tonemaps

    nx, ny = 8, 8
    img, nxt = _image(ny, nx, 1), _image(ny, nx, 2, 4.0)
    lib = abi.load_rtmi()
    r = ref.Tonemap()
    tm = Tonemap(nx, ny)
    _check(_host_apply(tm, img), r.apply(img), "first")
    # refused applies leave the next apply's bits unchanged
    st = abi.TonemapState()
    for args, word in (((tm.h, None, 0.0, None, None, C.byref(st)), "NULL linear"),
                       ((tm.h, img.ctypes.data, -1.0, None, None, C.byref(st)), "dt"),
                       ((tm.h, img.ctypes.data, float("nan"), None, None, C.byref(st)), "dt"),
                       ((tm.h, img.ctypes.data, 0.0, None, None, None), "every output"),
                       ((None, img.ctypes.data, 0.0, None, None, C.byref(st)), "handle")):
        assert lib.rtmi_tonemap_apply(*args) == 1 and word in lib.rtmi_last_error().decode(), word
    assert lib.rtmi_tonemap_apply_device(tm.h, img.ctypes.data, 0.0, None, None, None, None) == 1
    assert st.applies == 0
    _check(_host_apply(tm, nxt, 0.5), r.apply(nxt, 0.5), "after the refusals")
    # a closed handle
    tm.close()
    tm.close()  # twice is allowed
    with pytest.raises(HostError):
        tm.apply(img)
    with pytest.raises(HostError):
        tm.reset()
    # Host.free_all() closes what is open
    a, b = Tonemap(nx, ny), Tonemap(nx, ny, exposure="manual")
    assert a in _tonemaps and b in _tonemaps
    host.free_all()
    assert a.h is None and b.h is None and not _tonemaps
    with Tonemap(nx, ny) as c:
        assert c in _tonemaps
    assert c.h is None and c not in _tonemaps
