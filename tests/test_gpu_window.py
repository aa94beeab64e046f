"""Windowed adaptive sampling on the device (include/rtmi_window.h).

1. the spread kernel alone (rtmi_probe_window_spread, rtmi_window_spread_device) against the numpy restatement
   (tests/window_ref.py), every byte, with sentinels behind both planes;
2. the whole render: radius 0 against Scene.render_pixelwise, radii 1 and 2 against the restatement fed with the samples of
   Scene.render_pixels, bit for bit;
3. every pixel against the estimator's fixed render at the pixel's own count; monotone in the radius; the global rule;
4. invariance: pass_spp, FAST_CULL, repetition, the two forms, streams, no allocation, nothing written past an output;
5. the refusals that need a handle.
No inclusion is asserted against the tile-adaptive entry: a sliding window and a fixed 8x8 block are not nested."""
import ctypes as C

import numpy as np
import pytest

import scenes_extra
import window_ref as ref
from raytracing_rust_amd import abi, env_from_sky, scenes, window_spread

FC = abi.RTMI_FLAG_FAST_CULL
SENTINEL = 0x7FC0BEEF  # a NaN pattern no output holds
TAIL = 64
SPHERES = ((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 20.0)
SEED = 0
# name -> (scene, nx, ny, view, estimator, (min_spp, step_spp, cap), factor of the tolerance): the two plain inputs are those of
# tests/test_window_ref.py; NEE and the map start at 4 samples, their tolerance is half the median stderr there, the choice of
# tests/test_gpu_pixelwise.py for the same scenes
CASES = {name: (scene, nx, ny, ref.VIEW, "plain", lattice, factor) for name, (scene, nx, ny, lattice, factor) in ref.PLAIN_INPUTS.items()}
CASES["cornell-nee"] = ("cornell_box", 19, 13, ref.VIEW, "nee", (4, 4, 24), 0.5)
CASES["spheres-env_nee"] = ("random_spheres", 24, 16, SPHERES, "env_nee", (4, 4, 24), 0.5)
PLANES = ("spp", "linear", "rgb8", "stderr")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        diff = _bits(got) != _bits(want)
        raise AssertionError("%s: %d of %d words differ, first at %r" % (what, diff.sum(), diff.size, np.argwhere(diff)[0].tolist()))


# ---- 1. the spread kernel alone ---------------------------------------------------------------------------------------------------
IMAGES = [(1, 1), (1, 70), (70, 1), (63, 5), (64, 5), (65, 5), (129, 3), (257, 19), (200, 40)]  # (nx, ny)
RADII = (0, 1, 2, 7, 16)


def _probe(active, fail, nx, ny, r):
    """rtmi_probe_window_spread on copies with a sentinel tail behind both host planes: active after the call."""
    lib = abi.load_rtmi()
    n = nx * ny
    a, f = np.full(n + TAIL, 0xA5, np.uint8), np.full(n + TAIL, 0x5A, np.uint8)
    a[:n], f[:n] = np.asarray(active).reshape(-1), np.asarray(fail).reshape(-1)
    f0 = f.copy()
    rc = lib.rtmi_probe_window_spread(0, nx, ny, r, a.ctypes.data, f.ctypes.data)
    assert rc == 0, lib.rtmi_last_error()
    assert (a[n:] == 0xA5).all() and (f == f0).all(), "written behind active, or into fail"
    return a[:n]


def _planes(nx, ny):
    """(name, active, fail) of every crafted pair for this image"""
    n = nx * ny
    rng = np.random.default_rng(nx * 1000 + ny)
    ones, zeros = np.ones(n, np.uint8), np.zeros(n, np.uint8)
    yield "all-zero fail", ones, zeros
    yield "all-one fail", ones, ones
    yield "all-zero active", zeros, ones
    spots = {(0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1), (0, ny // 2), (nx - 1, ny // 2), (nx // 2, ny // 2)}
    spots |= {(x, y) for x in (62, 63, 64, 65, 127, 128, 191, 192, 255, 256) if x < nx for y in (0, ny - 1)}  # segment boundaries
    spots |= {(nx // 2, y) for y in (15, 16, 17, 31, 32, 33) if y < ny}  # the boundaries between tiles of rows
    for x, y in sorted(spots):
        f = zeros.copy()
        f[y * nx + x] = 1
        yield "single fail at (%d, %d)" % (x, y), ones, f
    for density in (0.01, 0.5):
        yield "random %g" % density, (rng.random(n) < 0.8).astype(np.uint8), (rng.random(n) < density).astype(np.uint8)
    f = ((rng.random(n) < 0.05) * rng.integers(2, 256, n)).astype(np.uint8)  # 2 .. 255 count as set; 128 and 255 have the sign bit
    f[rng.integers(0, n, 2)] = (128, 255)
    yield "fail bytes other than 0 / 1", ones, f
    yield "active bytes other than 0 / 1", ((rng.random(n) < 0.7) * rng.integers(2, 256, n)).astype(np.uint8), (rng.random(n) < 0.05).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny", IMAGES)
def test_spread_kernel_is_the_restatement(nx, ny):
    for name, a, f in _planes(nx, ny):
        for r in RADII:
            got = _probe(a, f, nx, ny, r)
            want = ref.spread(a, f, nx, ny, r)
            if got.tobytes() != want.tobytes():
                bad = np.flatnonzero(got != want)
                raise AssertionError("%dx%d r %d, %s: %d bytes differ, first at pixel (%d, %d): %d for %d" % (
                    nx, ny, r, name, bad.size, bad[0] % nx, bad[0] // nx, got[bad[0]], want[bad[0]]))
    if nx > 1 and ny > 2:  # no wrap: a fail at a row's end does not reach the next row's start
        f = np.zeros(nx * ny, np.uint8)
        f[1 * nx + nx - 1] = 1
        got = _probe(np.ones(nx * ny, np.uint8), f, nx, ny, 1).reshape(ny, nx)
        assert got[:, 0].sum() == (1 if nx == 2 else 0) * 3 and got[2, 0] == (1 if nx == 2 else 0)


@pytest.mark.gpu
def test_spread_on_device_planes_and_streams():
    import torch

    dev = torch.device("cuda", 0)
    nx, ny = 257, 19
    n = nx * ny
    rng = np.random.default_rng(3)
    a, f = (rng.random(n) < 0.8).astype(np.uint8), (rng.random(n) < 0.02).astype(np.uint8)
    side = torch.cuda.Stream(dev)
    for r in RADII:
        want = ref.spread(a, f, nx, ny, r)
        for stream in (None, side):
            buf_a, buf_f = torch.full((n + TAIL,), 0xA5, dtype=torch.uint8, device=dev), torch.full((n + TAIL,), 0x5A, dtype=torch.uint8, device=dev)
            buf_a[:n], buf_f[:n] = torch.from_numpy(a).to(dev), torch.from_numpy(f).to(dev)
            ta, tf = buf_a[:n].view(ny, nx), buf_f[:n].view(ny, nx)
            if stream is None:
                back = window_spread(ta, tf, r)
                torch.cuda.current_stream(dev).synchronize()
            else:
                stream.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(stream):
                    back = window_spread(ta, tf, r)
                stream.synchronize()
            assert back is ta
            got_a, got_f = buf_a.cpu().numpy(), buf_f.cpu().numpy()
            assert got_a[:n].tobytes() == want.tobytes(), (r, stream is not None)
            assert (got_a[n:] == 0xA5).all() and (got_f[n:] == 0x5A).all() and (got_f[:n] == f).all(), "written behind a plane, or into fail"
        assert window_spread(a.reshape(ny, nx), f.reshape(ny, nx), r).tobytes() == want.tobytes()  # the numpy face of the same call
    with pytest.raises(ValueError, match="radius"):
        window_spread(ta, tf, 17)


# ---- 2. the whole render against the restatement ------------------------------------------------------------------------------
_SAMPLES = {}  # case -> (samples f32 [n, cap, 3], abs_tol): computed once, shared, never changed


def _open(host, case):
    name, nx, ny, view, estimator, _, _ = CASES[case]
    _, world = (scenes.build if name in scenes.SCENES else scenes_extra.build)(host, name, nx, ny, seed=1)
    sc = host.lower(world).upload(0, nee=estimator in ("nee", "env_nee"))
    if estimator in ("env", "env_nee"):
        sc.attach_env(env_from_sky(64, 32))
    cam = scenes.set_camera(host, nx, ny, view[0], view[1], vertical_fov=view[2])  # aperture 0.1: a camera with a lens
    return sc, cam, nx, ny, estimator


def _reference_samples(case, sc, cam, nx, ny, estimator):
    """Every pixel's first cap samples by Scene.render_pixels (their bits are pinned to the renders by tests/test_gpu_sparse.py)
    and the tolerance: the case's factor times the median over pixels of the max-channel stderr at min_spp, from the samples."""
    if case not in _SAMPLES:
        (lo, _, cap), factor = CASES[case][5:]
        x = sc.render_pixels(cam, nx, ny, np.arange(nx * ny, dtype=np.uint32), cap, estimator=estimator, seed=SEED, samples=True, flags=FC)["samples"]
        x.setflags(write=False)
        _SAMPLES[case] = (x, ref.tolerance(x, lo, factor))
    return _SAMPLES[case]


def _windowed(sc, cam, nx, ny, estimator, lattice, abs_tol, r, **kw):
    lo, step, cap = lattice
    kw.setdefault("flags", FC)
    return sc.render_windowed(cam, nx, ny, cap, lo, step, radius=r, abs_tol=abs_tol, estimator=estimator, seed=SEED, **kw)


def _check_against(out, want, what):
    for k in PLANES:
        _same(out[k].reshape(want[k].shape), want[k], "%s: %s" % (what, k))
    _same(out["counts"], want["counts"], what + ": counts")


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_radius_0_is_the_per_pixel_render(host, case):
    sc, cam, nx, ny, estimator = _open(host, case)
    _, abs_tol = _reference_samples(case, sc, cam, nx, ny, estimator)
    lo, step, cap = CASES[case][5]
    want = sc.render_pixelwise(cam, nx, ny, cap, lo, step, abs_tol=abs_tol, estimator=estimator, seed=SEED, flags=FC)
    out = _windowed(sc, cam, nx, ny, estimator, (lo, step, cap), abs_tol, 0)
    for k in PLANES + ("counts",):
        _same(out[k], want[k], "%s radius 0: %s" % (case, k))
    assert out["samples"] == want["samples"]


def _says_something(want):
    return len(np.unique(want["spp"])) >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("case", sorted(CASES))
def test_render_is_the_restatement(host, case, r):
    sc, cam, nx, ny, estimator = _open(host, case)
    x, abs_tol = _reference_samples(case, sc, cam, nx, ny, estimator)
    lo, step, cap = CASES[case][5]
    want = ref.render(x, nx, ny, lo, step, abs_tol=abs_tol, r=r)
    print("%s r %d: abs_tol %.6g, spp histogram %r, counts %r" % (
        case, r, abs_tol, dict(zip(*[a.tolist() for a in np.unique(want["spp"], return_counts=True)])), want["counts"][:, 0].tolist()))
    if not _says_something(want):
        pytest.skip("the restatement stops every pixel of %s at one count under r = %d: the comparison would say nothing" % (case, r))
    out = _windowed(sc, cam, nx, ny, estimator, (lo, step, cap), abs_tol, r)
    _check_against(out, want, "%s r %d" % (case, r))
    per_step = np.diff([0] + ref.lattice(cap, lo, step))
    assert out["samples"] == int(out["spp"].sum()) == int((out["counts"][:, 0].astype(np.int64) * per_step).sum())
    if estimator == "plain":  # the conditions tests/test_window_ref.py checks on the oracle's samples
        assert len(np.unique(out["spp"])) >= 3 and (out["spp"] == lo).any() and (out["spp"] == cap).any()


@pytest.mark.gpu
def test_at_most_one_input_says_nothing(host):
    silent = []
    for case in sorted(CASES):
        sc, cam, nx, ny, estimator = _open(host, case)
        x, abs_tol = _reference_samples(case, sc, cam, nx, ny, estimator)
        lo, step, _ = CASES[case][5]
        if not all(_says_something(ref.render(x, nx, ny, lo, step, abs_tol=abs_tol, r=r)) for r in (1, 2)):
            silent.append(case)
    assert len(silent) <= 1 and not any(c.endswith("plain") for c in silent), silent


# ---- 3. the fixed render, the radius, the global rule -----------------------------------------------------------------------------
def _fixed(sc, cam, nx, ny, estimator, n, flags=FC):
    if estimator == "plain":
        return sc.render_adaptive(cam, nx, ny, n, n, n, seed=SEED, flags=flags)
    if estimator == "nee":
        return sc.render_nee(cam, nx, ny, n, seed=SEED, flags=flags)
    return sc.render_env(cam, nx, ny, n, nee=estimator == "env_nee", seed=SEED, flags=flags)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_every_pixel_is_the_fixed_render_at_its_count_and_the_radius_only_adds(host, case):
    sc, cam, nx, ny, estimator = _open(host, case)
    _, abs_tol = _reference_samples(case, sc, cam, nx, ny, estimator)
    lattice = CASES[case][5]
    outs = {r: _windowed(sc, cam, nx, ny, estimator, lattice, abs_tol, r) for r in (0, 1, 2, 4)}
    print("%s: samples %r" % (case, {r: o["samples"] for r, o in outs.items()}))
    for small, large in ((0, 1), (1, 2), (2, 4)):
        assert (outs[large]["spp"] >= outs[small]["spp"]).all(), (small, large)
    fixed = {}
    for r in (1, 2):
        spp = outs[r]["spp"]
        for n in np.unique(spp).tolist():
            if n not in fixed:
                fixed[n] = _fixed(sc, cam, nx, ny, estimator, n)
            at = spp == n
            for k in ("linear", "rgb8", "stderr"):
                _same(outs[r][k][at], fixed[n][k][at], "%s r %d: %s of the %d pixels with spp = %d" % (case, r, k, int(at.sum()), n))


@pytest.mark.gpu
def test_the_global_rule(host):
    """r = 16 on 16x16 covers the image from every pixel: all stop at the first count at which all pass, or at the cap."""
    case = "smoke-plain"
    sc, cam, nx, ny, estimator = _open(host, case)
    x, abs_tol = _reference_samples(case, sc, cam, nx, ny, estimator)
    lo, step, cap = CASES[case][5]
    assert (nx, ny) == (16, 16)
    for tol in (abs_tol, 1e30):  # with the case's tolerance some pixel fails to the cap; with a huge one all pass at min_spp
        out = _windowed(sc, cam, nx, ny, estimator, (lo, step, cap), tol, 16)
        want = ref.render(x, nx, ny, lo, step, abs_tol=tol, r=16)
        _check_against(out, want, "global rule, abs_tol %g" % tol)
        assert len(np.unique(out["spp"])) == 1 and out["spp"][0, 0] == (cap if tol == abs_tol else lo)
        full = _fixed(sc, cam, nx, ny, estimator, int(out["spp"][0, 0]))
        for k in ("linear", "rgb8", "stderr"):
            _same(out[k], full[k], "global rule: " + k)


# ---- 4. invariance ----------------------------------------------------------------------------------------------------------------
SHORT = (4, 4, 22)  # a shortened last step


@pytest.mark.gpu
def test_result_does_not_depend_on_how_it_ran(host):
    import torch

    case = "cornell-nee"
    sc, cam, nx, ny, estimator = _open(host, case)
    x, abs_tol = _reference_samples(case, sc, cam, nx, ny, estimator)
    want = ref.render(x[:, :22], nx, ny, 4, 4, abs_tol=abs_tol, r=1)
    _check_against(_windowed(sc, cam, nx, ny, estimator, SHORT, abs_tol, 1), want, "the blocking form")
    for pass_spp in (1, 3, 4):  # 4 = step_spp
        _check_against(_windowed(sc, cam, nx, ny, estimator, SHORT, abs_tol, 1, pass_spp=pass_spp), want, "pass_spp %d" % pass_spp)
    _check_against(_windowed(sc, cam, nx, ny, estimator, SHORT, abs_tol, 1, flags=0), want, "without FAST_CULL")
    _check_against(_windowed(sc, cam, nx, ny, estimator, SHORT, abs_tol, 1), want, "a second run")
    # the device form on torch tensors, on the current stream and on another; calls 2 to 4 are served from what calls 0 and 1
    # returned to torch's allocator
    dev = torch.device("cuda", sc.device)
    side = torch.cuda.Stream(dev)
    free_before = None
    for call in range(5):
        if call == 2:
            free_before = torch.cuda.mem_get_info(dev)[0]
        if call in (1, 3):
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                got = _windowed(sc, cam, nx, ny, estimator, SHORT, abs_tol, 1, out="torch", pass_spp=3)
            side.synchronize()
        else:
            got = _windowed(sc, cam, nx, ny, estimator, SHORT, abs_tol, 1, out="torch")
            torch.cuda.current_stream(dev).synchronize()
        assert all(got[k].device == dev for k in PLANES + ("counts",))
        host_of = {k: got[k].cpu().numpy() for k in PLANES + ("counts",)}
        host_of["spp"], host_of["counts"] = host_of["spp"].view(np.uint32), host_of["counts"].view(np.uint32)
        _check_against(host_of, want, "device form, call %d" % call)
        assert got["samples"]() == int(want["spp"].sum())
        del got
    free_after = torch.cuda.mem_get_info(dev)[0]
    assert free_before == free_after, "the device form allocated: %d bytes free before call 2, %d after call 4" % (free_before, free_after)


@pytest.mark.gpu
def test_nothing_is_written_past_an_output(host):
    import torch

    case = "cornell-nee"
    sc, cam, nx, ny, estimator = _open(host, case)
    _, abs_tol = _reference_samples(case, sc, cam, nx, ny, estimator)
    lo, step, cap = SHORT
    want = _windowed(sc, cam, nx, ny, estimator, SHORT, abs_tol, 2)
    dev = torch.device("cuda", sc.device)
    n, steps = nx * ny, 6
    lib = abi.load_rtmi()
    p = abi.RenderParams()
    p.nx, p.ny, p.ns, p.max_depth, p.t_min, p.flags, p.tile_world, p.seed = nx, ny, cap, 50, 0.001, FC, 1, SEED
    o = abi.WindowOpts(lo, step, abi.ROULETTE_ESTIMATORS[estimator], 3, abs_tol, 0.0, 0.5, 2)
    words = {"linear": 3 * n, "rgb8": (3 * n + 3) // 4, "stderr": 3 * n, "spp": n, "counts": 2 * steps}
    nbytes = int(lib.rtmi_window_scratch_bytes(n, 3, steps))
    assert int(lib.rtmi_window_steps(cap, lo, step)) == steps
    stream = torch.cuda.current_stream(dev)
    for which in (("linear", "rgb8", "stderr", "spp", "counts"), ("rgb8",), ("spp", "counts"), ("stderr",)):
        buf = {k: torch.full((words[k] + TAIL,), SENTINEL, dtype=torch.int32, device=dev) for k in which}
        scratch = torch.full((nbytes // 4 + TAIL,), SENTINEL, dtype=torch.int32, device=dev)
        host._check(host.lib.rth_render_window_device(
            sc.h, cam.h, C.byref(p), C.byref(o), *[C.c_void_p(buf[k].data_ptr()) if k in buf else None for k in words],
            C.c_void_p(scratch.data_ptr()), C.c_uint64(nbytes), C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        assert (scratch[nbytes // 4:].cpu().numpy().view(np.uint32) == SENTINEL).all(), "written past the scratch"
        for k in which:
            raw = buf[k].cpu().numpy().view(np.uint32)
            size = 3 * n if k == "rgb8" else 4 * words[k]
            assert raw.view(np.uint8)[:size].tobytes() == want[k].tobytes(), "%r: %s" % (which, k)
            tail = np.full(words[k] + TAIL, SENTINEL, np.uint32).view(np.uint8)[size:]
            assert raw.view(np.uint8)[size:].tobytes() == tail.tobytes(), "%r: written past %s" % (which, k)


# ---- 5. refusals, and the handle afterwards -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_with_a_scene(host):
    _, world = scenes.build(host, "cornell_box", 16, 16, seed=1)
    sc = host.lower(world).upload(0, nee=False)
    cam = scenes.set_camera(host, 16, 16, ref.VIEW[0], ref.VIEW[1], vertical_fov=ref.VIEW[2])
    p = abi.RenderParams()
    p.nx, p.ny, p.ns, p.max_depth, p.t_min, p.flags, p.tile_world = 16, 16, 8, 50, 0.001, FC, 1
    out = np.zeros(16 * 16 * 3, np.float32)
    for estimator, word in ((1, "no light table attached"), (2, "no environment map attached"), (3, "no environment map attached")):
        o = abi.WindowOpts(4, 4, estimator, 0, 0.0, 0.0, 0.5, 1)
        assert host.lib.rth_render_window(sc.h, cam.h, C.byref(p), C.byref(o), out.ctypes.data, None, None, None, None, None) != 0
        msg = (host.lib.rth_last_error() or b"").decode()
        assert "rtmi_render_window: " in msg and word in msg, msg
        o.radius = 17  # the attachment is asked for before the header's own checks
        assert host.lib.rth_render_window(sc.h, cam.h, C.byref(p), C.byref(o), out.ctypes.data, None, None, None, None, None) != 0
        assert word in (host.lib.rth_last_error() or b"").decode()
    assert not out.any()
    for estimator in ("env", "env_nee"):  # the Python face attaches the light table on first use, so it comes after the raw entry
        with pytest.raises(Exception, match="no environment map attached"):
            sc.render_windowed(cam, 16, 16, 8, 4, 4, estimator=estimator, flags=FC)
    with pytest.raises(Exception, match="radius"):
        sc.render_windowed(cam, 16, 16, 8, 4, 4, radius=17, flags=FC)
    for form in ("numpy", "torch"):  # a refused call leaves the handle usable; the default radius is 1
        got = sc.render_windowed(cam, 16, 16, 8, 4, 4, abs_tol=0.01, out=form, flags=FC)
        assert got["linear"].shape == (16, 16, 3)
    host.free_all()
