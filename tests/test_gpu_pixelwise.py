"""Per-pixel adaptive sampling on the device (include/rtmi_pixelwise.h).

1. the step kernel alone (rtmi_probe_pixelwise_step) against the numpy restatement (tests/pixelwise_ref.py),
   every word of the state and of every plane, the untouched ones included;
2. the whole render against the restatement fed with the samples of Scene.render_pixels, bit for bit;
3. every pixel against the estimator's fixed render at the pixel's own count;
4. against the tile-adaptive entry under the same arguments: never more samples in a pixel, fewer in all;
5. invariance: pass_spp, FAST_CULL, repetition, the two forms, streams, no allocation, nothing written past an output;
6. the neighbours keep their bits."""
import ctypes as C

import numpy as np
import pytest

import pixelwise_ref as ref
import scenes_extra
from raytracing_rust_amd import abi, env_from_sky, scenes

FC = abi.RTMI_FLAG_FAST_CULL
SENTINEL = 0x7FC0BEEF  # a NaN pattern no output holds
TAIL = 64
CORNELL = ((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), 40.0)
SPHERES = ((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 20.0)
SEED = 5
CASES = {
    "cornell-plain": ("cornell_box", 13, 13, CORNELL, "plain"),  # square: the box fills the image
    "cornell-nee": ("cornell_box", 19, 13, CORNELL, "nee"),
    "spheres-env": ("random_spheres", 24, 16, SPHERES, "env"),
    "spheres-env_nee": ("random_spheres", 24, 16, SPHERES, "env_nee"),
    "smoke-plain": ("lit_smoke", 16, 16, CORNELL, "plain"),
}
LATTICES = {"cap24": (4, 4, 24), "cap22": (4, 4, 22)}  # (min_spp, step_spp, cap); 22: a shortened last step
# The plain estimator finds the lamp of a closed box by chance.  Measured on an MI355X: on cornell_box 225 of 19x13 pixels
# have a standard error of exactly 0 after 4 samples, 185 after 16 (13x13: 147 and 109 of 169); on lit_smoke 16x16 145 of 256
# after 4 and 40 after 16.  The median, and with it the tolerance, would be 0, every noisy pixel would run to the cap and
# the counts would be two.  So these cases keep the rule and start later: the image size and the lattice are what changes.
LATE = {"cornell-plain": {"cap24": (64, 16, 144), "cap22": (64, 16, 142)},
        "smoke-plain": {"cap24": (16, 4, 36), "cap22": (16, 4, 34)}}
MOST = 144  # samples of the shared reference
PLANES = ("spp", "linear", "rgb8", "stderr")


def _scene(host, name, nx, ny, estimator="plain"):
    _, world = (scenes.build if name in scenes.SCENES else scenes_extra.build)(host, name, nx, ny, seed=1)
    sc = host.lower(world).upload(0, nee=estimator in ("nee", "env_nee"))
    if estimator in ("env", "env_nee"):
        sc.attach_env(env_from_sky(64, 32))
    return sc


def _camera(host, nx, ny, path=CORNELL):
    look_from, look_at, vfov = path
    return scenes.set_camera(host, nx, ny, look_from, look_at, vertical_fov=vfov)  # aperture 0.1: a camera with a lens


def _lattice(case, which):
    return LATE.get(case, LATTICES)[which]


def _open(host, case):
    name, nx, ny, path, estimator = CASES[case]
    return _scene(host, name, nx, ny, estimator), _camera(host, nx, ny, path), nx, ny, estimator


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def _same(got, want, what, nan_equal=False):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        diff = _bits(got) != _bits(want)
        if nan_equal and got.dtype.kind == "f":  # a NaN made by an operation has the sign of the machine that made it
            diff &= ~(np.isnan(got) & np.isnan(want))
        if diff.any():
            raise AssertionError("%s: %d of %d words differ, first at %r" % (what, diff.sum(), diff.size, np.argwhere(diff)[0].tolist()))


# ---- 1. the step kernel alone -----------------------------------------------------------------------------------------------
def _sentinel_planes(n):
    return {"active": np.full(n, 7, np.uint8), "linear": np.full((n, 3), SENTINEL, np.uint32).view(np.float32),
            "rgb8": np.full((n, 3), 0xAB, np.uint8), "stderr": np.full((n, 3), SENTINEL, np.uint32).view(np.float32),
            "spp": np.full(n, SENTINEL, np.uint32)}


def _probe(n_pixels, lst, count, samples, state, n_done, decide, cap, abs_tol, rel_tol, planes):
    """rtmi_probe_pixelwise_step on copies: (state, planes) after the call."""
    lib = abi.load_rtmi()
    lst = np.ascontiguousarray(lst, np.uint32)
    samples = np.ascontiguousarray(samples, np.float32)
    state = np.array(state, np.float64, order="C", copy=True)
    planes = {k: np.array(v, order="C", copy=True) for k, v in planes.items()}
    cnt = None if count is None else np.array([count, 777], np.uint32)
    ptr = {k: planes[k].ctypes.data if k in planes else None for k in ("active", "linear", "rgb8", "stderr", "spp")}
    rc = lib.rtmi_probe_pixelwise_step(0, n_pixels, lst.size, lst.ctypes.data, None if cnt is None else cnt.ctypes.data,
                                       samples.ctypes.data, state.ctypes.data, n_done, samples.shape[1], int(decide), cap, abs_tol, rel_tol,
                                       ptr["active"], ptr["linear"], ptr["rgb8"], ptr["stderr"], ptr["spp"])
    assert rc == 0, lib.rtmi_last_error()
    assert cnt is None or cnt.tolist() == [count, 777]
    return state, planes


def _check_step(what, n_pixels, lst, count, samples, state, n_done, decide, cap, abs_tol, rel_tol, planes, nan_equal=False):
    want_state, want_planes = ref.step(lst, count, samples, state, n_pixels, n_done, decide, cap, abs_tol, rel_tol, planes)
    got_state, got_planes = _probe(n_pixels, lst, count, samples, state, n_done, decide, cap, abs_tol, rel_tol, planes)
    _same(got_state, want_state, what + ": state", nan_equal)
    for k in planes:
        _same(got_planes[k], want_planes[k], "%s: %s" % (what, k), nan_equal)
    return got_state, got_planes


def _crafted(entries, n_pixels, seed):
    rng = np.random.default_rng(seed)
    lst = np.sort(rng.permutation(n_pixels)[:entries]).astype(np.uint32)
    scale = np.float32(10.0) ** rng.integers(-3, 2, (entries, 1, 1)).astype(np.float32)
    return rng, lst, scale


@pytest.mark.gpu
@pytest.mark.parametrize("entries", [1, 63, 64, 65, 257])
def test_step_kernel_is_the_restatement(entries):
    n = entries + 40
    rng, lst, scale = _crafted(entries, n, entries)
    for pass_ in (1, 3, 4, 5, 9):  # the 4-way unroll and its tail
        x = (rng.random((entries, 6 + pass_, 3)).astype(np.float32) * scale).astype(np.float32)
        x[rng.random(entries) < 0.2, :] = 0.25  # zero variance
        blank = np.full((9, n), -7.25)
        tol = 0.05
        # n_done = 0: the state is not read (the sentinel of an unlisted pixel stays), every decide and count form
        for decide in (0, 1):
            what = "entries %d pass %d n_done 0 decide %d" % (entries, pass_, decide)
            planes = _sentinel_planes(n)
            _, got = _check_step(what, n, lst, None, x[:, :pass_], blank, 0, decide, 24, tol, 0.1, planes)
            if not decide:  # the planes and the active bytes keep their sentinels
                for k, v in planes.items():
                    _same(got[k], v, what + ": untouched " + k)
        # n_done = 6: carried through two earlier launches of the restatement's
        carried, _ = ref.step(lst, None, x[:, :6], blank, n, 0, False, 99, 0, 0, {})
        for decide in (0, 1):
            what = "entries %d pass %d n_done 6 decide %d" % (entries, pass_, decide)
            _check_step(what, n, lst, None, x[:, 6:6 + pass_], carried, 6, decide, 6 + pass_ + decide, tol, 0.1, _sentinel_planes(n))
    # a device count below the capacity, above it, and 0: every other state word and plane element is untouched
    x = (rng.random((entries, 5, 3)).astype(np.float32) * scale).astype(np.float32)
    for count in sorted({0, 1, entries // 2, entries, entries + 1000}):
        what = "entries %d count %d" % (entries, count)
        st, got = _check_step(what, n, lst, count, x, blank, 0, 1, 24, 0.05, 0.1, _sentinel_planes(n))
        live = lst[:min(count, entries)]
        rest = np.setdiff1d(np.arange(n), live)
        assert (st[:, rest] == -7.25).all() and (got["spp"][rest] == SENTINEL).all() and (got["active"][rest] == 7).all(), what
        assert (got["spp"][live] == 5).all()
    # each plane is optional
    for only in ("active", "linear", "rgb8", "stderr", "spp"):
        _check_step("entries %d only %s" % (entries, only), n, lst, None, x, blank, 0, 1, 24, 0.05, 0.1,
                    {only: _sentinel_planes(n)[only]})


@pytest.mark.gpu
def test_step_kernel_on_one_pixel():
    """The smallest call: one pixel, one entry, so every part of the probe's allocation is shorter than its alignment."""
    x = np.array([[[0.5, 0.25, 0.125], [0.75, 0.25, 0.5], [0.25, 0.25, 0.25]]], np.float32)  # [entry][sample][channel]
    blank = np.full((9, 1), -7.25)
    for decide in (0, 1):
        _, got = _check_step("one pixel, decide %d" % decide, 1, [0], None, x, blank, 0, decide, 24, 0.05, 0.1, _sentinel_planes(1))
    assert got["spp"].tolist() == [3] and got["active"].tolist() == [1]  # the first channel's error is above the tolerance
    carried, _ = ref.step([0], None, x[:, :2], blank, 1, 0, False, 99, 0, 0, {})
    _check_step("one pixel, carried", 1, [0], 1, x[:, 2:], carried, 2, 1, 3, 0.05, 0.1, _sentinel_planes(1))


@pytest.mark.gpu
def test_step_kernel_special_values_and_lists():
    n = 100
    rng, lst, _ = _crafted(70, n, 7)
    x = rng.random((70, 5, 3)).astype(np.float32)
    x[0, 1, 0] = np.nan
    x[1, 4, 2] = np.inf
    x[2, 0, 1] = -np.inf
    x[3] = 0.375  # zero variance: converged with abs_tol = 0
    x[4] = 0.0
    blank = np.full((9, n), -7.25)
    for abs_tol, rel_tol, cap in ((0.0, 0.0, 24), (1e30, 1e30, 24), (0.0, 0.0, 5), (0.2, 0.0, 5), (0.2, 0.0, 6)):
        what = "tolerances %g %g cap %d" % (abs_tol, rel_tol, cap)
        _, got = _check_step(what, n, lst, None, x, blank, 0, 1, cap, abs_tol, rel_tol, _sentinel_planes(n), nan_equal=True)
        a = got["active"][lst]
        if cap == 5:  # n == cap: retired as it is, converged or not
            assert (a == 0).all(), what
        else:
            assert a[:3].tolist() == [1, 1, 1] and a[3:5].tolist() == [0, 0], what  # a non-finite value never converges
        assert np.isnan(got["linear"][lst[0], 0]) and got["rgb8"][lst[0], 0] == 0
        assert np.isposinf(got["linear"][lst[1], 2]) and got["rgb8"][lst[1], 2] == 255 and got["rgb8"][lst[2], 1] == 0
    # an unsorted list, and indices outside the planes (skipped: nothing is read or written for them)
    perm = rng.permutation(n)[:70].astype(np.uint32)
    _check_step("unsorted", n, perm, None, x, blank, 0, 1, 24, 0.1, 0.0, _sentinel_planes(n), nan_equal=True)
    wild = perm.copy()
    wild[[0, 13, 64, 69]] = [n, 2 ** 31 + 5, 2 ** 32 - 1, n + 1]
    st, got = _check_step("outside", n, wild, None, x, blank, 0, 1, 24, 0.1, 0.0, _sentinel_planes(n), nan_equal=True)
    for p in (perm[0], perm[13], perm[64], perm[69]):
        assert (st[:, p] == -7.25).all() and got["spp"][p] == SENTINEL
    carried, _ = ref.step(perm, None, x[:, :2], blank, n, 0, False, 99, 0, 0, {})
    _check_step("outside, carried", n, wild, 66, x[:, 2:], carried, 2, 1, 24, 0.1, 0.0, _sentinel_planes(n), nan_equal=True)


@pytest.mark.gpu
def test_step_kernel_folds_a_long_pass():
    """86 samples in one launch, a multiple of the unroll plus a tail of 2, over three workgroups' worth of lanes minus one."""
    n = 600
    rng, lst, scale = _crafted(600, n, 86)
    x = (rng.random((600, 86, 3)).astype(np.float32) * scale).astype(np.float32)
    _check_step("pass 86", n, lst, 599, x, np.zeros((9, n)), 0, 1, 100, 0.01, 0.05, _sentinel_planes(n))


# ---- 2. the whole render against the restatement ------------------------------------------------------------------------------
_SAMPLES = {}  # case -> (samples f32 [n, MOST, 3], abs_tol): computed once, shared, never changed


def _reference_samples(case, sc, cam, nx, ny, estimator):
    """Every pixel's first MOST samples by Scene.render_pixels (their bits are pinned to the renders by tests/test_gpu_sparse.py)
    and the tolerance: half the median over pixels of the max-channel stderr at min_spp, from a min_spp == ns run, as
    tests/test_gpu_adaptive.py chooses it."""
    if case not in _SAMPLES:
        x = sc.render_pixels(cam, nx, ny, np.arange(nx * ny, dtype=np.uint32), MOST, estimator=estimator, seed=SEED, samples=True, flags=FC)["samples"]
        x.setflags(write=False)
        lo = _lattice(case, "cap24")[0]
        at_min = sc.render_pixelwise(cam, nx, ny, lo, lo, 1, estimator=estimator, seed=SEED, flags=FC)
        assert (at_min["spp"] == lo).all()
        _SAMPLES[case] = (x, 0.5 * float(np.median(at_min["stderr"].reshape(-1, 3).max(axis=1))))
    return _SAMPLES[case]


def _pixelwise(sc, cam, nx, ny, estimator, lattice, abs_tol, **kw):
    lo, step, cap = lattice
    kw.setdefault("flags", FC)
    return sc.render_pixelwise(cam, nx, ny, cap, lo, step, abs_tol=abs_tol, estimator=estimator, seed=SEED, **kw)


def _check_against(out, want, nx, ny, what):
    for k in PLANES:
        _same(out[k].reshape(want[k].shape), want[k], "%s: %s" % (what, k))
    _same(out["counts"], want["counts"], what + ": counts")


@pytest.mark.gpu
@pytest.mark.parametrize("lattice", sorted(LATTICES))
@pytest.mark.parametrize("case", sorted(CASES))
def test_render_is_the_restatement(host, case, lattice):
    sc, cam, nx, ny, estimator = _open(host, case)
    x, abs_tol = _reference_samples(case, sc, cam, nx, ny, estimator)
    lo, step, cap = _lattice(case, lattice)
    assert abs_tol > 0.0
    want = ref.render(x[:, :cap], lo, step, abs_tol=abs_tol)
    out = _pixelwise(sc, cam, nx, ny, estimator, (lo, step, cap), abs_tol)
    spp = out["spp"].reshape(-1)
    print("%s %s: abs_tol %.6g, spp histogram %r, counts %r, samples %d" % (
        case, lattice, abs_tol, dict(zip(*[a.tolist() for a in np.unique(spp, return_counts=True)])), out["counts"][:, 0].tolist(),
        out["samples"]))
    _check_against(out, want, nx, ny, "%s %s" % (case, lattice))
    per_step = np.diff([0] + ref.lattice(cap, lo, step))
    assert out["samples"] == int(spp.sum()) == int((out["counts"][:, 0].astype(np.int64) * per_step).sum())
    # the conditions under which the comparison says something
    assert len(np.unique(spp)) >= 3 and (spp == lo).any() and (spp == cap).any()


# ---- 3. every pixel against the fixed render at its own count -------------------------------------------------------------------
def _fixed(sc, cam, nx, ny, estimator, n, flags=FC):
    if estimator == "plain":
        return sc.render_adaptive(cam, nx, ny, n, n, n, seed=SEED, flags=flags)
    if estimator == "nee":
        return sc.render_nee(cam, nx, ny, n, seed=SEED, flags=flags)
    return sc.render_env(cam, nx, ny, n, nee=estimator == "env_nee", seed=SEED, flags=flags)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_every_pixel_is_the_fixed_render_at_its_count(host, case):
    sc, cam, nx, ny, estimator = _open(host, case)
    _, abs_tol = _reference_samples(case, sc, cam, nx, ny, estimator)
    lattice = _lattice(case, "cap22")
    out = _pixelwise(sc, cam, nx, ny, estimator, lattice, abs_tol)
    spp = out["spp"]
    counts = np.unique(spp).tolist()
    assert len(counts) >= 3 and lattice[2] in counts
    for n in counts:
        full = _fixed(sc, cam, nx, ny, estimator, n)
        at = spp == n
        for k in ("linear", "rgb8", "stderr"):
            _same(out[k][at], full[k][at], "%s: %s of the %d pixels with spp = %d" % (case, k, int(at.sum()), n))


# ---- 4. against the tile-adaptive entry -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_never_more_samples_than_the_tile_entry(host, case):
    sc, cam, nx, ny, estimator = _open(host, case)
    _, abs_tol = _reference_samples(case, sc, cam, nx, ny, estimator)
    lo, step, cap = _lattice(case, "cap24")
    out = _pixelwise(sc, cam, nx, ny, estimator, (lo, step, cap), abs_tol)
    tile = sc.render_adaptive(cam, nx, ny, cap, lo, step, abs_tol=abs_tol, nee=estimator in ("nee", "env_nee"),
                              env=estimator in ("env", "env_nee"), seed=SEED, flags=FC)
    assert (out["spp"] <= tile["spp"]).all()
    total, total_tile = int(out["spp"].sum()), int(tile["spp"].astype(np.int64).sum())
    print("%s: %d paths per pixel, %d per tile over the in-image pixels" % (case, total, total_tile))
    assert total <= total_tile
    if case.startswith("cornell"):
        assert total < total_tile
    same = out["spp"] == tile["spp"]  # where the counts agree the pixels do: both are the fixed render at that count
    for k in ("linear", "rgb8", "stderr"):
        _same(out[k][same], tile[k][same], "%s: %s where the counts agree" % (case, k))


# ---- 5. invariance ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_result_does_not_depend_on_how_it_ran(host):
    import torch

    case = "cornell-nee"
    sc, cam, nx, ny, estimator = _open(host, case)
    _, abs_tol = _reference_samples(case, sc, cam, nx, ny, estimator)
    want = _pixelwise(sc, cam, nx, ny, estimator, LATTICES["cap22"], abs_tol)
    for pass_spp in (0, 1, 3, 4):  # 4 = step_spp
        _check_against(_pixelwise(sc, cam, nx, ny, estimator, LATTICES["cap22"], abs_tol, pass_spp=pass_spp), want, nx, ny, "pass_spp %d" % pass_spp)
    _check_against(_pixelwise(sc, cam, nx, ny, estimator, LATTICES["cap22"], abs_tol, flags=0), want, nx, ny, "without FAST_CULL")
    _check_against(_pixelwise(sc, cam, nx, ny, estimator, LATTICES["cap22"], abs_tol), want, nx, ny, "a second run")
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
                got = _pixelwise(sc, cam, nx, ny, estimator, LATTICES["cap22"], abs_tol, out="torch", pass_spp=3)
            side.synchronize()
        else:
            got = _pixelwise(sc, cam, nx, ny, estimator, LATTICES["cap22"], abs_tol, out="torch")
            torch.cuda.current_stream(dev).synchronize()
        assert all(got[k].device == dev for k in PLANES + ("counts",))
        host_of = {k: got[k].cpu().numpy() for k in PLANES + ("counts",)}
        host_of["spp"], host_of["counts"] = host_of["spp"].view(np.uint32), host_of["counts"].view(np.uint32)
        _check_against(host_of, want, nx, ny, "device form, call %d" % call)
        assert got["samples"]() == want["samples"]
        del got
    free_after = torch.cuda.mem_get_info(dev)[0]
    assert free_before == free_after, "the device form allocated: %d bytes free before call 2, %d after call 4" % (free_before, free_after)


@pytest.mark.gpu
def test_nothing_is_written_past_an_output(host):
    import torch

    case = "cornell-nee"
    sc, cam, nx, ny, estimator = _open(host, case)
    _, abs_tol = _reference_samples(case, sc, cam, nx, ny, estimator)
    lo, step, cap = LATTICES["cap22"]
    want = _pixelwise(sc, cam, nx, ny, estimator, LATTICES["cap22"], abs_tol)
    dev = torch.device("cuda", sc.device)
    n, steps = nx * ny, 6
    lib = abi.load_rtmi()
    p = abi.RenderParams()
    p.nx, p.ny, p.ns, p.max_depth, p.t_min, p.flags, p.tile_world, p.seed = nx, ny, cap, 50, 0.001, FC, 1, SEED
    o = abi.PixelwiseOpts(lo, step, abi.ROULETTE_ESTIMATORS[estimator], 3, abs_tol, 0.0, 0.5)
    words = {"linear": 3 * n, "rgb8": (3 * n + 3) // 4, "stderr": 3 * n, "spp": n, "counts": 2 * steps}
    nbytes = int(lib.rtmi_pixelwise_scratch_bytes(n, 3, steps))
    stream = torch.cuda.current_stream(dev)
    for which in (("linear", "rgb8", "stderr", "spp", "counts"), ("rgb8",), ("spp", "counts"), ("stderr",)):
        buf = {k: torch.full((words[k] + TAIL,), SENTINEL, dtype=torch.int32, device=dev) for k in which}
        scratch = torch.full((nbytes // 4 + TAIL,), SENTINEL, dtype=torch.int32, device=dev)
        host._check(host.lib.rth_render_pixelwise_device(
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


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["cornell-plain", "cornell-nee", "spheres-env_nee"])
def test_statistics_only_and_zero_tolerances(host, case):
    sc, cam, nx, ny, estimator = _open(host, case)
    # min_spp == ns: the fixed render plus its stderr, one step
    out = sc.render_pixelwise(cam, nx, ny, 6, 6, 4, abs_tol=0.5, estimator=estimator, seed=SEED, flags=FC)
    full = _fixed(sc, cam, nx, ny, estimator, 6)
    assert (out["spp"] == 6).all() and out["counts"].tolist() == [[nx * ny, nx * ny]] and out["samples"] == 6 * nx * ny
    for k in ("linear", "rgb8", "stderr"):
        _same(out[k], full[k], "%s min_spp == ns: %s" % (case, k))
    # tolerances 0: only a pixel without any variance stops before the cap, so every pixel that is not black runs to it
    lo, step, cap = _lattice(case, "cap22")
    zero = _pixelwise(sc, cam, nx, ny, estimator, (lo, step, cap), 0.0)
    early = zero["spp"] < cap
    print("%s: %d of %d pixels stop before the cap with tolerances 0, %d of them not black" % (
        case, int(early.sum()), early.size, int((zero["linear"][early] != 0).any(axis=1).sum())))
    assert (zero["stderr"][early] == 0).all() and (zero["spp"][early] == lo).all()
    assert (zero["spp"][(zero["linear"] != 0).any(axis=2)] == cap).all()
    full = _fixed(sc, cam, nx, ny, estimator, cap)
    for k in ("linear", "rgb8", "stderr"):
        _same(zero[k][~early], full[k][~early], "%s tolerances 0: %s" % (case, k))


# ---- 6. neighbours ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_neighbours_keep_their_bits(host):
    nx = ny = 32
    sc = _scene(host, "cornell_box", nx, ny, "nee")
    cam = _camera(host, nx, ny)
    ups = sc.upscaler(nx, ny, low=(16, 16), estimator="nee", flags=FC)
    px = np.arange(0, nx * ny, 7, dtype=np.uint32)

    def neighbours():
        a = sc.render_nee(cam, nx, ny, 8, seed=5, flags=FC)
        b = sc.render_pixels(cam, nx, ny, px, 4, estimator="nee", seed=5, samples=True, flags=FC)
        c = sc.render_adaptive(cam, nx, ny, 16, 4, 4, abs_tol=0.05, nee=True, seed=5, flags=FC)
        ups.reset()
        d = ups.render(cam, 4, seed=1)
        return b"".join(a[n].tobytes() for n in ("linear", "rgb8", "stderr")) + b"".join(b[n].tobytes() for n in ("mean", "stderr", "samples")) + \
            b"".join(c[n].tobytes() for n in ("linear", "rgb8", "stderr", "spp")) + b"".join(d[n].tobytes() for n in ("linear", "rgb8", "cls"))

    before = neighbours()
    for out in ("numpy", "torch"):
        got = sc.render_pixelwise(cam, nx, ny, 16, 4, 4, abs_tol=0.05, estimator="nee", seed=5, out=out, flags=FC)
        assert got["linear"].shape == (ny, nx, 3)
    assert neighbours() == before
    host.free_all()  # closes the open upscaler before its scene
    assert ups.h is None


@pytest.mark.gpu
def test_refusals_with_a_scene(host):
    sc = _scene(host, "cornell_box", 16, 16)
    cam = _camera(host, 16, 16)
    p = abi.RenderParams()
    p.nx, p.ny, p.ns, p.max_depth, p.t_min, p.flags, p.tile_world = 16, 16, 8, 50, 0.001, FC, 1
    out = np.zeros(16 * 16 * 3, np.float32)
    for estimator, word in ((1, "no light table attached"), (2, "no environment map attached"), (3, "no environment map attached")):
        o = abi.PixelwiseOpts(4, 4, estimator, 0, 0.0, 0.0, 0.5)
        assert host.lib.rth_render_pixelwise(sc.h, cam.h, C.byref(p), C.byref(o), out.ctypes.data, None, None, None, None, None) != 0
        msg = (host.lib.rth_last_error() or b"").decode()
        assert "rtmi_render_pixelwise: " in msg and word in msg, msg
        o.min_spp = 1  # the attachment is asked for before the header's own checks
        assert host.lib.rth_render_pixelwise(sc.h, cam.h, C.byref(p), C.byref(o), out.ctypes.data, None, None, None, None, None) != 0
        assert word in (host.lib.rth_last_error() or b"").decode()
    assert not out.any()
    for estimator in ("env", "env_nee"):  # the Python face attaches the light table on first use, so it comes after the raw entry
        with pytest.raises(Exception, match="no environment map attached"):
            sc.render_pixelwise(cam, 16, 16, 8, 4, 4, estimator=estimator, flags=FC)
    with pytest.raises(Exception, match="min_spp"):
        sc.render_pixelwise(cam, 16, 16, 8, 1, 4, flags=FC)
    got = sc.render_pixelwise(cam, 16, 16, 8, 4, 4, abs_tol=0.01, flags=FC)  # a refused call leaves the handle usable
    assert got["counts"][0].tolist() == [256, 256] and got["samples"] >= 4 * 256
