"""The handles' device and pinned memory: every buffer of rtmi_scene, rtmi_session and rtmi_multi is an
owner that knows its size, grows on demand and is reused by the next call.  A handle that grew, shrank and re-attached must
compute what a fresh handle computes, bit for bit, and destroyed handles must give their large buffers back.  No test here
provokes a device error; the owners' failure paths are tests/test_hostkit_owners.py's, on the host."""
import ctypes as C

import numpy as np
import pytest

from raytracing_rust_amd import abi, scenes
from raytracing_rust_amd.host import HIT_DTYPE, RAY_DTYPE, HostError, _outputs, default_params, primary_rays, release_cached

SMALL, LARGE = (8, 8, 2), (43, 21, 5)  # one tile; 6 x 3 = 18 tiles, the right column and the bottom row partial
SIZES = (SMALL, LARGE, SMALL)
COUNTS = (1, 130, 1)  # rays or points of a batch


def _world(host):
    return scenes.build(host, "cornell_box", 16, 16, seed=1)  # lights, no deferred items


def _planes(res):
    return {k: v for k, v in res.items() if isinstance(v, np.ndarray)}


def _same(got, want, what):
    got, want = _planes(got), _planes(want)
    assert sorted(got) == sorted(want), what
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), "%s: plane %s differs from the fresh handle's" % (what, k)


def _rays(cam, n):
    o, d = (a.reshape(-1, 3) for a in primary_rays(cam, 13, 10))
    return o[:n], d[:n]


def _surface(host, world, cam, n):
    """n surface points with their normals turned against the rays that found them (the hits, repeated cyclically)"""
    o, d = _rays(cam, n)
    h = host.lower(world).upload(0).trace(o, d)
    hit = np.flatnonzero(h["hit"])
    assert hit.size > n // 2
    hit = np.resize(hit, n)
    facing = np.einsum("nc,nc->n", h["normal"][hit], d[hit]) > 0.0
    return h["p"][hit], np.where(facing[:, None], -h["normal"][hit], h["normal"][hit])


IMAGE_MODES = {
    "render_sig": lambda sc, cam, nx, ny, ns: sc.render(cam, nx, ny, ns, sig=True),
    "render_adaptive": lambda sc, cam, nx, ny, ns: sc.render_adaptive(cam, nx, ny, 4 * ns, 2, 2, abs_tol=0.05),
    "render_features": lambda sc, cam, nx, ny, ns: sc.render_features(cam, nx, ny, ns, sig=True),
    "render_nee": lambda sc, cam, nx, ny, ns: sc.render_nee(cam, nx, ny, ns, sig=True),
    "render_roulette": lambda sc, cam, nx, ny, ns: sc.render_roulette(cam, nx, ny, ns),
    "render_pixelwise": lambda sc, cam, nx, ny, ns: sc.render_pixelwise(cam, nx, ny, 4 * ns, 2, 2, abs_tol=0.05),
    "render_f64": lambda sc, cam, nx, ny, ns: sc.render(cam, nx, ny, ns, sig=True, precision="f64"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(IMAGE_MODES))
def test_image_buffers_grow_and_are_reused(host, mode):
    """one tile, then 18 tiles with partial ones, then one tile again on one handle: each equals a fresh handle's"""
    cam, world = _world(host)
    used = host.lower(world).upload(0)
    for step, (nx, ny, ns) in enumerate(SIZES):
        _same(IMAGE_MODES[mode](used, cam, nx, ny, ns), IMAGE_MODES[mode](host.lower(world).upload(0), cam, nx, ny, ns),
              "%s step %d (%dx%dx%d)" % (mode, step, nx, ny, ns))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["trace", "radiance", "gather"])
def test_batch_buffers_grow_and_are_reused(host, mode):
    cam, world = _world(host)
    pts, nrm = _surface(host, world, cam, max(COUNTS))

    def run(sc, n):
        o, d = _rays(cam, n)
        if mode == "trace":
            res = sc.trace(o, d)
            res.pop("kernel_ms")
            return res
        if mode == "radiance":
            return sc.radiance(o, d, spp=3, estimator="nee", seed=5, samples=True)
        return sc.gather(pts[:n], nrm[:n], spp=4, estimator="nee", seed=5)

    used = host.lower(world).upload(0)
    for step, n in enumerate(COUNTS):
        _same(run(used, n), run(host.lower(world).upload(0), n), "%s step %d (n = %d)" % (mode, step, n))


def _nee(sc, cam, **kw):
    return sc.render_nee(cam, *LARGE, sig=True, **kw)


@pytest.mark.gpu
def test_reattached_lights_and_tree(host):
    cam, world = _world(host)
    fresh = _nee(host.lower(world).upload(0, nee=True), cam)
    fresh_tree = _nee(host.lower(world).upload(0, light_tree=True), cam, light_tree=True)
    sc = host.lower(world).upload(0, nee=True)
    sc.attach_lights()
    _same(_nee(sc, cam), fresh, "attach_lights twice")
    sc.attach_light_tree()
    _same(_nee(sc, cam, light_tree=True), fresh_tree, "tree attached")
    sc.attach_lights()  # the tree's leaves index the table it was built over: a new table detaches it
    _same(_nee(sc, cam), fresh, "attach_lights after the tree")
    p = default_params(8, 8, 1, flags=abi.RTMI_FLAG_LIGHT_TREE)  # (render_nee(light_tree=True) would attach the tree first)
    with pytest.raises(HostError, match="no light tree attached"):
        host._check(host.lib.rth_render_nee(sc.h, cam.h, C.byref(p), *_outputs(8, 8, ("linear", "rgb8", "stderr"), False)[1]))
    sc.attach_light_tree()
    _same(_nee(sc, cam, light_tree=True), fresh_tree, "tree attached again")


@pytest.mark.gpu
def test_reattached_environment_map(host):
    cam, world = _world(host)
    rng = np.random.default_rng(3)
    small, large = rng.random((2, 4, 3)).astype(np.float32), (rng.random((8, 16, 3)) ** 4 * 10).astype(np.float32)

    def env(sc):
        return sc.render_env(cam, *LARGE, sig=True)

    sc = host.lower(world).upload(0, nee=True).attach_env(small)
    _same(env(sc), env(host.lower(world).upload(0, nee=True).attach_env(small)), "4x2 map")
    _same(_nee(sc.detach_env(), cam), _nee(host.lower(world).upload(0, nee=True), cam), "map detached")
    with pytest.raises(HostError, match="no environment map attached"):
        env(sc)
    sc.attach_env(large)
    _same(env(sc), env(host.lower(world).upload(0, nee=True).attach_env(large)), "16x8 map after the detach")


@pytest.mark.gpu
def test_reattached_f64_planes(host):
    cam, world = _world(host)
    fresh = host.lower(world).upload(0, f64=True).render(cam, *LARGE, sig=True, precision="f64")
    sc = host.lower(world).upload(0, f64=True)
    sc.attach_f64()
    _same(sc.render(cam, *LARGE, sig=True, precision="f64"), fresh, "attach_f64 twice")
    _same(sc.render(cam, *LARGE, sig=True), host.lower(world).upload(0).render(cam, *LARGE, sig=True), "f32 beside the planes")


def _raw_trace(lib, handle, cam, n):
    o, d = _rays(cam, n)
    rays = np.empty(n, RAY_DTYPE)
    rays["o"], rays["d"], rays["t_min"], rays["t_max"] = o, d, 0.001, np.inf
    out, ms = np.zeros(n, HIT_DTYPE), C.c_double(0.0)
    p = abi.QueryParams(n, abi.RTMI_FLAG_FAST_CULL, 0, 0)
    assert lib.rtmi_trace(handle, C.byref(p), rays.ctypes.data, None, out.ctypes.data, C.byref(ms)) == 0, lib.rtmi_last_error()
    return {"hits": out}


@pytest.mark.gpu
def test_flips_attached_and_detached(host):
    """rtmi_scene_attach_flips through the C ABI (the Python face attaches the lowering's table at upload and never
    detaches): a table, no table, another table on one handle, each against a fresh handle in that state"""
    cam, world = _world(host)
    lib, desc = abi.load_rtmi(), host.lower(world).desc()
    tables = [None, (np.ones(desc.n_prims, np.uint32), np.zeros(desc.n_items, np.uint32)),
              (np.zeros(desc.n_prims, np.uint32), np.ones(desc.n_items, np.uint32))]

    def attach(handle, table):
        args = (None, 0, None, 0) if table is None else (table[0].ctypes.data, desc.n_prims, table[1].ctypes.data, desc.n_items)
        assert lib.rtmi_scene_attach_flips(handle, *args) == 0, lib.rtmi_last_error()

    def create():
        handle = C.c_void_p()
        assert lib.rtmi_scene_create(C.byref(desc), 0, C.byref(handle)) == 0, lib.rtmi_last_error()
        return handle

    used, want = create(), []
    try:
        for table in tables:
            fresh = create()
            try:
                attach(fresh, table)
                want.append(_raw_trace(lib, fresh, cam, 130))
            finally:
                lib.rtmi_scene_destroy(fresh)
        assert want[0]["hits"].tobytes() != want[1]["hits"].tobytes()  # the table is read
        for step in (1, 0, 2, 2, 0):
            attach(used, tables[step])
            _same(_raw_trace(lib, used, cam, 130), want[step], "flips table %d" % step)
    finally:
        lib.rtmi_scene_destroy(used)


@pytest.mark.gpu
def test_session_survives_export_destroy_create_import(host):
    cam, world = _world(host)
    sc = host.lower(world).upload(0, nee=True)
    nx, ny, _ = LARGE
    with sc.session(cam, nx, ny, estimator="nee", roulette=dict(min_depth=2, q_min=0.1)) as whole:
        whole.render(3)
        whole.render(2)
        want = whole.image()
    first = sc.session(cam, nx, ny, estimator="nee", roulette=dict(min_depth=2, q_min=0.1))
    first.render(3)
    blob = first.save()
    first.close()
    with sc.session(cam, nx, ny, estimator="nee", roulette=dict(min_depth=2, q_min=0.1)) as second:
        second.load(blob)
        second.render(2)
        _same(second.image(), want, "the session continued from its blob")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 65])
def test_probes_hold_one_allocation(host, n):
    """rtmi_probe_env and rtmi_probe_light_tree carve one arena: the same answers from a used and from a fresh handle"""
    cam, world = _world(host)
    rng = np.random.default_rng(n)
    envmap = (rng.random((8, 16, 3)) ** 4 * 10).astype(np.float32)
    dirs = rng.normal(size=(n, 3)).astype(np.float32)
    uv, u = rng.random((n, 2)).astype(np.float32), rng.random(n).astype(np.float32)
    pts = (rng.random((n, 3)) * 555.0).astype(np.float32)

    def probes(sc):
        light, p = sc.light_pick(pts, u)
        return {"lookup": sc.probe_env(abi.RTMI_ENV_PROBE_LOOKUP, dirs), "sample": sc.probe_env(abi.RTMI_ENV_PROBE_SAMPLE, uv),
                "light": light, "p": p, "pmf": sc.light_pmf(pts, light)}

    used = host.lower(world).upload(0, light_tree=True).attach_env(envmap)
    first = probes(used)
    assert np.isfinite(first["lookup"]).all() and (first["p"] > 0).all() and (first["pmf"] > 0).all()
    used.render(cam, *LARGE)
    _same(probes(used), first, "probes after a render")
    _same(probes(host.lower(world).upload(0, light_tree=True).attach_env(envmap)), first, "probes on a fresh handle")


# The spread of the parent commit's readings over cycles 2..6 of the loop below, measured on an MI355X
# (profiles/handles/memory.jsonl), plus half the smallest of the three buffers named in the test.
PARENT_SPREAD = 0  # both parent runs read 308388298752 B after every cycle
SMALLEST = 256 * 256 * 16  # the framebuffer: 16-B texels


def memory_cycles(host, cycles=6):
    """free device memory after each cycle of create, use at 256x256, destroy, release_cached (no torch allocation between)"""
    import torch

    free = []
    for _ in range(cycles):
        cam, world = _world(host)
        sc = host.lower(world).upload(0)
        sc.render(cam, 256, 256, 2)  # framebuffer 1 MiB, f64 sums 1.5 MiB, per-sample buffer 1.5 MiB
        host.free_all()
        release_cached()
        free.append(torch.cuda.mem_get_info(0)[0])
    return free


@pytest.mark.gpu
def test_destroyed_handles_return_their_memory(host):
    """sees leaks of the large buffers only; the small tables are owners like them (tests/test_hostkit_owners.py).  The six
    cycles take 0.2 s on an MI355X; run alone, the test takes 11 s, the rest being torch's first use of the device in the
    process."""
    free = memory_cycles(host)
    print("free bytes after each cycle:", free)
    assert free[5] >= free[1] - (PARENT_SPREAD + SMALLEST // 2), free
