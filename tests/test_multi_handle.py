"""The persistent multi-device handle (rtmi_multi_create / _prepare / _render / _destroy, SURVEY §8(b): the scene is
copied to each selected device ONCE, multi-GPU is internal to the render call) and the thread model of rtmi.h
(render calls on one handle serialise: per-handle mutex on the host, event chain on the device).

The loop the handle shards is create_image's (tests/test.rs:62-79); the reference's convention being replaced is a
single thread holding Rc's (src/bvh.rs:11-12).  CPU tests cover argument validation, symbol export and the
thread-locality of rtmi_last_error; the GPU tests compare with rtmi_render bit-for-bit."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import scenes_extra
from raytracing_rust_amd import abi
from raytracing_rust_amd.host import HostError, default_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ CPU
def test_multi_entry_points_validate_before_touching_a_device(host):
    from raytracing_rust_amd import scenes

    lib = abi.load_rtmi()
    cam, world = scenes.build(host, "two_spheres", 16, 16)
    d = host.lower(world).desc()
    dev = (C.c_int * 2)(0, 0)
    h = C.c_void_p()
    assert lib.rtmi_multi_create(C.byref(d), dev, 0, C.byref(h)) == 1 and not h.value       # empty list
    assert lib.rtmi_multi_create(C.byref(d), None, 2, C.byref(h)) == 1 and not h.value      # NULL list
    assert lib.rtmi_multi_create(C.byref(d), dev, 2, None) == 1                             # NULL out
    bad = abi.SceneDesc.from_buffer_copy(d)
    bad.abi_version = 4
    assert lib.rtmi_multi_create(C.byref(bad), dev, 2, C.byref(h)) == 1 and b"abi_version" in lib.rtmi_last_error()
    p = default_params(16, 16, 1)
    c = cam.lower()
    assert lib.rtmi_multi_render(None, C.byref(c), C.byref(p), None, None, None) == 1
    assert lib.rtmi_multi_prepare(None, C.byref(p)) == 1
    lib.rtmi_multi_destroy(None)  # a no-op, like free(NULL)
    if lib.rtmi_device_count() == 0:
        assert lib.rtmi_multi_create(C.byref(d), dev, 2, C.byref(h)) == 3 and not h.value   # RTMI_ERR_DEVICE: no fallback
        assert b"no HIP device" in lib.rtmi_last_error()


def test_last_error_is_thread_local_and_untile_is_reentrant():
    """Two host threads inside the library at once: each keeps its own error text (rtmi_last_error is thread-local)
    and rtmi_untile, which works only on its arguments, gives every thread the single-thread result."""
    lib = abi.load_rtmi()
    nx, ny = 40, 24
    p = default_params(nx, ny, 1)
    ntex = lib.rtmi_local_tiles(C.byref(p)) * 64
    rng = np.random.default_rng(5)
    tex = rng.random((ntex, 4), dtype=np.float32)
    tex.view(np.uint32)[:, 3] = rng.integers(0, 1 << 24, ntex, dtype=np.uint32)
    ref_lin = np.zeros((ny, nx, 3), np.float32)
    ref_rgb = np.zeros((ny, nx, 3), np.uint8)
    assert lib.rtmi_untile(C.byref(p), tex.ctypes.data, ref_lin.ctypes.data, ref_rgb.ctypes.data) == 0
    out = {}
    start = threading.Barrier(2)

    def good():
        start.wait()
        for _ in range(200):
            lin = np.zeros((ny, nx, 3), np.float32)
            rgb = np.zeros((ny, nx, 3), np.uint8)
            assert lib.rtmi_untile(C.byref(p), tex.ctypes.data, lin.ctypes.data, rgb.ctypes.data) == 0
            assert np.array_equal(lin, ref_lin) and np.array_equal(rgb, ref_rgb)
        out["good"] = True

    def bad():
        start.wait()
        q = default_params(nx, ny, 1, tile_rank=3, tile_world=2)
        for _ in range(200):
            assert lib.rtmi_untile(C.byref(q), tex.ctypes.data, None, None) == 1
            assert b"tile_rank" in lib.rtmi_last_error()
        out["bad"] = True

    ts = [threading.Thread(target=good), threading.Thread(target=bad)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert out == {"good": True, "bad": True}


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("devices", [[0], [0, 0, 0]])
def test_resident_scene_renders_like_rtmi_render(host, devices):
    """One upload, several renders of different sizes and cameras from the same handle (buffers grow, then are
    reused for a smaller image): every image == rtmi_render's, bit for bit; the one-shot rtmi_render_multi too."""
    sc = None
    try:
        for k, (nx, ny, ns, seed) in enumerate([(100, 60, 12, 42), (160, 96, 6, 7), (50, 30, 20, 42)]):
            cam, world = scenes_extra.build(host, "lit_final_scene", nx, ny, seed=1)
            if sc is None:
                sc = host.lower(world)
                sc.upload(0)
                sc.upload_multi(devices)
            if k == 1:
                sc.prepare_resident(nx, ny, ns, seed=seed, flags=abi.RTMI_FLAG_FAST_CULL)
            one = sc.render(cam, nx, ny, ns, seed=seed, flags=abi.RTMI_FLAG_FAST_CULL)
            res = sc.render_resident(cam, nx, ny, ns, seed=seed, flags=abi.RTMI_FLAG_FAST_CULL)
            assert np.array_equal(res["linear"], one["linear"]) and np.array_equal(res["rgb8"], one["rgb8"]), (k, devices)
            assert res["stats"]["samples"] == nx * ny * ns and res["stats"]["render_ms"] > 0
            assert res["stats"]["kernel"] == one["stats"]["kernel"] == abi.RTMI_KERNEL_WAVE_COOP
            assert one["linear"].mean() > 0.01
        shot = sc.render_multi(cam, nx, ny, ns, devices, seed=seed, flags=abi.RTMI_FLAG_FAST_CULL)
        assert np.array_equal(shot["linear"], one["linear"])
        with pytest.raises(HostError):  # whole-image calls only
            sc.render_resident(cam, nx, ny, ns, tile_rank=1, tile_world=2)
        with pytest.raises(HostError):
            host.lower(world).upload_multi([0, 99])
    finally:
        if sc is not None:
            sc.free_multi()


@pytest.mark.gpu
def test_two_threads_on_one_handle_each_get_the_single_thread_image(host):
    """rtmi.h thread model: two host threads render on ONE rtmi_scene (and on ONE rtmi_multi) at the same time, with
    different seeds and sizes; each must receive exactly the image a single thread gets (the handle's unit queue,
    status words, per-sample buffer and texel buffers are shared scratch: without the per-handle serialisation units
    are skipped or doubled).  ctypes releases the GIL during the calls, so the threads really overlap."""
    jobs = [(96, 64, 16, 42), (64, 40, 24, 1234)]
    cams = []
    sc = None
    for nx, ny, ns, seed in jobs:
        cam, world = scenes_extra.build(host, "lit_final_scene", nx, ny, seed=1)
        cams.append(cam)
        if sc is None:
            sc = host.lower(world)
            sc.upload(0)
            sc.upload_multi([0, 0])
    try:
        want = [sc.render(cams[k], nx, ny, ns, seed=seed, flags=abi.RTMI_FLAG_FAST_CULL)
                for k, (nx, ny, ns, seed) in enumerate(jobs)]
        for fn in (sc.render, sc.render_resident):
            got, errs = {}, []
            start = threading.Barrier(2)

            def work(k):
                try:
                    nx, ny, ns, seed = jobs[k]
                    start.wait()
                    for rep in range(4):
                        r = fn(cams[k], nx, ny, ns, seed=seed, flags=abi.RTMI_FLAG_FAST_CULL)
                        assert np.array_equal(r["linear"], want[k]["linear"]), (fn.__name__, k, rep)
                        assert np.array_equal(r["rgb8"], want[k]["rgb8"])
                    got[k] = True
                except BaseException as e:  # noqa: BLE001 — reported by the main thread
                    errs.append(repr(e))
                    try:
                        start.abort()
                    except Exception:
                        pass

            ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
            [t.start() for t in ts]
            [t.join() for t in ts]
            assert not errs, errs
            assert got == {0: True, 1: True}
    finally:
        sc.free_multi()


@pytest.mark.gpu
def test_render_device_on_two_streams_of_one_handle_serialises_on_the_device(host):
    """The asynchronous entry point, two torch streams, one handle: the second launch must wait for the first on the
    device (event chain) — both framebuffers equal the blocking render's."""
    import torch

    from raytracing_rust_amd import dist as rdist

    nx, ny, ns = 128, 80, 32
    cam, world = scenes_extra.build(host, "lit_final_scene", nx, ny, seed=1)
    sc = host.lower(world)
    sc.upload(0)
    want = {s: sc.render(cam, nx, ny, ns, seed=s, flags=abi.RTMI_FLAG_FAST_CULL) for s in (42, 43)}
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    params = [rdist.rank_params(nx, ny, ns, 0, 1, seed=s, flags=abi.RTMI_FLAG_FAST_CULL) for s in (42, 43)]
    bufs = [rdist.new_local_framebuffer(p, dev) for p in params]
    torch.cuda.synchronize()
    for rep in range(3):
        for k in (0, 1):
            sc.render_device(cam, params[k], bufs[k].data_ptr(), streams[k].cuda_stream)
    torch.cuda.synchronize()
    sc.check_status()
    for k, s in enumerate((42, 43)):
        lin, rgb = rdist.untile(params[k], bufs[k].cpu().numpy()[None])
        assert np.array_equal(lin, want[s]["linear"]) and np.array_equal(rgb, want[s]["rgb8"])


@pytest.mark.gpu
def test_a_per_sample_buffer_is_parked_only_after_the_renders_that_write_it(host):
    """A render that outgrows its handle's per-sample buffer X takes a parked larger one and parks X for other handles of
    the device.  An asynchronous render of the same handle may still be writing X then: X is parked only after it has
    finished, so that the next handle to take X does not write it at the same time.  All images equal serial renders.
    (The overlap depends on timing: without the wait this test fails only when it happens.)"""
    import torch

    from raytracing_rust_amd import dist as rdist
    from raytracing_rust_amd.host import release_cached

    nx, ny, ns_small, ns_large, ns_parked = 256, 160, 256, 384, 512
    flags = abi.RTMI_FLAG_FAST_CULL
    cam, world = scenes_extra.build(host, "lit_final_scene", nx, ny, seed=1)
    release_cached()
    a, b, d = (host.lower(world).upload(0) for _ in range(3))
    a.render(cam, nx, ny, ns_small, seed=7, flags=flags)  # A's buffer X: ns_small samples
    d.render(cam, nx, ny, ns_parked, seed=7, flags=flags)  # D's buffer: ns_parked samples ...
    d.upload(0)  # ... parked: D's handle is destroyed (a fresh one replaces it)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    params = [rdist.rank_params(nx, ny, ns, 0, 1, seed=42, flags=flags) for ns in (ns_small, ns_large)]
    bufs = [rdist.new_local_framebuffer(p, dev) for p in params]
    torch.cuda.synchronize()
    a.render_device(cam, params[0], bufs[0].data_ptr(), stream.cuda_stream)  # writes X
    a.render_device(cam, params[1], bufs[1].data_ptr(), stream.cuda_stream)  # takes D's buffer, parks X
    got_b = b.render(cam, nx, ny, ns_small, seed=43, flags=flags)  # takes X
    torch.cuda.synchronize()
    a.check_status()
    for k, ns in enumerate((ns_small, ns_large)):
        lin, rgb = rdist.untile(params[k], bufs[k].cpu().numpy()[None])
        want = d.render(cam, nx, ny, ns, seed=42, flags=flags)
        assert np.array_equal(lin, want["linear"]) and np.array_equal(rgb, want["rgb8"]), ns
    want = d.render(cam, nx, ny, ns_small, seed=43, flags=flags)
    assert np.array_equal(got_b["linear"], want["linear"]) and np.array_equal(got_b["rgb8"], want["rgb8"])


@pytest.mark.gpu
def test_c5_x5000_as_eight_ranks_through_the_multi_handle(host):
    """BASELINE config C5 — final_scene 1920x1080x5000 spp tile-split over 8 GPUs — at FULL size through the C ABI's
    persistent handle, all eight ranks on this one GPU (rtmi_multi_create with the same device eight times: eight
    resident scenes, eight 15.6-GB per-sample buffers = 124 GB of the 288, eight streams, the gather into one
    framebuffer and the 8-way un-tiling): the image equals rtmi_render's of the whole frame bit for bit.  The lit
    variant of the scene (light rect the right way round) so that the radiance carries information; 10.4 G paths each
    way.  What this leaves unmeasured of the 8-GPU config: the RCCL gather between DISTINCT devices."""
    import torch

    free, _total = torch.cuda.mem_get_info(0)
    if free < 200 * 2**30:  # + the 45-GiB buffer of the whole-frame render afterwards
        pytest.skip("needs 124 GB of free HBM for the eight per-sample buffers, %.0f GB free" % (free / 2**30))
    nx, ny, ns = 1920, 1080, 5000
    cam, world = scenes_extra.build(host, "lit_final_scene", nx, ny, seed=1)
    sc = host.lower(world)
    sc.upload_multi([0] * 8)
    try:
        res = sc.render_resident(cam, nx, ny, ns, seed=42, flags=abi.RTMI_FLAG_FAST_CULL)
        assert res["stats"]["samples"] == nx * ny * ns
        print("8 ranks on one GPU: %.0f ms" % res["stats"]["kernel_ms"])
    finally:
        sc.free_multi()
    sc.upload(0)
    one = sc.render(cam, nx, ny, ns, seed=42, flags=abi.RTMI_FLAG_FAST_CULL)  # passes within the default 48-GiB budget
    print("1 rank: %.0f ms, mean radiance %.4f" % (one["stats"]["kernel_ms"], float(one["linear"].mean())))
    assert float(one["linear"].mean()) > 0.01
    assert np.array_equal(res["linear"], one["linear"]) and np.array_equal(res["rgb8"], one["rgb8"])


# ------------------------------------------------------------------------------------------------ RCCL on one GPU
@pytest.mark.gpu
def test_one_rank_rccl_gather_through_the_multi_handle(host, monkeypatch):
    """Every line of the collective path that ONE GPU can execute: with RTMI_FORCE_RCCL=1 a one-entry device list gets a
    one-rank communicator — dlopen(librccl) -> six dlsym -> ncclCommInitAll(1) at create, ncclGroupStart / ncclGather /
    ncclGroupEnd on the scene's stream in every render, D2H, un-tiling — and rtmi_multi_collective() says so.  Image ==
    rtmi_render's bit for bit; without the knob the same list reports no exchange; a device listed twice reports peer
    copies.  The loop whose tiles the gather brings together: tests/test.rs:62-70.
    Also the communicator pool: two LIVE handles on the same list hold different sets (they may render from two
    threads), a destroyed handle's set is taken over by the next create."""
    nx, ny, ns = 200, 120, 24
    cam, world = scenes_extra.build(host, "lit_final_scene", nx, ny, seed=1)
    sc = host.lower(world)
    sc.upload(0)
    want = sc.render(cam, nx, ny, ns, seed=42, flags=abi.RTMI_FLAG_FAST_CULL)
    assert want["linear"].mean() > 0.01
    monkeypatch.delenv("RTMI_FORCE_RCCL", raising=False)
    sc.upload_multi([0])
    assert sc.multi_collective() == "none"
    sc.upload_multi([0, 0])
    assert sc.multi_collective() == "peer_copy"
    sc.free_multi()
    monkeypatch.setenv("RTMI_FORCE_RCCL", "1")
    sc.upload_multi([0])
    try:
        assert sc.multi_collective() == "rccl"
        for rep in range(3):
            got = sc.render_resident(cam, nx, ny, ns, seed=42, flags=abi.RTMI_FLAG_FAST_CULL)
            assert np.array_equal(got["linear"], want["linear"]) and np.array_equal(got["rgb8"], want["rgb8"]), rep
        # a second live handle on the same list: its own communicator; both render at the same time
        sc2 = host.lower(world)
        sc2.upload_multi([0])
        try:
            assert sc2.multi_collective() == "rccl"
            errs = []

            def work(s):
                try:
                    for _ in range(3):
                        r = s.render_resident(cam, nx, ny, ns, seed=42, flags=abi.RTMI_FLAG_FAST_CULL)
                        assert np.array_equal(r["rgb8"], want["rgb8"]) and np.array_equal(r["linear"], want["linear"])
                except BaseException as e:  # noqa: BLE001
                    errs.append(repr(e))

            ts = [threading.Thread(target=work, args=(s,)) for s in (sc, sc2)]
            [t.start() for t in ts]
            [t.join() for t in ts]
            assert not errs, errs
        finally:
            sc2.free_multi()
        # the one-shot form takes a pooled set over (no ncclCommInitAll per image) and gives the same image
        shot = sc.render_multi(cam, nx, ny, ns, [0], seed=42, flags=abi.RTMI_FLAG_FAST_CULL)
        assert np.array_equal(shot["linear"], want["linear"])
    finally:
        sc.free_multi()


@pytest.mark.gpu
def test_one_rank_torch_distributed_nccl_gather_in_a_fresh_process(tmp_path):
    """dist.py's host at world 1 under backend "nccl": init_process_group(collective_at_1=True) + gather_framebuffer
    really call torch.distributed (RCCL communicator of one rank, one gather per image) — the code the N > 1 ranks of
    bench.py run — and the image equals the blocking single-device render.  In a fresh child: a process group is made
    once per process, and this test process may already hold one."""
    import subprocess
    import sys

    code = r'''
import json, os, sys
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np, torch, torch.distributed as dist
import scenes_extra
from raytracing_rust_amd import Host, abi, dist as rdist
host = Host()
nx, ny, ns = 160, 96, 16
cam, world = scenes_extra.build(host, "lit_final_scene", nx, ny, seed=1)
sc = host.lower(world); sc.upload(0)
want = sc.render(cam, nx, ny, ns, seed=42, flags=abi.RTMI_FLAG_FAST_CULL)
rank, world_n, local_rank = rdist.init_process_group("nccl", collective_at_1=True)
assert dist.is_initialized() and dist.get_backend() == "nccl" and dist.get_world_size() == 1
dev = torch.device("cuda", 0)
p = rdist.rank_params(nx, ny, ns, rank, world_n, seed=42, flags=abi.RTMI_FLAG_FAST_CULL)
local = rdist.new_local_framebuffer(p, dev)
stream = torch.cuda.current_stream(dev)
for rep in range(3):
    sc.render_device(cam, p, local.data_ptr(), stream.cuda_stream)
    g = rdist.gather_framebuffer(local, rank, world_n)
    assert g.data_ptr() != local.data_ptr()  # the gather's own output buffer, not a view of the input
torch.cuda.synchronize(); dist.barrier(); sc.check_status()
lin, rgb = rdist.untile(p, g.cpu().numpy())
dist.destroy_process_group()
print(json.dumps({"equal": bool(np.array_equal(lin, want["linear"]) and np.array_equal(rgb, want["rgb8"])),
                  "mean": float(lin.mean())}))
''' % (ROOT, ROOT)
    env = dict(os.environ)
    env.pop("RANK", None); env.pop("WORLD_SIZE", None); env.pop("LOCAL_RANK", None); env.pop("MASTER_PORT", None)
    env["MASTER_ADDR"] = "127.0.0.1"
    cp = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert cp.returncode == 0, cp.stderr.decode(errors="replace")[-2000:]
    import json

    res = json.loads(cp.stdout.decode().strip().splitlines()[-1])
    assert res["equal"] and res["mean"] > 0.01, res
