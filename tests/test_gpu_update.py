"""Scene updates on the device (include/rtmi_update.h): after update_prims a resident handle holds, byte for byte, what a
fresh handle created from the refit description holds, renders the same bits on every kernel, and — with its old topology
— the image the fp32 oracle gives for a world built afresh at the new positions."""
import ctypes as C

import numpy as np
import pytest

import refit_ref as R
from oracle.oracle import ARITH_DEVICE, THROUGHPUT_FORM
from raytracing_rust_amd import abi, default_params, primary_rays

pytestmark = pytest.mark.gpu

NX, NY, NS, DEPTH = 24, 20, 4, 8  # partial tiles
FAST = abi.RTMI_FLAG_FAST_CULL
REPORT_INST = 1 << 19  # RTMI_KNOB_REPORT_INST
INST_ONE_TREE = 2


def _words(scene):
    return {k: scene.device_words(k).tobytes() for k in abi.SCENE_WORDS}


def _assert_same_memory(upd, fresh, what):
    a, b = _words(upd), _words(fresh)
    for k in a:
        assert len(a[k]) == len(b[k]) and a[k] == b[k], (what, k)


def _pair(host, kind):
    """-> spec, the resident scene, a second lowering of the same world that is not resident, its arrays"""
    spec = R.spec_of(kind)
    world = R.build_world(host, spec)
    upd, fresh = host.lower(world).upload(), host.lower(world)
    return spec, upd, fresh, R.from_desc(fresh.desc())


def _apply(upd, fresh, first, a, b, form):
    """the update on the resident handle in one form; on the other scene through its description, then a fresh handle"""
    if form == "device":
        import torch

        ta, tb = torch.tensor(a, device="cuda"), None if b is None else torch.tensor(b, device="cuda")
        upd.update_prims(first, ta, tb)
        torch.cuda.synchronize()
    else:
        hollow = bool(((a[:, 3] <= 0) & (R.from_desc(fresh.desc())["prim_meta"]["type"][first:first + len(a)] == abi.PRIM_SPHERE)).any())
        if hollow:  # the blocking form refuses the negative radius of a hollow sphere inside a tree, and changes nothing
            before = _words(upd)
            with pytest.raises(Exception, match="radius"):
                upd.update_prims(first, a, b)
            assert _words(upd) == before
            import torch

            for k in range(len(a)):  # one by one: the hollow spheres through the device form, the others (the emitter) blocking
                pa, pb = a[k:k + 1], None if b is None else b[k:k + 1]
                if a[k, 3] <= 0:
                    pa, pb = torch.tensor(pa, device="cuda"), None if pb is None else torch.tensor(pb, device="cuda")
                upd.update_prims(first + k, pa, pb)
            torch.cuda.synchronize()
        else:
            upd.update_prims(first, a, b)
    fresh.update_prims(first, a, b)
    fresh.upload()


def _ranges(kind, arr):
    n = len(arr["prim_a"])
    if kind != "two":
        return [(0, n)]
    bvh = [i for i, it in enumerate(arr["items"]) if it["kind"] == abi.ITEM_BVH]
    second = sorted(R.item_leaves(arr, bvh[1]))
    lists = [(int(it["first"]), int(it["count"])) for it in arr["items"] if it["kind"] == abi.ITEM_LIST]
    tail = (lists[-2][0], lists[-2][1] + lists[-1][1])  # the medium's boundary sphere and the rect emitter behind it
    assert lists[-2][0] + lists[-2][1] == lists[-1][0] and arr["prim_meta"][tail[0] + 1]["type"] == abi.PRIM_RECT
    return [(second[3], 4), tail, (second[0], len(second)), (5, 0), (0, n)]  # a part of an item first; the last two in a row


@pytest.mark.parametrize("form", ["blocking", "device"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_memory_equals_a_fresh_handle_of_the_refit_description(host, kind, form):
    spec, upd, fresh, arr = _pair(host, kind)
    items = np.frombuffer(upd.device_words("items"), np.uint8).reshape(-1, 96)
    assert len(items) == len(arr["items"])
    if kind == "two":
        flags = items[:, 12:16].copy().view("<u4")[:, 0]
        assert (flags & (1 << 16)).any()  # the medium's sphere rides in its item record (RTMI_ITEMFLAG_DEV_MEDIUM_SPHERE)
    for step, (first, count) in enumerate(_ranges(kind, arr)):
        a, b = R.new_planes(arr, spec, R.moved_spec(spec, 40 + step))
        before = _words(upd)
        _apply(upd, fresh, first, a[first:first + count], b[first:first + count] if step % 2 == 0 else None, form)
        _assert_same_memory(upd, fresh, (kind, form, step))
        assert (_words(upd) == before) == (count == 0)
    # the updated handle's boxes are the restatement's, not merely the same as another run of the library
    want = R.from_desc(fresh.desc())
    nodes = np.frombuffer(upd.device_words("nodes"), R.NODE)
    for f in R.BOX_FIELDS["nodes"] + ("left", "right"):
        assert nodes[f].tobytes() == want["nodes"][f].tobytes(), f


def _renders(scene, cam, sig_only=False):
    out = {}
    for label, flags in (("coop", FAST), ("perlane", FAST | abi.RTMI_FLAG_SYNC), ("reftree", FAST | abi.RTMI_FLAG_REF_TREE), ("exact", 0)):
        r = scene.render(cam, NX, NY, NS, seed=11, flags=flags, sig=True, max_depth=DEPTH)
        out[label] = (r["linear"].tobytes(), r["rgb8"].tobytes(), r["sig"].tobytes())
    r = scene.render(cam, NX, NY, NS, seed=11, flags=FAST | REPORT_INST, max_depth=DEPTH)
    out["default"] = (r["linear"].tobytes(), r["rgb8"].tobytes())
    inst = (r["stats"]["kernel"] >> 8) & 255
    r = scene.render_nee(cam, NX, NY, NS, seed=11, flags=FAST, sig=True, max_depth=DEPTH)
    out["nee"] = (r["linear"].tobytes(), r["rgb8"].tobytes(), r["sig"].tobytes())
    o, d = primary_rays(cam, NX, NY)
    t = scene.trace(o.reshape(-1, 3), d.reshape(-1, 3))
    out["trace"] = tuple(np.asarray(t[k]).tobytes() for k in sorted(t) if k != "kernel_ms")  # (a time, not a result)
    return out, inst


@pytest.mark.parametrize("kind", R.KINDS)
def test_renders_equal_the_fresh_handle_on_every_kernel(host, kind):
    spec, upd, fresh, arr = _pair(host, kind)
    cam = R.camera(host, NX, NY)
    upd.attach_lights()
    old, _ = _renders(upd, cam)
    a, b = R.new_planes(arr, spec, R.moved_spec(spec, 50, amount=0.05))
    _apply(upd, fresh, 0, a, b, "blocking")  # the emitter moves too: the wrapper attaches the lights again
    got, inst = _renders(upd, cam)
    want, inst_fresh = _renders(fresh, cam)
    for label in want:
        assert got[label] == want[label], (kind, label)
    assert got["coop"] != old["coop"]  # the scene did move (the primary rays of the smallest scenes meet the ground alone)
    every_tree_gated = all(it["alt_first"] >= 0 for it in arr["items"] if it["kind"] == abi.ITEM_BVH)
    assert inst == inst_fresh and (inst == INST_ONE_TREE) == every_tree_gated, (kind, inst)


@pytest.mark.parametrize("kind", R.KINDS)
def test_updated_handle_equals_the_oracle_on_a_world_built_afresh(host, orc32, kind):
    """The handle keeps the topology of the old positions; the oracle builds its own tree over the new ones.  Equal with
    zero differing pixels: the primitives do not touch, so no exact tie exists, and a difference is a finding about the
    refit's gates or boxes."""
    spec, upd, fresh, arr = _pair(host, kind)
    new = R.moved_spec(spec, 60)
    a, b = R.new_planes(arr, spec, new)
    _apply(upd, fresh, 0, a, b, "blocking")  # (the device form where the blocking one refuses: the hollow sphere)
    ref = orc32.render(R.camera(orc32, NX, NY), R.build_world(orc32, new), NX, NY, NS, seed=11, flags=ARITH_DEVICE | THROUGHPUT_FORM,
                       max_depth=DEPTH)
    cam = R.camera(host, NX, NY)
    assert np.count_nonzero(ref["linear"]) > 0
    for label, flags in (("coop", FAST), ("perlane", FAST | abi.RTMI_FLAG_SYNC), ("reftree", FAST | abi.RTMI_FLAG_REF_TREE)):
        got = upd.render(cam, NX, NY, NS, seed=11, flags=flags, sig=True, max_depth=DEPTH)
        differing = int((got["linear"] != ref["linear"]).any(axis=2).sum()) + int((got["sig"] != ref["sig"]).sum())
        assert differing == 0, (kind, label, differing)
    orc32.free_all()


def test_list_edits_equal_a_real_fresh_lowering(host):
    """No box depends on a list primitive: moving the run of top-level spheres, the medium's boundary and the emitter gives
    the memory and the image of a scene lowered afresh from a world with them at the new places"""
    spec, upd, _, arr = _pair(host, "two")
    moving = [e for e, ent in enumerate(spec) if ent[0] != "bvh"]
    new = R.moved_spec(spec, 70, entries=moving, amount=0.3)
    a, b = R.new_planes(arr, spec, new)
    changed = np.flatnonzero((a != arr["prim_a"]).any(axis=1) | (b != arr["prim_b"]).any(axis=1))
    assert len(changed) == 3  # (the ground stays)
    for p in changed:
        upd.update_prims(int(p), a[p:p + 1], b[p:p + 1])
    relowered = host.lower(R.build_world(host, new)).upload()
    _assert_same_memory(upd, relowered, "list")
    cam = R.camera(host, NX, NY)
    for flags in (FAST, FAST | abi.RTMI_FLAG_SYNC):
        x, y = (s.render(cam, NX, NY, NS, seed=3, flags=flags, sig=True, max_depth=DEPTH) for s in (upd, relowered))
        assert all(x[k].tobytes() == y[k].tobytes() for k in ("linear", "rgb8", "sig"))


def test_transform_edits_equal_a_real_fresh_lowering(host):
    """A Traslate(Rotate(Cube)) item and a translated list sphere moved by update_xforms with the records of a scene lowered
    afresh: that scene's memory (the item records' copies of their transforms among it) and its image"""
    def build(angle, offset, shift):
        spec = R.spec_of("s5")
        world = R.build_world(host, spec)
        mats = R._materials(host)
        world.push(host.Traslate(host.Rotate(1, host.Cube((0.0, 0.0, 0.0), (1.2, 1.5, 1.0), mats[3]), angle), offset))
        lst = host.HittableList()
        lst.push(host.Sphere((0.0, 0.0, 0.0), 0.4, mats[1]))
        lst.push(host.Traslate(host.Sphere((0.0, 0.0, 0.0), 0.4, mats[5]), shift))
        world.push(lst)
        return host.lower(world)

    upd = build(25.0, (4.0, 0.0, 1.0), (3.0, 1.0, 6.0)).upload()
    new = build(-40.0, (4.5, 0.3, 2.0), (2.0, 1.5, 5.0)).upload()
    recs = R.from_desc(new.desc())["xforms"]
    assert len(recs) == 3 and recs.tobytes() != R.from_desc(upd.desc())["xforms"].tobytes()
    upd.update_xforms(1, [tuple(r) for r in recs[1:].tolist()])
    upd.update_xforms(0, [tuple(recs[0].tolist())])
    _assert_same_memory(upd, new, "xforms")
    assert R.from_desc(upd.desc())["xforms"].tobytes() == recs.tobytes()
    cam = R.camera(host, NX, NY)
    for flags in (FAST, FAST | abi.RTMI_FLAG_SYNC, 0):
        x, y = (s.render(cam, NX, NY, NS, seed=3, flags=flags, sig=True, max_depth=DEPTH) for s in (upd, new))
        assert all(x[k].tobytes() == y[k].tobytes() for k in ("linear", "rgb8", "sig"))
    # a record must keep its kind; a record of a primitive inside a tree is refused
    before = _words(upd)
    with pytest.raises(Exception, match="kind"):
        upd.update_xforms(0, [(abi.XF_ROTATE_Y, 0.0, 1.0, 0.0)])
    host.seed_scene_rng(3)
    mat = host.Lambertian(host.SolidTexture(0.5, 0.5, 0.5))
    world = host.HittableList()
    world.push(host.BVHNode([host.Sphere((0.0, 0.0, 0.0), 0.3, mat), host.Traslate(host.Sphere((0.0, 0.0, 0.0), 0.3, mat), (1.0, 0.0, 0.0))], 0.0, 1.0))
    tree = host.lower(world).upload()
    with pytest.raises(Exception, match="inside a BVH item") as e:
        tree.update_xforms(0, [(abi.XF_TRANSLATE, 2.0, 0.0, 0.0)])
    assert type(e.value).__name__ == "Unsupported" and _words(upd) == before


def test_an_update_is_ordered_among_the_renders_of_its_stream(host):
    import torch

    spec, upd, fresh, arr = _pair(host, "mix67")
    old_scene = host.lower(R.build_world(host, spec)).upload()
    cam = R.camera(host, NX, NY)
    p = default_params(NX, NY, NS, seed=5, flags=FAST, max_depth=DEPTH)
    a, b = R.new_planes(arr, spec, R.moved_spec(spec, 80, amount=0.3))
    ta, tb = torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda")
    ntex = upd.local_tiles(p) * 64
    tex = [torch.zeros((ntex, 4), dtype=torch.float32, device="cuda") for _ in range(4)]
    upd.prepare(p)
    upd.prepare_updates().prepare_updates()  # the handle's tables, which its first update would build after waiting for the handle
    torch.cuda.synchronize()
    assert _words(upd) == _words(old_scene)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        upd.render_device(cam, p, tex[0].data_ptr(), stream.cuda_stream)
        upd.update_prims(0, ta, tb)
        upd.render_device(cam, p, tex[1].data_ptr(), stream.cuda_stream)
    stream.synchronize()  # the only wait
    fresh.update_prims(0, a, b)
    fresh.upload()
    old_scene.render_device(cam, p, tex[2].data_ptr())
    fresh.render_device(cam, p, tex[3].data_ptr())
    torch.cuda.synchronize()
    t = [x.cpu().numpy().tobytes() for x in tex]
    assert t[0] == t[2] and t[1] == t[3] and t[0] != t[1]
    upd.check_status()


def test_a_frame_bound_before_the_update_renders_the_moved_scene(host):
    spec, upd, fresh, arr = _pair(host, "s5")
    cam = R.camera(host, NX, NY)
    frame = upd.frame(NX, NY, temporal=None, flags=FAST, max_depth=DEPTH)
    before = frame.render(cam, NS, seed=9)
    a, b = R.new_planes(arr, spec, R.moved_spec(spec, 90, amount=0.3))
    _apply(upd, fresh, 0, a, b, "blocking")
    after = frame.render(cam, NS, seed=9)  # the same handle, not recreated
    want = fresh.frame(NX, NY, temporal=None, flags=FAST, max_depth=DEPTH).render(cam, NS, seed=9)
    assert after["linear"].tobytes() == want["linear"].tobytes() and after["rgb8"].tobytes() == want["rgb8"].tobytes()
    assert after["linear"].tobytes() != before["linear"].tobytes()


def test_refusals_leave_the_handle_as_it_was(host):
    mat = host.Lambertian(host.SolidTexture(0.5, 0.5, 0.5))
    sph = lambda x: host.Sphere((x, 0.0, 0.0), 0.3, mat)
    for name, odd in (("moving", host.MovingSphere((1.0, 0.0, 0.0), (1.0, 0.2, 0.0), 0.0, 1.0, 0.3, mat)),
                      ("rect", host.Rect(0, 0.0, 0.0, 1.0, 1.0, 1.0, mat))):
        host.seed_scene_rng(3)
        world = host.HittableList()
        world.push(host.BVHNode([sph(0.0), odd, sph(2.0)], 0.0, 1.0))
        world.push(sph(9.0))
        scene = host.lower(world).upload()
        planes = R.from_desc(scene.desc())["prim_a"]
        before = _words(scene)
        for form in ("numpy", "torch"):
            with pytest.raises(Exception, match="cannot be refit") as e:
                if form == "torch":
                    import torch

                    scene.update_prims(1, torch.tensor(planes[1:2] + np.float32(0.5), device="cuda"))
                else:
                    scene.update_prims(1, planes[1:2] + np.float32(0.5))
            assert type(e.value).__name__ == "Unsupported", name
        assert _words(scene) == before, name
        # a list primitive sits under no box: its planes are taken as rtmi_scene_create takes them, also an infinite one
        n = len(planes)
        far = planes[n - 1:].copy()
        far[0, 0] = np.inf
        scene.update_prims(n - 1, far)
        assert np.frombuffer(scene.device_words("prim_a"), np.float32).reshape(-1, 4)[n - 1].tobytes() == far[0].tobytes()
        scene.update_prims(n - 1, planes[n - 1:])
        assert _words(scene) == before
    # a refittable item: a non-positive radius and an inverted cube
    spec, upd, _, arr = _pair(host, "mix67")
    before = _words(upd)
    sphere = int(np.flatnonzero(arr["prim_meta"]["type"] == abi.PRIM_SPHERE)[0])
    cube = int(np.flatnonzero(arr["prim_meta"]["type"] == abi.PRIM_CUBE)[0])
    for p, col, word in ((sphere, 3, "radius"), (cube, 3, "inverted"), (sphere, 1, "not finite"), (cube, 2, "not finite")):
        bad = arr["prim_a"][p:p + 1].copy()
        bad[0, col] = {"radius": -1.0, "inverted": bad[0, 0] - 1.0, "not finite": np.nan}[word]
        with pytest.raises(Exception, match=word):
            upd.update_prims(p, bad, arr["prim_b"][p:p + 1])
    assert _words(upd) == before
    # the double planes of an edited scene hold the positions it was lowered with: they can no longer be attached
    edited = host.lower(R.build_world(host, spec)).upload()
    edited.update_prims(sphere, arr["prim_a"][sphere:sphere + 1] + np.float32(0.01))
    for call in (edited.attach_f64, lambda: edited.render(R.camera(host, NX, NY), NX, NY, 2, precision="f64")):
        with pytest.raises(Exception, match="edited") as e:
            call()
        assert type(e.value).__name__ == "Unsupported"
    # f64 planes attached: they would go stale
    upd.attach_f64()
    with pytest.raises(Exception, match="f64") as e:
        upd.update_prims(0, arr["prim_a"], arr["prim_b"])
    assert type(e.value).__name__ == "Unsupported" and _words(upd) == before
    # a scene resident on a device list has no update entry, and its description is left alone
    multi = host.lower(R.build_world(host, R.spec_of("s2")))
    multi.upload_multi([0])
    planes = R.from_desc(multi.desc())["prim_a"]
    with pytest.raises(Exception, match="multi-GPU") as e:
        multi.update_prims(0, planes + np.float32(0.5))
    assert type(e.value).__name__ == "Unsupported" and R.from_desc(multi.desc())["prim_a"].tobytes() == planes.tobytes()


def test_a_moved_emitter_detaches_the_lights_until_they_are_attached_again(host):
    """through the C ABI itself: rtmi_render_nee refuses after the update, and renders after rtmi_scene_attach_lights"""
    lib = abi.load_rtmi()
    spec = R.spec_of("s2")
    low = host.lower(R.build_world(host, spec))
    arr = R.from_desc(low.desc())
    h = C.c_void_p()
    d = low.desc()
    assert lib.rtmi_scene_create(C.byref(d), 0, C.byref(h)) == 0
    try:
        cam = R.camera(host, NX, NY).lower()
        p = default_params(NX, NY, NS, seed=1, flags=FAST, max_depth=DEPTH)
        lin = np.zeros((NY, NX, 3), np.float32)
        nee = lambda: lib.rtmi_render_nee(h, C.byref(cam), C.byref(p), lin.ctypes.data, None, None, None, None)
        assert lib.rtmi_scene_attach_lights(h, C.byref(d)) == 0 and nee() == 0
        emitter = int(np.flatnonzero(arr["prim_meta"]["type"] == abi.PRIM_RECT)[0])
        other = 0 if emitter else 1
        assert lib.rtmu_scene_update_prims(h, other, 1, arr["prim_a"][other:other + 1].ctypes.data, None) == 0 and nee() == 0
        moved = arr["prim_a"][emitter:emitter + 1] + np.float32(0.25)
        assert lib.rtmu_scene_update_prims(h, emitter, 1, moved.ctypes.data, None) == 0
        assert nee() != 0 and b"lights" in lib.rtmi_last_error()
        low.update_prims(emitter, moved)  # (not resident through the wrapper: its description alone)
        d2 = low.desc()
        assert lib.rtmi_scene_attach_lights(h, C.byref(d2)) == 0 and nee() == 0
    finally:
        lib.rtmi_scene_destroy(h)
