"""Lean addressing and quad rounds in the wave-cooperative traversal: the node and leaf records are
gathered through a scalar base and a 32-bit byte offset, and a round of the 4-wide walk that meets at most
RTMI_COOP_QUAD_MAX pending entries gives every entry four lanes, one per child.  The same cull decisions and the same
order-independent fold of the leaf hits, so every comparison is np.array_equal on float32 output, through the C ABI
(rtmi_scene_create / rtmi_render) as tests/test_coop_ray_constants.py goes.

 1. final_scene and random_spheres, 64x48 at 4 spp, seed 42, FAST_CULL | SKY: the default call reports the one-tree
    instantiation; its image is non-zero and equals the general instantiation's (knob value 4) and the per-lane kernel's
    (RTMI_FLAG_SYNC), also under the small-pool knob (bit 11), where the stack spills to global memory all the time.
    Quad rounds are switched off while a part of the stack is spilled (the stack bound): under the knob a
    quad round's publishes fill the small pool, the next round spills, and quad rounds resume when the spilled part is
    back — the knob covers that alternation, not a quad round over a spilled stack, which does not exist.  The general
    instantiation compiles the walk without either form (they cost it registers it does not have): it is the reference
    here beside the per-lane kernel;
 2. hand-built BVHs of n spheres, n in {2, 5, 16, 17, 64, 65, 300}, and a BVH of 20 cubes, bare and under
    Traslate(Rotate(Y)), 32x32 at 2 spp: the default call equals RTMI_FLAG_SYNC.  The small trees keep nearly every worker
    idle from the first round, 17 and 65 cross a quarter and a whole wavefront of leaves, 300 mixes full and sparse rounds;
 3. 1x1 and 3x1 images at 1 spp of the 65-sphere scene — one to three rays own the whole wavefront: equal to RTMI_FLAG_SYNC;
 4. path signatures (RTMI_FLAG_PATH_SIG) of the scenes of 1 at 32x32x2: image and signatures of the default call equal
    RTMI_FLAG_SYNC's;
 5. radiance queries on the cooperative batch kernel for 132 caller rays at two spheres of a tree — direction lengths
    2^-40, 1 and 2^40, axis-aligned rays, rays tangent in fp32 and one ulp either side, a t_min of each lane's own (the
    ray context's word carries q_min there): bitwise the per-lane query (the batch kernels compile the walk as it was:
    the case pins that the shared body still serves them);
 6. the profiling build (RTMI_FLAG_PROFILE) on random_spheres 64x48x4 counts quad rounds and dense rounds, both more than
    none, and no quad round met more than RTMI_COOP_QUAD_MAX entries.  The case knows the default of that compile-time
    constant, 16: a library built with 0 (the A/B build without quad rounds) fails `quads > 0` by design, one built with
    8 or 12 passes;
 7. RTMI_FLAG_TEST_OVERFLOW still makes the call fail loudly;
 8. a scene record that claims 2^25 nodes of 4-wide trees is refused by rtmi_scene_create (a node's byte offset and its
    pool reference assume fewer)."""
import ctypes as C

import numpy as np
import pytest

import scenes_extra
import test_gpu_batch_coop as B
from raytracing_rust_amd import abi, default_params, scenes

pytestmark = pytest.mark.gpu

SEED = 42
BASE = abi.RTMI_FLAG_FAST_CULL | abi.RTMI_FLAG_SKY
GENERAL = 4 << 8  # knob value 4 of flag bits 8..10: the general 4-wave instantiation
SMALL_POOL = 1 << 11  # a 256-entry LDS pool: the traversal stack spills to global memory all the time
REPORT_INST = 1 << 19  # RTMI_KNOB_REPORT_INST: rtmi_stats.kernel also carries the instantiation, in bits 8..15
INST_NONE, INST_GENERAL, INST_ONE_TREE = 0, 1, 2  # include/rtmi.h: RTMI_INST_*
RTMI_ERR_UNSUPPORTED = 2  # include/rtmi.h
QUAD_MAX = 16  # csrc/rtmi_bvh_coop.hpp: the default of RTMI_COOP_QUAD_MAX (see case 6 above)
f32 = np.float32


class _Device:
    """A lowered scene on device 0 through the C ABI with the report knob set."""

    def __init__(self, low, cam, nx, ny, ns):
        self.lib, self.low, self.cam, self.nx, self.ny, self.ns = abi.load_rtmi(), low, cam.lower(), nx, ny, ns
        self.h = C.c_void_p()
        desc = low.desc()
        assert self.lib.rtmi_scene_create(C.byref(desc), 0, C.byref(self.h)) == 0, self.lib.rtmi_last_error()

    def close(self):
        self.lib.rtmi_scene_destroy(self.h)

    def render(self, flags, sig=False, expect=0):
        """-> (linear, RTMI_KERNEL_*, RTMI_INST_*), with sig=True -> (linear, signatures, RTMI_KERNEL_*, RTMI_INST_*)"""
        p = default_params(self.nx, self.ny, self.ns, seed=SEED, flags=flags | REPORT_INST)
        lin, rgb = np.zeros((self.ny, self.nx, 3), f32), np.zeros((self.ny, self.nx, 3), np.uint8)
        sg = np.zeros((self.ny, self.nx), np.uint64)
        st = abi.Stats()
        rc = self.lib.rtmi_render(self.h, C.byref(self.cam), C.byref(p), lin.ctypes.data, rgb.ctypes.data,
                                  sg.ctypes.data if sig else None, C.byref(st))
        assert rc == expect, (rc, self.lib.rtmi_last_error())
        if sig:
            return lin, sg, abi.stats_kernel(st), abi.stats_instantiation(st)
        return lin, abi.stats_kernel(st), abi.stats_instantiation(st)


@pytest.fixture
def device():
    made = []

    def make(low, cam, nx, ny, ns):
        made.append(_Device(low, cam, nx, ny, ns))
        return made[-1]

    yield make
    for d in made:
        d.close()


# ---- 1. the headline scenes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["final_scene", "random_spheres"])
def test_headline_scenes_are_one_image(host, device, name):
    nx, ny = 64, 48
    cam, world = scenes_extra.build(host, name, nx, ny, seed=1)
    sc = device(host.lower(world), cam, nx, ny, 4)
    sync, kern, inst = sc.render(BASE | abi.RTMI_FLAG_SYNC)
    assert kern == abi.RTMI_KERNEL_PERLANE and inst == INST_NONE
    for pool in (0, SMALL_POOL):
        one, kern, inst = sc.render(BASE | pool)
        assert kern == abi.RTMI_KERNEL_WAVE_COOP and inst == INST_ONE_TREE
        assert np.count_nonzero(one) > 0
        gen, kern, inst = sc.render(BASE | pool | GENERAL)
        assert kern == abi.RTMI_KERNEL_WAVE_COOP and inst == INST_GENERAL
        assert np.array_equal(one, gen)
        assert np.array_equal(one, sync)


# ---- 2. hand-built trees ------------------------------------------------------------------------------------------------------
def _spheres(api, n):
    """n seeded spheres in the box [-3, 3] x [0.3, 3.3] x [-3, 3], radii 0.15 .. 0.4, four materials in turn"""
    rng = np.random.default_rng(1000 + n)
    mats = [api.Lambertian(api.SolidTexture(0.7, 0.3, 0.2)), api.Metal(api.SolidTexture(0.8, 0.8, 0.9), 0.1), api.Dielectric(1.5),
            api.Lambertian(api.SolidTexture(0.2, 0.5, 0.8))]
    out = []
    for k in range(n):
        c = (float(rng.uniform(-3, 3)), float(rng.uniform(0.3, 3.3)), float(rng.uniform(-3, 3)))
        out.append(api.Sphere(c, float(rng.uniform(0.15, 0.4)), mats[k % 4]))
    return out


def _cubes(api, n):
    rng = np.random.default_rng(2000 + n)
    mats = [api.Lambertian(api.SolidTexture(0.2 + 0.03 * k, 0.8 - 0.03 * k, 0.5)) for k in range(n)]
    out = []
    for k in range(n):
        lo = (float(rng.uniform(-3, 2.4)), float(rng.uniform(0.0, 2.7)), float(rng.uniform(-3, 2.4)))
        out.append(api.Cube(lo, tuple(c + float(rng.uniform(0.3, 0.6)) for c in lo), mats[k]))
    return out


TREES = [("spheres", n) for n in (2, 5, 16, 17, 64, 65, 300)] + [("cubes", 20)]


def _tree_scene(host, kind, n, wrapped, nx, ny):
    tree = host.BVHNode((_spheres if kind == "spheres" else _cubes)(host, n), 0.0, 1.0)
    if wrapped:
        tree = host.Traslate(host.Rotate(host.AXIS_Y, tree, 25.0), (0.4, 0.2, -0.3))
    world = host.HittableList()
    world.push(tree)
    low = host.lower(world)
    items = low.arrays()["items"]
    assert [it.kind for it in items] == [abi.ITEM_BVH] and items[0].alt_first >= 0 and items[0].xform_count == (2 if wrapped else 0)
    return low, scenes.set_camera(host, nx, ny, (9.0, 4.0, 7.0), (0.0, 1.5, 0.0), vertical_fov=40.0)


@pytest.mark.parametrize("wrapped", [False, True], ids=["bare", "traslate_rotate_y"])
@pytest.mark.parametrize("kind,n", TREES, ids=["%s%d" % t for t in TREES])
def test_hand_built_trees(host, device, kind, n, wrapped):
    nx, ny = 32, 32
    low, cam = _tree_scene(host, kind, n, wrapped, nx, ny)
    sc = device(low, cam, nx, ny, 2)
    got, kern, inst = sc.render(BASE)
    assert kern == abi.RTMI_KERNEL_WAVE_COOP and inst == INST_ONE_TREE
    sync, kern, _ = sc.render(BASE | abi.RTMI_FLAG_SYNC)
    assert kern == abi.RTMI_KERNEL_PERLANE
    assert np.count_nonzero(sync) > 0
    assert np.array_equal(got, sync)


# ---- 3. a wavefront of one to three rays ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [1, 3])
def test_tiny_images(host, device, nx):
    low, cam = _tree_scene(host, "spheres", 65, False, nx, 1)
    sc = device(low, cam, nx, 1, 1)
    got, kern, _ = sc.render(BASE)
    assert kern == abi.RTMI_KERNEL_WAVE_COOP
    sync, kern, _ = sc.render(BASE | abi.RTMI_FLAG_SYNC)
    assert kern == abi.RTMI_KERNEL_PERLANE
    assert np.count_nonzero(sync) > 0
    assert np.array_equal(got, sync)


# ---- 4. path signatures -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["final_scene", "random_spheres"])
def test_path_signatures(host, device, name):
    nx, ny = 32, 32
    cam, world = scenes_extra.build(host, name, nx, ny, seed=1)
    sc = device(host.lower(world), cam, nx, ny, 2)
    got, sg, kern, _ = sc.render(BASE | abi.RTMI_FLAG_PATH_SIG, sig=True)
    assert kern == abi.RTMI_KERNEL_WAVE_COOP
    sync, sg_sync, kern, _ = sc.render(BASE | abi.RTMI_FLAG_PATH_SIG | abi.RTMI_FLAG_SYNC, sig=True)
    assert kern == abi.RTMI_KERNEL_PERLANE
    assert np.count_nonzero(sync) > 0 and np.count_nonzero(sg_sync) > 0
    assert np.array_equal(got, sync)
    assert np.array_equal(sg, sg_sync)


# ---- 5. caller rays on the cooperative batch kernel ---------------------------------------------------------------------------
def _tree_of_eight(api):
    """8 spheres on the corners of a box, radius 0.6 (the tree of tests/test_coop_ray_constants.py)"""
    out = []
    for k in range(8):
        c = (2.0 * (k & 1) - 1.0, 2.0 * ((k >> 1) & 1) + 0.6, 2.0 * (k >> 2) - 1.0)
        out.append(api.Sphere(c, 0.6, api.Lambertian(api.SolidTexture(0.2 + 0.1 * k, 0.8 - 0.1 * k, 0.5))))
    return out


def _caller_rays():
    """Rays at the tree's spheres (1, 0.6, 1) and (-1, 2.6, -1), radius 0.6: per target and per direction length 2^-40, 1,
    2^40 — along +x grazing the top of the sphere (exactly tangent in fp32), one ulp below and above it, along -z through
    the centre, along +y from below, a diagonal tangent in the xz plane, a diagonal through the centre.  Then seeded rays
    of the three lengths from a ring around the tree.  t_min scales with 1 / length: the same distance for every length,
    and another value from lane to lane."""
    o, d, tmin = [], [], []
    for c, r in (((1.0, 0.6, 1.0), 0.6), ((-1.0, 2.6, -1.0), 0.6)):
        cx, cy, cz = (f32(v) for v in c)
        top = f32(cy + f32(r))
        for e in (-40, 0, 40):
            s = f32(2.0) ** e
            cases = [((cx - 10, top, cz), (s, 0, 0)), ((cx - 10, np.nextafter(top, f32(-np.inf)), cz), (s, 0, 0)),
                     ((cx - 10, np.nextafter(top, f32(np.inf)), cz), (s, 0, 0)), ((cx, cy, cz + 8), (0, 0, -s)),
                     ((cx, cy - 6, cz), (0, s, 0)),
                     ((cx - 4 + f32(r) * f32(0.70710677), cy, cz - 4 - f32(r) * f32(0.70710677)), (s, 0, s)),
                     ((cx - 3, cy - 3, cz - 3), (s, s, s))]
            for oo, dd in cases:
                o.append(oo); d.append(dd); tmin.append(f32(0.001) / s)
    rng = np.random.default_rng(12)
    for k in range(90):
        s = f32(2.0) ** (-40, 0, 40)[k % 3]
        ang = rng.uniform(0.0, 2.0 * np.pi)
        oo = np.array([6.0 * np.cos(ang), rng.uniform(0.2, 3.0), 6.0 * np.sin(ang)], f32)
        at = np.array([rng.uniform(-1.5, 1.5), rng.uniform(0.0, 3.0), rng.uniform(-1.5, 1.5)], f32)
        o.append(oo); d.append(((at - oo) * s).astype(f32)); tmin.append(f32(0.001) / s)
    return np.array(o, f32), np.array(d, f32), np.array(tmin, f32)


def test_caller_rays_on_the_batch_kernel(host):
    world = host.HittableList()
    world.push(host.BVHNode(_tree_of_eight(host), 0.0, 1.0))
    sc = host.lower(world).upload(0, nee=False)
    o, d, tmin = _caller_rays()
    assert o.shape[0] == 132 and o.shape[0] % 64 != 0
    a = np.sum(d.astype(np.float64) ** 2, axis=1)
    assert a.min() < 2.0 ** -75 and a.max() > 2.0 ** 75 and np.all(np.isfinite(d)) and np.any(np.sum(d != 0, axis=1) == 1)
    got = B._pair("caller rays", lambda **kw: sc.radiance(o, d, t_min=tmin, spp=4, estimator="plain", seed=SEED, samples=True, **kw),
                  B.RAD, flags=BASE)
    assert np.all(np.isfinite(got["samples"])) and np.count_nonzero(got["samples"]) > 0
    first = sc.trace(o, d, t_min=tmin, flags=abi.RTMI_FLAG_FAST_CULL)
    hit = np.asarray(first["hit"]).astype(bool)
    assert hit[3] and hit[4] and hit[6] and not hit[2]  # through the centre: a hit; one ulp above the sphere: none
    assert 0.3 < hit.mean() < 1.0


# ---- 6. the profiling build's round counters ------------------------------------------------------------------------------------
def test_profile_counts_quad_and_dense_rounds(host, device):
    import torch

    nx, ny = 64, 48
    cam, world = scenes_extra.build(host, "random_spheres", nx, ny, seed=1)
    sc = device(host.lower(world), cam, nx, ny, 4)
    prof = torch.zeros(64, dtype=torch.int64, device="cuda:0")
    p = default_params(nx, ny, 4, seed=SEED, flags=BASE | abi.RTMI_FLAG_PROFILE)
    p.prof = prof.data_ptr()
    lin, rgb = np.zeros((ny, nx, 3), f32), np.zeros((ny, nx, 3), np.uint8)
    st = abi.Stats()
    assert sc.lib.rtmi_render(sc.h, C.byref(sc.cam), C.byref(p), lin.ctypes.data, rgb.ctypes.data, None, C.byref(st)) == 0, sc.lib.rtmi_last_error()
    torch.cuda.synchronize()
    c = prof.cpu().numpy()
    rounds, quads, most = int(c[40:50].sum()), int(c[2 * 17]), int(c[2 * 19])  # csrc/rtmi_prof.hpp
    print("rounds %d, quad rounds %d, most entries entering a quad round %d" % (rounds, quads, most))
    assert quads > 0
    assert rounds - quads > 0
    assert 0 < most <= QUAD_MAX
    plain, _, _ = sc.render(BASE)
    assert np.array_equal(lin, plain)  # the profiling build renders the same image


# ---- 7. the overflow report ---------------------------------------------------------------------------------------------------
def test_overflow_knob_still_fails_loudly(host, device):
    low, cam = _tree_scene(host, "spheres", 65, False, 32, 32)
    sc = device(low, cam, 32, 32, 2)
    _, _, inst = sc.render(BASE | abi.RTMI_FLAG_TEST_OVERFLOW, expect=abi.RTMI_ERR_DEVICE)
    assert inst == INST_ONE_TREE
    assert b"overflow" in sc.lib.rtmi_last_error()
    good, _, inst = sc.render(BASE)  # and the next call is clean
    assert inst == INST_ONE_TREE and np.count_nonzero(good) > 0


# ---- 8. the bound of the 32-bit node offsets ----------------------------------------------------------------------------------
def test_scene_with_too_many_alt_nodes_is_refused(host):
    low, _ = _tree_scene(host, "spheres", 5, False, 8, 8)
    lib = abi.load_rtmi()
    desc = low.desc()
    assert 0 < desc.n_alt_nodes < (1 << 25)
    h = C.c_void_p()
    assert lib.rtmi_scene_create(C.byref(desc), 0, C.byref(h)) == 0, lib.rtmi_last_error()
    lib.rtmi_scene_destroy(h)
    desc.n_alt_nodes = 1 << 25  # refused on the count alone: the records behind the array's true end are never read
    h = C.c_void_p()
    assert lib.rtmi_scene_create(C.byref(desc), 0, C.byref(h)) == RTMI_ERR_UNSUPPORTED
    assert b"alternative tree nodes" in lib.rtmi_last_error() and not h.value
