"""Per-ray constants of the wave-cooperative kernel: 1/(d.d) is evaluated once per ray in the item loop
and travels to the traversal's workers in the ray context, in the word that held the wave-uniform t_min.  The same
operations on the same values, so every comparison is np.array_equal on float32 output.

 1. final_scene and random_spheres, 64x48 at 4 spp, seed 42, FAST_CULL | SKY: the default call reports the one-tree
    instantiation; its image, the general instantiation's (knob value 4) and the per-lane kernel's (RTMI_FLAG_SYNC) are
    one image, non-zero, also under the small-pool knob (bit 11);
 2. cornell_smoke and two_perlin_spheres, 64x64 at 4 spp: the lean instantiation (no tree; a medium's draw, the camera's
    draws) equals the per-lane kernel;
 3. hand-built scenes, a BVH of 8 spheres and a list of 2 spheres, each under Traslate, Rotate(Y), Traslate(Rotate(Y)),
    Rotate(X) and a chain of three: the default call equals RTMI_FLAG_SYNC.  The instantiation report says one-tree for all
    five: the per-scene transform-pair trait (part C of §39), which would have sent the last two to the general
    instantiation, measured slower and is not in the library (profiles/rayconst/part_C_transform_pair.patch), so a
    chain's shape does not enter the choice;
 4. radiance queries on the cooperative batch kernel (include/rtmi_batch_coop.h) for caller rays whose directions have
    lengths 2^-40, 1 and 2^40 — d.d and its reciprocal at 2^-80 and 2^80 — axis-aligned, tangent and nearly tangent to a
    top-level sphere and to a sphere of the BVH: bitwise the per-lane radiance query."""
import ctypes as C

import numpy as np
import pytest

import scenes_extra
import test_gpu_batch_coop as B
from raytracing_rust_amd import abi, default_params, scenes

pytestmark = pytest.mark.gpu

NS, SEED = 4, 42
BASE = abi.RTMI_FLAG_FAST_CULL | abi.RTMI_FLAG_SKY
GENERAL = 4 << 8  # knob value 4 of flag bits 8..10: the general 4-wave instantiation
SMALL_POOL = 1 << 11  # a 256-entry LDS pool: the traversal stack spills to global memory all the time
REPORT_INST = 1 << 19  # RTMI_KNOB_REPORT_INST: rtmi_stats.kernel also carries the instantiation, in bits 8..15
INST_NONE, INST_GENERAL, INST_ONE_TREE = 0, 1, 2  # include/rtmi.h: RTMI_INST_*
f32 = np.float32


class _Device:
    """A lowered scene on device 0 through the C ABI (rtmi_scene_create / rtmi_render) with the report knob set."""

    def __init__(self, low, cam, nx, ny):
        self.lib, self.low, self.cam, self.nx, self.ny = abi.load_rtmi(), low, cam.lower(), nx, ny
        self.h = C.c_void_p()
        desc = low.desc()
        assert self.lib.rtmi_scene_create(C.byref(desc), 0, C.byref(self.h)) == 0, self.lib.rtmi_last_error()

    def close(self):
        self.lib.rtmi_scene_destroy(self.h)

    def render(self, flags):
        """-> (linear, RTMI_KERNEL_*, RTMI_INST_*)"""
        p = default_params(self.nx, self.ny, NS, seed=SEED, flags=flags | REPORT_INST)
        lin, rgb = np.zeros((self.ny, self.nx, 3), f32), np.zeros((self.ny, self.nx, 3), np.uint8)
        st = abi.Stats()
        rc = self.lib.rtmi_render(self.h, C.byref(self.cam), C.byref(p), lin.ctypes.data, rgb.ctypes.data, None, C.byref(st))
        assert rc == 0, (rc, self.lib.rtmi_last_error())
        return lin, abi.stats_kernel(st), abi.stats_instantiation(st)


@pytest.fixture
def device():
    made = []

    def make(low, cam, nx, ny):
        made.append(_Device(low, cam, nx, ny))
        return made[-1]

    yield make
    for d in made:
        d.close()


# ---- 1. the headline scenes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["final_scene", "random_spheres"])
def test_one_tree_general_and_perlane_are_one_image(host, device, name):
    nx, ny = 64, 48
    cam, world = scenes_extra.build(host, name, nx, ny, seed=1)
    sc = device(host.lower(world), cam, nx, ny)
    one, kern, inst = sc.render(BASE)
    assert kern == abi.RTMI_KERNEL_WAVE_COOP and inst == INST_ONE_TREE
    assert np.count_nonzero(one) > 0
    gen, kern, inst = sc.render(BASE | GENERAL)
    assert kern == abi.RTMI_KERNEL_WAVE_COOP and inst == INST_GENERAL
    sync, kern, inst = sc.render(BASE | abi.RTMI_FLAG_SYNC)
    assert kern == abi.RTMI_KERNEL_PERLANE and inst == INST_NONE
    assert np.array_equal(one, gen)
    assert np.array_equal(one, sync)
    spill, kern, inst = sc.render(BASE | SMALL_POOL)
    assert kern == abi.RTMI_KERNEL_WAVE_COOP and inst == INST_ONE_TREE
    spill_gen, _, inst = sc.render(BASE | SMALL_POOL | GENERAL)
    assert inst == INST_GENERAL
    assert np.array_equal(spill, sync)
    assert np.array_equal(spill_gen, sync)


# ---- 2. the lean instantiation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_smoke", "two_perlin_spheres"])
def test_lean_instantiation_equals_perlane(host, device, name):
    nx, ny = 64, 64
    cam, world = scenes.build(host, name, nx, ny, seed=1)
    sc = device(host.lower(world), cam, nx, ny)
    got, kern, inst = sc.render(BASE)
    assert kern == abi.RTMI_KERNEL_WAVE_COOP and inst == INST_GENERAL
    sync, kern, _ = sc.render(BASE | abi.RTMI_FLAG_SYNC)
    assert kern == abi.RTMI_KERNEL_PERLANE
    assert np.count_nonzero(sync) > 0
    assert np.array_equal(got, sync)


# ---- 3. transform chains ------------------------------------------------------------------------------------------------------
def _tree_spheres(api):
    """8 spheres on the corners of a box, radius 0.6, one material each"""
    out = []
    for k in range(8):
        c = (2.0 * (k & 1) - 1.0, 2.0 * ((k >> 1) & 1) + 0.6, 2.0 * (k >> 2) - 1.0)
        out.append(api.Sphere(c, 0.6, api.Lambertian(api.SolidTexture(0.2 + 0.1 * k, 0.8 - 0.1 * k, 0.5))))
    return out


def _list_spheres(api):
    lst = api.HittableList()
    lst.push(api.Sphere((0.0, 1.6, 0.0), 0.5, api.Metal(api.SolidTexture(0.8, 0.8, 0.9), 0.1)))
    lst.push(api.Sphere((0.0, -100.0, 0.0), 100.0, api.Lambertian(api.SolidTexture(0.5, 0.5, 0.5))))
    return lst


CHAINS = {
    "traslate": lambda api, o: api.Traslate(o, (0.4, 0.2, -0.3)),
    "rotate_y": lambda api, o: api.Rotate(api.AXIS_Y, o, 25.0),
    "traslate_rotate_y": lambda api, o: api.Traslate(api.Rotate(api.AXIS_Y, o, 25.0), (0.4, 0.2, -0.3)),
    "rotate_x": lambda api, o: api.Rotate(api.AXIS_X, o, 10.0),
    "three": lambda api, o: api.Traslate(api.Rotate(api.AXIS_Y, api.Rotate(api.AXIS_Z, o, 8.0), 25.0), (0.4, 0.2, -0.3)),
}


@pytest.mark.parametrize("chain", list(CHAINS))
def test_transform_chains(host, device, chain):
    nx, ny = 64, 48
    world = host.HittableList()
    world.push(CHAINS[chain](host, host.BVHNode(_tree_spheres(host), 0.0, 1.0)))
    world.push(CHAINS[chain](host, _list_spheres(host)))
    low = host.lower(world)
    items = low.arrays()["items"]
    assert [it.kind for it in items] == [abi.ITEM_BVH, abi.ITEM_LIST] and items[0].alt_first >= 0
    assert all(it.xform_count == (3 if chain == "three" else 2 if chain == "traslate_rotate_y" else 1) for it in items)
    cam = scenes.set_camera(host, nx, ny, (7.0, 3.5, 6.0), (0.0, 1.2, 0.0), vertical_fov=35.0)
    sc = device(low, cam, nx, ny)
    got, kern, inst = sc.render(BASE)
    assert kern == abi.RTMI_KERNEL_WAVE_COOP and inst == INST_ONE_TREE
    sync, kern, _ = sc.render(BASE | abi.RTMI_FLAG_SYNC)
    assert kern == abi.RTMI_KERNEL_PERLANE
    assert np.count_nonzero(sync) > 0
    assert np.array_equal(got, sync)
    gen, _, inst = sc.render(BASE | GENERAL)
    assert inst == INST_GENERAL and np.array_equal(gen, sync)


# ---- 4. extreme caller rays on the cooperative batch kernel ---------------------------------------------------------------------
def _extreme_rays():
    """Rays at the top-level sphere (0, 1.6, 0) r 0.5 and at the tree's sphere (1, 0.6, 1) r 0.6 of the scene of part 3
    without transforms: per target and per direction length 2^-40, 1, 2^40 — along +x grazing the top of the sphere
    (exactly tangent in fp32: the origin's y is centre + radius), one ulp below and above it, along -z through the centre,
    along +y from below, a diagonal tangent in the xz plane, and a diagonal through the centre.  Then seeded rays of the
    three lengths from a ring around the scene.  The first segment's t_min scales with 1 / length, so that it means the
    same distance for every length."""
    o, d, tmin = [], [], []
    for c, r in (((0.0, 1.6, 0.0), 0.5), ((1.0, 0.6, 1.0), 0.6)):
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
    rng = np.random.default_rng(11)
    for k in range(90):
        s = f32(2.0) ** (-40, 0, 40)[k % 3]
        ang = rng.uniform(0.0, 2.0 * np.pi)
        oo = np.array([6.0 * np.cos(ang), rng.uniform(0.2, 3.0), 6.0 * np.sin(ang)], f32)
        at = np.array([rng.uniform(-1.5, 1.5), rng.uniform(0.0, 2.5), rng.uniform(-1.5, 1.5)], f32)
        o.append(oo); d.append(((at - oo) * s).astype(f32)); tmin.append(f32(0.001) / s)
    return np.array(o, f32), np.array(d, f32), np.array(tmin, f32)


def test_extreme_caller_rays_on_the_batch_kernel(host):
    world = host.HittableList()
    world.push(host.BVHNode(_tree_spheres(host), 0.0, 1.0))
    world.push(_list_spheres(host))
    sc = host.lower(world).upload(0, nee=False)
    o, d, tmin = _extreme_rays()
    assert o.shape[0] == 132 and o.shape[0] % 64 != 0
    a = np.sum(d.astype(np.float64) ** 2, axis=1)
    assert a.min() < 2.0 ** -75 and a.max() > 2.0 ** 75 and np.all(np.isfinite(d)) and np.any(np.sum(d != 0, axis=1) == 1)
    got = B._pair("extreme rays", lambda **kw: sc.radiance(o, d, t_min=tmin, spp=4, estimator="plain", seed=SEED, samples=True, **kw),
                  B.RAD, flags=BASE)
    assert np.all(np.isfinite(got["samples"])) and np.count_nonzero(got["samples"]) > 0
    first = sc.trace(o, d, t_min=tmin, flags=abi.RTMI_FLAG_FAST_CULL)
    hit = np.asarray(first["hit"]).astype(bool)
    assert hit[3] and hit[4] and hit[6] and not hit[2]  # through the centre: a hit; one ulp above the sphere: none
    assert 0.3 < hit.mean() < 1.0


# ---- 5. Philox with block-local round keys --------------------------------------------------------------------------------------
def test_philox_known_answers_with_block_local_keys():
    """The Random123 known answers through the form whose round keys are formed inside the block (philox<true>,
    csrc/rtmi_rng.hpp): rtmi_probe_philox evaluates it for a wavefront whose cases share one key — 64 copies of a vector —
    and the default form otherwise (tests/test_math_contract.py sends the three vectors in one wavefront)."""
    from test_philox import KAT

    lib = abi.load_rtmi()
    for ctr, key, want in KAT:
        c = np.tile(np.array(ctr, np.uint32), (64, 1))
        k = np.tile(np.array(key, np.uint32), (64, 1))
        out = np.zeros((64, 4), np.uint32)
        assert lib.rtmi_probe_philox(c.ctypes.data, k.ctypes.data, out.ctypes.data, 64) == 0
        assert out.tolist() == [list(want)] * 64
