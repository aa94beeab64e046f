"""The one-tree instantiation of the wave-cooperative kernel (csrc/rtmi_onetree.hip): selected exactly for
the scenes it was compiled for, bit for bit the general instantiation and the per-lane kernel, with and without a
spilling pool, loud about an overflow; every other scene or call falls back to the general instantiation.

Every comparison is np.array_equal on the float32 `linear` image of a 64x48 render at 4 spp, seed 42, under
RTMI_FLAG_FAST_CULL | RTMI_FLAG_SKY (final_scene is black without the sky, which would make equality vacuous: the
general kernel's image is asserted to have non-zero pixels)."""
import ctypes as C

import numpy as np
import pytest

import scenes_extra
from raytracing_rust_amd import abi, default_params, scenes

pytestmark = pytest.mark.gpu

NX, NY, NS, SEED = 64, 48, 4, 42
BASE = abi.RTMI_FLAG_FAST_CULL | abi.RTMI_FLAG_SKY
GENERAL = 4 << 8  # knob value 4 of flag bits 8..10: the general 4-wave instantiation
SMALL_POOL = 1 << 11  # a 256-entry LDS pool: the traversal stack spills to global memory all the time
REPORT_INST = 1 << 19  # RTMI_KNOB_REPORT_INST: rtmi_stats.kernel also carries the instantiation, in bits 8..15
INST_NONE, INST_GENERAL, INST_ONE_TREE = 0, 1, 2  # include/rtmi.h: RTMI_INST_*


class _Device:
    """A lowered scene on device 0 through the C ABI itself (rtmi_scene_create / rtmi_render): the rtmi_stats of a call
    that sets the report knob carry the instantiation (rtmi_stats_instantiation, include/rtmi.h; abi.stats_instantiation)."""

    def __init__(self, low, cam):
        self.lib, self.low, self.cam = abi.load_rtmi(), low, cam.lower()
        self.h = C.c_void_p()
        desc = low.desc()
        assert self.lib.rtmi_scene_create(C.byref(desc), 0, C.byref(self.h)) == 0, self.lib.rtmi_last_error()

    def close(self):
        self.lib.rtmi_scene_destroy(self.h)

    def render(self, flags, sig=False, expect=0, report=True):
        """-> (linear, RTMI_KERNEL_*, RTMI_INST_*); `expect`: the call's return code; report=False: without the knob, the
        raw rtmi_stats.kernel word in both places."""
        p = default_params(NX, NY, NS, seed=SEED, flags=flags | (REPORT_INST if report else 0))
        lin, rgb = np.zeros((NY, NX, 3), np.float32), np.zeros((NY, NX, 3), np.uint8)
        sg = np.zeros((NY, NX), np.uint64)
        st = abi.Stats()
        rc = self.lib.rtmi_render(self.h, C.byref(self.cam), C.byref(p), lin.ctypes.data, rgb.ctypes.data,
                                  sg.ctypes.data if sig else None, C.byref(st))
        assert rc == expect, (rc, self.lib.rtmi_last_error())
        if not report:
            return lin, st.kernel, st.kernel
        return lin, abi.stats_kernel(st), abi.stats_instantiation(st)


@pytest.fixture
def device():
    made = []

    def make(low, cam):
        made.append(_Device(low, cam))
        return made[-1]

    yield make
    for d in made:
        d.close()


def _cubes(api):
    mats = [api.Lambertian(api.SolidTexture(0.2 + 0.1 * k, 0.8 - 0.1 * k, 0.5)) for k in range(8)]
    out = []
    for k in range(8):
        lo = (2.0 * (k & 1) - 2.0, 2.0 * ((k >> 1) & 1), 2.0 * (k >> 2) - 2.0)
        out.append(api.Cube(lo, tuple(c + 1.2 for c in lo), mats[k]))
    return out


def _camera(api):
    return scenes.set_camera(api, NX, NY, (9.0, 4.0, 7.0), (0.0, 1.5, 0.0), vertical_fov=35.0)


@pytest.mark.parametrize("name", ["final_scene", "random_spheres"])
def test_selected_and_bit_identical(host, device, name):
    """Both scenes qualify (every BVH item gated, every medium a sphere's): the default call takes the one-tree
    instantiation, also with the spilling pool, and its image is the general instantiation's and the per-lane kernel's.
    The report knob changes neither the image nor, when it is off, the kernel word."""
    cam, world = scenes_extra.build(host, name, NX, NY, seed=1)
    sc = device(host.lower(world), cam)
    gen, kern, inst = sc.render(BASE | GENERAL)
    assert kern == abi.RTMI_KERNEL_WAVE_COOP and inst == INST_GENERAL
    assert np.count_nonzero(gen) > 0
    sync, kern, inst = sc.render(BASE | abi.RTMI_FLAG_SYNC)
    assert kern == abi.RTMI_KERNEL_PERLANE and inst == INST_NONE
    one, kern, inst = sc.render(BASE)
    assert kern == abi.RTMI_KERNEL_WAVE_COOP and inst == INST_ONE_TREE
    assert np.array_equal(one, gen)
    assert np.array_equal(one, sync)
    plain, word, _ = sc.render(BASE, report=False)  # without the knob rtmi_stats.kernel is RTMI_KERNEL_* alone, as ever
    assert word == abi.RTMI_KERNEL_WAVE_COOP and np.array_equal(plain, one)
    spill, kern, inst = sc.render(BASE | SMALL_POOL)
    assert kern == abi.RTMI_KERNEL_WAVE_COOP and inst == INST_ONE_TREE
    assert np.array_equal(spill, gen)
    assert np.array_equal(spill, sync)
    spill_gen, _, inst = sc.render(BASE | SMALL_POOL | GENERAL)
    assert inst == INST_GENERAL
    assert np.array_equal(spill_gen, gen)


def test_overflow_knob_reports_through_one_tree(host, device):
    """RTMI_FLAG_TEST_OVERFLOW: the one-tree instantiation keeps the kernel's overflow report, the call fails loudly."""
    cam, world = scenes_extra.build(host, "final_scene", NX, NY, seed=1)
    sc = device(host.lower(world), cam)
    _, _, inst = sc.render(BASE | abi.RTMI_FLAG_TEST_OVERFLOW, expect=abi.RTMI_ERR_DEVICE)
    assert inst == INST_ONE_TREE
    assert b"overflow" in sc.lib.rtmi_last_error()
    assert sc.lib.rtmi_scene_status(sc.h, None) == 0  # reported once
    good, _, inst = sc.render(BASE)  # and the next call is clean
    assert inst == INST_ONE_TREE and np.count_nonzero(good) > 0


@pytest.mark.parametrize("case", ["ref_tree", "path_sig"])
def test_calls_that_fall_back(host, device, case):
    """final_scene qualifies as a scene; a call that walks the reference-topology tree or accumulates path signatures
    does not: the general instantiation, same image as the per-lane kernel."""
    cam, world = scenes_extra.build(host, "final_scene", NX, NY, seed=1)
    sc = device(host.lower(world), cam)
    sync, _, _ = sc.render(BASE | abi.RTMI_FLAG_SYNC)
    assert np.count_nonzero(sync) > 0
    if case == "ref_tree":
        got, kern, inst = sc.render(BASE | abi.RTMI_FLAG_REF_TREE)
    else:
        got, kern, inst = sc.render(BASE, sig=True)
    assert kern == abi.RTMI_KERNEL_WAVE_COOP and inst == INST_GENERAL
    assert np.array_equal(got, sync)


def test_cube_bounded_medium_falls_back(host, device):
    """A gated BVH of 8 cubes and a ConstantMedium whose boundary is a cube: the medium needs the general boundary
    queries, so the scene does not qualify although its only tree is gated."""
    world = host.HittableList()
    world.push(host.BVHNode(_cubes(host), 0.0, 1.0))
    world.push(host.ConstantMedium(host.Cube((-3.0, -0.5, -3.0), (3.0, 4.0, 3.0), host.Dielectric(1.5)), 0.3,
                                   host.SolidTexture(0.9, 0.9, 0.9)))
    low = host.lower(world)
    items = low.arrays()["items"]
    assert [it.kind for it in items] == [abi.ITEM_BVH, abi.ITEM_LIST] and items[0].alt_first >= 0
    sc = device(low, _camera(host))
    got, kern, inst = sc.render(BASE)
    assert kern == abi.RTMI_KERNEL_WAVE_COOP and inst == INST_GENERAL
    sync, _, _ = sc.render(BASE | abi.RTMI_FLAG_SYNC)
    assert np.count_nonzero(sync) > 0
    assert np.array_equal(got, sync)


def test_bvh_without_alternative_tree_falls_back(host, device):
    """Two BVH items of which one has no alternative tree — expressible through the host API: a BVHNode over a single
    primitive gets none (the lowering builds one over two primitives or more).  The scene is rejected like the others."""
    world = host.HittableList()
    world.push(host.BVHNode(_cubes(host), 0.0, 1.0))
    world.push(host.BVHNode([host.Sphere((0.0, 5.0, 0.0), 1.0, host.Lambertian(host.SolidTexture(0.5, 0.5, 0.5)))], 0.0, 1.0))
    low = host.lower(world)
    items = low.arrays()["items"]
    assert [it.kind for it in items] == [abi.ITEM_BVH, abi.ITEM_BVH]
    assert items[0].alt_first >= 0 and items[1].alt_first < 0
    sc = device(low, _camera(host))
    got, kern, inst = sc.render(BASE)
    assert kern == abi.RTMI_KERNEL_WAVE_COOP and inst == INST_GENERAL
    sync, _, _ = sc.render(BASE | abi.RTMI_FLAG_SYNC)
    assert np.count_nonzero(sync) > 0
    assert np.array_equal(got, sync)
