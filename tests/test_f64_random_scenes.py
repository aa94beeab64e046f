"""The random compositions (tests/scenes_random.py) as test scenes of the f64 render mode (include/rtmi_f64.h), without
a GPU: which seeds the mode supports, what the two scene sets cover, that ExactOps builds the same world through the host
mirror and through the f64 oracle, and that the double planes of every scene round to the fp32 description.

Two sets (tests/test_gpu_f64_random.py renders them and takes its seed lists from the constants below):
  * the EXACT set: exact_ops=True — nothing but + - * / and sqrt at render time (and the sign of a checker's sines), so
    the device is held to the f64 oracle bit for bit;
  * the FULL set: the scenes as they are, with sin, log, atan2 and asin — held to the project's ULP-born bounds."""
import numpy as np
import pytest

import scenes_random
from raytracing_rust_amd import abi
from raytracing_rust_amd.host import HostError
from test_f64_mode_abi import _Recorder

SEEDS = list(range(1, 25))
# rtmi_render_f64 refuses DEFERRED, NESTED_MEDIUM and LISTSCAN items (include/rtmi_f64.h)
UNSUPPORTED_ITEMFLAGS = (abi.ITEMFLAG_DEFERRED | abi.ITEMFLAG_NESTED_MEDIUM | abi.ITEMFLAG_LISTSCAN_BEGIN
                         | abi.ITEMFLAG_LISTSCAN_MEMBER | abi.ITEMFLAG_LISTSCAN_END)
assert UNSUPPORTED_ITEMFLAGS == 8 | 16 | 32 | 64 | 128
# instanced=True under exact_ops: seeds 2 and 4 keep an instanced subtree (a DEFERRED BVH item), seed 9 gets a BVHNode
# inside a list leaf once its medium is replaced by the boundary, which the lowering refuses
EXACT_INSTANCED_UNSUPPORTED = [2, 4]
EXACT_INSTANCED_NOT_LOWERED = [9]
EXACT_INSTANCED = [s for s in SEEDS if s not in EXACT_INSTANCED_UNSUPPORTED + EXACT_INSTANCED_NOT_LOWERED]
# instanced=True as it is (media in BVHs, nested media, list scans): the supported ones among seeds 1-60
FULL_INSTANCED = [1, 3, 5, 10, 12, 19, 20, 22, 24, 25, 30, 36, 39, 41, 42, 43, 45, 47, 48, 51, 53, 54, 57, 59]
EXACT_SET = [(s, False) for s in SEEDS] + [(s, True) for s in EXACT_INSTANCED]  # (seed, instanced)
FULL_SET = [(s, False) for s in SEEDS] + [(s, True) for s in FULL_INSTANCED]
# the first scenes of the exact set whose lowered materials hold a Dielectric / a Metal of fuzz >= 1
GLASS_CASE = (1, False)
METAL_CASE = (1, False)
# both picks are seed 1 plain, so the depth and pass tests of the GPU tier add the next scene with such a metal
DEPTH_CASES = [(1, False), (2, False)]
PLANE_SHIFT = 8  # RTMI_PRIMFLAG_PLANE_SHIFT of include/rtmi.h
FLT_MAX = 3.4028234663852886e38


def case_id(case):
    return "%d-%s" % (case[0], "instanced" if case[1] else "plain")


def _lowered(host, seed, instanced, exact_ops):
    _cam, world = scenes_random.build(host, seed, 43, 21, instanced=instanced, exact_ops=exact_ops)
    return host.lower(world)


def _supported(host, seed, instanced, exact_ops):
    return all(it.flags & UNSUPPORTED_ITEMFLAGS == 0 for it in _lowered(host, seed, instanced, exact_ops).arrays()["items"])


def test_supported_seeds(host):
    assert len(EXACT_SET) == 45 and len(FULL_SET) == 48
    for exact_ops in (False, True):
        assert [s for s in SEEDS if _supported(host, s, False, exact_ops)] == SEEDS
    unsupported, not_lowered = [], []
    for s in SEEDS:
        try:
            if not _supported(host, s, True, True):
                unsupported.append(s)
        except HostError:
            not_lowered.append(s)
    assert unsupported == EXACT_INSTANCED_UNSUPPORTED and not_lowered == EXACT_INSTANCED_NOT_LOWERED
    assert [s for s in range(1, 61) if _supported(host, s, True, False)] == FULL_INSTANCED


def _census(host, cases, exact_ops):
    c = {"prim_types": set(), "planes": set(), "xf_kinds": set(), "mat_kinds": set(), "tex_kinds": set(), "prims_2xf": 0,
         "scenes_with_2xf": 0, "flipped_prims": 0, "flipped_items": 0, "bvh_items": 0, "scenes_with_media": 0, "scenes_with_outer_media": 0,
         "glass": [], "metal_fuzz_ge_1": []}
    for seed, instanced in cases:
        a = _lowered(host, seed, instanced, exact_ops).arrays()
        for m in a["prim_meta"]:
            c["prim_types"].add(m.type)
            if m.type == abi.PRIM_RECT:
                c["planes"].add((m.flags >> PLANE_SHIFT) & 3)
            c["prims_2xf"] += ((m.flags >> abi.RTMI_PRIMFLAG_XF_COUNT_SHIFT) & 15) >= 2
            c["flipped_prims"] += m.flags & 1
        c["scenes_with_2xf"] += any(((m.flags >> abi.RTMI_PRIMFLAG_XF_COUNT_SHIFT) & 15) >= 2 for m in a["prim_meta"])
        c["xf_kinds"] |= {x.kind for x in a["xforms"]}
        c["mat_kinds"] |= {m.kind for m in a["materials"]}
        c["tex_kinds"] |= {t.kind for t in a["textures"]}
        c["flipped_items"] += sum(it.flags & abi.ITEMFLAG_FLIP for it in a["items"])
        c["bvh_items"] += sum(it.kind == abi.ITEM_BVH for it in a["items"])
        media = [it for it in a["items"] if it.flags & abi.ITEMFLAG_MEDIUM]
        c["scenes_with_media"] += bool(media)
        c["scenes_with_outer_media"] += any((it.flags >> abi.RTMI_ITEMFLAG_MEDIUM_OUTER_SHIFT) & 15 for it in media)
        if any(m.kind == abi.MAT_DIELECTRIC for m in a["materials"]):
            c["glass"].append((seed, instanced))
        if any(m.kind == abi.MAT_METAL and m.param >= 1.0 for m in a["materials"]):
            c["metal_fuzz_ge_1"].append((seed, instanced))
    return c


def test_exact_set_covers_the_geometry_and_the_materials(host):
    c = _census(host, EXACT_SET, True)
    print({k: v for k, v in c.items() if not isinstance(v, list)})
    assert c["prim_types"] == {abi.PRIM_SPHERE, abi.PRIM_MSPHERE, abi.PRIM_RECT, abi.PRIM_CUBE}
    assert c["planes"] == {0, 1, 2}
    assert c["xf_kinds"] >= {abi.XF_TRANSLATE, abi.XF_ROTATE_X, abi.XF_ROTATE_Y, abi.XF_ROTATE_Z}
    # counted: primitives with two or more own transforms in 19 scenes (118 primitives), 302 flipped primitives, 51
    # flipped items, 71 BVH items
    assert c["scenes_with_2xf"] >= 10 and c["flipped_prims"] >= 50 and c["flipped_items"] >= 10 and c["bvh_items"] >= 30
    assert c["mat_kinds"] == {abi.MAT_LAMBERTIAN, abi.MAT_METAL, abi.MAT_DIELECTRIC, abi.MAT_DIFFUSE_LIGHT}
    # no sin beyond a checker's sign, no log, no atan2 / asin
    assert c["tex_kinds"] <= {abi.TEX_SOLID, abi.TEX_CHECKER} and c["scenes_with_media"] == 0
    assert c["glass"][0] == GLASS_CASE and c["metal_fuzz_ge_1"][0] == METAL_CASE
    assert DEPTH_CASES == [GLASS_CASE, c["metal_fuzz_ge_1"][1]]


def test_full_set_covers_the_media_and_the_textures(host):
    c = _census(host, FULL_SET, False)
    print({k: v for k, v in c.items() if not isinstance(v, list)})
    # counted: media in 37 scenes, with outer wrappers in 7
    assert c["scenes_with_media"] >= 30 and c["scenes_with_outer_media"] >= 5
    assert c["tex_kinds"] == {abi.TEX_SOLID, abi.TEX_CHECKER, abi.TEX_NOISE, abi.TEX_IMAGE}
    assert abi.MAT_ISOTROPIC in c["mat_kinds"]


@pytest.mark.parametrize("case", EXACT_SET, ids=case_id)
def test_exact_ops_mirror_equals_f64_oracle(host, orc64, case):
    """ExactOps builds the same world on both sides: one row of the mirror's f64 evaluation equals the f64 oracle bitwise
    (as test_random_scenes.py::test_mirror_equals_f64_oracle_and_lowers holds the scenes as they are)."""
    seed, instanced = case
    nx, ny, row = 16, 12, 5
    cam, world = scenes_random.build(host, seed, nx, ny, instanced=instanced, exact_ops=True)
    camo, worldo = scenes_random.build(orc64, seed, nx, ny, instanced=instanced, exact_ops=True)
    ref = orc64.render(camo, worldo, nx, ny, 1, seed=42, rows=(row, row + 1))
    for i in range(nx):
        c = host.color_sample(cam, world, nx, ny, i, ny - 1 - row, 0, seed=42)
        assert np.array_equal(c, ref["mean"][row, i]), (case, i)
    orc64.free_all()


def _to_f32(a):
    """one rounding to nearest, saturating at +-FLT_MAX: a box of a Rotate is the whole f64 space (rotate.rs:36-37), and
    the fp32 lowering keeps such a coordinate at +-FLT_MAX (sat_f32 of the host lowering)"""
    return np.clip(a, -FLT_MAX, FLT_MAX).astype(np.float32)


@pytest.mark.parametrize("exact_ops,case", [(True, c) for c in EXACT_SET] + [(False, c) for c in FULL_SET],
                         ids=lambda v: ("exact" if v else "full") if isinstance(v, bool) else case_id(v))
def test_wide_lowering_of_random_scenes_rounds_to_the_fp32_description(host, orc64, exact_ops, case):
    """The invariants of test_f64_mode_abi.py::test_wide_lowering_matches_the_f64_oracle on the double planes of a random
    composition: instanced primitives' own xforms, prim_dt, and the two planes that test never reads, nodes and prim_gate.
    No plane of the fp32 lowering is widened outward: node boxes, gates and root boxes are rounded once to nearest
    (saturating at +-FLT_MAX) from the same double box that the wide plane keeps, so equality after rounding is asserted
    for all of them, not containment."""
    seed, instanced = case
    hrec, orec = _Recorder(host), _Recorder(orc64)
    _cam, world = scenes_random.build(hrec, seed, 43, 21, instanced=instanced, exact_ops=exact_ops)
    scenes_random.build(orec, seed, 43, 21, instanced=instanced, exact_ops=exact_ops)
    sc = host.lower(world)
    a32, a64 = sc.arrays(), sc.arrays_f64()
    meta = a32["prim_meta"]
    assert np.array_equal(a64["prim_a"].astype(np.float32), a32["prim_a"])
    # plane B of a MovingSphere: fp32 keeps float(c1) - float(c0), the wide plane the f64 difference c1 - c0
    moving = np.array([m.type == abi.PRIM_MSPHERE for m in meta], bool)
    assert np.array_equal(a64["prim_b"][~moving].astype(np.float32), a32["prim_b"][~moving])
    assert np.array_equal(a64["prim_b"][moving, 3].astype(np.float32), a32["prim_b"][moving, 3])
    assert np.allclose(a64["prim_b"][moving, :3], a32["prim_b"][moving, :3], rtol=0.0, atol=1e-5)
    # prim_dt: time1 - time0 of a MovingSphere as built (1 - 0 here), 1 elsewhere; a static sphere that a BVH with moving
    # spheres turns into a moving one stands still (c1 - c0 = 0)
    assert a64["prim_dt"].shape == (len(meta),) and np.all(a64["prim_dt"] == 1.0)
    xf32 = np.array([[x.x, x.y, x.z] for x in a32["xforms"]], np.float32).reshape(-1, 3)
    assert a64["xforms"].shape == (len(a32["xforms"]), 4)
    assert np.array_equal(a64["xforms"][:, :3].astype(np.float32), xf32) and np.all(a64["xforms"][:, 3] == 0.0)
    for m in meta:  # every instanced primitive's own chain lies inside the plane
        cnt = (m.flags >> abi.RTMI_PRIMFLAG_XF_COUNT_SHIFT) & 15
        assert cnt == 0 or (m.flags >> abi.RTMI_PRIMFLAG_XF_FIRST_SHIFT) + cnt <= len(a64["xforms"])
    assert np.array_equal(a64["material_param"].astype(np.float32), np.array([m.param for m in a32["materials"]], np.float32))
    assert np.array_equal(a64["texture_f"].astype(np.float32),
                          np.array([[t.f0, t.f1, t.f2, t.f3] for t in a32["textures"]], np.float32).reshape(-1, 4))
    # nodes and gates: the double box, rounded once
    n32 = np.array([list(n.lmin) + list(n.lmax) + list(n.rmin) + list(n.rmax) for n in a32["nodes"]], np.float32).reshape(-1, 12)
    assert a64["nodes"].shape == n32.shape and np.array_equal(_to_f32(a64["nodes"]), n32)
    assert a64["prim_gate"].shape == a32["prim_gate"].shape == (len(meta), 8)
    assert np.array_equal(_to_f32(a64["prim_gate"]), a32["prim_gate"])
    # BVH items: the root box is the bounding_box of one of the oracle's BVHNodes bit for bit, and rounds to the item's
    oracle_boxes = {np.concatenate(orc64.bounding_box(n)).astype(np.float64).tobytes() for n in orec.bvh}
    for k, it in enumerate(a32["items"]):
        if it.kind == abi.ITEM_BVH:
            assert a64["item_root"][k].tobytes() in oracle_boxes, (case, k)
            assert np.array_equal(_to_f32(a64["item_root"][k]), np.array(list(it.root_min) + list(it.root_max), np.float32))
    # media: -(1/density) in double, exactly (density 0 is drawn too: -inf), and it rounds to the item's
    with np.errstate(divide="ignore"):
        want = {float(-(np.float64(1.0) / np.float64(d))) for d in hrec.density}
    media = [k for k, it in enumerate(a32["items"]) if it.flags & abi.ITEMFLAG_MEDIUM]
    assert {float(a64["item_neg_inv_density"][k]) for k in media} == want and (not exact_ops or not media)
    for k in media:
        assert np.float32(a64["item_neg_inv_density"][k]) == np.float32(a32["items"][k].neg_inv_density)
    orc64.free_all()


def top_level_ties_world(api):
    """Exact ties inside the scan of a nested list at the top level (hittable.rs:37-47), where the shrinking t_max itself
    decides and no tree fold does: two coincident rects (the LAST wins: Rect reports at t == t_max, rect.rs:47), two
    coincident spheres (the FIRST wins: Sphere reports only below t_max, sphere.rs:44), and a rect on the front face of a
    cube pushed before it (the rect wins).  Every winner emits its own colour, so it is in the pixels.  The list sits in a
    Traslate, so it stays one item."""
    red = api.DiffuseLight(api.SolidTexture(4.0, 0.2, 0.2))
    green = api.DiffuseLight(api.SolidTexture(0.2, 4.0, 0.2))
    blue = api.DiffuseLight(api.SolidTexture(0.2, 0.2, 4.0))
    grey = api.Lambertian(api.SolidTexture(0.7, 0.7, 0.7))
    lst = api.HittableList()
    lst.push(api.Rect(api.PLANE_XY, -2.0, 0.0, -1.0, 1.0, 0.0, blue))
    lst.push(api.Rect(api.PLANE_XY, -2.0, 0.0, -1.0, 1.0, 0.0, green))
    lst.push(api.Sphere((0.0, 0.5, 0.0), 0.5, red))
    lst.push(api.Sphere((0.0, 0.5, 0.0), 0.5, green))
    lst.push(api.Cube((1.0, 0.0, -0.5), (2.0, 1.0, 0.5), grey))
    lst.push(api.Rect(api.PLANE_XY, 1.0, 0.0, 2.0, 1.0, 0.5, blue))
    w = api.HittableList()
    w.push(api.Sphere((0.0, 9.0, 2.0), 3.0, api.DiffuseLight(api.SolidTexture(4.0, 4.0, 4.0))))
    w.push(api.Sphere((0.0, -100.0, 0.0), 100.0, grey))
    w.push(api.Traslate(lst, (0.25, 0.0, 0.0)))
    return w


TIES_CAMERA = (((0.5, 1.2, 6.0), (0.3, 0.6, 0.0), (0.0, 1.0, 0.0), 40.0), (0.0, 6.0, 0.0, 1.0))  # before / after the aspect


def test_top_level_ties_world_is_one_scanned_item_and_shows_the_winners(host, orc64):
    nx, ny, ns = 48, 32, 2
    wh, wo = top_level_ties_world(host), top_level_ties_world(orc64)
    cams = [api.Camera(*TIES_CAMERA[0], nx / ny, *TIES_CAMERA[1]) for api in (host, orc64)]
    a = host.lower(wh).arrays()
    scan = [it for it in a["items"] if it.kind == abi.ITEM_LIST and it.count == 6]
    assert len(scan) == 1 and scan[0].xform_count == 1 and scan[0].flags & UNSUPPORTED_ITEMFLAGS == 0
    types = [a["prim_meta"][scan[0].first + k].type for k in range(6)]
    assert types == [abi.PRIM_RECT, abi.PRIM_RECT, abi.PRIM_SPHERE, abi.PRIM_SPHERE, abi.PRIM_CUBE, abi.PRIM_RECT]  # scan order
    ref = orc64.render(cams[1], wo, nx, ny, ns, seed=42, flags=2)  # THROUGHPUT_FORM
    lin = ref["mean"]
    green, red, blue = lin[..., 1] > 3.0, lin[..., 0] > 3.0, lin[..., 2] > 3.0
    cols = np.arange(nx)[None, :] * np.ones((ny, 1), int)
    # left: the rect pair shows green (the later one), never blue; middle: the sphere pair red (the first); right: the
    # rect on the cube's face blue
    assert green.sum() > 10 and red.sum() > 10 and blue.sum() > 10
    assert cols[green].max() < cols[red].min() and cols[red].max() < cols[blue].min()
    for row in (10, 20):
        for i in range(nx):
            c = host.color_sample(cams[0], wh, nx, ny, i, ny - 1 - row, 0, seed=42)
            one = orc64.render(cams[1], wo, nx, ny, 1, seed=42, rows=(row, row + 1))["mean"][row, i]
            assert np.array_equal(c, one), (row, i)
    orc64.free_all()


def test_prim_dt_is_the_span_of_the_sphere_times(host):
    """prim_dt = time1 - time0 of a MovingSphere as it was built (the divisor of sphere.rs:115-118), 1 on everything else —
    also on the static spheres that a BVH with a moving sphere lowers as moving ones"""
    from test_random_scenes import _bvh_world

    host.seed_scene_rng(1)
    sc = host.lower(_bvh_world(host, False, sphere_times=(0.25, 0.75)))
    a32, a64 = sc.arrays(), sc.arrays_f64()
    moved = [k for k in range(len(a32["prim_meta"])) if np.any(a64["prim_b"][k, :3] != 0.0)]
    assert len(moved) == 1 and a32["prim_meta"][moved[0]].type == abi.PRIM_MSPHERE
    assert a64["prim_dt"][moved[0]] == 0.5 and a64["prim_b"][moved[0], 3] == 0.25
    assert np.all(np.delete(a64["prim_dt"], moved[0]) == 1.0)
