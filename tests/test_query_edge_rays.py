"""The edge-ray corpus of the ray queries (tests/query_edge_rays.py) checked on its own, without a GPU: that it holds the
rays it is meant to hold, that every one of them passes the validation of include/rtmi_query.h, and that the classes are
what the device tests (tests/test_gpu_query_edges.py) take them for."""
from fractions import Fraction

import numpy as np
import pytest

import query_edge_rays as E
from oracle.oracle import ARITH_DEVICE

ALL = E.SCENES + ["cube_lattice_flat"]


def _is_b(s):
    return s["cls"] == "B"


@pytest.mark.parametrize("name", ALL)
def test_every_family_exists_and_every_ray_is_valid(host, orc32, name):
    c = E.families(E.corpus(orc32, host, name))
    want = [f for f in E.FAMILIES if f != "grazing" or name.startswith(tuple(E.LATTICES))]
    assert sorted(c) == sorted(want), (name, sorted(c))
    for fam, s in c.items():
        n = len(s["cls"])
        assert 0 < n <= 1024, (name, fam, n)
        assert s["o"].dtype == np.float32 and s["d"].dtype == np.float32 and s["o"].shape == s["d"].shape == (n, 3), (name, fam)
        assert s["t_min"].shape == s["t_max"].shape == (n,) and len(s["ref"]["hit"]) == n, (name, fam)
        assert s["times"] is None or s["times"].shape == (n,), (name, fam)
        bad = np.flatnonzero(~E.valid(s))
        assert bad.size == 0, (name, fam, bad[:8], s["o"][bad[:2]], s["d"][bad[:2]])
        assert set(np.unique(s["cls"])) <= {"A", "B"}, (name, fam)
        # the tagging rule: a NaN in the oracle's t or p is class B, whatever the family
        nan = np.isnan(s["ref"]["t"]) | np.isnan(s["ref"]["p"]).any(axis=1)
        assert np.all(_is_b(s)[nan]), (name, fam)
        assert np.all(_is_b(s)) if fam == "in_plane" else np.array_equal(_is_b(s), nan), (name, fam)
        # class B stays the exception outside the two families that are made of it
        if fam not in ("in_plane", "scaled"):
            assert _is_b(s).sum() <= 0.05 * n, (name, fam, int(_is_b(s).sum()), n)
    print(name, E.counts(c))


@pytest.mark.parametrize("name", ALL)
def test_families_hold_what_they_are_named_for(host, orc32, name):
    c = E.corpus(orc32, host, name)
    for fam in ("axis", "planar", "grazing"):
        if fam in c:
            hit = c[fam]["ref"]["hit"]
            assert hit.any() and not hit.all(), (name, fam, int(hit.sum()), len(hit))
    d = c["axis"]["d"]
    assert np.all((d != 0).sum(axis=1) == 1) and np.all(np.abs(d).max(axis=1) == 1), name
    zeros = {tuple(np.signbit(v).tolist()) + (int(np.argmax(np.abs(v))),) for v in d}
    assert len(zeros) == 24, (name, len(zeros))  # six axes, the two zeros in all four sign combinations
    d = c["planar"]["d"]
    assert np.all((d == 0).sum(axis=1) >= 1), name
    seen = {(int(k), bool(np.signbit(v[k]))) for v in d for k in np.flatnonzero(v == 0)}
    assert seen >= {(k, neg) for k in range(3) for neg in (False, True)}, (name, seen)
    s = c["on_surface"]
    assert set(np.unique(s["t_min"]).tolist()) == {0.0, float(np.float32(0.001))}, name
    s = c["scaled"]
    with np.errstate(over="ignore", under="ignore"):
        a = (s["d"] * s["d"]).sum(axis=1, dtype=np.float32)
    assert np.isinf(a).any() and a.min() < 1e-35, name  # d.d overflows, and is tiny or (scenes of unit scale) denormal
    if name in E.LATTICES + ["random_spheres", "media_in_bvh"]:
        assert ((a > 0) & (a < np.finfo(np.float32).tiny)).any(), name
    s = c["interval"]
    assert (s["t_min"] < 0).any() and (s["t_min"] == s["t_max"]).any() and (s["t_min"] <= np.float32(-1e30)).any(), name
    s = c["in_plane"]
    inf = E.inv_d_infinite(s["d"])
    assert np.all(inf.any(axis=1)), name
    denormal = (inf & (s["d"] != 0)).any(axis=1)  # 1 / d_k overflows without a zero component in that place
    assert denormal.sum() >= len(denormal) // 2 and (~denormal).sum() >= len(denormal) // 4, (name, int(denormal.sum()))
    assert (denormal & ~(s["d"] == 0).any(axis=1)).sum() >= len(denormal) // 4, name  # ... and no zero anywhere


@pytest.mark.parametrize("name", ["cornell_box", "final_scene", "media_in_bvh", "cube_lattice", "cube_lattice_flat"])
def test_in_plane_rays_meet_nan_acceptances(host, orc32, name):
    """a scene with rects or cubes: the reference accepts the ray in the plane with t = NaN, and often nothing overwrites it"""
    s = E.corpus(orc32, host, name)["in_plane"]
    nan = np.isnan(s["ref"]["t"])
    assert nan.sum() >= 32, (name, int(nan.sum()))
    assert np.all(s["ref"]["hit"][nan]), name


def test_in_plane_rays_of_final_scene_lie_in_the_dropped_rects_plane(host, orc32):
    s = E.corpus(orc32, host, "final_scene")["in_plane"]
    k = s["dropped"]
    assert k.sum() >= 32 and np.all(s["o"][k, 1] == np.float32(E.LIGHT_K)) and np.all(E.inv_d_infinite(s["d"])[k, 1])
    # with the rect every one of them is accepted by it or by something before it; without it some see past it
    assert np.all(s["ref"]["hit"][k])
    low = s["ref_lowered"]
    assert np.isnan(s["ref"]["t"][k]).sum() >= 16 and not np.isnan(low["t"][k]).any()
    other = ~k  # the rect takes part in no other ray's record
    for key in s["ref"]:
        assert np.asarray(s["ref"][key][other]).tobytes() == np.asarray(low[key][other]).tobytes(), key


def test_axis_rays_of_the_sphere_lattice_meet_nan_slabs(host, orc32):
    """0 * inf in AABB::hit: recomputed here from the node boxes of the lowered scene"""
    c = E.corpus(orc32, host, "sphere_lattice")
    s = c["axis"]
    boxes = E.node_boxes(c["arrays"])
    assert boxes.shape[0] >= 2 * 64
    bad = E.nan_slab(s["o"], s["d"], boxes)
    assert bad.sum() >= 64, int(bad.sum())
    assert (bad & s["ref"]["hit"]).sum() >= 8 and (bad & ~s["ref"]["hit"]).sum() >= 8  # finite results behind NaN slabs
    assert not np.any(_is_b(s))  # spheres: nothing accepts a NaN


def test_exact_tangent_rays_have_a_zero_discriminant(host, orc32):
    s = E.corpus(orc32, host, "sphere_lattice")["grazing"]
    idx = np.flatnonzero(s["tangent"])
    assert idx.size >= 64
    for i in idx:
        o, d = [Fraction(float(v)) for v in s["o"][i]], [Fraction(float(v)) for v in s["d"][i]]
        oc = [o[k] - Fraction(float(s["centre"][i][k])) for k in range(3)]
        a, b = sum(v * v for v in d), sum(p * q for p, q in zip(oc, d))
        cc = sum(v * v for v in oc) - Fraction(float(s["radius"][i])) ** 2
        assert b * b - a * cc == 0, (i, s["o"][i], s["d"][i])  # sphere.rs:40-43
    assert not s["ref"]["hit"][idx].any()  # disc > 0 is strict: the touching ray misses
    near = np.flatnonzero(~s["tangent"])
    assert s["ref"]["hit"][near].any() and not s["ref"]["hit"][near].all()


@pytest.mark.parametrize("name", E.LATTICES)
def test_fp32_and_f64_oracles_agree_on_the_lattices_class_a_hit_flags(host, orc32, orc64, name):
    """all inputs are exact there, so the decision is the same in either precision"""
    c = E.corpus(orc32, host, name)
    world = E.build_world(orc64, name)
    for fam in ("axis", "planar", "grazing"):
        s = c[fam]
        for i in np.flatnonzero(s["cls"] == "A"):
            h = orc64.hit(world, s["o"][i].astype(np.float64), s["d"][i].astype(np.float64),
                          time=0.0 if s["times"] is None else float(s["times"][i]), t_min=float(s["t_min"][i]),
                          t_max=float(s["t_max"][i]), seed=E.Q.SEED + int(i))
            assert (h is not None) == bool(s["ref"]["hit"][i]), (name, fam, i, s["o"][i], s["d"][i], h)
    orc64.free_all()
    assert ARITH_DEVICE == 1  # the records of the corpus are the fp32 oracle's in the device's arithmetic (query_ref)


def test_the_sequential_leaf_fold_is_the_oracle_on_class_a_and_not_in_plane(host, orc32):
    """the restatement of the device's rule under a tree (query_edge_rays.cube_lattice_leaf_fold) gives the oracle's own
    records wherever no NaN is accepted — so it states the traversal — and another leaf than BVHNode::hit's pairwise fold
    for some in-plane ray, with the same hit flag throughout"""
    c = E.corpus(orc32, host, "cube_lattice")
    for fam in ("axis", "planar", "on_surface", "scaled", "interval", "grazing"):
        s = c[fam]
        _, rec = E.cube_lattice_leaf_fold(orc32, c["arrays"], s)
        for k in rec:
            assert np.asarray(rec[k]).tobytes() == np.asarray(s["ref"][k]).tobytes(), (fam, k)
    s = c["in_plane"]
    prim, rec = E.cube_lattice_leaf_fold(orc32, c["arrays"], s)
    assert np.array_equal(rec["hit"], s["ref"]["hit"]) and np.array_equal(prim >= 0, rec["hit"])
    other = ~((rec["t"] == s["ref"]["t"]) | (np.isnan(rec["t"]) & np.isnan(s["ref"]["t"])))
    assert 1 <= other.sum() <= 0.05 * len(other), int(other.sum())
    assert np.all(s["meets_nan"][other])  # only where a face accepts a NaN
    orc32.free_all()
