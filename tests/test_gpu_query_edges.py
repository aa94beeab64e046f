"""Ray queries with the rays a caller sends and a renderer never produces (tests/query_edge_rays.py builds them, their
oracle records and their classes; tests/test_query_edge_rays.py checks that corpus on the CPU).

Class A (no NaN in the oracle's record, not in a plane of the scene): every word equals the fp32 oracle's, by the
assertions of tests/test_gpu_query.py (query_ref.check_set), in both flag settings, trace and occluded — axis-aligned rays
with signed zeros, NaN slab values at node boxes (the gate argument of DESIGN.md §3.1/§5 on 0 * inf), origins on a surface
with t_min = 0, directions scaled until d.d underflows or overflows, t_min at, next to and far below a hit, rays that
touch a sphere.  The gate argument once more through the render kernels: the lattice worlds seen along an axis from an
integer eye, reference-topology and default trees against the oracle's render.

Class B (in-plane rays, d_k = +-0 or a denormal whose reciprocal overflows: a rect or a cube face accepts them with
t = NaN, rect.rs:46-51):
  flat lists       equal to the oracle: NaN where it has NaN, every other word bit for bit;
  under a tree     the device's rule (include/rtmi_query.h): the hit flag is the oracle's; a ray that lies in node-box
                   planes only equals the oracle bit for bit; a ray in the plane of a rect or cube face may return another
                   accepted leaf than the reference's pairwise fold: the measured rays do (OTHER_LEAF: 4 of 2628 over
                   three scenes), every other one equals the oracle, and what the four return is the record of the
                   returned leaf alone, on cube_lattice the very leaf a restatement of the sequential fold keeps.  Every
                   record is valid, the same in every call, alone or in a batch and under both flag settings (1 / d_k is
                   infinite — d_k = +-0 or denormal — so both take one traversal), with occluded == hit, and without
                   effect on the other rays of its wavefront;
  the dropped rect final_scene's light (x0 > x1) is not in the device's world: the rays in its plane follow the oracle's
                   records of the world without it."""
import numpy as np
import pytest

import query_edge_rays as E
import query_ref as Q
from oracle.oracle import ARITH_DEVICE, SKY, THROUGHPUT_FORM
from raytracing_rust_amd import abi

FC = Q.FC
TREES = [n for n in E.SCENES if n not in E.FLAT]
FLOATS = ("t", "u", "v", "p", "normal")


def _upload(host, name):
    sc = host.lower(E.build_world(host, name)).upload(0)
    return sc, sc.arrays()


def _query(sc, s, flags, idx=slice(None), first_ray=0):
    times = None if s["times"] is None else s["times"][idx]
    kw = dict(t_min=s["t_min"][idx], t_max=s["t_max"][idx], seed=Q.SEED, first_ray=first_ray, flags=flags)
    return sc.trace(s["o"][idx], s["d"][idx], times, **kw), sc.occluded(s["o"][idx], s["d"][idx], times, **kw)


def _differs(got, ref, kinds):
    """bool [n]: the record differs from the oracle's — the hit flag, a word of t, u, v, p, normal (a NaN of the oracle's
    is met by any NaN: payloads are not compared) or the kind of the material"""
    n = len(ref["hit"])
    bad = got["hit"] != ref["hit"]
    for k in FLOATS:
        g, r = np.asarray(got[k], np.float32).reshape(n, -1), np.asarray(ref[k], np.float32).reshape(n, -1)
        bad |= (np.where(np.isnan(r), np.isnan(g), g.view(np.uint32) == r.view(np.uint32)) == 0).any(axis=1)
    return bad | (kinds[got["material"]] != ref["mat_kind"])


def _valid_records(a, got, what):
    """every record is the exact miss record or a hit whose item, prim and material name something of the scene"""
    miss = ~got["hit"]
    assert np.all(got["item"][miss] == -1) and np.all(got["prim"][miss] == -1) and np.all(got["material"][miss] == -1), what
    assert np.all(np.isposinf(got["t"][miss])), what
    for k in ("u", "v", "p", "normal"):
        assert not np.any(np.asarray(got[k][miss]).view(np.uint32)), (what, k)
    Q.check_indices(a, got, what)


def _own_record(orc, a, got, s, i):
    """the oracle's record of ray i of s against the primitive the device returned for it, alone: an axis-aligned cube or a
    rect of an item without transforms, rebuilt from the lowered arrays (anything else is not restated here and fails)"""
    it, pr = a["items"][int(got["item"][i])], int(got["prim"][i])
    m, A, B = a["prim_meta"][pr], a["prim_a"][pr], a["prim_b"][pr]
    assert pr >= 0 and it.xform_count == 0 and not (it.flags & 3) and m.flags & ~0x300 == 0 and m.type in (2, 3), (i, pr, m.type)
    mat = orc.Lambertian(orc.SolidTexture(0.5, 0.5, 0.5))
    if m.type == 3:
        obj = orc.Cube(tuple(float(v) for v in A[:3]), (float(A[3]), float(B[0]), float(B[1])), mat)
    else:
        obj = orc.Rect((m.flags >> 8) & 3, float(A[0]), float(A[1]), float(A[2]), float(A[3]), float(B[0]), mat)
    rec = Q.oracle_records(orc, obj, s["o"][i:i + 1], s["d"][i:i + 1], None if s["times"] is None else s["times"][i:i + 1],
                           s["t_min"][i:i + 1], s["t_max"][i:i + 1])
    rec["mat_kind"] = np.array([a["materials"][m.material].kind])
    return rec


# in-plane rays (indices into the in_plane family) for which the device's sequential fold of the accepted leaves keeps
# another leaf than BVHNode::hit's pairwise fold: measured on the MI355X, the same under both flag settings
OTHER_LEAF = {"final_scene": [121], "media_in_bvh": [361, 696], "cube_lattice": [277]}


# ---- class A -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", E.SCENES + ["cube_lattice_flat"])
def test_class_a_rays_equal_the_fp32_oracle(host, orc32, name):
    c = E.corpus(orc32, host, name)
    sc, a = _upload(host, name)
    for fam, s in E.families(c).items():
        sub = s["A"]
        if len(sub["ref"]["hit"]) == 0:
            assert fam == "in_plane", (name, fam)
            continue
        got = Q.check_set(sc, a, sub, (name, fam))
        print(name, fam, "rays", len(s["cls"]), "hits", int(s["ref"]["hit"].sum()), "class B", int((s["cls"] == "B").sum()),
              "class A rays", len(got["hit"]), "disagreements", 0)
    if name == "sphere_lattice":  # the gate argument on 0 * inf: these rays met NaN slab values and finite primitives
        s = c["axis"]
        assert E.nan_slab(s["o"], s["d"], E.node_boxes(a)).sum() >= 64 and not np.any(s["cls"] == "B")


@pytest.mark.gpu
@pytest.mark.parametrize("name", E.LATTICES)
def test_lattice_renders_along_an_axis_equal_the_oracle_in_every_tree(host, orc32, name):
    """the eye at an integer point, on node planes of the lattice, looking along z without a lens: the slab values of the
    planes through the eye are 0 * (1 / d) = 0 for every primary ray.  Reference-topology tree, default trees and the
    per-lane kernel against the oracle's render."""
    nx, ny, ns = 32, 32, 4
    eye, at = ((3.0, 3.0, -5.0), (3.0, 3.0, 3.0)) if name == "sphere_lattice" else ((2.0, 3.0, -4.0), (2.0, 3.0, 2.0))
    args = (eye, at, (0.0, 1.0, 0.0), 60.0, nx / ny, 0.0, 8.0, 0.0, 1.0)
    ref = orc32.render(orc32.Camera(*args), E.build_world(orc32, name), nx, ny, ns, seed=42, flags=ARITH_DEVICE | THROUGHPUT_FORM | SKY)
    orc32.free_all()
    sc = host.lower(E.build_world(host, name))
    cam = host.Camera(*args)
    assert 0.05 < float(np.nanmean(ref["linear"]))
    for flags in (0, FC, FC | abi.RTMI_FLAG_REF_TREE, FC | abi.RTMI_FLAG_SYNC):
        got = sc.render(cam, nx, ny, ns, seed=42, flags=flags | abi.RTMI_FLAG_SKY, sig=True)
        assert np.array_equal(got["sig"], ref["sig"]), (name, flags)
        assert np.array_equal(got["linear"], ref["linear"], equal_nan=True), (name, flags)


# ---- class B in flat lists ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", E.FLAT)
def test_class_b_rays_in_flat_lists_equal_the_fp32_oracle(host, orc32, name):
    c = E.corpus(orc32, host, name)
    sc, a = _upload(host, name)
    assert all(it.kind == 0 for it in a["items"]), name  # RTMI_ITEM_LIST throughout
    kinds = np.array([m.kind for m in a["materials"]] + [-1])
    n_b = n_nan = 0
    for fam, s in E.families(c).items():
        sub = s["B"]
        ref = sub["ref"]
        if len(ref["hit"]) == 0:
            continue
        for flags in (0, FC):
            got, occ = _query(sc, sub, flags)
            bad = np.flatnonzero(_differs(got, ref, kinds))
            assert bad.size == 0, (name, fam, flags, bad.size, bad[:8], [(k, got[k][bad[:2]], ref[k][bad[:2]]) for k in ("hit", "t", "p")])
            assert np.array_equal(occ, ref["hit"]), (name, fam, flags, np.flatnonzero(occ != ref["hit"])[:8])
            _valid_records(a, got, (name, fam, flags))
        n_b += len(ref["hit"])
        n_nan += int(np.isnan(ref["t"]).sum())
        print(name, fam, "class B rays", len(ref["hit"]), "hits", int(ref["hit"].sum()), "NaN records", int(np.isnan(ref["t"]).sum()),
              "disagreements", 0)
    assert n_b >= 256 and n_nan >= 32, (name, n_b, n_nan)


# ---- class B under a tree ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", TREES)
def test_class_b_rays_under_a_tree_follow_the_stated_rule(host, orc32, name):
    c = E.corpus(orc32, host, name)
    sc, a = _upload(host, name)
    kinds = np.array([m.kind for m in a["materials"]] + [-1])
    for fam, s in E.families(c).items():
        sub = s["B"]
        n = len(sub["ref"]["hit"])
        if n == 0:
            continue
        # the device's world has no never-hit rect: the rays in its plane are held to the oracle's records without it
        ref = s["ref_lowered"] if "ref_lowered" in s else sub["ref"]
        in_face = s["meets_nan"][sub["index"]] if "index" in sub else s["meets_nan"]
        model = E.cube_lattice_leaf_fold(orc32, a, sub) if name == "cube_lattice" else None
        by_flag = {}
        for flags in (0, FC):
            got, occ = _query(sc, sub, flags)  # (a call that returns at all returned RTMI_OK: the host raises otherwise)
            by_flag[flags] = got
            what = (name, fam, flags)
            _valid_records(a, got, what)
            assert np.array_equal(occ, got["hit"]), (what, np.flatnonzero(occ != got["hit"])[:8])
            again, occ2 = _query(sc, sub, flags)
            assert Q.same(got, again) and np.array_equal(occ, occ2), what
            # alone as in the batch
            for i in range(n):
                one, occ1 = _query(sc, sub, flags, idx=slice(i, i + 1), first_ray=int(i))
                for k in one:
                    if k != "kernel_ms":
                        assert one[k].tobytes() == got[k][i:i + 1].tobytes(), (what, i, k)
                assert occ1[0] == occ[i], (what, i)
            # the rule
            bad = _differs(got, ref, kinds)
            plain = np.flatnonzero(bad & ~in_face)  # node-box planes only: NaN slab values change nothing
            print(name, fam, "flags", flags, "class B rays", n, "hits", int(ref["hit"].sum()), "in a face plane", int(in_face.sum()),
                  "NaN records: oracle", int(np.isnan(ref["t"]).sum()), "device", int(np.isnan(got["t"]).sum()),
                  "disagreements", int(bad.sum()), "of them outside face planes", plain.size,
                  "in the hit flag", int((got["hit"] != ref["hit"]).sum()))
            assert np.array_equal(got["hit"], ref["hit"]), (what, np.flatnonzero(got["hit"] != ref["hit"])[:8])
            assert plain.size == 0, (what, plain.size, plain[:8], [(k, got[k][plain[:2]], ref[k][plain[:2]]) for k in ("t", "p")])
            # in a face plane: the measured rays, no others, return another accepted leaf than the pairwise fold's, and
            # what they return is that leaf's own record for the ray (NaN for NaN)
            assert np.flatnonzero(bad).tolist() == OTHER_LEAF.get(name, []), (what, np.flatnonzero(bad))
            for i in np.flatnonzero(bad):
                own = _own_record(orc32, a, got, sub, i)
                one = {k: got[k][i:i + 1] for k in got if k != "kernel_ms"}
                assert not _differs(one, own, kinds)[0], (what, i, [(k, one[k], own[k]) for k in FLOATS])
            if model is not None:  # the hand-built tree: exactly the leaf the sequential fold keeps, and its record
                prim, rec = model
                off = np.flatnonzero(_differs(got, rec, kinds) | (got["prim"] != prim))
                assert off.size == 0, (what, off[:8], got["prim"][off[:8]], prim[off[:8]])
        # a zero component in the direction: one traversal for both flag settings
        assert Q.same(by_flag[0], by_flag[FC]), (name, fam)
        if "dropped" in s:
            assert s["dropped"].sum() >= 32 and not in_face[s["dropped"]].any()  # so they were held to the bits above


@pytest.mark.gpu
@pytest.mark.parametrize("name", TREES)
def test_class_b_rays_leave_their_wavefronts_class_a_rays_alone(host, orc32, name):
    """16 class B rays among the 48 class A rays of one wavefront, each class A ray at its own index (its Philox key):
    the class A records keep the oracle's bits"""
    c = E.corpus(orc32, host, name)
    sc, a = _upload(host, name)
    kinds = np.array([m.kind for m in a["materials"]] + [-1])
    b = c["in_plane"]
    nan_first = np.argsort(~np.isnan(b["ref"]["t"]), kind="stable")  # the rays with a NaN record first
    for fam in ("axis", "planar", "on_surface"):
        s = c[fam]["A"]
        slots = np.arange(2, 64, 4)
        mix = {k: (None if s[k] is None else s[k][:64].copy()) for k in ("o", "d", "times", "t_min", "t_max")}
        for k in ("o", "d", "t_min", "t_max"):
            mix[k][slots] = b[k][nan_first[:16]]
        keep = np.setdiff1d(np.arange(64), slots)
        for flags in (0, FC):
            got, occ = _query(sc, mix, flags)
            ref = {k: v[:64][keep] for k, v in s["ref"].items()}
            sub = {k: (v[keep] if k != "kernel_ms" else v) for k, v in got.items()}
            bad = np.flatnonzero(_differs(sub, ref, kinds))
            assert bad.size == 0, (name, fam, flags, keep[bad])
            assert np.array_equal(occ[keep], ref["hit"]), (name, fam, flags)
            _valid_records(a, got, (name, fam, flags))
