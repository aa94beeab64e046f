"""rtmu_refit_desc (include/rtmi_update.h, csrc/rtmi_refit.hpp) against the numpy restatement of its rules (refit_ref.py),
bit for bit, without a device; then what the rules promise: exact containment, untouched bytes, and that they mirror the
lowering."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import refit_ref as R
from raytracing_rust_amd import abi


def _lowered(host, kind):
    spec = R.spec_of(kind)
    scene = host.lower(R.build_world(host, spec))
    return spec, scene, R.from_desc(scene.desc())


def _c_refit(scene, arr, first, count):
    """rtmu_refit_desc on copies: -> the refit arrays"""
    out = {k: v.copy() for k, v in arr.items()}
    d = R.to_desc(arr, scene.desc())
    gate = out["prim_gate"].ctypes.data if out["prim_gate"].size else None
    rc = abi.load_rtmi().rtmu_refit_desc(C.byref(d), first, count, out["items"].ctypes.data_as(C.POINTER(abi.Item)),
                                         out["nodes"].ctypes.data_as(C.POINTER(abi.BvhNode)),
                                         out["alt_nodes"].ctypes.data_as(C.POINTER(abi.Bvh4Node)), gate)
    assert rc == 0, abi.load_rtmi().rtmi_last_error()
    return out


def _same(x, y):
    return all(x[k].tobytes() == y[k].tobytes() for k in x)


def _ranges(kind, arr):
    n = len(arr["prim_a"])
    if kind != "two":
        return [(0, n)]
    bvh = [i for i, it in enumerate(arr["items"]) if it["kind"] == abi.ITEM_BVH]
    second = sorted(R.item_leaves(arr, bvh[1]))
    return [(0, n), (second[0], len(second)), (second[3], 4)]  # everything; the second item alone; a part of it


@pytest.mark.parametrize("kind", R.KINDS)
def test_refit_desc_equals_the_restatement_bit_for_bit(host, kind):
    spec, scene, arr = _lowered(host, kind)
    assert R.from_desc(scene.desc())["items"].tobytes() == arr["items"].tobytes()
    refittable = scene.refittable()
    assert refittable.tolist() == [bool(it["kind"] == abi.ITEM_BVH) for it in arr["items"]]
    if kind == "s1":  # a node over one element, no alternative tree
        n = arr["nodes"][arr["items"][0]["first"]]
        assert n["left"] == n["right"] < 0 and arr["items"][0]["alt_first"] < 0
    for case, (first, count) in enumerate(_ranges(kind, arr)):
        moved = {k: v.copy() for k, v in arr.items()}
        a, b = R.new_planes(arr, spec, R.moved_spec(spec, 100 + case))
        moved["prim_a"][first:first + count], moved["prim_b"][first:first + count] = a[first:first + count], b[first:first + count]
        assert count == 0 or not np.array_equal(moved["prim_a"], arr["prim_a"])
        want, boxes = R.refit(moved, first, count)
        got = _c_refit(scene, moved, first, count)
        for k in want:
            assert got[k].tobytes() == want[k].tobytes(), (kind, case, k)
        # ---- untouched items and every word that is no box keep their bytes
        for name, fields in R.BOX_FIELDS.items():
            rest = [f for f in got[name].dtype.names if f not in fields]
            for f in rest:
                assert got[name][f].tobytes() == arr[name][f].tobytes(), (name, f)
        touched = set(boxes)
        assert touched and all(arr["items"][i]["kind"] == abi.ITEM_BVH for i in touched)
        for i, it in enumerate(arr["items"]):
            if it["kind"] != abi.ITEM_BVH or i in touched:
                continue
            assert got["items"][i].tobytes() == it.tobytes()
            for p in R.item_leaves(arr, i):
                assert got["prim_gate"][p].tobytes() == arr["prim_gate"][p].tobytes()
        if kind == "two" and case > 0:
            assert len(touched) == 1
        # ---- containment, exactly
        fr = lambda box: ([Fraction(float(v)) for v in box[0]], [Fraction(float(v)) for v in box[1]])
        inside = lambda inner, outer: all(o <= i for i, o in zip(inner[0], outer[0])) and all(i <= o for i, o in zip(inner[1], outer[1]))
        for i in touched:
            nodes, alt = got["nodes"], got["alt_nodes"]

            def extent(p):  # the primitive's own, exactly, from its fp32 planes
                A, B = [Fraction(float(v)) for v in got["prim_a"][p]], [Fraction(float(v)) for v in got["prim_b"][p]]
                if got["prim_meta"][p]["type"] == abi.PRIM_CUBE:
                    return [A[0], A[1], A[2]], [A[3], B[0], B[1]]
                return [A[k] - abs(A[3]) for k in range(3)], [A[k] + abs(A[3]) for k in range(3)]  # (a hollow sphere: |r|)

            for n, own in boxes[i].items():
                for ref, mn, mx in ((int(nodes[n]["left"]), "lmin", "lmax"), (int(nodes[n]["right"]), "rmin", "rmax")):
                    stored = fr((nodes[n][mn], nodes[n][mx]))
                    if ref < 0:
                        assert inside(extent(R.prim_of(ref)), stored)
                        g = got["prim_gate"][R.prim_of(ref)]
                        assert g[0:3].tobytes() == np.array(own[0], "<f4").tobytes() and g[4:7].tobytes() == np.array(own[1], "<f4").tobytes()
                        assert g[3] == 0 and g[7] == 0
                    else:
                        child = nodes[ref]
                        for cmn, cmx in (("lmin", "lmax"), ("rmin", "rmax")):  # the child's own child boxes, up to the leaves' padding
                            cref = int(child["left" if cmn == "lmin" else "right"])
                            if cref >= 0:
                                assert inside(fr((child[cmn], child[cmx])), stored)
                            else:
                                # (a leaf below it: its fp32 leaf box.  Its stored box is padded beyond every node box, and
                                # its exact extent may leave the fp32 one by half an ulp, as in the lowering: the leaf's
                                # own stored box, checked above, is what has to hold it)
                                assert inside(fr(R.leaf_box(got, R.prim_of(cref))), stored)

            def alt_check(n):
                for c in range(4):
                    ref = int(alt[n]["child"][c])
                    if ref == R.NO_CHILD:
                        assert alt[n]["minx"][c] > alt[n]["maxx"][c]
                        continue
                    stored = fr(([alt[n][f][c] for f in ("minx", "miny", "minz")], [alt[n][f][c] for f in ("maxx", "maxy", "maxz")]))
                    if ref < 0:
                        assert inside(extent(R.prim_of(ref)), stored)
                        continue
                    for q in range(4):
                        if int(alt[ref]["child"][q]) != R.NO_CHILD:
                            assert inside(fr(([alt[ref][f][q] for f in ("minx", "miny", "minz")],
                                              [alt[ref][f][q] for f in ("maxx", "maxy", "maxz")])), stored)
                    alt_check(ref)

            if got["items"][i]["alt_first"] >= 0:
                alt_check(int(got["items"][i]["alt_first"]))


@pytest.mark.parametrize("kind", R.KINDS)
def test_the_rules_mirror_the_lowering(host, kind):
    """Refitting UNCHANGED planes moves no box coordinate by more than 2^-21 scale from the lowering's value: each fp32 input is
    off from the f64 value by at most 2^-24 scale, two inputs and the final rounding on either side give 2^-22 scale, doubled
    for margin.  A larger difference means a rule is not the lowering's."""
    spec, scene, arr = _lowered(host, kind)
    got = _c_refit(scene, arr, 0, len(arr["prim_a"]))
    for i, it in enumerate(arr["items"]):
        if it["kind"] != abi.ITEM_BVH:
            continue
        bound = float(it["scale"]) * 2.0 ** -21
        assert abs(float(got["items"][i]["scale"]) - float(it["scale"])) <= bound
        for f in ("root_min", "root_max"):
            assert np.all(np.abs(got["items"][i][f].astype(np.float64) - it[f].astype(np.float64)) <= bound), f
        for p in R.item_leaves(arr, i):
            assert np.all(np.abs(got["prim_gate"][p].astype(np.float64) - arr["prim_gate"][p].astype(np.float64)) <= bound), p
        # the item's nodes: those its tree reaches
        stack, seen = [int(it["first"])], []
        while stack:
            n = stack.pop()
            seen.append(n)
            stack += [int(r) for r in {int(arr["nodes"][n]["left"]), int(arr["nodes"][n]["right"])} if r >= 0]
        for n in seen:
            for f in R.BOX_FIELDS["nodes"]:
                assert np.all(np.abs(got["nodes"][n][f].astype(np.float64) - arr["nodes"][n][f].astype(np.float64)) <= bound), (n, f)
        stack = [int(it["alt_first"])] if it["alt_first"] >= 0 else []
        while stack:
            n = stack.pop()
            for c in range(4):
                ref = int(arr["alt_nodes"][n]["child"][c])
                for f in R.BOX_FIELDS["alt_nodes"]:
                    if ref == R.NO_CHILD:
                        assert got["alt_nodes"][n][f][c].tobytes() == arr["alt_nodes"][n][f][c].tobytes()
                    else:
                        assert abs(float(got["alt_nodes"][n][f][c]) - float(arr["alt_nodes"][n][f][c])) <= bound, (n, c, f)
                if ref >= 0 and ref != R.NO_CHILD:
                    stack.append(ref)


def test_update_of_a_scene_that_is_not_resident_edits_its_description(host):
    """Scene.update_prims without upload: the planes go into the lowered arrays, which are refit in place; list primitives
    move without any box changing"""
    spec, scene, arr = _lowered(host, "two")
    new = R.moved_spec(spec, 5)
    a, b = R.new_planes(arr, spec, new)
    scene.update_prims(0, a, b)
    want, boxes = R.refit(dict(arr, prim_a=a, prim_b=b), 0, len(a))
    assert len(boxes) == 2 and _same(R.from_desc(scene.desc()), want)
    lists = [it for it in arr["items"] if it["kind"] == abi.ITEM_LIST]
    first, count = int(lists[0]["first"]), int(lists[0]["count"])
    a2 = a.copy()
    a2[first:first + count, 0] += np.float32(0.25)
    scene.update_prims(first, a2[first:first + count])
    want["prim_a"] = a2
    assert _same(R.from_desc(scene.desc()), want)
    scene.update_prims(3, a2[:0])  # count == 0
    assert _same(R.from_desc(scene.desc()), want)
