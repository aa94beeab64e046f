"""The relight rules on the host (include/rtmi_relight.h), without a GPU: rtml_relight_desc against a numpy restatement with
explicit loops, against the attach's own table and tree on unchanged planes, against rtmi_lights_from_desc of the edited
description on moved ones, the consistency of pick and pmf on the refit tree, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import refit_ref as R
import relight_ref as L
from raytracing_rust_amd import abi
from raytracing_rust_amd.host import LIGHT_PATH_DTYPE


def _scene(host, n):
    scene = host.lower(L.light_list(host, n))
    return scene, R.from_desc(scene.desc()), L.table_of(scene)


def _same(got, want, fields, what):
    for f in fields:
        assert got[f].tobytes() == want[f].tobytes(), (what, f)


@pytest.mark.parametrize("n", L.COUNTS)
def test_unchanged_planes_reproduce_the_attached_table_and_tree(host, n):
    scene, arr, (lights, nodes, paths) = _scene(host, n)
    assert len(lights) == n and len(nodes) == 2 * n
    assert len(set(lights["weight"].tolist())) > (1 if n > 1 else 0) and (1.0 in lights["weight"].tolist()) == (n >= 5)
    rc, got_l, got_n = L.relight(arr, scene.desc(), lights, nodes)
    assert rc == 0, L.last_error()
    assert got_l.tobytes() == lights.tobytes() and got_n.tobytes() == nodes.tobytes()
    rc, only_table, _ = L.relight(arr, scene.desc(), lights, None)  # no tree: the table alone
    assert rc == 0 and only_table.tobytes() == lights.tobytes()


@pytest.mark.parametrize("n", L.COUNTS)
def test_moved_planes_equal_the_restatement_and_the_edited_description(host, n):
    scene, arr, (lights, nodes, paths) = _scene(host, n)
    a, b = L.moved_planes(arr, lights, 10 + n)
    moved = dict(arr, prim_a=a, prim_b=b)
    rc, got_l, got_n = L.relight(moved, scene.desc(), lights, nodes)
    assert rc == 0, L.last_error()
    want_l, want_n = L.restate(moved, lights, nodes)
    assert got_l.tobytes() == want_l.tobytes() and got_n.tobytes() == want_n.tobytes()
    assert got_l.tobytes() != lights.tobytes() and got_n.tobytes() != nodes.tobytes()
    _same(got_n, nodes, ("link", "pad"), "links are kept")
    # the table does not depend on topology: it is the fresh table of the edited description, every field
    assert got_l.tobytes() == L.lights_of(moved, scene.desc()).tobytes()
    # any topology gives a consistent pick and pmf: the probability a pick returns is the pmf of the light it returns
    lib = abi.load_rtmi()
    rng = np.random.default_rng(n)
    k = 512
    pts = rng.uniform(-12.0, 12.0, (k, 3)).astype(np.float32)
    us = (rng.integers(0, 1 << 24, k).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    picked, p = np.zeros(k, np.uint32), np.zeros(k, np.float32)
    node_p = got_n.ctypes.data_as(C.POINTER(abi.LightNode))
    assert lib.rtmi_light_tree_pick(node_p, len(got_n), pts.ctypes.data_as(C.POINTER(C.c_float)), us.ctypes.data_as(C.POINTER(C.c_float)), k,
                                    picked.ctypes.data_as(C.POINTER(C.c_uint32)), p.ctypes.data_as(C.POINTER(C.c_float))) == 0
    pmf = np.zeros(k, np.float32)
    paths = np.ascontiguousarray(paths, LIGHT_PATH_DTYPE)
    assert lib.rtmi_light_tree_pmf(node_p, len(got_n), paths.ctypes.data_as(C.POINTER(abi.LightPath)), pts.ctypes.data_as(C.POINTER(C.c_float)),
                                   picked.ctypes.data_as(C.POINTER(C.c_uint32)), k, pmf.ctypes.data_as(C.POINTER(C.c_float))) == 0
    assert p.tobytes() == pmf.tobytes() and (picked < n).all() and (n == 1 or len(set(picked.tolist())) > 1)


def test_refusals_write_nothing(host):
    scene, arr, (lights, nodes, paths) = _scene(host, 3)
    base = scene.desc()

    def refused(arr_, lights_, nodes_, word):
        rc, l2, n2 = L.relight(arr_, base, lights_, nodes_)
        assert rc == 1 and L.last_error().startswith("rtml_relight_desc: ") and word in L.last_error(), (word, L.last_error())
        assert l2.tobytes() == lights_.tobytes() and (nodes_ is None or n2.tobytes() == nodes_.tobytes())

    kinds = lights["kind"].tolist()
    rect, sphere = kinds.index(abi.PRIM_RECT), kinds.index(abi.PRIM_SPHERE)
    for li, col, value, word in ((rect, 2, None, "a0 >= a1"), (rect, 3, None, "b0 >= b1"), (sphere, 3, 0.0, "r <= 0"),
                                 (sphere, 3, -1.0, "r <= 0"), (sphere, 1, np.inf, "not finite"), (sphere, 0, np.nan, "not finite"),
                                 (sphere, 3, np.inf, "area * weight"), (rect, 2, np.inf, "area * weight")):
        a = arr["prim_a"].copy()
        p = int(lights[li]["prim"])
        a[p, col] = a[p, col - 2] if value is None else value
        refused(dict(arr, prim_a=a), lights, nodes, word)
    foreign = lights.copy()
    foreign[1]["prim"] = len(arr["prim_a"])
    refused(arr, foreign, nodes, "outside the description")
    foreign = lights.copy()
    foreign[rect]["kind"] = abi.PRIM_SPHERE  # the primitive is a rect
    refused(arr, foreign, nodes, "another primitive type")
    refused(arr, lights, nodes[:5], "even")  # an odd n_nodes
    refused(arr, lights, nodes[:4], "2 * n_lights")
    broken = nodes.copy()
    interior = next(i for i in range(1, len(nodes)) if not nodes[i]["link"] & L.LEAF)
    broken[interior]["link"] = len(nodes) + 2
    refused(arr, lights, broken, "a link leaves the array")
    broken[interior]["link"] = interior  # a link that does not point behind its node
    refused(arr, lights, broken, "a link leaves the array")
    lib = abi.load_rtmi()
    d = R.to_desc(arr, base)
    assert lib.rtml_relight_desc(None, lights.ctypes.data_as(C.POINTER(abi.Light)), 3, None, 0) == 1 and "NULL" in L.last_error()
    assert lib.rtml_relight_desc(C.byref(d), None, 3, None, 0) == 1 and "NULL" in L.last_error()
    assert lib.rtml_relight_desc(C.byref(d), lights.ctypes.data_as(C.POINTER(abi.Light)), 3, None, 6) == 1 and "NULL" in L.last_error()
