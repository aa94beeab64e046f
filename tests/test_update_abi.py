"""The scene updates' public interface (include/rtmi_update.h), without a GPU.

* the header compiles as C99; librtmi.so and librt_host.so export the entries, abi.py and sys.rs declare them;
* rtmu_refittable gives the expected mask, one description per reason that keeps a BVH item from being refit;
* rtmu_refit_desc refuses NULL arrays, ranges outside the primitives and ranges that touch what cannot be refit, and does
  nothing for an empty range;
* the host evaluation (csrc/rtmi_refit.hpp), compiled alone into a program of its own under the address and
  undefined-behaviour sanitizers, gives the library's bytes on the shared scenes and refuses malformed trees.  Nothing is
  loaded into Python for that."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import abi_kit as kit
import refit_ref as R
from raytracing_rust_amd import abi

ENTRIES = ["rtmu_probe_scene_words", "rtmu_refit_desc", "rtmu_refittable", "rtmu_scene_update_prepare", "rtmu_scene_update_prims", "rtmu_scene_update_prims_device",
           "rtmu_scene_update_xforms"]
HOST_ENTRIES = ["rthu_prims_of", "rthu_probe_scene_words", "rthu_refittable", "rthu_update_prepare", "rthu_update_prims", "rthu_update_prims_device",
                "rthu_update_xforms"]
# The family carries the prefix rtmu_ (rthu_ in the host library) and its own tables in abi.py (UPDATE_ENTRIES,
# UPDATE_HOST_ENTRIES), beside the render ABI's abi.FAMILIES: the kit's parsers read rtmi_ / rth_ names, so this file
# states the same chain for the other prefix.  Family serves the checks that need no name: C99, structs, isolation.
FAMILY = kit.Family("rtmi_update.h", ENTRIES)
WORDS = ["ITEMS", "PRIM_A", "PRIM_B", "GATE", "NODES", "ALT_NODES", "LEAF_REC", "SHADE_PRIM", "XFORMS"]
BIG = np.float32(3.40282346638528859811704183484516925e+38)


def test_header_is_c99(tmp_path):
    FAMILY.c99(tmp_path, holds=" && ".join("RTMI_SCENE_WORDS_%s == %d" % (w, k) for k, w in enumerate(WORDS)))


def _prototypes():
    return kit._c_functions(kit.header_text("rtmi_update.h"), r"^(?!static\b|typedef\b)([A-Za-z_][\w \t\*]*?)\b(rtmu_\w+)\s*\(([^;{}]*?)\)\s*;")


def _agree(name, proto, restype, argtypes):
    ret, args = proto
    assert kit.c_class(ret) == kit.ctypes_class(restype), name
    assert [kit.c_class(a) for a in args] == [kit.ctypes_class(t) for t in argtypes], name


def test_exports_and_declarations_agree():
    """header prototypes == abi.UPDATE_ENTRIES == ENTRIES == the block of sys.rs == what librtmi.so exports with the prefix,
    argument by argument; the host wrappers likewise against their definitions"""
    FAMILY.layout()
    FAMILY.isolation()
    assert kit.prototypes("rtmi_update.h") == {}  # nothing here is an entry of the render ABI's tables
    protos = _prototypes()
    assert sorted(protos) == sorted(abi.UPDATE_ENTRIES) == ENTRIES
    lib = abi.load_rtmi()
    for name, proto in protos.items():
        _agree(name, proto, *abi.UPDATE_ENTRIES[name])
        fn = getattr(lib, name)
        assert (fn.restype, fn.argtypes) == abi.UPDATE_ENTRIES[name]
    nm = lambda path: subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(rtmu_\w+)\b", nm(lib._name)))) == ENTRIES
    # sys.rs: the block declares exactly these, with the header's arity and pointer classes
    rust = {n: (ret, [a.split(":", 1)[1].strip() for a in kit._split_args(args)])
            for n, args, ret in re.findall(r"pub fn (rtmu_\w+)\s*\((.*?)\)\s*(?:->\s*([^;{]+?))?\s*;", kit.sys_block("rtmi_update.h"), re.S)}
    assert sorted(rust) == ENTRIES and not re.findall(r"pub fn rtmu_", kit.SYS.replace(kit.sys_block("rtmi_update.h"), ""))
    for name, (rret, rargs) in rust.items():
        assert rret == "c_int" and [kit.rust_is_pointer(t) for t in rargs] == [kit.c_class(a) == "ptr" for a in protos[name][1]], name
    # the host library's wrappers: definitions == abi.UPDATE_HOST_ENTRIES == HOST_ENTRIES == exported
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(kit.HOST_SOURCE).read(), flags=re.S)
    defined = kit._c_functions(text, r"^RTH_API\s+([A-Za-z_][\w \t\*]*?)\b(rthu_\w+)\s*\(([^;{}]*?)\)\s*\{")
    assert sorted(defined) == sorted(abi.UPDATE_HOST_ENTRIES) == HOST_ENTRIES
    host = abi.bind_host_update(abi.load_host())
    for name, proto in defined.items():
        _agree(name, proto, *abi.UPDATE_HOST_ENTRIES[name])
    assert sorted(set(re.findall(r"\b(rthu_\w+)\b", nm(host._name)))) == HOST_ENTRIES
    consts = kit.header_constants("rtmi_update.h")
    assert {k[len("RTMI_SCENE_WORDS_"):].lower(): v for k, v in consts.items()} == abi.SCENE_WORDS and len(consts) == len(WORDS)


def _err():
    return (abi.load_rtmi().rtmi_last_error() or b"").decode()


def _mask(arr, base):
    d = R.to_desc(arr, base)
    mask = np.full(len(arr["items"]), 7, np.uint8)
    rc = abi.load_rtmi().rtmu_refittable(C.byref(d), mask.ctypes.data)
    return rc, mask.tolist()


def test_refittable_mask_one_reason_at_a_time(host):
    scene = host.lower(R.build_world(host, R.spec_of("s5")))
    base, arr = scene.desc(), R.from_desc(scene.desc())
    bvh = [i for i, it in enumerate(arr["items"]) if it["kind"] == abi.ITEM_BVH]
    assert len(bvh) == 1 and len(arr["items"]) > 1
    want = [i == bvh[0] for i in range(len(arr["items"]))]
    assert _mask(arr, base) == (0, [int(w) for w in want])  # LIST items are 0

    def broken(edit):
        a = {k: v.copy() for k, v in arr.items()}
        edit(a, a["items"][bvh[0]])
        rc, mask = _mask(a, base)
        return rc, mask[bvh[0]], sum(mask)

    def flag(bit):
        def edit(a, it):
            it["flags"] |= bit
        return edit

    def no_alt(a, it):
        it["alt_first"] = -1

    def never_prune(a, it):
        it["scale"] = 1e30

    root = int(arr["items"][bvh[0]]["first"])
    leaf_node = next(n for n in range(len(arr["nodes"])) if arr["nodes"][n]["left"] < 0)

    def moving(a, it):  # the leaf and its primitive become a MovingSphere
        p = R.prim_of(a["nodes"][leaf_node]["left"])
        a["prim_meta"][p]["type"] = abi.PRIM_MSPHERE
        for f in ("left", "right"):
            if a["nodes"][leaf_node][f] < 0 and R.prim_of(a["nodes"][leaf_node][f]) == p:
                a["nodes"][leaf_node][f] = np.int32(-(1 << 31) + (abi.PRIM_MSPHERE << 28) + p)

    def rect(a, it):  # the primitive's type alone: the leaf reference no longer agrees either
        a["prim_meta"][R.prim_of(a["nodes"][leaf_node]["left"])]["type"] = abi.PRIM_RECT

    def chained(a, it):
        a["prim_meta"][R.prim_of(a["nodes"][leaf_node]["left"])]["flags"] |= 1 << abi.RTMI_PRIMFLAG_XF_COUNT_SHIFT

    def list_child(a, it):  # an internal child whose box passes every ray (lower_list_leaf)
        n = a["nodes"][root]
        side = ("lmin", "lmax") if n["left"] >= 0 else ("rmin", "rmax")
        assert n["left"] >= 0 or n["right"] >= 0
        n[side[0]], n[side[1]] = -BIG, BIG

    for edit in (flag(abi.ITEMFLAG_DEFERRED), flag(abi.ITEMFLAG_SAVE_T0), never_prune, no_alt, moving, rect, chained, list_child):
        assert broken(edit) == (0, 0, 0), edit
    assert broken(lambda a, it: None) == (0, 1, 1)


def test_refittable_on_lowered_worlds(host):
    """what the lowering itself makes non-refittable: a MovingSphere or a rect in the tree, an instanced leaf, a list as a child"""
    mat = host.Lambertian(host.SolidTexture(0.5, 0.5, 0.5))
    sph = lambda x: host.Sphere((x, 0.0, 0.0), 0.3, mat)
    cases = {"plain": [sph(0.0), sph(1.0), sph(2.0)],
             "moving": [sph(0.0), host.MovingSphere((1.0, 0.0, 0.0), (1.0, 0.2, 0.0), 0.0, 1.0, 0.3, mat), sph(2.0)],
             "rect": [sph(0.0), host.Rect(0, 0.0, 0.0, 1.0, 1.0, 1.0, mat), sph(2.0)],
             "instanced": [sph(0.0), host.Traslate(sph(0.0), (1.0, 0.0, 0.0)), sph(2.0)]}
    lst = host.HittableList()
    lst.push(sph(1.0))
    lst.push(sph(1.0 + 0.7))
    cases["list"] = [sph(0.0), lst, sph(3.0)]
    for name, members in cases.items():
        host.seed_scene_rng(3)
        world = host.HittableList()
        world.push(host.BVHNode(members, 0.0, 1.0))
        world.push(sph(9.0))
        scene = host.lower(world)
        assert scene.refittable().tolist() == [name == "plain", False], name
        n = scene.desc().n_prims
        planes = R.from_desc(scene.desc())["prim_a"]
        if name == "plain":
            scene.update_prims(0, planes)
        else:
            before = R.from_desc(scene.desc())
            with pytest.raises(Exception, match="cannot be refit"):
                scene.update_prims(0, planes + np.float32(0.5))
            after = R.from_desc(scene.desc())
            assert all(before[k].tobytes() == after[k].tobytes() for k in before), name  # refused: nothing changed
            scene.update_prims(n - 1, planes[n - 1:] + np.float32(0.5))  # the list primitive behind the tree may move


def test_refit_desc_refusals_and_the_empty_range(host):
    lib = abi.load_rtmi()
    scene = host.lower(R.build_world(host, R.spec_of("two")))
    base, arr = scene.desc(), R.from_desc(scene.desc())
    n = len(arr["prim_a"])
    out = {k: v.copy() for k, v in arr.items()}
    ptrs = lambda o: [o["items"].ctypes.data_as(C.POINTER(abi.Item)), o["nodes"].ctypes.data_as(C.POINTER(abi.BvhNode)),
                      o["alt_nodes"].ctypes.data_as(C.POINTER(abi.Bvh4Node)), o["prim_gate"].ctypes.data]
    d = R.to_desc(arr, base)
    assert lib.rtmu_refit_desc(None, 0, 1, *ptrs(out)) == 1 and _err().startswith("rtmu_refit_desc: ")
    assert lib.rtmu_refittable(None, None) == 1 and _err().startswith("rtmu_refittable: ")
    assert lib.rtmu_refittable(C.byref(d), None) == 1
    for k in range(3):  # a NULL output array
        p = ptrs(out)
        p[k] = None
        assert lib.rtmu_refit_desc(C.byref(d), 0, n, *p) == 1 and "NULL" in _err()
    for first, count in ((0, n + 1), (n, 1), (n + 1, 0), (2 ** 32 - 1, 2)):
        assert lib.rtmu_refit_desc(C.byref(d), first, count, *ptrs(out)) == 1 and "range" in _err(), (first, count)
    for first in (0, 3, n):  # count == 0: RTMI_OK and nothing written, whatever the output pointers are
        assert lib.rtmu_refit_desc(C.byref(d), first, 0, None, None, None, None) == 0
    assert all(out[k].tobytes() == arr[k].tobytes() for k in arr)
    # a range that touches a BVH item that cannot be refit: RTMI_ERR_UNSUPPORTED, nothing written
    a = {k: v.copy() for k, v in arr.items()}
    bvh = [i for i, it in enumerate(a["items"]) if it["kind"] == abi.ITEM_BVH]
    a["items"][bvh[1]]["scale"] = 1e30
    d2 = R.to_desc(a, base)
    leaves = sorted(R.item_leaves(a, bvh[1]))
    out = {k: v.copy() for k, v in a.items()}
    assert lib.rtmu_refit_desc(C.byref(d2), leaves[2], 1, *ptrs(out)) == 2 and "cannot be refit" in _err()
    assert all(out[k].tobytes() == a[k].tobytes() for k in a)
    first = sorted(R.item_leaves(a, bvh[0]))
    assert lib.rtmu_refit_desc(C.byref(d2), first[0], len(first), *ptrs(out)) == 0  # the other item still refits


def test_null_handles_are_refused_by_name():
    lib = abi.load_rtmi()
    x = np.zeros(4, np.float32)
    rec = abi.Xform(0, 0.0, 0.0, 0.0)
    for name, call in (("rtmu_scene_update_prims", lambda: lib.rtmu_scene_update_prims(None, 0, 1, x.ctypes.data, None)),
                       ("rtmu_scene_update_prims_device", lambda: lib.rtmu_scene_update_prims_device(None, 0, 1, None, None, None)),
                       ("rtmu_scene_update_xforms", lambda: lib.rtmu_scene_update_xforms(None, 0, 1, C.byref(rec))),
                       ("rtmu_probe_scene_words", lambda: lib.rtmu_probe_scene_words(None, 0, None, 0, None))):
        assert call() == 1 and _err().startswith(name + ": ") and "scene" in _err(), name


def test_prims_of_names_what_was_lowered_from_an_object(host):
    host.seed_scene_rng(5)
    mat = host.Lambertian(host.SolidTexture(0.5, 0.5, 0.5))
    spheres = [host.Sphere((float(k), 0.0, 0.0), 0.25 + 0.01 * k, mat) for k in range(7)]
    cube = host.Cube((0.0, 2.0, 0.0), (1.0, 3.0, 1.0), mat)
    bvh = host.BVHNode(spheres[:5], 0.0, 1.0)
    moved = host.Traslate(host.Rotate(1, cube, 30.0), (0.0, 0.0, 2.0))
    fog = host.ConstantMedium(spheres[5], 0.5, host.SolidTexture(1.0, 1.0, 1.0))
    world = host.HittableList()
    for obj in (bvh, host.FlipNormals(spheres[6]), moved, fog):
        world.push(obj)
    scene = host.lower(world)
    a = R.from_desc(scene.desc())["prim_a"]
    n = len(a)
    assert n == 8 and sorted(scene.prims_of(world).tolist()) == list(range(n))
    for k, s in enumerate(spheres):  # a primitive, wherever it sits: found by its radius
        (p,) = scene.prims_of(s).tolist()
        assert a[p][3] == np.float32(0.25 + 0.01 * k) and a[p][0] == np.float32(k)
    in_tree = scene.prims_of(bvh).tolist()
    assert len(in_tree) == 5 and sorted(in_tree) == sorted(int(scene.prims_of(s)[0]) for s in spheres[:5])
    assert scene.prims_of(fog).tolist() == scene.prims_of(spheres[5]).tolist()
    assert scene.prims_of(moved).tolist() == scene.prims_of(cube).tolist() and a[scene.prims_of(cube)[0]][1] == 2.0
    assert scene.prims_of(host.Sphere((0.0, 0.0, 0.0), 1.0, mat)).tolist() == []  # not in this world
    assert scene.desc().n_prims == n  # the description itself is what it was (its byte dumps: tests/golden)


def test_update_xforms_of_a_scene_that_is_not_resident(host):
    mat = host.Lambertian(host.SolidTexture(0.5, 0.5, 0.5))
    world = host.HittableList()
    world.push(host.Traslate(host.Rotate(1, host.Cube((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), mat), 30.0), (1.0, 2.0, 3.0)))
    world.push(host.Sphere((5.0, 0.0, 0.0), 1.0, mat))
    scene = host.lower(world)
    d = scene.desc()
    assert d.n_xforms == 2 and (d.xforms[0].kind, d.xforms[1].kind) == (abi.XF_TRANSLATE, abi.XF_ROTATE_Y)
    scene.update_xforms(0, [(abi.XF_TRANSLATE, 4.0, 5.0, 6.0), (abi.XF_ROTATE_Y, 0.6, 0.8, 0.0)])
    d = scene.desc()
    assert [(x.kind, x.x, x.y, x.z) for x in (d.xforms[0], d.xforms[1])] == [(0, 4.0, 5.0, 6.0), (2, np.float32(0.6), np.float32(0.8), 0.0)]
    with pytest.raises(Exception, match="kind"):
        scene.update_xforms(0, [(abi.XF_ROTATE_Y, 0.6, 0.8, 0.0)])
    with pytest.raises(Exception, match="range"):
        scene.update_xforms(1, [(abi.XF_ROTATE_Y, 0.6, 0.8, 0.0)] * 2)
    scene.update_xforms(2, [])


# ---- the host evaluation under sanitizers, in a program of its own -----------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = r"""
#include "rtmi_refit.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
// file: n_items n_prims n_nodes n_alt first count (uint32 each), then items, prim_a, prim_b, prim_meta, prim_gate, nodes, alt_nodes
template <typename T> static bool rd(FILE *f, std::vector<T> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }
template <typename T> static bool wr(FILE *f, const std::vector<T> &v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }
int main(int argc, char **argv) {
    if (argc < 4) return 2;
    FILE *f = fopen(argv[1], "rb");
    uint32_t h[6];
    if (!f || fread(h, 4, 6, f) != 6) return 2;
    std::vector<rtmi_item> items; std::vector<float> a, b, gate; std::vector<rtmi_prim_meta> meta;
    std::vector<rtmi_bvh_node> nodes; std::vector<rtmi_bvh4_node> alt;
    if (!rd(f, items, h[0]) || !rd(f, a, (size_t)h[1] * 4) || !rd(f, b, (size_t)h[1] * 4) || !rd(f, meta, h[1]) || !rd(f, gate, (size_t)h[1] * 8) ||
        !rd(f, nodes, h[2]) || !rd(f, alt, h[3])) return 2;
    fclose(f);
    const std::string mode = argv[3];
    if (mode == "child") nodes[(size_t)items[0].first].right = (int32_t)h[2] + 5;        // a child outside the array
    if (mode == "cycle") nodes[(size_t)items[0].first].left = items[0].first;             // a node that is its own child
    if (mode == "altcycle") { for (auto &n : alt) for (int c = 0; c < 4; c++) if (n.child[c] >= 0 && n.child[c] != RTMI_NO_CHILD) n.child[c] = items[0].alt_first; }
    if (mode == "leaf") nodes[(size_t)items[0].first].left = RTMI_LEAF(0, h[1] + 7);    // a leaf outside the primitives
    rtmi_scene_desc d{};
    d.n_items = h[0]; d.items = items.data(); d.n_prims = h[1]; d.prim_a = a.data(); d.prim_b = b.data(); d.prim_meta = meta.data();
    d.prim_gate = gate.data(); d.n_nodes = h[2]; d.nodes = nodes.data(); d.n_alt_nodes = h[3]; d.alt_nodes = alt.data();
    std::vector<uint8_t> mask(h[0] + 1, 9);
    std::string err;
    int rc = refit_refittable(&d, mask.data(), err);
    if (!rc) rc = refit_desc(&d, h[4], h[5], items.data(), nodes.data(), alt.data(), gate.data(), err); // in place: desc's own arrays
    printf("%d %s\n", rc, err.c_str());
    if (rc) return 0;
    FILE *o = fopen(argv[2], "wb");
    if (!o || !wr(o, items) || !wr(o, gate) || !wr(o, nodes) || !wr(o, alt) || fwrite(mask.data(), 1, h[0], o) != h[0]) return 2;
    fclose(o);
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("refit")
    src, exe = d / "refit.cpp", d / "refit"
    src.write_text(PROG)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "raytracing_rust_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe)], check=True)

    def run(arr, first, count, mode="refit"):
        inp, out = d / "in.bin", d / "out.bin"
        head = np.array([len(arr["items"]), len(arr["prim_a"]), len(arr["nodes"]), len(arr["alt_nodes"]), first, count], "<u4")
        inp.write_bytes(b"".join(x.tobytes() for x in (head, arr["items"], arr["prim_a"], arr["prim_b"], arr["prim_meta"],
                                                        arr["prim_gate"], arr["nodes"], arr["alt_nodes"])))
        if out.exists():
            out.unlink()
        r = subprocess.run([str(exe), str(inp), str(out), mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
        assert r.returncode == 0 and b"Sanitizer" not in r.stderr and b"runtime error" not in r.stderr, r.stderr.decode()
        rc, _, msg = r.stdout.decode().strip().partition(" ")
        return int(rc), msg, out.read_bytes() if out.exists() else None
    return run


@pytest.mark.parametrize("kind", R.KINDS)
def test_host_evaluation_under_sanitizers_gives_the_library_bytes(host, program, kind):
    spec = R.spec_of(kind)
    scene = host.lower(R.build_world(host, spec))
    arr = R.from_desc(scene.desc())
    a, b = R.new_planes(arr, spec, R.moved_spec(spec, 31))
    moved = dict(arr, prim_a=a, prim_b=b)
    n = len(a)
    for first, count in ((0, n), (n // 3, max(1, n // 2)), (n - 1, 0)):
        out = {k: v.copy() for k, v in moved.items()}
        d = R.to_desc(moved, scene.desc())
        rc = abi.load_rtmi().rtmu_refit_desc(C.byref(d), first, count, out["items"].ctypes.data_as(C.POINTER(abi.Item)),
                                             out["nodes"].ctypes.data_as(C.POINTER(abi.BvhNode)),
                                             out["alt_nodes"].ctypes.data_as(C.POINTER(abi.Bvh4Node)), out["prim_gate"].ctypes.data)
        mask = np.zeros(len(arr["items"]), np.uint8)
        assert rc == 0 and abi.load_rtmi().rtmu_refittable(C.byref(d), mask.ctypes.data) == 0
        got = program(moved, first, count)
        assert got[0] == 0, got[1]
        want = b"".join(x.tobytes() for x in (out["items"], out["prim_gate"], out["nodes"], out["alt_nodes"], mask))
        assert got[2] == want, (kind, first, count)


def test_malformed_trees_are_refused_under_sanitizers(host, program):
    scene = host.lower(R.build_world(host, R.spec_of("mix67")))
    arr = R.from_desc(scene.desc())
    assert arr["items"][0]["kind"] == abi.ITEM_BVH and arr["items"][0]["alt_first"] >= 0
    for mode in ("child", "cycle", "altcycle", "leaf"):
        rc, msg, out = program(arr, 0, len(arr["prim_a"]), mode)
        assert rc == 1 and out is None and ("node" in msg or "leaf" in msg), (mode, msg)
