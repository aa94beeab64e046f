"""The public interface of the lights that follow an update (include/rtmi_relight.h), without a GPU.

* the header compiles as C99; librtmi.so and librt_host.so export the entries, abi.py and sys.rs declare them;
* NULL handles are refused by name;
* the host evaluation (csrc/rtmi_relight.hpp), compiled alone into a program of its own under the address and
  undefined-behaviour sanitizers, gives the library's bytes on the shared light lists and refuses malformed trees.  Nothing
  is loaded into Python for that."""
import os
import re
import subprocess

import numpy as np
import pytest

import abi_kit as kit
import refit_ref as R
import relight_ref as L
from raytracing_rust_amd import abi

ENTRIES = ["rtml_probe_light_words", "rtml_relight_desc", "rtml_scene_follow_lights"]
HOST_ENTRIES = ["rthl_follow_lights", "rthl_probe_light_words"]
# The family carries the prefix rtml_ (rthl_ in the host library) and its own tables in abi.py (RELIGHT_ENTRIES,
# RELIGHT_HOST_ENTRIES), as the update family does: the kit's parsers read rtmi_ / rth_ names, so this file states the same
# chain for the other prefix.  Family serves the checks that need no name: C99, structs, isolation.
FAMILY = kit.Family("rtmi_relight.h", ENTRIES, includes=["rtmi_nee.h"])
WORDS = ["LIGHTS", "PRIM_LIGHT", "TREE_NODES", "TREE_PATHS"]


def test_header_is_c99(tmp_path):
    FAMILY.c99(tmp_path, holds=" && ".join("RTML_WORDS_%s == %d" % (w, k) for k, w in enumerate(WORDS)))


def _prototypes():
    return kit._c_functions(kit.header_text("rtmi_relight.h"), r"^(?!static\b|typedef\b)([A-Za-z_][\w \t\*]*?)\b(rtml_\w+)\s*\(([^;{}]*?)\)\s*;")


def _agree(name, proto, restype, argtypes):
    ret, args = proto
    assert kit.c_class(ret) == kit.ctypes_class(restype), name
    assert [kit.c_class(a) for a in args] == [kit.ctypes_class(t) for t in argtypes], name


def test_exports_and_declarations_agree():
    """header prototypes == abi.RELIGHT_ENTRIES == ENTRIES == the block of sys.rs == what librtmi.so exports with the prefix,
    argument by argument; the host wrappers likewise against their definitions"""
    FAMILY.layout()
    FAMILY.isolation()
    assert kit.prototypes("rtmi_relight.h") == {}  # nothing here is an entry of the render ABI's tables
    protos = _prototypes()
    assert sorted(protos) == sorted(abi.RELIGHT_ENTRIES) == ENTRIES
    lib = abi.load_rtmi()
    for name, proto in protos.items():
        _agree(name, proto, *abi.RELIGHT_ENTRIES[name])
        fn = getattr(lib, name)
        assert (fn.restype, fn.argtypes) == abi.RELIGHT_ENTRIES[name]
    nm = lambda path: subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(rtml_\w+)\b", nm(lib._name)))) == ENTRIES
    block = kit.sys_block("rtmi_relight.h")
    rust = {n: (ret, [a.split(":", 1)[1].strip() for a in kit._split_args(args)])
            for n, args, ret in re.findall(r"pub fn (rtml_\w+)\s*\((.*?)\)\s*(?:->\s*([^;{]+?))?\s*;", block, re.S)}
    assert sorted(rust) == ENTRIES and not re.findall(r"pub fn rtml_", kit.SYS.replace(block, ""))
    for name, (rret, rargs) in rust.items():
        assert rret == "c_int" and [kit.rust_is_pointer(t) for t in rargs] == [kit.c_class(a) == "ptr" for a in protos[name][1]], name
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(kit.HOST_SOURCE).read(), flags=re.S)
    defined = kit._c_functions(text, r"^RTH_API\s+([A-Za-z_][\w \t\*]*?)\b(rthl_\w+)\s*\(([^;{}]*?)\)\s*\{")
    assert sorted(defined) == sorted(abi.RELIGHT_HOST_ENTRIES) == HOST_ENTRIES
    host = abi.bind_host_relight(abi.load_host())
    for name, proto in defined.items():
        _agree(name, proto, *abi.RELIGHT_HOST_ENTRIES[name])
    assert sorted(set(re.findall(r"\b(rthl_\w+)\b", nm(host._name)))) == HOST_ENTRIES
    consts = re.findall(r"\b(RTML_WORDS_\w+)\s*=\s*(\d+)", kit.header_text("rtmi_relight.h"))
    assert {k[len("RTML_WORDS_"):].lower(): int(v) for k, v in consts} == abi.LIGHT_WORDS and len(consts) == len(WORDS)


def test_null_handles_are_refused_by_name():
    lib = abi.load_rtmi()
    err = lambda: (lib.rtmi_last_error() or b"").decode()
    for name, call in (("rtml_scene_follow_lights", lambda: lib.rtml_scene_follow_lights(None, 1)),
                       ("rtml_probe_light_words", lambda: lib.rtml_probe_light_words(None, 0, None, 0, None)),
                       ("rtml_relight_desc", lambda: lib.rtml_relight_desc(None, None, 0, None, 0))):
        assert call() == 1 and err().startswith(name + ": "), name


# ---- the host evaluation under sanitizers, in a program of its own -----------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = r"""
#include "rtmi_relight.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
// file: n_prims n_lights n_nodes (uint32 each), then prim_a, prim_b, prim_meta, lights, nodes
template <typename T> static bool rd(FILE *f, std::vector<T> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }
template <typename T> static bool wr(FILE *f, const std::vector<T> &v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }
int main(int argc, char **argv) {
    if (argc < 4) return 2;
    FILE *f = fopen(argv[1], "rb");
    uint32_t h[3];
    if (!f || fread(h, 4, 3, f) != 3) return 2;
    std::vector<float> a, b; std::vector<rtmi_prim_meta> meta; std::vector<rtmi_light> lights; std::vector<rtmi_light_node> nodes;
    if (!rd(f, a, (size_t)h[0] * 4) || !rd(f, b, (size_t)h[0] * 4) || !rd(f, meta, h[0]) || !rd(f, lights, h[1]) || !rd(f, nodes, h[2])) return 2;
    fclose(f);
    const std::string mode = argv[3];
    if (mode == "link") nodes[1].link = h[2] + 6;                   // a link outside the array
    if (mode == "self") nodes[1].link = 0;                          // a link that does not point behind its node
    if (mode == "leaf") nodes.back().link = RTMI_RELIGHT_LEAF | h[1]; // a leaf outside the table
    if (mode == "prim") lights[0].prim = (int32_t)h[0] + 3;         // a table entry outside the description
    rtmi_scene_desc d{};
    d.n_items = 1u << 20; // (the items are not read: every item index of the table passes)
    d.n_prims = h[0]; d.prim_a = a.data(); d.prim_b = b.data(); d.prim_meta = meta.data();
    std::string err;
    const int rc = relight_desc(&d, lights.data(), h[1], nodes.empty() ? nullptr : nodes.data(), h[2], err);
    std::vector<uint32_t> order, lvl;
    if (!rc && h[2]) relight_levels(nodes.data(), h[2], order, lvl);
    printf("%d %s\n", rc, err.c_str());
    if (rc) return 0;
    FILE *o = fopen(argv[2], "wb");
    if (!o || !wr(o, lights) || !wr(o, nodes) || !wr(o, order)) return 2;
    fclose(o);
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("relight")
    src, exe = d / "relight.cpp", d / "relight"
    src.write_text(PROG)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "raytracing_rust_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe)], check=True)

    def run(arr, lights, nodes, mode="relight"):
        inp, out = d / "in.bin", d / "out.bin"
        head = np.array([len(arr["prim_a"]), len(lights), len(nodes)], "<u4")
        inp.write_bytes(b"".join(x.tobytes() for x in (head, arr["prim_a"], arr["prim_b"], arr["prim_meta"], lights, nodes)))
        if out.exists():
            out.unlink()
        r = subprocess.run([str(exe), str(inp), str(out), mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
        assert r.returncode == 0 and b"Sanitizer" not in r.stderr and b"runtime error" not in r.stderr, r.stderr.decode()
        rc, _, msg = r.stdout.decode().strip().partition(" ")
        return int(rc), msg, out.read_bytes() if out.exists() else None
    return run


@pytest.mark.parametrize("n", L.COUNTS)
def test_host_evaluation_under_sanitizers_gives_the_library_bytes(host, program, n):
    scene = host.lower(L.light_list(host, n))
    arr = R.from_desc(scene.desc())
    lights, nodes, _ = L.table_of(scene)
    a, b = L.moved_planes(arr, lights, 20 + n)
    moved = dict(arr, prim_a=a, prim_b=b)
    rc, want_l, want_n = L.relight(moved, scene.desc(), lights, nodes)
    assert rc == 0
    got = program(moved, lights, nodes)
    assert got[0] == 0, got[1]
    size = want_l.nbytes + want_n.nbytes
    assert got[2][:size] == want_l.tobytes() + want_n.tobytes()
    order = np.frombuffer(got[2][size:], "<u4")  # the kernel's levels: every slot below the root once, children before parents
    assert sorted(order.tolist()) == list(range(1, 2 * n))
    place = {int(s): k for k, s in enumerate(order)}
    for s in range(1, 2 * n):
        link = int(nodes[s]["link"])
        assert link & L.LEAF or (place[link] < place[s] and place[link + 1] < place[s])


def test_malformed_tables_are_refused_under_sanitizers(host, program):
    scene = host.lower(L.light_list(host, 65))
    arr = R.from_desc(scene.desc())
    lights, nodes, _ = L.table_of(scene)
    for mode, word in (("link", "link"), ("self", "link"), ("leaf", "leaf"), ("prim", "outside")):
        rc, msg, out = program(arr, lights, nodes, mode)
        assert rc == 1 and out is None and word in msg, (mode, msg)
