"""Adaptive sampling's public interface (include/rtmi_adaptive.h), without a GPU.

* the header compiles as C99; the layout of rtmi_adaptive holds through header -> ctypes (abi.py) -> #[repr(C)]
  (bindings/rust/src/sys.rs), with the machinery of test_abi_layout.py;
* librtmi.so exports exactly the functions the header declares, and abi.py and sys.rs declare them;
* every bad argument is refused before any device work: RTMI_ERR_INVALID for bad values and a NULL scene,
  RTMI_ERR_UNSUPPORTED for the flags and the tile split the mode does not carry."""
import ctypes as C
import os
import re
import subprocess

import pytest

from raytracing_rust_amd import abi
from raytracing_rust_amd.host import default_params

from test_abi_layout import rust_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtmi_adaptive.h")
FIELDS = ["min_spp", "step_spp", "abs_tol", "rel_tol"]


def _c_layout(tmp_path):
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "rtmi_adaptive.h"', "int main(void) {",
             '  printf("%zu %zu\\n", sizeof(rtmi_adaptive), _Alignof(rtmi_adaptive));']
    for f in FIELDS:
        lines.append('  printf("%s %%zu %%zu\\n", offsetof(rtmi_adaptive, %s), sizeof(((rtmi_adaptive *)0)->%s));' % (f, f, f))
    lines += ["  return 0;", "}"]
    src, exe = str(tmp_path / "l.c"), str(tmp_path / "l")
    open(src, "w").write("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode().split("\n")
    size, align = map(int, out[0].split())
    return size, align, [(t[0], int(t[1]), int(t[2])) for t in (ln.split() for ln in out[1:] if ln)]


def test_header_is_c99(tmp_path):
    src = tmp_path / "c99.c"
    src.write_text('#include "rtmi_adaptive.h"\n'
                   "int main(void) { rtmi_adaptive a = {2u, 1u, 0.0, 0.0}; (void)a; (void)&rtmi_render_adaptive; return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-c", "-o", str(tmp_path / "c99.o")], check=True)


def test_layout_chain_header_ctypes_rust(tmp_path):
    size, align, fields = _c_layout(tmp_path)
    assert [f[0] for f in fields] == FIELDS and (size, align) == (24, 8)
    assert (C.sizeof(abi.Adaptive), C.alignment(abi.Adaptive)) == (size, align)
    assert [(n, getattr(abi.Adaptive, n).offset, getattr(abi.Adaptive, n).size) for n, _ in abi.Adaptive._fields_] == fields
    assert rust_layout("RtmiAdaptive") == (size, align, fields)


def test_exports_and_declarations_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rtmi_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(abi.RTMI_ADAPTIVE_SYMBOLS) == ["rtmi_render_adaptive"]
    lib = abi.load_rtmi()
    for n in declared:
        assert hasattr(lib, n), n
    sysrs = open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()
    for n in declared:
        assert re.search(r"pub fn %s\(" % n, sysrs), n
    assert not set(declared) & (set(abi.RTMI_SYMBOLS) | set(abi.RTMI_F64_SYMBOLS))
    host = abi.load_host()
    assert hasattr(host, "rth_render_adaptive")


def _call(params=None, adaptive=None, scene=None, cam=True):
    lib = abi.load_rtmi()
    p = default_params(32, 24, 16) if params is None else params
    a = abi.Adaptive(4, 4, 0.0, 0.0) if adaptive is None else adaptive
    c = abi.Camera()
    rc = lib.rtmi_render_adaptive(scene, C.byref(c) if cam else None, C.byref(p), C.byref(a), None, None, None, None, None)
    return rc, (lib.rtmi_last_error() or b"").decode()


@pytest.mark.parametrize("adaptive, what", [
    (abi.Adaptive(1, 4, 0.0, 0.0), "min_spp"),
    (abi.Adaptive(0, 4, 0.0, 0.0), "min_spp"),
    (abi.Adaptive(17, 4, 0.0, 0.0), "min_spp"),
    (abi.Adaptive(4, 0, 0.0, 0.0), "step_spp"),
    (abi.Adaptive(4, 4, -1e-3, 0.0), "abs_tol"),
    (abi.Adaptive(4, 4, 0.0, -0.5), "rel_tol"),
    (abi.Adaptive(4, 4, float("nan"), 0.0), "abs_tol"),
    (abi.Adaptive(4, 4, 0.0, float("nan")), "rel_tol"),
    (abi.Adaptive(4, 4, float("inf"), 0.0), "abs_tol"),
])
def test_bad_adaptive_arguments_are_invalid_without_a_device(adaptive, what):
    rc, msg = _call(adaptive=adaptive)
    assert rc == 1 and what in msg, msg


def test_null_arguments_and_bad_params_are_invalid():
    assert _call()[0] == 1 and "scene" in _call()[1]  # every value valid: the NULL scene is what is refused
    assert _call(cam=False)[0] == 1
    lib = abi.load_rtmi()
    p = default_params(32, 24, 16)
    assert lib.rtmi_render_adaptive(None, C.byref(abi.Camera()), C.byref(p), None, None, None, None, None, None) == 1
    assert lib.rtmi_render_adaptive(None, C.byref(abi.Camera()), None, C.byref(abi.Adaptive(4, 4, 0.0, 0.0)), None, None, None, None,
                                    None) == 1
    assert _call(params=default_params(0, 24, 16))[0] == 1
    assert _call(params=default_params(32, 24, 16), adaptive=abi.Adaptive(16, 4, 0.0, 0.0))[0] == 1  # statistics only: valid values
    assert "scene" in _call(params=default_params(32, 24, 16), adaptive=abi.Adaptive(16, 4, 0.0, 0.0))[1]


@pytest.mark.parametrize("flag", [abi.RTMI_FLAG_PATH_SIG, 4, abi.RTMI_FLAG_ASYNC, 32768, abi.RTMI_FLAG_PROGRESSIVE, 8192, 1 << 11, 3 << 8])
def test_unsupported_flags(flag):
    rc, msg = _call(params=default_params(32, 24, 16, flags=flag | abi.RTMI_FLAG_FAST_CULL))
    assert rc == 2 and "flags" in msg, msg


def test_tile_split_is_unsupported():
    rc, msg = _call(params=default_params(32, 24, 16, tile_rank=1, tile_world=2))
    assert rc == 2 and "tile_world" in msg, msg


def test_accepted_flags_reach_the_scene_check():
    accepted = (abi.RTMI_FLAG_FAST_CULL | abi.RTMI_FLAG_SYNC | abi.RTMI_FLAG_REF_TREE | abi.RTMI_FLAG_SKY |
                abi.RTMI_FLAG_FACE_FORWARD | abi.RTMI_FLAG_UV_BOOK)
    rc, msg = _call(params=default_params(32, 24, 16, flags=accepted))
    assert rc == 1 and "scene" in msg, msg
