"""The public interface of RTMI_FLAG_LIGHT_COOP (include/rtmi_light_coop.h): the NEE and environment entries on the
wave-cooperative kernel, without a GPU.

* the header compiles as C99 -pedantic next to rtmi.h;
* the flag is bit 16, disjoint from every RTMI_FLAG_* of rtmi.h and from the knob bits 8-11, and abi.py and sys.rs say
  the same;
* the four lighting entries accept the flag (and bit 11, the small-pool knob, together with it): with valid params and a
  NULL scene the call gets as far as the scene check; every other bit beside the flag is still refused;
* every other whole-image entry refuses the flag as an unknown bit;
* render_adaptive(coop=True) without nee or env raises ValueError before any native call."""
import ctypes as C
import os
import re

import pytest

import abi_kit as kit
from raytracing_rust_amd import abi
from raytracing_rust_amd.host import Scene, default_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "rtmi_light_coop.h")
FLAG = 65536
FC = abi.RTMI_FLAG_FAST_CULL
LIT = ["nee", "env", "adaptive_nee", "adaptive_env"]
OTHERS = ["roulette", "adaptive_roulette", "features", "adaptive"]
ERR_INVALID, ERR_UNSUPPORTED = 1, 2  # RTMI_ERR_INVALID, RTMI_ERR_UNSUPPORTED (include/rtmi.h)


def _header_define(path, name):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    m = re.search(r"#define\s+%s\s+\(?\s*(0x[0-9a-fA-F]+|\d+)u?" % name, text)
    assert m, name
    return int(m.group(1), 0)


# no entries and no word: the header is one flag of the NEE / environment entries
FAMILY = kit.Family("rtmi_light_coop.h", [])


def test_header_is_c99(tmp_path):
    FAMILY.c99(tmp_path, before=("rtmi.h",), run=True, body="rtmi_render_params p; p.flags = RTMI_FLAG_FAST_CULL | RTMI_FLAG_LIGHT_COOP;",
               holds="p.flags == 65537u")
    FAMILY.exports()
    FAMILY.layout()  # no function, no struct
    FAMILY.isolation()


def test_flag_value_and_disjointness():
    assert _header_define(HEADER, "RTMI_FLAG_LIGHT_COOP") == FLAG == 1 << 16
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "rtmi.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"#define\s+(RTMI_FLAG_[A-Z0-9_]+)\b", text) + re.findall(r"\b(RTMI_FLAG_[A-Z0-9_]+)\s*=", text)))
    assert len(names) >= 12, names
    taken = 0
    for n in names:
        m = re.search(r"%s\s*(?:=\s*)?\(?\s*(0x[0-9a-fA-F]+|\d+)u?(?:\s*<<\s*(\d+))?" % n, text)
        assert m, n
        v = int(m.group(1), 0) << int(m.group(2) or 0)
        assert v & FLAG == 0, n
        taken |= v
    assert taken & FLAG == 0 and (0xf << 8) & FLAG == 0
    assert taken | (0xf << 8) == 0xffff  # bits 0-15 are flags and knobs: bit 16 is the first free one


def test_python_and_rust_constants():
    assert FAMILY.constants() == (["RTMI_FLAG_LIGHT_COOP"], ["RTMI_FLAG_LIGHT_COOP"]) and abi.RTMI_FLAG_LIGHT_COOP == FLAG
    kit.assert_rust_const("RTMI_FLAG_LIGHT_COOP", "u32", FLAG)


def _call(entry, flags, scene=None):
    """The entry with valid params, a camera and a NULL scene -> (return code, message)."""
    lib = abi.load_rtmi()
    p = default_params(32, 24, 16, flags=flags)
    a = abi.Adaptive(4, 4, 0.0, 0.0)
    o = abi.EnvRender(1, 0.5)
    r = abi.Roulette(abi.RTMI_ROULETTE_NEE, 3, 0.05, 0.5)
    c = abi.Camera()
    pc, cc = C.byref(p), C.byref(c)
    if entry == "nee":
        rc = lib.rtmi_render_nee(scene, cc, pc, None, None, None, None, None)
    elif entry == "env":
        rc = lib.rtmi_render_env(scene, cc, pc, C.byref(o), None, None, None, None, None)
    elif entry == "adaptive_nee":
        rc = lib.rtmi_render_adaptive_nee(scene, cc, pc, C.byref(a), None, None, None, None, None)
    elif entry == "adaptive_env":
        rc = lib.rtmi_render_adaptive_env(scene, cc, pc, C.byref(o), C.byref(a), None, None, None, None, None)
    elif entry == "roulette":
        rc = lib.rtmi_render_roulette(scene, cc, pc, C.byref(r), None, None, None, None, None)
    elif entry == "adaptive_roulette":
        rc = lib.rtmi_render_adaptive_roulette(scene, cc, pc, C.byref(r), C.byref(a), None, None, None, None, None, None)
    elif entry == "features":
        rc = lib.rtmi_render_features(scene, cc, pc, None, None, None, None, None, None)
    else:
        rc = lib.rtmi_render_adaptive(scene, cc, pc, C.byref(a), None, None, None, None, None)
    return rc, (lib.rtmi_last_error() or b"").decode()


@pytest.mark.parametrize("entry", LIT)
@pytest.mark.parametrize("extra", [0, 1 << 11], ids=["flag", "flag+pool_knob"])
def test_lighting_entries_accept_the_flag(entry, extra):
    """The flag check passes, so the NULL scene is what is refused (without the feature: RTMI_ERR_UNSUPPORTED)."""
    for base in (FC, 0, FC | abi.RTMI_FLAG_SYNC, FC | abi.RTMI_FLAG_REF_TREE):
        rc, msg = _call(entry, FLAG | extra | base)
        assert rc == ERR_INVALID and "scene is NULL" in msg, (entry, base, rc, msg)


@pytest.mark.parametrize("entry", LIT)
def test_pool_knob_alone_is_still_refused(entry):
    rc, msg = _call(entry, (1 << 11) | FC)
    assert rc == ERR_UNSUPPORTED and "flags" in msg, msg


@pytest.mark.parametrize("entry", LIT)
@pytest.mark.parametrize("extra", [1 << 20, 3 << 8, abi.RTMI_FLAG_PROFILE, 1 << 17, abi.RTMI_FLAG_TEST_OVERFLOW, abi.RTMI_FLAG_ASYNC,
                                   abi.RTMI_FLAG_BLOCK_COOP, abi.RTMI_FLAG_PROGRESSIVE])
def test_other_bits_beside_the_flag_are_unsupported(entry, extra):
    rc, msg = _call(entry, FLAG | extra | FC)
    assert rc == ERR_UNSUPPORTED and "flags" in msg, (rc, msg)


@pytest.mark.parametrize("entry", OTHERS)
def test_other_entries_refuse_the_flag(entry):
    rc, msg = _call(entry, FLAG | FC)
    assert rc == ERR_UNSUPPORTED, (entry, rc, msg)
    rc, msg = _call(entry, FC)  # the same call without it gets as far as the scene
    assert rc == ERR_INVALID and "scene" in msg, (entry, rc, msg)


def test_render_adaptive_coop_needs_a_lit_estimator():
    """Raised before the scene is touched: an object without any native state is enough."""
    sc = object.__new__(Scene)
    with pytest.raises(ValueError, match="coop"):
        sc.render_adaptive(None, 32, 24, 16, 4, 4, coop=True)
    with pytest.raises(ValueError, match="coop"):
        sc.render_denoised(None, 32, 24, 16, coop=True)
