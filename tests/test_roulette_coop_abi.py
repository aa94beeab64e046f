"""The public interface of RTMI_FLAG_ROULETTE_COOP (include/rtmi_roulette_coop.h): the roulette entries on the
wave-cooperative kernel, without a GPU.

* the header compiles as C99 -pedantic next to rtmi.h and rtmi_roulette.h;
* the flag is bit 17, disjoint from every RTMI_FLAG_* of rtmi.h, from the knob bits 8-11 and from RTMI_FLAG_LIGHT_COOP,
  and abi.py and sys.rs say the same;
* both roulette entries accept the flag for all four estimators (and bit 11, the small-pool knob, together with it): with
  valid params and a NULL scene the call gets as far as the scene check; every other bit beside the flag, bit 16 among
  them, is still refused, and SKY with the map estimators is still invalid;
* every other whole-image entry refuses the flag as an unknown bit;
* render_roulette(coop=True) and render_adaptive_roulette(coop=True) OR exactly bit 17 into the params."""
import ctypes as C
import os
import re

import pytest

import abi_kit as kit
from raytracing_rust_amd import abi, host as host_mod
from raytracing_rust_amd.host import Scene, default_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "rtmi_roulette_coop.h")
FLAG = 131072
LIGHT_COOP = 65536
FC = abi.RTMI_FLAG_FAST_CULL
POOL_KNOB = 1 << 11
ENTRIES = ["roulette", "adaptive_roulette"]
ESTIMATORS = ["plain", "nee", "env", "env_nee"]
OTHERS = ["nee", "env", "adaptive_nee", "adaptive_env", "features", "adaptive"]
ERR_INVALID, ERR_UNSUPPORTED = 1, 2  # RTMI_ERR_INVALID, RTMI_ERR_UNSUPPORTED (include/rtmi.h)


def _header_define(path, name):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    m = re.search(r"#define\s+%s\s+\(?\s*(0x[0-9a-fA-F]+|\d+)u?" % name, text)
    assert m, name
    return int(m.group(1), 0)


# no entries and no word: the header is one flag of the roulette entries
FAMILY = kit.Family("rtmi_roulette_coop.h", [], includes=["rtmi.h", "rtmi_roulette.h"])


def test_header_is_c99(tmp_path):
    FAMILY.c99(tmp_path, before=("rtmi.h", "rtmi_roulette.h"), run=True,
               body="rtmi_render_params p; rtmi_roulette o; o.estimator = RTMI_ROULETTE_PLAIN; p.flags = RTMI_FLAG_FAST_CULL | RTMI_FLAG_ROULETTE_COOP;",
               holds="p.flags == 131073u && o.estimator == 0u")
    # the header alone pulls in what it names
    FAMILY.c99(tmp_path, body="rtmi_roulette o; o.min_depth = 1u;", holds="o.min_depth == 1u")
    FAMILY.exports()
    FAMILY.layout()  # no function, no struct
    FAMILY.isolation()


def test_flag_value_and_disjointness():
    assert _header_define(HEADER, "RTMI_FLAG_ROULETTE_COOP") == FLAG == 1 << 17
    assert FC | FLAG == 131073
    assert _header_define(os.path.join(INCLUDE, "rtmi_light_coop.h"), "RTMI_FLAG_LIGHT_COOP") == LIGHT_COOP
    assert LIGHT_COOP & FLAG == 0
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
    assert (taken | (0xf << 8) | LIGHT_COOP) & FLAG == 0
    assert taken | (0xf << 8) | LIGHT_COOP == 0x1ffff  # bits 0-16 are flags and knobs: bit 17 is the first free one


def test_python_and_rust_constants():
    assert FAMILY.constants() == (["RTMI_FLAG_ROULETTE_COOP"], ["RTMI_FLAG_ROULETTE_COOP"]) and abi.RTMI_FLAG_ROULETTE_COOP == FLAG
    kit.assert_rust_const("RTMI_FLAG_ROULETTE_COOP", "u32", FLAG)


def _call(entry, flags, estimator="nee", scene=None):
    """The entry with valid params, a camera and a NULL scene -> (return code, message)."""
    lib = abi.load_rtmi()
    p = default_params(32, 24, 16, flags=flags)
    a = abi.Adaptive(4, 4, 0.0, 0.0)
    o = abi.EnvRender(1, 0.5)
    r = abi.Roulette(abi.ROULETTE_ESTIMATORS[estimator], 3, 0.05, 0.5)
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


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("est", ESTIMATORS)
@pytest.mark.parametrize("extra", [0, POOL_KNOB], ids=["flag", "flag+pool_knob"])
def test_roulette_entries_accept_the_flag(entry, est, extra):
    """The flag check passes, so the NULL scene is what is refused (without the feature: RTMI_ERR_UNSUPPORTED)."""
    for base in (FC, 0, FC | abi.RTMI_FLAG_SYNC, FC | abi.RTMI_FLAG_REF_TREE):
        rc, msg = _call(entry, FLAG | extra | base, est)
        assert rc == ERR_INVALID and "scene is NULL" in msg, (entry, est, base, rc, msg)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("est", ESTIMATORS)
def test_pool_knob_alone_is_still_refused(entry, est):
    rc, msg = _call(entry, POOL_KNOB | FC, est)
    assert rc == ERR_UNSUPPORTED and "flags" in msg, msg


BESIDE = [1 << 20, 3 << 8, abi.RTMI_FLAG_PROFILE, abi.RTMI_FLAG_ASYNC, abi.RTMI_FLAG_BLOCK_COOP, abi.RTMI_FLAG_PROGRESSIVE,
          abi.RTMI_FLAG_TEST_OVERFLOW, abi.RTMI_FLAG_PATH_SIG, LIGHT_COOP]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("extra", BESIDE)
def test_other_bits_beside_the_flag_are_unsupported(entry, extra):
    for est in ESTIMATORS:
        rc, msg = _call(entry, FLAG | extra | FC, est)
        assert rc == ERR_UNSUPPORTED, (est, rc, msg)
        assert ("PATH_SIG" if extra == abi.RTMI_FLAG_PATH_SIG else "flags") in msg, msg
    rc, msg = _call(entry, LIGHT_COOP | FC)  # bit 16 alone as well (tests/test_light_coop_abi.py)
    assert rc == ERR_UNSUPPORTED, (rc, msg)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("est", ["env", "env_nee"])
def test_sky_with_a_map_estimator_is_still_invalid(entry, est):
    for extra in (0, POOL_KNOB):
        rc, msg = _call(entry, FLAG | extra | FC | abi.RTMI_FLAG_SKY, est)
        assert rc == ERR_INVALID and "SKY" in msg, (rc, msg)
    rc, msg = _call(entry, FLAG | FC | abi.RTMI_FLAG_SKY, "nee")  # the other two estimators take the sky
    assert rc == ERR_INVALID and "scene is NULL" in msg, (rc, msg)


@pytest.mark.parametrize("entry", OTHERS)
def test_other_entries_refuse_the_flag(entry):
    rc, msg = _call(entry, FLAG | FC)
    assert rc == ERR_UNSUPPORTED, (entry, rc, msg)
    rc, msg = _call(entry, FC)  # the same call without it gets as far as the scene
    assert rc == ERR_INVALID and "scene" in msg, (entry, rc, msg)


class _Stop(Exception):
    pass


@pytest.mark.parametrize("adaptive", [False, True], ids=["fixed", "adaptive"])
def test_python_coop_ors_exactly_bit_17(monkeypatch, adaptive):
    """On the params struct, with no native render: default_params is watched and the call stopped right after it."""
    seen = []

    def spy(*a, **kw):
        seen.append(int(kw.get("flags", 0)))
        raise _Stop()

    monkeypatch.setattr(host_mod, "default_params", spy)
    sc = object.__new__(Scene)
    sc.uploaded = True       # _ready() has nothing to do: no upload, no light table for the plain estimator
    sc.lights_attached = True
    for base in (0, FC, FC | abi.RTMI_FLAG_REF_TREE):
        for coop in (False, True):
            with pytest.raises(_Stop):
                if adaptive:
                    sc.render_adaptive_roulette(None, 32, 24, 16, 4, 4, estimator="plain", flags=base, coop=coop)
                else:
                    sc.render_roulette(None, 32, 24, 16, estimator="plain", flags=base, coop=coop)
            assert seen[-1] == (base | (FLAG if coop else 0)), (base, coop, seen[-1])
    # and the struct carries the word unchanged
    assert default_params(32, 24, 16, flags=FC | FLAG).flags == FC | FLAG == 131073
