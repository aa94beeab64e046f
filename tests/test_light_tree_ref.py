"""The light tree (include/rtmi_light_tree.h) without a GPU: the host build and the host form of the device's walks against
the numpy restatement of tests/light_tree_ref.py, and the properties the estimator rests on.

* rtmi_light_tree_from_desc is the numpy build byte for byte, nodes and paths;
* rtmi_light_tree_pick and rtmi_light_tree_pmf are numpy's bit for bit on more than 10^4 (x, u) per scene, with x at lamp
  centres and 10^6 away and u = 0 and 1 - 2^-24 among them;
* the probability a pick returns is the pmf of the light it returns, bit for bit;
* the pmf sums to 1 over the lights within 4 (depth + 1) 2^-24: two roundings per level (the quotient and the product)
  plus the sum's own;
* picks over 2^16 stratified uniforms reproduce the pmf within five binomial standard deviations per light."""
import ctypes as C

import numpy as np
import pytest

import light_tree_ref as ref
import light_tree_scenes as lts
from raytracing_rust_amd import abi

ALL = lts.WITH_LIGHTS + ["no_light", "final_scene"]


def _scene(host, name):
    return host.lower(lts.build(host, name, 16, 16)[1])


def _c_pick(nodes, x, u):
    lib = abi.load_rtmi()
    light, p = np.zeros(len(u), np.uint32), np.zeros(len(u), np.float32)
    rc = lib.rtmi_light_tree_pick(nodes.ctypes.data, len(nodes), x.ctypes.data, u.ctypes.data, len(u), light.ctypes.data, p.ctypes.data)
    assert rc == 0, lib.rtmi_last_error()
    return light, p


def _c_pmf(nodes, paths, x, lights):
    lib = abi.load_rtmi()
    lights = np.ascontiguousarray(lights, np.uint32)
    p = np.zeros(len(lights), np.float32)
    rc = lib.rtmi_light_tree_pmf(nodes.ctypes.data, len(nodes), paths.ctypes.data, x.ctypes.data, lights.ctypes.data, len(lights),
                                 p.ctypes.data)
    assert rc == 0, lib.rtmi_last_error()
    return p


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", ALL)
def test_build_is_the_numpy_build(host, name):
    sc = _scene(host, name)
    nodes, paths = sc.light_tree()
    n = len(sc.lights())
    assert len(nodes) == 2 * n and len(paths) == n
    want_nodes, want_paths = ref.build_scene(sc)
    assert nodes.tobytes() == want_nodes.tobytes()
    assert paths.tobytes() == want_paths.tobytes()
    if n == 0:
        return
    # the layout the header promises: slot 0 zero, even links, leaves name every light once, depth <= ceil(log2 n)
    assert not np.any(nodes[:1].view(np.uint8))
    leaf = (nodes["link"][1:] & ref.LEAF) != 0
    assert sorted((nodes["link"][1:][leaf] & 0x7FFFFFFF).tolist()) == list(range(n))
    assert np.all(nodes["link"][1:][~leaf] % 2 == 0) and np.all(nodes["r2"][1:] > 0) and np.all(nodes["power"][1:] > 0)
    assert paths["depth"].max() == int(np.ceil(np.log2(n))) if n > 1 else paths["depth"].max() == 0
    # a capped call writes what fits and still reports the full count
    lib = abi.load_rtmi()
    d = sc.desc()
    cnt = C.c_uint32(0)
    few = np.zeros(2, nodes.dtype)
    assert lib.rtmi_light_tree_from_desc(C.byref(d), few.ctypes.data_as(C.POINTER(abi.LightNode)), 2, C.byref(cnt), None) == 0
    assert cnt.value == 2 * n and few.tobytes() == nodes[:2].tobytes()


def test_one_light_has_probability_one(host):
    sc = _scene(host, "one_light")
    nodes, paths = sc.light_tree()
    assert len(nodes) == 2 and nodes["link"][1] == ref.LEAF and paths[0].tolist() == (0, 0)
    x, u = lts.probe_points(*ref.light_boxes(sc)[:2], n=256)
    light, p = _c_pick(nodes, x, u)
    assert not light.any() and np.all(_bits(p) == _bits(np.float32(1.0)))
    assert np.all(_bits(_c_pmf(nodes, paths, x, light)) == _bits(np.float32(1.0)))


@pytest.mark.parametrize("name", lts.WITH_LIGHTS)
def test_walks_are_numpy_bit_for_bit(host, name):
    sc = _scene(host, name)
    nodes, paths = sc.light_tree()
    lo, hi, _ = ref.light_boxes(sc)
    x, u = lts.probe_points(lo, hi)
    assert len(u) >= 10 ** 4
    light, p = _c_pick(nodes, x, u)
    want_light, want_p = ref.pick(nodes, x, u)
    assert np.array_equal(light, want_light)
    assert np.array_equal(_bits(p), _bits(want_p))
    assert np.all(p > 0) and np.all(p <= 1)
    # the reverse walk: of the picked light (the same bits as the pick's probability) and of unrelated lights
    back = _c_pmf(nodes, paths, x, light)
    assert np.array_equal(_bits(back), _bits(p))
    assert np.array_equal(_bits(back), _bits(ref.pmf(nodes, paths, x, light)))
    other = np.random.default_rng(5).integers(0, len(paths), len(u)).astype(np.uint32)
    assert np.array_equal(_bits(_c_pmf(nodes, paths, x, other)), _bits(ref.pmf(nodes, paths, x, other)))


@pytest.mark.parametrize("name", lts.WITH_LIGHTS)
def test_pmf_sums_to_one(host, name):
    sc = _scene(host, name)
    nodes, paths = sc.light_tree()
    n = len(paths)
    lo, hi, _ = ref.light_boxes(sc)
    x = lts.probe_points(lo, hi, n=4096)[0][:160:5]  # lamp centres, near them, 10^6 away and ordinary points
    pts = np.repeat(x, n, axis=0)
    p = _c_pmf(nodes, paths, pts, np.tile(np.arange(n, dtype=np.uint32), len(x))).astype(np.float64).reshape(len(x), n)
    bound = 4.0 * (int(paths["depth"].max()) + 1) * 2.0 ** -24
    err = np.abs(p.sum(1) - 1.0)
    print("\nLIGHT-TREE-SUM %s lights %d depth %d max |sum - 1| %.3g (bound %.3g)" % (name, n, paths["depth"].max(), err.max(), bound))
    assert err.max() <= bound, (name, err.max(), bound)


@pytest.mark.parametrize("name", lts.WITH_LIGHTS)
def test_stratified_picks_reproduce_the_pmf(host, name):
    sc = _scene(host, name)
    nodes, paths = sc.light_tree()
    n = len(paths)
    lo, hi, _ = ref.light_boxes(sc)
    N = 1 << 16
    u = ((np.arange(N) + 0.5) / N).astype(np.float32)
    rng = np.random.default_rng(11)
    blo, bhi = lo.min(0), hi.max(0)
    for x in rng.uniform(blo - 1.0, bhi + 1.0, (4, 3)).astype(np.float32):
        pts = np.repeat(x[None, :], N, axis=0)
        light, _ = _c_pick(nodes, pts, u)
        count = np.bincount(light, minlength=n).astype(np.float64)
        p = _c_pmf(nodes, paths, np.repeat(x[None, :], n, axis=0), np.arange(n, dtype=np.uint32)).astype(np.float64)
        sigma = np.sqrt(N * p * (1.0 - p))
        assert np.all(np.abs(count - N * p) <= 5.0 * sigma), (name, x, np.abs(count - N * p).max())
