"""The f64 render mode (include/rtmi_f64.h) against the f64 oracle on the random compositions (tests/scenes_random.py)
and on the hand-built worlds of tests/test_random_scenes.py.

The mode is the reference's double arithmetic on the device; + - * / and sqrt are correctly rounded on both sides, sin
(checker, noise), log (media), atan2 and asin (image texture on a sphere) are not.  Hence two tiers:
  * EXACT: scenes built with exact_ops=True (scenes_random.ExactOps: no noise, no image texture, no medium; a checker's
    sines enter through a sign only) and hand-built worlds of solid colours — double radiance, rgb8 and path signatures
    equal the oracle's, no tolerance.  This is where every transform chain, AABB::hit, primitive test, tree walk, tie
    rule, material and the camera of the f64 kernel are held bit for bit;
  * TOLERANCE: the scenes as they are, in groups of eight, inside the bounds of
    test_gpu_f64_mode.py::test_scenes_with_transcendentals_within_ulps_of_the_f64_oracle, plus a per-scene cap.
The image is 43 x 21: partial tiles on both axes (the resolve kernel's and the pass budget's ragged edge).  The seed lists
are the constants of tests/test_f64_random_scenes.py, which asserts them on the CPU: no scene is skipped at run time."""
import json
import os
import sys

import numpy as np
import pytest

import scenes_random
import test_f64_random_scenes as cpu
from oracle.oracle import FACE_FORWARD, SKY, THROUGHPUT_FORM
from raytracing_rust_amd import abi
from test_random_scenes import (PLACEMENTS, _bvh_world, _instanced_bvh_world, _list_leaf_world,
                                _medium_in_instanced_list_world)

pytestmark = pytest.mark.gpu

NX, NY, NS = 43, 21, 16
UNIT = (1.0, (0.0, 0.0, 0.0))
UP = (0.0, 1.0, 0.0)


def _extras(seed):
    """(device flags, oracle flags): SKY where seed % 3 == 0 (as test_random_scenes.py), FACE_FORWARD where seed % 4 == 0"""
    d, o = 0, 0
    if seed % 3 == 0:
        d, o = d | abi.RTMI_FLAG_SKY, o | SKY
    if seed % 4 == 0:
        d, o = d | abi.RTMI_FLAG_FACE_FORWARD, o | FACE_FORWARD
    return d, o


def _random_pair(host, orc64, seed, instanced, exact_ops, placement=UNIT, nx=NX, ny=NY):
    kw = dict(instanced=instanced, exact_ops=exact_ops, scale=placement[0], offset=placement[1])
    return scenes_random.build(host, seed, nx, ny, **kw), scenes_random.build(orc64, seed, nx, ny, **kw)


def _compositions(api):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import dump_flat_scene as dfs

    return dfs.compositions(api, 1)


def _seeded(seed, world_fn):
    def build(api):
        api.seed_scene_rng(seed)
        return world_fn(api)
    return build


# name -> (world(api), camera arguments before the aspect, camera arguments after it): the worlds and the cameras of
# tests/test_random_scenes.py
HAND_BUILT = {
    "instanced_bvh": (_seeded(1, _instanced_bvh_world), ((4.0, 3.0, 7.0), (0.0, 0.5, 0.0), UP, 40.0), (0.1, 8.0, 0.0, 1.0)),
    "list_leaf": (_list_leaf_world, ((0.5, 1.2, 6.0), (0.3, 0.6, 0.0), UP, 40.0), (0.05, 6.0, 0.0, 1.0)),
    "zx_rect_in_bvh": (_seeded(1, lambda api: _bvh_world(api, True)), ((5.0, 4.0, 7.0), (0.0, 0.5, 0.0), UP, 45.0),
                       (0.0, 10.0, 0.0, 1.0)),
    "shutter_beyond_sphere_times": (_seeded(1, lambda api: _bvh_world(api, False, (0.25, 0.75))),
                                    ((5.0, 4.0, 7.0), (0.0, 0.5, 0.0), UP, 45.0), (0.0, 10.0, 0.0, 1.0)),
    "medium_in_instanced_list": (_medium_in_instanced_list_world, ((0.5, 1.5, 7.0), (0.0, 0.5, 0.0), UP, 40.0),
                                 (0.05, 7.0, 0.0, 1.0)),
    "top_level_ties": (cpu.top_level_ties_world,) + cpu.TIES_CAMERA,
    "compositions": (_compositions, ((0.5, 1.5, 7.0), (0.0, 0.8, 0.0), UP, 40.0), (0.05, 7.0, 0.0, 1.0)),
}


def _hand_built_pair(host, orc64, name, nx, ny):
    world_fn, head, tail = HAND_BUILT[name]
    return tuple((api.Camera(*head, nx / ny, *tail), world_fn(api)) for api in (host, orc64))


def _render_both(host, orc64, pair, nx, ny, ns, dflags=0, oflags=0, max_depth=50, **kw):
    (cam, world), (camo, worldo) = pair
    sc = host.lower(world).upload(0, f64=True)
    got = sc.render(cam, nx, ny, ns, sig=True, seed=42, precision="f64", flags=dflags, max_depth=max_depth, **kw)
    ref = orc64.render(camo, worldo, nx, ny, ns, seed=42, flags=THROUGHPUT_FORM | oflags, max_depth=max_depth)
    return sc, cam, got, ref


def _assert_identical(got, ref, what):
    assert got["linear"].dtype == np.float64 and got["linear"].shape == ref["mean"].shape
    same = (got["linear"] == ref["mean"]) | (np.isnan(got["linear"]) & np.isnan(ref["mean"]))
    bad = np.argwhere((got["sig"] != ref["sig"]) | np.any(~same, axis=2))  # (row, column) of the pixels that differ
    assert np.array_equal(got["sig"], ref["sig"]), (what, "sig", bad[:8].tolist(), len(bad))
    assert np.array_equal(got["linear"], ref["mean"], equal_nan=True), (what, "linear", bad[:8].tolist(), len(bad))
    assert np.array_equal(got["rgb8"].astype(np.int32), ref["rgb"]), (what, "rgb8")


# ---- exact tier ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", cpu.EXACT_SET, ids=cpu.case_id)
def test_exact_random_scene_bit_identical_to_the_f64_oracle(host, orc64, case):
    seed, instanced = case
    dflags, oflags = _extras(seed)
    _sc, _cam, got, ref = _render_both(host, orc64, _random_pair(host, orc64, seed, instanced, True), NX, NY, NS, dflags, oflags)
    assert float(np.nanmean(ref["mean"])) > 0.0
    _assert_identical(got, ref, case)
    orc64.free_all()


@pytest.mark.parametrize("seed,placement", [pytest.param(s, (sc, off), id="%d-%s" % (s, name)) for name, sc, off in PLACEMENTS
                                            for s in cpu.SEEDS[:8]])
def test_exact_placed_scene_bit_identical_to_the_f64_oracle(host, orc64, seed, placement):
    """the scenes scaled and shifted away from the unit box (PLACEMENTS of test_random_scenes.py)"""
    dflags, oflags = _extras(seed)
    pair = _random_pair(host, orc64, seed, False, True, placement)
    _sc, _cam, got, ref = _render_both(host, orc64, pair, NX, NY, NS, dflags, oflags)
    _assert_identical(got, ref, (seed, placement))
    orc64.free_all()


@pytest.mark.parametrize("name", ["instanced_bvh", "list_leaf", "zx_rect_in_bvh", "shutter_beyond_sphere_times", "top_level_ties"])
def test_exact_hand_built_world_bit_identical_to_the_f64_oracle(host, orc64, name):
    """instanced BVH leaves, a HittableList as a BVH leaf with its tie rules (the tree's fold decides), a BVH whose boxes do
    not contain a ZX rect, a shutter wider than the moving sphere's times (prim_dt = 0.5), and exact ties inside the scan
    of a top-level list (the shrinking t_max decides: rect_test_d's t > t_max, sphere_test_d's t < t_max)"""
    nx, ny, ns = 48, 32, 8
    _sc, _cam, got, ref = _render_both(host, orc64, _hand_built_pair(host, orc64, name, nx, ny), nx, ny, ns)
    assert float(ref["mean"].mean()) > 0.0
    _assert_identical(got, ref, name)
    orc64.free_all()


@pytest.mark.parametrize("case", cpu.DEPTH_CASES, ids=cpu.case_id)
def test_exact_glass_and_metal_at_depth_limits_and_in_passes(host, orc64, case):
    """A scene with dielectrics and one with a Metal of fuzz >= 1 (cpu.GLASS_CASE, cpu.METAL_CASE and the next one) at
    max_depth 1, 2 and 50 (color.rs:9 at the limit), and at 50 once more in passes: sample_buffer_bytes of five samples
    for the 6 x 3 tiles, all with a partial edge — passes of 5, 5, 5 and 1 samples."""
    seed, instanced = case
    dflags, oflags = _extras(seed)
    for max_depth in (1, 2, 50):
        pair = _random_pair(host, orc64, seed, instanced, True)
        sc, cam, got, ref = _render_both(host, orc64, pair, NX, NY, NS, dflags, oflags, max_depth=max_depth)
        _assert_identical(got, ref, (case, max_depth))
    tiles = ((NX + abi.RTMI_TILE - 1) // abi.RTMI_TILE) * ((NY + abi.RTMI_TILE - 1) // abi.RTMI_TILE)
    assert tiles == 18
    budget = abi.SAMPLE_SLOT_BYTES_F64 * tiles * 64 * 5
    assert budget == 24 * 18 * 64 * 5
    passes = sc.render(cam, NX, NY, NS, sig=True, seed=42, precision="f64", flags=dflags, sample_buffer_bytes=budget)
    _assert_identical(passes, ref, (case, "passes"))
    for k in ("linear", "rgb8", "sig"):
        assert np.array_equal(passes[k], got[k], equal_nan=True), (case, k)
    orc64.free_all()


# ---- tolerance tier ------------------------------------------------------------------------------------------------------

def _groups():
    rnd = [("random", c) for c in cpu.FULL_SET]
    groups = [rnd[k:k + 8] for k in range(0, len(rnd), 8)]
    groups[-1] = groups[-1] + [("hand", "medium_in_instanced_list"), ("hand", "compositions")]  # 48 + 2 scenes: the last has ten
    return groups


SCENE_CAP = 9  # at most 1 % of the 903 pixels of a scene may differ in signature


@pytest.mark.parametrize("group", range(6))
def test_full_scenes_within_ulps_of_the_f64_oracle(host, orc64, group):
    """The scenes with sin, log, atan2 and asin, eight (the last group: ten) per test, pixels pooled, inside the bounds of
    test_gpu_f64_mode.py::test_scenes_with_transcendentals_within_ulps_of_the_f64_oracle.  Per scene, as a condition: at
    most SCENE_CAP pixels of another path signature — a wrong chain, norm or density breaks every pixel that sees the
    item, while ULP-born flips are two orders rarer (13 of 36 864 pixels at 56 spp on the named scenes)."""
    # measured (MI355X), every one of the six groups: sig_mismatch 0, share within 1e-12 relative 1.0, rgb8_mismatch 0 — no
    # path signature and no rgb8 value differs in any of the 50 scenes (largest per-scene count: 0 of 903 pixels); the
    # radiance differs in the last places only, max |d| 4.4e-16
    n_pix = n_sig = n_ch = n_ch_in = n_rgb = 0
    worst = 0
    for kind, what in _groups()[group]:
        if kind == "random":
            seed, instanced = what
            dflags, oflags = _extras(seed)
            pair = _random_pair(host, orc64, seed, instanced, False)
        else:
            dflags, oflags = 0, 0
            pair = _hand_built_pair(host, orc64, what, NX, NY)
        _sc, _cam, got, ref = _render_both(host, orc64, pair, NX, NY, NS, dflags, oflags)
        both_nan = np.isnan(got["linear"]) & np.isnan(ref["mean"])
        with np.errstate(invalid="ignore"):
            d = np.abs(got["linear"] - ref["mean"])
            inside = (d <= 1e-12 * np.maximum(1.0, np.abs(ref["mean"]))) | both_nan
        sig_bad = got["sig"] != ref["sig"]
        rgb_bad = got["rgb8"].astype(np.int32) != ref["rgb"]
        bad = np.argwhere(sig_bad | np.any(~inside, axis=2) | np.any(rgb_bad, axis=2))
        print(json.dumps({"scene": "%s %s %dx%dx%d" % (kind, what, NX, NY, NS), "sig_mismatch_pixels": int(sig_bad.sum()),
                          "channels_outside_1e-12_rel": int((~inside).sum()), "rgb8_mismatch_values": int(rgb_bad.sum()),
                          "max_abs": float(np.nanmax(d)) if not np.all(np.isnan(d)) else 0.0,
                          "pixels_row_col": bad.tolist()}))
        assert int(sig_bad.sum()) <= SCENE_CAP, (kind, what, int(sig_bad.sum()))
        n_pix += sig_bad.size
        n_sig += int(sig_bad.sum())
        n_ch += inside.size
        n_ch_in += int(inside.sum())
        n_rgb += int(rgb_bad.sum())
        worst = max(worst, int(sig_bad.sum()))
        orc64.free_all()
        host.free_all()
    res = {"group": group, "sig_mismatch": n_sig / n_pix, "share_within_1e-12_rel": n_ch_in / n_ch,
           "rgb8_mismatch": n_rgb / n_ch, "largest_scene_sig_mismatch_pixels": worst}
    print(json.dumps(res))
    assert res["sig_mismatch"] <= 1e-3
    assert res["share_within_1e-12_rel"] >= 0.9999
    assert res["rgb8_mismatch"] <= 5e-4
