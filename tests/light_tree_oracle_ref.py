"""Host-side helpers for the oracle tests of the light tree (include/rtmi_light_tree.h): the oracle's tree, built from the
oracle's own emitters and never from the code under test, two hand-built scenes for the header's "known limit", and the
corpus of scenes whose reference renders must reach the tree's branches.  numpy and the oracle only; no GPU."""
import numpy as np

import light_tree_ref
import light_tree_scenes as lts
from nee_oracle_ref import EDGE, device_geometry, match_emitters, oracle_lights
from oracle.oracle import (ARITH_DEVICE, FACE_FORWARD, KIND_RECT, LIGHT_NODE_DTYPE, LIGHT_PATH_DTYPE, SKY, THROUGHPUT_FORM,
                           TREE_COUNTERS, UV_BOOK)
from raytracing_rust_amd import scenes

SEED = 42


def emitter_boxes(em):
    """(lo, hi, power) in f64 of oracle emitters (Oracle.emitters): a rect's box is degenerate on its plane's axis, a
    sphere's is c +- r; power = area * weight."""
    n = len(em)
    lo, hi = np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        g = em["geo"][i]
        if em["kind"][i] == KIND_RECT:
            ka, kb, kk = ((1, 2, 0), (2, 0, 1), (0, 1, 2))[int(em["plane"][i])]  # YZ: a = y, b = z; ZX: a = z, b = x; XY: a = x, b = y
            lo[i, ka], hi[i, ka] = g[0], g[2]
            lo[i, kb], hi[i, kb] = g[1], g[3]
            lo[i, kk] = hi[i, kk] = g[4]
        else:
            lo[i], hi[i] = g[:3] - g[3], g[:3] + g[3]
    return lo, hi, em["area"] * em["weight"]


def emitter_tree(em):
    """(nodes, paths), in the oracle's dtypes, of the tree over the emitters `em` in their order"""
    nodes, paths = light_tree_ref.build(*emitter_boxes(em))
    return (np.frombuffer(nodes.tobytes(), LIGHT_NODE_DTYPE).copy(), np.frombuffer(paths.tobytes(), LIGHT_PATH_DTYPE).copy())


def oracle_tree(orc, world, sc):
    """The light tree of `world` (built on `orc`) over the device's table order of `sc` (the same scene lowered by the
    host): boxes and powers from the oracle's emitters, the build from the numpy restatement.  Asserts that it is
    sc.light_tree() byte for byte."""
    em = orc.emitters(world)
    _, geo = device_geometry(sc)
    nodes, paths = emitter_tree(em[np.array(match_emitters(em, geo), np.int64)])
    dev_nodes, dev_paths = sc.light_tree()
    assert nodes.tobytes() == dev_nodes.tobytes(), "the oracle's tree nodes are not the host's"
    assert paths.tobytes() == dev_paths.tobytes(), "the oracle's tree paths are not the host's"
    return nodes, paths


# ---- the header's "known limit": pl (or pr) rounds to exactly 1 -----------------------------------------------------------
def _extreme(api, x):
    """light_tree_scenes.far_powers with the speck 0.01 x 0.01 and at (x, 0.5, 0): powers 1e4 and 2.5e-5, an importance
    ratio above 2^25 over most of the floor"""
    world = api.HittableList()
    world.push(lts._floor(api))
    world.push(api.Rect(api.PLANE_ZX, -5.0, -5.0, 5.0, 5.0, 6.0, api.DiffuseLight(api.SolidTexture(100.0, 100.0, 100.0))))
    world.push(lts._lamp(api, x, 0.0, 0.25, y=0.5, half=0.005))
    return world


EXTREME = {"extreme_powers": lambda api: _extreme(api, 8.0),  # the speck is the right child: pl rounds to 1
           "extreme_powers_left": lambda api: _extreme(api, -8.0)}  # ... the left child: pr rounds to 1


def build(api, name, nx, ny):
    """(camera, world) of a scene of this file or of light_tree_scenes.build"""
    if name in EXTREME:
        return scenes.set_camera(api, nx, ny, (0.0, 3.0, -12.0), (0.0, 0.0, 0.0), vertical_fov=40.0), EXTREME[name](api)
    return lts.build(api, name, nx, ny)


# ---- the corpus -----------------------------------------------------------------------------------------------------------
NAMED_SIZE = (40, 30, 12)
NAMED = [("lit_random_spheres", 0), ("lit_random_spheres", UV_BOOK | SKY), ("lamp_grid", 0), ("equal_lamps_4096", 0),
         ("same_place", 0), ("far_powers", 0), ("mixed", 0), ("extreme_powers", 0), ("extreme_powers_left", 0),
         ("cornell_box", 0), ("lit_smoke", FACE_FORWARD)]  # the last two: one-light controls
EDGE_SIZES = {"cdf_boundaries": (64, 64, 48)}
EDGE_DEFAULT_SIZE = (32, 24, 16)
# every scene whose reference render counts toward the branches reached: ("named", name, oflags) and ("edge", name, 0)
CORPUS = [("named", n, f) for n, f in NAMED] + [("edge", n, 0) for n in sorted(EDGE)]


def corpus_build(api, case):
    """(camera, world, nx, ny, ns) of a CORPUS entry"""
    kind, name, _ = case
    if kind == "named":
        nx, ny, ns = NAMED_SIZE
        return build(api, name, nx, ny) + (nx, ny, ns)
    nx, ny, ns = EDGE_SIZES.get(name, EDGE_DEFAULT_SIZE)
    return EDGE[name](api, nx, ny) + (nx, ny, ns)


def tree_reference(orc, cam_o, world_o, sc, nx, ny, ns, oflags=0, seed=SEED):
    """The oracle's render_nee under the tree of the scene `sc` lowered by the host: (render dict with samples, the
    TREE_COUNTERS of that render alone)."""
    lights = oracle_lights(orc, world_o, sc)
    tree = oracle_tree(orc, world_o, sc)
    orc.reset_counters()
    ref = orc.render_nee(cam_o, world_o, lights, nx, ny, ns, seed=seed, flags=ARITH_DEVICE | THROUGHPUT_FORM | oflags,
                         samples=True, tree=tree)
    cnt = orc.counters()
    return ref, {k: cnt[k] for k in TREE_COUNTERS}


_COUNTED = {}  # CORPUS entry -> the counters of its reference render; filled by whoever renders it first


def note_counters(case, cnt):
    _COUNTED[case] = cnt


def corpus_counters(host, orc, case):
    """The TREE_COUNTERS of a CORPUS entry's reference render (rendered once per process)."""
    if case not in _COUNTED:
        cam_h, world_h, nx, ny, ns = corpus_build(host, case)
        cam_o, world_o, _, _, _ = corpus_build(orc, case)
        _, cnt = tree_reference(orc, cam_o, world_o, host.lower(world_h), nx, ny, ns, case[2])
        orc.free_all()
        _COUNTED[case] = cnt
    return _COUNTED[case]


REACHED = ("tree_left", "tree_right", "tree_floor", "tree_no_sample", "tree_hit_pmf", "tree_hit_picked", "tree_p_one")


def assert_branches_reached(host, orc):
    """The union over CORPUS reaches every branch of the tree estimator, each extreme_powers scene reaches pl or pr == 1 on
    its own, inside_sphere_light has walks without a sample, and the pmf of a picked light is the pick's probability."""
    total = dict.fromkeys(TREE_COUNTERS, 0)
    for case in CORPUS:
        cnt = corpus_counters(host, orc, case)
        print("TREE-COUNTERS %s-%s-%d %s" % (case + (" ".join("%s %d" % (k[5:], cnt[k]) for k in TREE_COUNTERS),)))
        assert cnt["tree_hit_picked_mismatch"] == 0, case
        for k in TREE_COUNTERS:
            total[k] += cnt[k]
    print("TREE-COUNTERS union %s (tree_clamp is reported, not required)" % " ".join("%s %d" % (k[5:], total[k]) for k in TREE_COUNTERS))
    for k in REACHED:
        assert total[k] > 0, k
    assert total["tree_hit_picked_mismatch"] == 0
    for name in EXTREME:
        assert _COUNTED[("named", name, 0)]["tree_p_one"] > 0, name
    assert _COUNTED[("edge", "inside_sphere_light", 0)]["tree_no_sample"] > 0
