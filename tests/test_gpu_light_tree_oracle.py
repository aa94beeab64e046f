"""rtmi_render_nee under RTMI_FLAG_LIGHT_TREE (include/rtmi_light_tree.h) against the fp32 oracle's restatement of it
(orc_render_nee_tree), bit for bit: mean radiance, rgb8 and path signatures, and the standard-error plane against
rtmi_adaptive.h's Welford recurrence over the oracle's per-sample radiances.  The oracle's tree comes from its own emitters
(tests/light_tree_oracle_ref.py); its walks are pinned to numpy and the host without a GPU (tests/test_light_tree_oracle.py).
There are no tolerances in this file."""
import numpy as np
import pytest

import light_tree_oracle_ref as lto
import scenes_random
from nee_oracle_ref import EDGE
from oracle.oracle import FACE_FORWARD, SKY
from test_gpu_nee_oracle import DEVICE_FLAGS, PLACEMENTS, _check, _dev_ext

SEED = lto.SEED


def _tree_case(host, orc32, label, cam_h, world_h, cam_o, world_o, nx, ny, ns, oflags=0, flag_sets=DEVICE_FLAGS, min_lights=1):
    sc = host.lower(world_h).upload(0, light_tree=True)
    assert len(sc.lights()) >= min_lights, (label, len(sc.lights()))
    ref, cnt = lto.tree_reference(orc32, cam_o, world_o, sc, nx, ny, ns, oflags, seed=SEED)
    assert cnt["tree_hit_picked_mismatch"] == 0, label
    assert (cnt["tree_walk"] > 0) == (len(sc.lights()) > 1), label
    for fl, dflags in flag_sets:
        got = sc.render_nee(cam_h, nx, ny, ns, sig=True, seed=SEED, flags=dflags | _dev_ext(oflags), light_tree=True)
        _check("%s/%s" % (label, fl), got, ref)
    orc32.free_all()
    return ref, cnt


# ---- named scenes ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,oflags", lto.NAMED, ids=["%s-%d" % c for c in lto.NAMED])
def test_named_scenes_equal_oracle(host, orc32, name, oflags):
    case = ("named", name, oflags)
    cam_h, world_h, nx, ny, ns = lto.corpus_build(host, case)
    cam_o, world_o, _, _, _ = lto.corpus_build(orc32, case)
    one_light = name in ("cornell_box", "lit_smoke")
    ref, cnt = _tree_case(host, orc32, name, cam_h, world_h, cam_o, world_o, nx, ny, ns, oflags, min_lights=1 if one_light else 2)
    lto.note_counters(case, cnt)
    assert np.any(ref["linear"] > 0)
    if name in lto.EXTREME:
        assert cnt["tree_p_one"] > 0, name


@pytest.mark.gpu
def test_ragged_image_equals_oracle(host, orc32):
    """25 x 17: partial 8 x 8 tiles on both edges."""
    nx, ny, ns = 25, 17, 16
    cam_h, world_h = lto.build(host, "lamp_grid", nx, ny)
    cam_o, world_o = lto.build(orc32, "lamp_grid", nx, ny)
    _tree_case(host, orc32, "ragged", cam_h, world_h, cam_o, world_o, nx, ny, ns, min_lights=2)


# ---- hand-built edge scenes -----------------------------------------------------------------------------------------------
ONE_LIGHT_EDGE = ("light_in_medium", "isotropic_rect")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(EDGE))
def test_edge_scenes_equal_oracle(host, orc32, name):
    case = ("edge", name, 0)
    cam_h, world_h, nx, ny, ns = lto.corpus_build(host, case)
    cam_o, world_o, _, _, _ = lto.corpus_build(orc32, case)
    ref, cnt = _tree_case(host, orc32, name, cam_h, world_h, cam_o, world_o, nx, ny, ns, flag_sets=DEVICE_FLAGS[:2],
                          min_lights=1 if name in ONE_LIGHT_EDGE else 2)
    lto.note_counters(case, cnt)
    assert np.any(ref["linear"] > 0), name
    if name == "inside_sphere_light":
        assert cnt["tree_no_sample"] > 0


# ---- random compositions with two or more lights --------------------------------------------------------------------------
# the seeds of 1 .. 24 whose table has two or more lights (2 to 11), counted from scenes_random.build -> lower -> lights()
PLAIN_SEEDS = (2, 4, 6, 8, 9, 10, 17, 19, 21, 22, 23)
INSTANCED_SEEDS = (2, 4, 6, 8, 10, 17, 19, 21, 23)
RANDOM = [pytest.param(s, PLACEMENTS[0], inst, id="%d-unit-%s" % (s, "instanced" if inst else "plain"))
          for inst, seeds in ((False, PLAIN_SEEDS), (True, INSTANCED_SEEDS)) for s in seeds]
# other placements: N.c - x and r2 round differently there, where a fused or reassociated d2 on the device would show
RANDOM += [pytest.param(s, p, inst, id="%d-%s-%s" % (s, p[0], "instanced" if inst else "plain"))
           for inst in (False, True) for p in PLACEMENTS[1:] for s in (2, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("seed,placement,instanced", RANDOM)
def test_random_scenes_equal_oracle(host, orc32, seed, placement, instanced):
    nx, ny, ns = 24, 16, 6
    _, scale, off = placement
    cam_h, world_h = scenes_random.build(host, seed, nx, ny, instanced=instanced, scale=scale, offset=off)
    cam_o, world_o = scenes_random.build(orc32, seed, nx, ny, instanced=instanced, scale=scale, offset=off)
    oflags = SKY if seed % 3 == 0 else (FACE_FORWARD if seed % 3 == 1 else 0)
    flag_sets = DEVICE_FLAGS[:2] if seed % 2 else [DEVICE_FLAGS[0], DEVICE_FLAGS[3]]
    _tree_case(host, orc32, "random %d %s" % (seed, placement[0]), cam_h, world_h, cam_o, world_o, nx, ny, ns, oflags, flag_sets,
               min_lights=2)


# ---- the references above reached the branches ----------------------------------------------------------------------------
@pytest.mark.gpu
def test_branches_reached(host, orc32):
    """The union of the tree counters over the named and edge references (those a test above rendered, the others rendered
    here by the oracle alone): every branch of the estimator was compared, and no picked light's pmf differed from the pick's
    probability."""
    print()
    lto.assert_branches_reached(host, orc32)
