"""The f64 render mode's public interface (include/rtmi_f64.h) and its wide lowering, without a GPU.

* the header compiles as C99; the layout chain header -> ctypes (abi.py) -> #[repr(C)] (bindings/rust/src/sys.rs) holds
  for its structs, with the machinery of test_abi_layout.py; librtmi.so exports exactly the functions it declares;
* the double planes the host lowering keeps are the f64 oracle's values bit for bit (camera state, Perlin vectors, BVH
  root boxes), and every one of them rounds to the value the fp32 description carries."""

import numpy as np
import pytest

from raytracing_rust_amd import abi, scenes

import scenes_extra
import abi_kit as kit

STRUCTS = {"rtmi_scene_f64": (abi.SceneF64, "RtmiSceneF64", None, None), "rtmi_camera_f64": (abi.CameraF64, "RtmiCameraF64", None, None)}
# isolated=False: "f64" is the name of a number format, which the other headers' comments use freely
FAMILY = kit.Family("rtmi_f64.h", ["rtmi_probe_math_f64", "rtmi_render_f64", "rtmi_scene_attach_f64"], STRUCTS, word="f64",
                    isolated=False)


def test_header_is_c99(tmp_path):
    FAMILY.c99(tmp_path, body="rtmi_scene_f64 s; rtmi_camera_f64 c; (void)s; (void)c;", run=True)


@pytest.mark.parametrize("sname", sorted(STRUCTS))
def test_layout_chain_header_ctypes_rust(sname):
    FAMILY.layout(only=sname)


def test_exports_and_declarations_agree():
    FAMILY.exports()
    FAMILY.isolation()
    assert "RTMI_SAMPLE_SLOT_BYTES_F64" in FAMILY.constants()[1]
    assert kit.header_constants("rtmi_f64.h")["RTMI_SAMPLE_SLOT_BYTES_F64"] == abi.SAMPLE_SLOT_BYTES_F64 == 24


def test_attach_and_render_fail_cleanly_without_a_device(host):
    """Argument checks come before any device work: NULL planes / handles are RTMI_ERR_INVALID."""
    lib = abi.load_rtmi()
    assert lib.rtmi_scene_attach_f64(None, None) == 1
    assert lib.rtmi_render_f64(None, None, None, 0.001, None, None, None, None) == 1
    assert lib.rtmi_probe_math_f64(9, None, None, None, 0) == 1


def _wide_names():
    return sorted(scenes.SCENES) + ["lit_final_scene", "lit_smoke", "lit_random_spheres", "hollow_glass"]


class _Recorder:
    """The scene API of the host or of the oracle, recording what a scene builder constructs: Perlin textures, BVH nodes
    and media densities, in construction order."""

    def __init__(self, api):
        self._api = api
        self.noise, self.bvh, self.density = [], [], []

    def __getattr__(self, name):
        return getattr(self._api, name)

    def NoiseTexture(self, scale):
        t = self._api.NoiseTexture(scale)
        self.noise.append(t)
        return t

    def BVHNode(self, hittables, time0, time1):
        n = self._api.BVHNode(hittables, time0, time1)
        self.bvh.append(n)
        return n

    def ConstantMedium(self, boundary, density, texture):
        self.density.append(float(density))
        return self._api.ConstantMedium(boundary, density, texture)


@pytest.mark.parametrize("name", _wide_names())
def test_wide_lowering_matches_the_f64_oracle(host, orc64, name):
    nx, ny = 64, 48
    hrec, orec = _Recorder(host), _Recorder(orc64)
    cam, world = scenes_extra.build(hrec, name, nx, ny, seed=1)
    ocam, _oworld = scenes_extra.build(orec, name, nx, ny, seed=1)
    # camera: Oracle("f64").camera_state, bit for bit
    c = cam.lower_f64()
    got = np.array(list(c.origin) + list(c.lower_left_corner) + list(c.horizontal) + list(c.vertical) + list(c.u) + list(c.v)
                   + [c.time0, c.time1, c.lens_radius])
    assert got.tobytes() == np.asarray(orc64.camera_state(ocam), np.float64).tobytes()
    c32 = cam.lower()
    assert np.array_equal(got[:18].astype(np.float32), np.array([list(getattr(c32, f)) for f in
                          ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v")], np.float32).ravel())
    sc = host.lower(world)
    a32, a64 = sc.arrays(), sc.arrays_f64()
    # Perlin ranvec: every lowered table is one of the oracle's perlin_tables, bit for bit (the scene stream draws the
    # same numbers in the same order on both sides)
    oracle_tables = {np.asarray(orc64.perlin_tables(t)[0], np.float64).ravel().tobytes() for t in orec.noise}
    assert a64["perlin_ranvec"].shape[0] == a32["n_perlin"] == len(oracle_tables)
    for row in a64["perlin_ranvec"]:
        assert row.tobytes() in oracle_tables
    # BVH root boxes: every BVH item's root box is the bounding_box of one of the oracle's BVHNodes, bit for bit
    oracle_boxes = {np.concatenate(orc64.bounding_box(n)).astype(np.float64).tobytes() for n in orec.bvh}
    bvh_items = [k for k, it in enumerate(a32["items"]) if it.kind == 1]
    assert len(bvh_items) > 0 or not orec.bvh
    for k in bvh_items:
        assert a64["item_root"][k].tobytes() in oracle_boxes, (name, k)
    # media: -(1/density) in double, exactly
    nids = {float(a64["item_neg_inv_density"][k]) for k, it in enumerate(a32["items"]) if it.flags & 2}
    assert nids == {-(1.0 / d) for d in hrec.density}
    # every other wide value rounds to the fp32 value of the existing lowering
    assert np.array_equal(a64["prim_a"].astype(np.float32), a32["prim_a"])
    # (plane B of a MovingSphere: fp32 keeps float(c1) - float(c0), the wide plane the f64 difference c1 - c0)
    moving = np.array([m.type == 1 for m in a32["prim_meta"]], bool)
    assert np.array_equal(a64["prim_b"][~moving].astype(np.float32), a32["prim_b"][~moving])
    assert np.array_equal(a64["prim_b"][moving, 3].astype(np.float32), a32["prim_b"][moving, 3])
    assert np.array_equal(a64["xforms"][:, :3].astype(np.float32), np.array([[x.x, x.y, x.z] for x in a32["xforms"]], np.float32).reshape(-1, 3))
    assert np.array_equal(a64["material_param"].astype(np.float32), np.array([m.param for m in a32["materials"]], np.float32))
    assert np.array_equal(a64["texture_f"].astype(np.float32), np.array([[t.f0, t.f1, t.f2, t.f3] for t in a32["textures"]], np.float32).reshape(-1, 4))


def test_wide_perlin_and_root_boxes_bit_for_bit(host, orc64):
    """Perlin::new and BVHNode::new draw from the scene stream in the same order on both sides: the same scene built
    through the host and through the oracle yields the same f64 tables and root boxes."""
    host.seed_scene_rng(5)
    orc64.seed_scene_rng(5)
    ht, ot = host.NoiseTexture(4.0), orc64.NoiseTexture(4.0)
    mat_h, mat_o = host.Lambertian(ht), orc64.Lambertian(ot)
    hs = [host.Sphere((float(i), 0.0, float(i % 3)), 0.5 + 0.1 * i, mat_h) for i in range(7)]
    os_ = [orc64.Sphere((float(i), 0.0, float(i % 3)), 0.5 + 0.1 * i, mat_o) for i in range(7)]
    hb, ob = host.BVHNode(hs, 0.0, 1.0), orc64.BVHNode(os_, 0.0, 1.0)
    world = host.HittableList()
    world.push(hb)
    sc = host.lower(world)
    a64 = sc.arrays_f64()
    ranvec, _perm = orc64.perlin_tables(ot)
    assert a64["perlin_ranvec"][0].tobytes() == np.asarray(ranvec, np.float64).ravel().tobytes()
    box = orc64.bounding_box(ob)
    assert a64["item_root"][0].tobytes() == np.asarray(box, np.float64).ravel().tobytes()
