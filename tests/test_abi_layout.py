"""The layout chain header -> ctypes -> Rust, link by link and field by field.

include/rtmi.h is the contract; raytracing_rust_amd/abi.py (ctypes, what every GPU test calls through) and
bindings/rust/src/sys.rs (#[repr(C)], what a Rust host binds — it cannot be compiled in this image) restate it.  This
test compiles a C program FROM THE HEADER that prints sizeof / alignof of every public struct and offsetof / sizeof of
every field, and demands the same numbers from ctypes and from the repr(C) layout rules applied to sys.rs — so a
mistake in abi.py cannot propagate into the Rust source unseen, and a header change cannot leave either behind.
The machinery is tests/abi_kit.py, which every other header's test shares.
The boundary these structs stand for: Hittable (src/hittable.rs:18-21), Camera (src/camera.rs:20-68) and the arguments
of create_image (tests/test.rs:55)."""
import pytest

import abi_kit as kit
from raytracing_rust_amd import abi

# C struct -> (ctypes class, Rust struct); no size or offset is pinned here: the numbers come from the compiled header
STRUCTS = {
    "rtmi_texture": (abi.Texture, "RtmiTexture"), "rtmi_perlin": (abi.Perlin, "RtmiPerlin"),
    "rtmi_image": (abi.ImageDesc, "RtmiImage"), "rtmi_material": (abi.Material, "RtmiMaterial"),
    "rtmi_prim_meta": (abi.PrimMeta, "RtmiPrimMeta"), "rtmi_bvh_node": (abi.BvhNode, "RtmiBvhNode"),
    "rtmi_bvh4_node": (abi.Bvh4Node, "RtmiBvh4Node"), "rtmi_xform": (abi.Xform, "RtmiXform"),
    "rtmi_item": (abi.Item, "RtmiItem"), "rtmi_scene_desc": (abi.SceneDesc, "RtmiSceneDesc"),
    "rtmi_camera": (abi.Camera, "RtmiCamera"), "rtmi_render_params": (abi.RenderParams, "RtmiRenderParams"),
    "rtmi_texel": (abi.Texel, "RtmiTexel"), "rtmi_stats": (abi.Stats, "RtmiStats"),
}
CORE = kit.Family("rtmi.h", abi.RTMI_SYMBOLS, {s: v + (None, None) for s, v in STRUCTS.items()}, includes=[])
# what a host needs, pinned by name: the constants test must have compared each of these
ABI_CONSTANTS = ("RTMI_ABI_VERSION", "RTMI_MAX_BVH_DEPTH", "RTMI_TILE", "RTMI_SAMPLE_SLOT_BYTES", "RTMI_FLAG_FAST_CULL",
                 "RTMI_FLAG_PATH_SIG", "RTMI_FLAG_PROFILE", "RTMI_FLAG_SYNC", "RTMI_FLAG_ASYNC", "RTMI_FLAG_SKY",
                 "RTMI_FLAG_REF_TREE", "RTMI_FLAG_BLOCK_COOP", "RTMI_FLAG_FACE_FORWARD", "RTMI_FLAG_UV_BOOK",
                 "RTMI_FLAG_TEST_OVERFLOW", "RTMI_FLAG_PROGRESSIVE", "RTMI_PRIMFLAG_XF_COUNT_SHIFT",
                 "RTMI_PRIMFLAG_XF_FIRST_SHIFT", "RTMI_ITEMFLAG_MEDIUM_OUTER_SHIFT", "RTMI_ERR_DEVICE", "RTMI_ERR_CANCELLED",
                 "RTMI_COLLECTIVE_NONE", "RTMI_COLLECTIVE_PEER_COPY", "RTMI_COLLECTIVE_RCCL")
RUST_CONSTANTS = ("RTMI_ABI_VERSION", "RTMI_MAX_BVH_DEPTH", "RTMI_FLAG_FAST_CULL", "RTMI_FLAG_PROGRESSIVE", "RTMI_SAMPLE_SLOT_BYTES")


def test_every_public_struct_of_the_header_is_covered():
    compiled = kit.compiled_layout("rtmi.h")
    assert sorted(compiled) == sorted(STRUCTS), "a struct of rtmi.h has no ctypes / Rust counterpart in this test"
    assert sum(len(v[2]) for v in compiled.values()) == sum(len(c._fields_) for c, _ in STRUCTS.values()) >= 110  # the parser saw the fields, not just the names


@pytest.mark.parametrize("sname", sorted(STRUCTS))
def test_ctypes_layout_equals_the_compiled_header(sname):
    CORE.layout(only=sname, links=("ctypes",))


@pytest.mark.parametrize("sname", sorted(STRUCTS))
def test_rust_repr_c_layout_equals_the_compiled_header(sname):
    CORE.layout(only=sname, links=("rust",))


def test_constants_agree_three_ways():
    """The #defines / enums a host needs, header vs abi.py vs sys.rs."""
    in_abi, in_rust = CORE.constants()
    assert not set(ABI_CONSTANTS) - set(in_abi) and not set(RUST_CONSTANTS) - set(in_rust)
