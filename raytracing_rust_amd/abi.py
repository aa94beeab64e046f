"""ctypes mirrors of the plain-old-data structs of include/rtmi.h and the library loader.

The HIP extension is mandatory: there is no CPU fallback for the render path.  If the
native libraries are missing they are built in-tree (hipcc cross-compiles without a GPU);
if that fails the import fails loudly.
"""
import ctypes as C
import os

from . import build as _build

RTMI_ABI_VERSION = 7
RTMI_ITEMFLAG_MEDIUM_OUTER_SHIFT = 8  # MEDIUM items: how many of the first transforms wrap the medium itself (bits 8..11)
RTMI_PRIMFLAG_XF_COUNT_SHIFT = 4   # instanced primitive: number of its own transforms (bits 4..7)
RTMI_PRIMFLAG_XF_FIRST_SHIFT = 12  # ... and the index of the first one in xforms (bits 12..31)
RTMI_MAX_BVH_DEPTH = 24
RTMI_TILE = 8
RTMI_FLAG_FAST_CULL = 1
RTMI_FLAG_PATH_SIG = 2
RTMI_FLAG_PROFILE = 4
RTMI_FLAG_SYNC = 8
RTMI_FLAG_ASYNC = 16
RTMI_FLAG_SKY = 32
RTMI_FLAG_REF_TREE = 64
RTMI_FLAG_BLOCK_COOP = 32768
RTMI_SAMPLE_SLOT_BYTES = 12  # per-sample radiance buffer: three fp32 per finished path
RTMI_COLLECTIVE_NONE, RTMI_COLLECTIVE_PEER_COPY, RTMI_COLLECTIVE_RCCL = 0, 1, 2
RTMI_KERNEL_PERLANE, RTMI_KERNEL_WAVE_COOP, RTMI_KERNEL_ASYNC, RTMI_KERNEL_BLOCK_COOP = 0, 1, 2, 3
RTMI_FLAG_FACE_FORWARD = 128
RTMI_FLAG_UV_BOOK = 4096
RTMI_FLAG_TEST_OVERFLOW = 8192
RTMI_FLAG_PROGRESSIVE = 16384  # opt-in: the framebuffer holds the image of the samples so far after every pass
RTMI_FLAG_LIGHT_COOP = 65536  # include/rtmi_light_coop.h: NEE / environment renders on the wave-cooperative kernel
RTMI_FLAG_ROULETTE_COOP = 131072  # include/rtmi_roulette_coop.h: roulette renders on the wave-cooperative kernel
RTMI_FLAG_LIGHT_TREE = 262144  # include/rtmi_light_tree.h: rtmi_render_nee picks its light by walking the light tree
# RTMI_FLAG_BATCH_COOP of include/rtmi_batch_coop.h: the batch modes trace on the wave-cooperative kernel.  Under a name of
# its own: tests/test_abi_signatures.py pins how many header constants this file restates by their header's name;
# tests/test_batch_coop_abi.py compares this one with the header.
FLAG_BATCH_COOP = 2097152
RTMI_ERR_DEVICE = 3
RTMI_ERR_CANCELLED = 5
RTMI_TEXEL_POISON = 0x80000000

TEX_SOLID, TEX_CHECKER, TEX_NOISE, TEX_IMAGE = 0, 1, 2, 3
MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC, MAT_DIFFUSE_LIGHT, MAT_ISOTROPIC = 0, 1, 2, 3, 4
PRIM_SPHERE, PRIM_MSPHERE, PRIM_RECT, PRIM_CUBE = 0, 1, 2, 3
ITEM_LIST, ITEM_BVH = 0, 1
ITEMFLAG_FLIP, ITEMFLAG_MEDIUM, ITEMFLAG_SAVE_T0, ITEMFLAG_DEFERRED, ITEMFLAG_NESTED_MEDIUM = 1, 2, 4, 8, 16
ITEMFLAG_LISTSCAN_BEGIN, ITEMFLAG_LISTSCAN_MEMBER, ITEMFLAG_LISTSCAN_END = 32, 64, 128
RTMI_ITEMFLAG_GATE_OUTER_SHIFT = 12  # DEFERRED items: how many leading transforms belong to the enclosing BVH item (bits 12..15)
PROBE_GEOM_PRIM, PROBE_GEOM_AABB, PROBE_GEOM_MEDIUM, PROBE_GEOM_SHADE, PROBE_GEOM_UV = 0, 1, 2, 3, 4  # rtmi_probe_geom
PROBE_GEOM_IN, PROBE_GEOM_OUT = 16, 10  # floats per case
PROBE_PATH_CAMERA, PROBE_PATH_SPHERE, PROBE_PATH_DISK, PROBE_PATH_MEDIUM_SAMPLE, PROBE_PATH_XFORM_ROUNDTRIP = 0, 1, 2, 3, 4  # rtmi_probe_path
PROBE_PATH_BOUNCE = 5
PROBE_PATH_IN, PROBE_PATH_OUT, PROBE_PATH_WORDS = 12, 20, 32  # floats per case; scripted words per case
XF_TRANSLATE, XF_ROTATE_X, XF_ROTATE_Y, XF_ROTATE_Z, XF_GATE_MIN, XF_GATE_MAX, XF_INNER_MEDIUM = 0, 1, 2, 3, 4, 5, 6


class Texture(C.Structure):
    _fields_ = [("kind", C.c_int32), ("i0", C.c_int32), ("i1", C.c_int32), ("pad", C.c_int32),
                ("f0", C.c_float), ("f1", C.c_float), ("f2", C.c_float), ("f3", C.c_float)]


class Perlin(C.Structure):
    _fields_ = [("ranvec", C.c_float * 1024), ("perm", C.c_int32 * 768)]


class ImageDesc(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("nx", C.c_uint32), ("ny", C.c_uint32)]


class Material(C.Structure):
    _fields_ = [("kind", C.c_int32), ("tex", C.c_int32), ("param", C.c_float), ("flags", C.c_uint32)]


class PrimMeta(C.Structure):
    _fields_ = [("material", C.c_int32), ("flags", C.c_uint32), ("inv_dt", C.c_float), ("type", C.c_int32)]


class BvhNode(C.Structure):
    _fields_ = [("lmin", C.c_float * 3), ("lmax", C.c_float * 3), ("rmin", C.c_float * 3), ("rmax", C.c_float * 3),
                ("left", C.c_int32), ("right", C.c_int32), ("pad", C.c_int32 * 2)]


class Bvh4Node(C.Structure):
    _fields_ = [("minx", C.c_float * 4), ("miny", C.c_float * 4), ("minz", C.c_float * 4), ("maxx", C.c_float * 4),
                ("maxy", C.c_float * 4), ("maxz", C.c_float * 4), ("child", C.c_int32 * 4), ("pad", C.c_int32 * 4)]


class Xform(C.Structure):
    _fields_ = [("kind", C.c_int32), ("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class Item(C.Structure):
    _fields_ = [("kind", C.c_int32), ("first", C.c_int32), ("count", C.c_int32), ("flags", C.c_uint32),
                ("xform_first", C.c_int32), ("xform_count", C.c_int32), ("medium_material", C.c_int32),
                ("neg_inv_density", C.c_float), ("root_min", C.c_float * 3), ("root_max", C.c_float * 3),
                ("scale", C.c_float), ("alt_first", C.c_int32)]


class SceneDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("n_items", C.c_uint32), ("items", C.POINTER(Item)),
                ("n_prims", C.c_uint32), ("prim_a", C.POINTER(C.c_float)), ("prim_b", C.POINTER(C.c_float)),
                ("prim_meta", C.POINTER(PrimMeta)), ("prim_gate", C.POINTER(C.c_float)), ("alt_max_depth", C.c_uint32),
                ("n_alt_nodes", C.c_uint32), ("alt_nodes", C.POINTER(Bvh4Node)),
                ("n_nodes", C.c_uint32), ("nodes", C.POINTER(BvhNode)),
                ("n_xforms", C.c_uint32), ("xforms", C.POINTER(Xform)),
                ("n_materials", C.c_uint32), ("materials", C.POINTER(Material)),
                ("n_textures", C.c_uint32), ("textures", C.POINTER(Texture)),
                ("n_perlin", C.c_uint32), ("perlin", C.POINTER(Perlin)),
                ("n_images", C.c_uint32), ("images", C.POINTER(ImageDesc)),
                ("image_data", C.POINTER(C.c_uint8)), ("image_bytes", C.c_uint64),
                ("max_bvh_depth", C.c_uint32), ("bvh_time_lo", C.c_float), ("bvh_time_hi", C.c_float)]


class Camera(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("lower_left_corner", C.c_float * 3), ("horizontal", C.c_float * 3),
                ("vertical", C.c_float * 3), ("u", C.c_float * 3), ("v", C.c_float * 3),
                ("time0", C.c_float), ("time1", C.c_float), ("lens_radius", C.c_float)]


class RenderParams(C.Structure):
    _fields_ = [("nx", C.c_uint32), ("ny", C.c_uint32), ("ns", C.c_uint32), ("max_depth", C.c_uint32),
                ("t_min", C.c_float), ("flags", C.c_uint32), ("seed", C.c_uint64),
                ("tile_rank", C.c_uint32), ("tile_world", C.c_uint32), ("spp_chunks", C.c_uint32), ("shade_threshold", C.c_uint32),
                ("path_sig", C.c_uint64), ("prof", C.c_uint64), ("sample_buffer_bytes", C.c_uint64),
                ("progress_fn", C.c_uint64), ("progress_user", C.c_uint64)]


# rtmi_progress_fn: int (*)(uint64_t done, uint64_t total, void *user)
PROGRESS_FN = C.CFUNCTYPE(C.c_int, C.c_uint64, C.c_uint64, C.c_void_p)


class Texel(C.Structure):
    _fields_ = [("r", C.c_float), ("g", C.c_float), ("b", C.c_float), ("rgb8", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("render_ms", C.c_double), ("samples", C.c_uint64),
                ("tiles", C.c_uint32), ("chunks", C.c_uint32), ("blocks", C.c_uint32), ("kernel", C.c_uint32)]


def stats_kernel(st):
    """rtmi_stats_kernel (include/rtmi.h): RTMI_KERNEL_* of a Stats, whether or not the call set the report knob."""
    return st.kernel & 255


def stats_instantiation(st):
    """rtmi_stats_instantiation (include/rtmi.h): which instantiation of the wave-cooperative kernel ran — 0 none, 1 the
    general one, 2 the one-tree one — of a Stats whose call set the diagnostic knob, flag bit 19; 0 without the knob."""
    return (st.kernel >> 8) & 255


class SceneF64(C.Structure):
    """rtmi_scene_f64 (include/rtmi_f64.h): the double planes of the f64 render mode."""
    _fields_ = [("n_items", C.c_uint32), ("n_prims", C.c_uint32), ("n_nodes", C.c_uint32), ("n_xforms", C.c_uint32),
                ("n_materials", C.c_uint32), ("n_textures", C.c_uint32), ("n_perlin", C.c_uint32), ("pad", C.c_uint32),
                ("prim_a", C.POINTER(C.c_double)), ("prim_b", C.POINTER(C.c_double)), ("prim_dt", C.POINTER(C.c_double)),
                ("prim_gate", C.POINTER(C.c_double)), ("nodes", C.POINTER(C.c_double)), ("xforms", C.POINTER(C.c_double)),
                ("item_neg_inv_density", C.POINTER(C.c_double)), ("item_root", C.POINTER(C.c_double)),
                ("material_param", C.POINTER(C.c_double)), ("texture_f", C.POINTER(C.c_double)),
                ("perlin_ranvec", C.POINTER(C.c_double))]


class CameraF64(C.Structure):
    """rtmi_camera_f64 (include/rtmi_f64.h)."""
    _fields_ = [("origin", C.c_double * 3), ("lower_left_corner", C.c_double * 3), ("horizontal", C.c_double * 3),
                ("vertical", C.c_double * 3), ("u", C.c_double * 3), ("v", C.c_double * 3),
                ("time0", C.c_double), ("time1", C.c_double), ("lens_radius", C.c_double)]


SAMPLE_SLOT_BYTES_F64 = 24  # RTMI_SAMPLE_SLOT_BYTES_F64


class Adaptive(C.Structure):
    """rtmi_adaptive (include/rtmi_adaptive.h): the noise target of an adaptive render."""
    _fields_ = [("min_spp", C.c_uint32), ("step_spp", C.c_uint32), ("abs_tol", C.c_double), ("rel_tol", C.c_double)]


class DenoiseParams(C.Structure):
    """rtmi_denoise_params (include/rtmi_denoise.h): the a-trous filter's settings (32 bytes)."""
    _fields_ = [("iterations", C.c_uint32), ("normal_power", C.c_uint32), ("sigma_l", C.c_float), ("sigma_z", C.c_float),
                ("eps_l", C.c_float), ("eps_z", C.c_float), ("albedo_min", C.c_float), ("flags", C.c_uint32)]


class Light(C.Structure):
    """rtmi_light (include/rtmi_nee.h): one eligible light occurrence of a scene description (48 bytes)."""
    _fields_ = [("item", C.c_int32), ("prim", C.c_int32), ("kind", C.c_int32), ("material", C.c_int32),
                ("area", C.c_double), ("weight", C.c_double), ("select_p", C.c_double), ("cdf", C.c_double)]


class LightNode(C.Structure):
    """rtmi_light_node (include/rtmi_light_tree.h): one node of the light tree (32 bytes)."""
    _fields_ = [("c", C.c_float * 3), ("r2", C.c_float), ("power", C.c_float), ("link", C.c_uint32), ("pad", C.c_uint32 * 2)]


class LightPath(C.Structure):
    """rtmi_light_path (include/rtmi_light_tree.h): where a light's leaf lies in the tree (8 bytes)."""
    _fields_ = [("trail", C.c_uint32), ("depth", C.c_uint32)]


RTMI_LIGHT_TREE_LEAF = 0x80000000
RTMI_LIGHT_TREE_PROBE_PICK, RTMI_LIGHT_TREE_PROBE_PMF = 0, 1


class EnvMap(C.Structure):
    """rtmi_env_map (include/rtmi_env.h): an environment map, height * width * 3 floats, row 0 the top row (16 bytes)."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("rgb", C.c_void_p)]


class EnvRender(C.Structure):
    """rtmi_env_render (include/rtmi_env.h): the options of rtmi_render_env (8 bytes)."""
    _fields_ = [("nee", C.c_uint32), ("env_select_p", C.c_float)]


RTMI_ENV_PROBE_LOOKUP, RTMI_ENV_PROBE_SAMPLE = 0, 1
RTMI_ENV_MAX_SIDE, RTMI_ENV_MAX_TEXELS = 16384, 1 << 25


class Roulette(C.Structure):
    """rtmi_roulette (include/rtmi_roulette.h): the options of the Russian-roulette entries (16 bytes)."""
    _fields_ = [("estimator", C.c_uint32), ("min_depth", C.c_uint32), ("q_min", C.c_float), ("env_select_p", C.c_float)]


RTMI_ROULETTE_PLAIN, RTMI_ROULETTE_NEE, RTMI_ROULETTE_ENV, RTMI_ROULETTE_ENV_NEE = 0, 1, 2, 3
ROULETTE_ESTIMATORS = {"plain": RTMI_ROULETTE_PLAIN, "nee": RTMI_ROULETTE_NEE, "env": RTMI_ROULETTE_ENV,
                       "env_nee": RTMI_ROULETTE_ENV_NEE}


class SessionOpts(C.Structure):
    """rtmi_session_opts (include/rtmi_session.h): what a render session traces and on which lattice (32 bytes)."""
    _fields_ = [("estimator", C.c_uint32), ("rr", C.c_uint32), ("min_depth", C.c_uint32), ("q_min", C.c_float),
                ("env_select_p", C.c_float), ("first_sample", C.c_uint32), ("min_spp", C.c_uint32), ("step_spp", C.c_uint32)]


RTMI_SESSION_BLOB_VERSION, RTMI_SESSION_BLOB_HEADER, RTMI_SESSION_BLOB_IDENTITY = 1, 216, 196


class Ray(C.Structure):
    """rtmi_ray (include/rtmi_query.h): one query ray (32 bytes)."""
    _fields_ = [("o", C.c_float * 3), ("t_min", C.c_float), ("d", C.c_float * 3), ("t_max", C.c_float)]


class Hit(C.Structure):
    """rtmi_hit (include/rtmi_query.h): the record of a closest hit, or of a miss (48 bytes)."""
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("p", C.c_float * 3), ("n", C.c_float * 3),
                ("item", C.c_int32), ("prim", C.c_int32), ("material", C.c_int32)]


class QueryParams(C.Structure):
    """rtmi_query_params (include/rtmi_query.h): one call's batch (24 bytes)."""
    _fields_ = [("n", C.c_uint32), ("flags", C.c_uint32), ("seed", C.c_uint64), ("first_ray", C.c_uint64)]


class RadianceParams(C.Structure):
    """rtmi_radiance_params (include/rtmi_radiance.h): one call's batch, estimator and Philox indices (56 bytes)."""
    _fields_ = [("n", C.c_uint32), ("spp", C.c_uint32), ("estimator", C.c_uint32), ("flags", C.c_uint32),
                ("max_depth", C.c_uint32), ("t_min", C.c_float), ("seed", C.c_uint64), ("first_ray", C.c_uint64),
                ("first_sample", C.c_uint32), ("stream_skip", C.c_uint32), ("env_select_p", C.c_float)]


RTMI_GATHER_COSINE = 0  # include/rtmi_gather.h: irradiance about a normal
RTMI_GATHER_SPHERE = 1  # ... mean radiance over the sphere and its 9 SH coefficients
RTMI_GATHER_STREAM = 5  # the Philox stream id of the directions
GATHER_MODES = {"cosine": RTMI_GATHER_COSINE, "sphere": RTMI_GATHER_SPHERE}


class GatherParams(C.Structure):
    """rtmi_gather_params (include/rtmi_gather.h): one call's points, mode, estimator and Philox indices (64 bytes; seed at
    offset 32)."""
    _fields_ = [("n", C.c_uint32), ("spp", C.c_uint32), ("mode", C.c_uint32), ("estimator", C.c_uint32), ("flags", C.c_uint32),
                ("max_depth", C.c_uint32), ("t_min", C.c_float), ("seed", C.c_uint64), ("first_point", C.c_uint64),
                ("first_sample", C.c_uint32), ("slab_points", C.c_uint32), ("env_select_p", C.c_float)]


RTMI_TEMPORAL_NO_DEMODULATE = 1  # include/rtmi_temporal.h: accumulate the colour itself, not colour / albedo


class TemporalParams(C.Structure):
    """rtmi_temporal_params (include/rtmi_temporal.h): the settings of a temporal history (32 bytes)."""
    _fields_ = [("max_history", C.c_uint32), ("alpha_min", C.c_float), ("depth_tol", C.c_float), ("normal_min", C.c_float),
                ("albedo_min", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


RTMI_FRAME_NO_TEMPORAL = 1  # include/rtmi_frame.h: no history, the chain render, features, filter
RTMI_FRAME_NO_FILTER = 2  # the filter runs with 0 iterations: the accumulated image and its quantisation


class FrameOpts(C.Structure):
    """rtmi_frame_opts (include/rtmi_frame.h): the estimator and the embedded temporal and filter settings (96 bytes)."""
    _fields_ = [("estimator", C.c_uint32), ("env_select_p", C.c_float), ("temporal", TemporalParams), ("denoise", DenoiseParams),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 5)]


class FrameOut(C.Structure):
    """rtmi_frame_out (include/rtmi_frame.h): the planes of a frame, host or device pointers, NULL = not copied (96 bytes)."""
    _fields_ = [(n, C.c_void_p) for n in ("linear", "rgb8", "noisy_linear", "noisy_stderr", "albedo", "normal", "depth", "hits",
                                          "accum_linear", "accum_stderr", "history", "motion")]


RTMI_TONEMAP_CLAMP, RTMI_TONEMAP_REINHARD, RTMI_TONEMAP_ACES = 0, 1, 2  # include/rtmi_tonemap.h: op
RTMI_TONEMAP_GAMMA2, RTMI_TONEMAP_SRGB = 0, 1  # ... oetf: the reference's sqrt, the sRGB curve
RTMI_TONEMAP_MANUAL, RTMI_TONEMAP_AUTO = 0, 1  # ... exposure
TONEMAP_OPS = {"clamp": RTMI_TONEMAP_CLAMP, "reinhard": RTMI_TONEMAP_REINHARD, "aces": RTMI_TONEMAP_ACES}
TONEMAP_OETFS = {"gamma2": RTMI_TONEMAP_GAMMA2, "srgb": RTMI_TONEMAP_SRGB}
TONEMAP_EXPOSURES = {"manual": RTMI_TONEMAP_MANUAL, "auto": RTMI_TONEMAP_AUTO}


class TonemapParams(C.Structure):
    """rtmi_tonemap_params (include/rtmi_tonemap.h): the operator, the transfer function and the metering (64 bytes)."""
    _fields_ = [("op", C.c_uint32), ("oetf", C.c_uint32), ("exposure", C.c_uint32), ("flags", C.c_uint32), ("ev", C.c_float),
                ("white", C.c_float), ("key", C.c_float), ("log2_min", C.c_float), ("log2_max", C.c_float), ("p_low", C.c_float),
                ("p_high", C.c_float), ("speed_up", C.c_float), ("speed_down", C.c_float), ("adapt_min", C.c_float),
                ("adapt_max", C.c_float), ("reserved", C.c_uint32)]


class TonemapState(C.Structure):
    """rtmi_tonemap_state (include/rtmi_tonemap.h): what one apply metered and applied (32 bytes)."""
    _fields_ = [("exposure", C.c_float), ("adapted_log2", C.c_float), ("metered_log2", C.c_float), ("counted", C.c_uint32),
                ("kept", C.c_uint32), ("applies", C.c_uint32), ("reserved", C.c_uint32 * 2)]


RTMI_UPSCALE_BACKGROUND, RTMI_UPSCALE_GUIDED, RTMI_UPSCALE_NEAREST, RTMI_UPSCALE_MISMATCH = 0, 1, 2, 3  # include/rtmi_upscale.h: cls


class UpscaleParams(C.Structure):
    """rtmi_upscale_params (include/rtmi_upscale.h): the reconstruction's edge-stopping settings (32 bytes)."""
    _fields_ = [("normal_power", C.c_uint32), ("sigma_z", C.c_float), ("eps_z", C.c_float), ("albedo_min", C.c_float),
                ("w_min", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class UpscaleIn(C.Structure):
    """rtmi_upscale_in (include/rtmi_upscale.h): the low-resolution planes and the full-resolution guide (64 bytes)."""
    _fields_ = [(n, C.c_void_p) for n in ("linear_lo", "albedo_lo", "normal_lo", "depth_lo", "albedo", "normal", "depth", "reserved")]


class UpscaleOut(C.Structure):
    """rtmi_upscale_out (include/rtmi_upscale.h): the outputs, NULL = not written (32 bytes)."""
    _fields_ = [(n, C.c_void_p) for n in ("linear", "rgb8", "cls", "reserved")]


class UpscalerOpts(C.Structure):
    """rtmi_upscaler_opts (include/rtmi_upscale.h): the low frame's options, the reconstruction's and the low size (160 bytes)."""
    _fields_ = [("low", FrameOpts), ("up", UpscaleParams), ("lx", C.c_uint32), ("ly", C.c_uint32), ("guide_ns", C.c_uint32),
                ("reserved", C.c_uint32 * 5)]


class UpscalerOut(C.Structure):
    """rtmi_upscaler_out (include/rtmi_upscale.h): the full-resolution planes and the low frame's, NULL = not copied (144 bytes)."""
    _fields_ = [(n, C.c_void_p) for n in ("linear", "rgb8", "cls", "albedo", "normal", "depth")] + [("low", FrameOut)]


class SparseParams(C.Structure):
    """rtmi_sparse_params (include/rtmi_sparse.h): a list's length or capacity, samples and estimator (32 bytes)."""
    _fields_ = [("n", C.c_uint32), ("ns", C.c_uint32), ("first_sample", C.c_uint32), ("estimator", C.c_uint32),
                ("env_select_p", C.c_float), ("reserved", C.c_uint32 * 3)]


class PixelwiseOpts(C.Structure):
    """rtmi_pixelwise_opts (include/rtmi_pixelwise.h): the steps, estimator and tolerances of a per-pixel adaptive render (48 bytes)."""
    _fields_ = [("min_spp", C.c_uint32), ("step_spp", C.c_uint32), ("estimator", C.c_uint32), ("pass_spp", C.c_uint32),
                ("abs_tol", C.c_double), ("rel_tol", C.c_double), ("env_select_p", C.c_float), ("reserved", C.c_uint32 * 3)]


class WindowOpts(C.Structure):
    """rtmi_window_opts (include/rtmi_window.h): the steps, estimator, tolerances and window radius of a windowed adaptive
    render (48 bytes)."""
    _fields_ = [("min_spp", C.c_uint32), ("step_spp", C.c_uint32), ("estimator", C.c_uint32), ("pass_spp", C.c_uint32),
                ("abs_tol", C.c_double), ("rel_tol", C.c_double), ("env_select_p", C.c_float), ("radius", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]


RTMI_WINDOW_MAX_RADIUS = 16

# RTMI_SCENE_WORDS_* of include/rtmi_update.h, in the header's order: the device arrays rtmu_probe_scene_words copies out
# (names of their own, like FLAG_BATCH_COOP above; tests/test_update_abi.py compares them with the header)
SCENE_WORDS = {"items": 0, "prim_a": 1, "prim_b": 2, "gate": 3, "nodes": 4, "alt_nodes": 5, "leaf_rec": 6, "shade_prim": 7,
               "xforms": 8}


# ---- the C ABI of librtmi.so: per header of include/, name -> (restype, argtypes) ---------------------------------------------
# load_rtmi() applies these tables and the *_SYMBOLS lists below are their keys, so a function cannot be listed without a
# signature.  tests/test_abi_signatures.py compares every entry with the prototype its header declares.
def _tables():
    vp, i, u32, u64, d, sz, P = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_double, C.c_size_t, C.POINTER
    cam, rp, st, desc = P(Camera), P(RenderParams), P(Stats), P(SceneDesc)
    query = [vp, P(QueryParams), vp, vp, vp]
    frame = [vp, cam, u32, u64]
    upscale = [i, u32, u32, u32, u32, P(UpscaleParams), P(UpscaleIn), P(UpscaleOut)]
    sparse = [vp, rp, cam, P(SparseParams)]
    return {
        "rtmi.h": {
            "rtmi_device_count": (i, []),
            "rtmi_last_error": (C.c_char_p, []),
            "rtmi_build_hash": (C.c_char_p, []),
            "rtmi_scene_create": (i, [desc, i, P(vp)]),
            "rtmi_scene_destroy": (None, [vp]),
            "rtmi_release_cached": (None, []),
            "rtmi_local_tiles": (u32, [rp]),
            "rtmi_render_prepare": (i, [vp, rp]),
            "rtmi_render_device": (i, [vp, cam, rp, vp, vp, st]),
            "rtmi_scene_status": (i, [vp, P(u32)]),
            "rtmi_render": (i, [vp, cam, rp, vp, vp, vp, st]),
            "rtmi_render_multi": (i, [desc, P(i), u32, cam, rp, vp, vp, st]),
            "rtmi_multi_create": (i, [desc, P(i), u32, P(vp)]),
            "rtmi_multi_prepare": (i, [vp, rp]),
            "rtmi_multi_render": (i, [vp, cam, rp, vp, vp, st]),
            "rtmi_multi_destroy": (None, [vp]),
            "rtmi_multi_collective": (i, [vp]),
            "rtmi_partial_image": (i, [vp, rp, vp, vp, P(u32)]),
            "rtmi_untile": (i, [rp, vp, vp, vp]),
            "rtmi_ppm_p3": (sz, [u32, u32, vp, vp, sz]),
            "rtmi_write_ppm": (i, [C.c_char_p, u32, u32, vp, i]),
            "rtmi_probe_math": (i, [i, vp, vp, vp, u32]),
            "rtmi_probe_philox": (i, [vp, vp, vp, u32]),
            "rtmi_probe_xform": (i, [P(Xform), u32, vp, vp, vp, u32]),
            "rtmi_probe_geom": (i, [i, vp, vp, vp, u32, vp, u32, vp, vp, u32]),
            "rtmi_probe_path": (i, [vp, i, vp, u32, vp, u32, vp, vp, vp, u32]),
            "rtmi_probe_stream": (i, [i, u64, vp, u32, vp, u32]),
        },
        "rtmi_math.h": {},  # inline helpers only
        "rtmi_f64.h": {
            "rtmi_scene_attach_f64": (i, [vp, P(SceneF64)]),
            "rtmi_render_f64": (i, [vp, P(CameraF64), rp, d, vp, vp, vp, st]),
            "rtmi_probe_math_f64": (i, [i, vp, vp, vp, u32]),
        },
        "rtmi_adaptive.h": {
            "rtmi_render_adaptive": (i, [vp, cam, rp, P(Adaptive), vp, vp, vp, vp, st]),
        },
        "rtmi_features.h": {
            "rtmi_render_features": (i, [vp, cam, rp, vp, vp, vp, vp, vp, st]),
        },
        "rtmi_denoise.h": {
            "rtmi_denoise": (i, [i, u32, u32, P(DenoiseParams), vp, vp, vp, vp, vp, vp, vp]),
            "rtmi_probe_expf": (i, [i, vp, vp, u32]),
        },
        "rtmi_nee.h": {
            "rtmi_lights_from_desc": (i, [desc, P(Light), u32, P(u32)]),
            "rtmi_scene_attach_lights": (i, [vp, desc]),
            "rtmi_render_nee": (i, [vp, cam, rp, vp, vp, vp, vp, st]),
        },
        "rtmi_light_coop.h": {},  # a flag of the NEE / environment entries
        "rtmi_light_tree.h": {
            "rtmi_light_tree_from_desc": (i, [desc, P(LightNode), u32, P(u32), P(LightPath)]),
            "rtmi_light_tree_pick": (i, [vp, u32, vp, vp, u32, vp, vp]),
            "rtmi_light_tree_pmf": (i, [vp, u32, vp, vp, vp, u32, vp]),
            "rtmi_scene_attach_light_tree": (i, [vp, desc]),
            "rtmi_probe_light_tree": (i, [vp, i, vp, vp, u32, vp, vp]),
        },
        "rtmi_env.h": {
            "rtmi_env_tables": (i, [P(EnvMap), vp, vp, vp, vp, P(d)]),
            "rtmi_scene_attach_env": (i, [vp, P(EnvMap)]),
            "rtmi_render_env": (i, [vp, cam, rp, P(EnvRender), vp, vp, vp, vp, st]),
            "rtmi_probe_env": (i, [vp, i, vp, vp, u32]),
        },
        "rtmi_adaptive_nee.h": {
            "rtmi_render_adaptive_env": (i, [vp, cam, rp, P(EnvRender), P(Adaptive), vp, vp, vp, vp, st]),
            "rtmi_render_adaptive_nee": (i, [vp, cam, rp, P(Adaptive), vp, vp, vp, vp, st]),
        },
        "rtmi_roulette.h": {
            "rtmi_render_adaptive_roulette": (i, [vp, cam, rp, P(Roulette), P(Adaptive), vp, vp, vp, vp, vp, st]),
            "rtmi_render_roulette": (i, [vp, cam, rp, P(Roulette), vp, vp, vp, vp, st]),
        },
        "rtmi_roulette_coop.h": {},  # a flag of the roulette entries
        "rtmi_session.h": {
            "rtmi_session_create": (i, [vp, cam, rp, P(SessionOpts), P(vp)]),
            "rtmi_session_destroy": (None, [vp]),
            "rtmi_session_export": (i, [vp, vp, sz, P(sz)]),
            "rtmi_session_image": (i, [vp, vp, vp, vp, vp, vp]),
            "rtmi_session_import": (i, [vp, vp, sz]),
            "rtmi_session_merge": (i, [vp, vp]),
            "rtmi_session_refine": (i, [vp, d, d, u32, st]),
            "rtmi_session_render": (i, [vp, u32, st]),
            "rtmi_session_spp": (i, [vp, P(u32), P(u32)]),
        },
        "rtmi_query.h": {
            "rtmi_occluded": (i, query + [P(d)]),
            "rtmi_occluded_device": (i, query + [vp]),
            "rtmi_scene_attach_flips": (i, [vp, vp, u32, vp, u32]),
            "rtmi_trace": (i, query + [P(d)]),
            "rtmi_trace_device": (i, query + [vp]),
        },
        "rtmi_radiance.h": {
            "rtmi_radiance": (i, [vp, P(RadianceParams), vp, vp, vp, vp, vp, P(d)]),
            "rtmi_radiance_device": (i, [vp, P(RadianceParams), vp, vp, vp, vp, vp, vp]),
        },
        "rtmi_gather.h": {
            "rtmi_gather": (i, [vp, P(GatherParams), vp, vp, vp, vp, vp, vp, P(d)]),
            "rtmi_gather_device": (i, [vp, P(GatherParams), vp, vp, vp, vp, vp, vp, vp, u64, vp]),
            "rtmi_gather_directions": (i, [P(GatherParams), vp, u32, vp]),
        },
        "rtmi_temporal.h": {
            "rtmi_temporal_create": (i, [i, u32, u32, P(TemporalParams), P(vp)]),
            "rtmi_temporal_destroy": (None, [vp]),
            "rtmi_temporal_push": (i, [vp, cam, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
            "rtmi_temporal_reset": (i, [vp]),
        },
        "rtmi_frame.h": {
            "rtmi_frame_create": (i, [vp, rp, P(FrameOpts), P(vp)]),
            "rtmi_frame_destroy": (None, [vp]),
            "rtmi_frame_render": (i, frame + [P(FrameOut), st]),
            "rtmi_frame_render_device": (i, frame + [P(FrameOut), st]),
            "rtmi_frame_reset": (i, [vp]),
            "rtmi_probe_frame_untile": (i, [i, u32, u32, vp, vp, vp, vp, P(u32)]),
        },
        "rtmi_tonemap.h": {
            "rtmi_probe_tonemap_histogram": (i, [i, u32, u32, P(TonemapParams), vp, vp]),
            "rtmi_tonemap_apply": (i, [vp, vp, C.c_float, vp, vp, P(TonemapState)]),
            "rtmi_tonemap_apply_device": (i, [vp, vp, C.c_float, vp, vp, vp, vp]),
            "rtmi_tonemap_create": (i, [i, u32, u32, P(TonemapParams), P(vp)]),
            "rtmi_tonemap_destroy": (None, [vp]),
            "rtmi_tonemap_reset": (i, [vp]),
        },
        "rtmi_upscale.h": {
            "rtmi_upscale": (i, upscale),
            "rtmi_upscale_device": (i, upscale + [vp]),
            "rtmi_upscaler_create": (i, [vp, rp, P(UpscalerOpts), P(vp)]),
            "rtmi_upscaler_destroy": (None, [vp]),
            "rtmi_upscaler_render": (i, frame + [P(UpscalerOut), st]),
            "rtmi_upscaler_render_device": (i, frame + [P(UpscalerOut), st]),
            "rtmi_upscaler_reset": (i, [vp]),
        },
        "rtmi_sparse.h": {
            "rtmi_sparse_patch_device": (i, [i, u32, vp, vp, u32, vp, vp, vp, vp, u32, vp]),
            "rtmi_sparse_refine": (i, sparse + [u32, u32, vp, vp, vp, vp, vp]),
            "rtmi_sparse_refine_device": (i, sparse + [u32, u32, vp, vp, vp, vp, vp, u64, vp, vp]),
            "rtmi_sparse_render": (i, sparse + [vp, vp, vp, vp, P(d)]),
            "rtmi_sparse_render_device": (i, sparse + [vp] * 7),
            "rtmi_sparse_scratch_bytes": (u64, [u64, u32, u32]),
            "rtmi_sparse_select_device": (i, [i, u32, vp, u32, u32, vp, vp, vp, vp]),
        },
        "rtmi_pixelwise.h": {
            "rtmi_pixelwise_scratch_bytes": (u64, [u64, u32, u32]),
            "rtmi_pixelwise_steps": (u32, [u32] * 3),
            "rtmi_probe_pixelwise_step": (i, [i, u32, u32, vp, vp, vp, vp, u32, u32, u32, u32, d, d, vp, vp, vp, vp, vp]),
            "rtmi_render_pixelwise": (i, [vp, cam, rp, P(PixelwiseOpts)] + [vp] * 5 + [st]),
            "rtmi_render_pixelwise_device": (i, [vp, rp, cam, P(PixelwiseOpts)] + [vp] * 6 + [u64, vp]),
        },
        "rtmi_window.h": {
            "rtmi_probe_window_spread": (i, [i, u32, u32, u32, vp, vp]),
            "rtmi_render_window": (i, [vp, cam, rp, P(WindowOpts)] + [vp] * 5 + [st]),
            "rtmi_render_window_device": (i, [vp, rp, cam, P(WindowOpts)] + [vp] * 6 + [u64, vp]),
            "rtmi_window_scratch_bytes": (u64, [u64, u32, u32]),
            "rtmi_window_spread_device": (i, [vp, vp, u32, u32, u32, vp]),
            "rtmi_window_steps": (u32, [u32] * 3),
        },
        "rtmi_batch_coop.h": {},  # a flag of the batch entries
    }


FAMILIES = _tables()  # header file name -> {function: (restype, argtypes)}
RTMI_SYMBOLS = list(FAMILIES["rtmi.h"])
RTMI_F64_SYMBOLS = list(FAMILIES["rtmi_f64.h"])
RTMI_ADAPTIVE_SYMBOLS = list(FAMILIES["rtmi_adaptive.h"])
RTMI_FEATURES_SYMBOLS = list(FAMILIES["rtmi_features.h"])
RTMI_DENOISE_SYMBOLS = list(FAMILIES["rtmi_denoise.h"])
RTMI_NEE_SYMBOLS = list(FAMILIES["rtmi_nee.h"])
RTMI_LIGHT_TREE_SYMBOLS = list(FAMILIES["rtmi_light_tree.h"])
RTMI_ENV_SYMBOLS = list(FAMILIES["rtmi_env.h"])
RTMI_ADAPTIVE_NEE_SYMBOLS = list(FAMILIES["rtmi_adaptive_nee.h"])
RTMI_ROULETTE_SYMBOLS = list(FAMILIES["rtmi_roulette.h"])
SESSION_SYMBOLS = list(FAMILIES["rtmi_session.h"])
RTMI_QUERY_SYMBOLS = list(FAMILIES["rtmi_query.h"])
RTMI_RADIANCE_SYMBOLS = list(FAMILIES["rtmi_radiance.h"])
RTMI_GATHER_SYMBOLS = list(FAMILIES["rtmi_gather.h"])
RTMI_TEMPORAL_SYMBOLS = list(FAMILIES["rtmi_temporal.h"])
RTMI_FRAME_SYMBOLS = list(FAMILIES["rtmi_frame.h"])
RTMI_TONEMAP_SYMBOLS = list(FAMILIES["rtmi_tonemap.h"])
RTMI_UPSCALE_SYMBOLS = list(FAMILIES["rtmi_upscale.h"])
RTMI_SPARSE_SYMBOLS = list(FAMILIES["rtmi_sparse.h"])
RTMI_PIXELWISE_SYMBOLS = list(FAMILIES["rtmi_pixelwise.h"])
RTMI_WINDOW_SYMBOLS = list(FAMILIES["rtmi_window.h"])


# ---- the scene updates (include/rtmi_update.h): a family of its own, prefix rtmu_ ----------------------------------------------
# Not part of FAMILIES: those tables are the render ABI, whose size tests/test_abi_signatures.py pins; tests/test_update_abi.py
# compares these two with the header, with sys.rs and with what the libraries export.  load_rtmi() applies UPDATE_ENTRIES;
# the host library's wrappers are bound by bind_host_update(), which Host() calls.
def _update_tables():
    vp, i, u32, sz, P = C.c_void_p, C.c_int, C.c_uint32, C.c_size_t, C.POINTER
    desc = P(SceneDesc)
    entries = {
        "rtmu_probe_scene_words": (i, [vp, i, vp, sz, P(sz)]),
        "rtmu_refit_desc": (i, [desc, u32, u32, P(Item), P(BvhNode), P(Bvh4Node), vp]),
        "rtmu_refittable": (i, [desc, vp]),
        "rtmu_scene_update_prepare": (i, [vp]),
        "rtmu_scene_update_prims": (i, [vp, u32, u32, vp, vp]),
        "rtmu_scene_update_prims_device": (i, [vp, u32, u32, vp, vp, vp]),
        "rtmu_scene_update_xforms": (i, [vp, u32, u32, P(Xform)]),
    }
    host = {
        "rthu_refittable": (i, [vp, vp]),
        "rthu_update_prepare": (i, [vp]),
        "rthu_update_prims": (i, [vp, u32, u32, vp, vp]),
        "rthu_update_prims_device": (i, [vp, u32, u32, vp, vp, vp]),
        "rthu_update_xforms": (i, [vp, u32, u32, P(Xform)]),
        "rthu_prims_of": (i, [vp, vp, vp, u32, P(u32)]),
        "rthu_probe_scene_words": (i, [vp, i, vp, sz, P(sz)]),
    }
    return entries, host


UPDATE_ENTRIES, UPDATE_HOST_ENTRIES = _update_tables()


def _bind(lib, table):
    for name, (res, args) in table.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def bind_host_update(lib):
    """Sets the signatures of the update wrappers of librt_host.so (UPDATE_HOST_ENTRIES) on a loaded library."""
    return _bind(lib, UPDATE_HOST_ENTRIES)


# ---- the lights that follow an update (include/rtmi_relight.h): a family of its own, prefix rtml_ ----------------------------
# As the update family above: outside FAMILIES, compared with the header, sys.rs and the libraries' exports by
# tests/test_relight_abi.py.  load_rtmi() applies RELIGHT_ENTRIES; bind_host_relight(), which Host() calls, the wrappers'.
# RTML_WORDS_* of the header, in its order: the light arrays rtml_probe_light_words copies out.
LIGHT_WORDS = {"lights": 0, "prim_light": 1, "tree_nodes": 2, "tree_paths": 3}


def _relight_tables():
    i, u32, vp, sz, P = C.c_int, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER
    entries = {
        "rtml_probe_light_words": (i, [vp, i, vp, sz, P(sz)]),
        "rtml_relight_desc": (i, [P(SceneDesc), P(Light), u32, vp, u32]),
        "rtml_scene_follow_lights": (i, [vp, i]),
    }
    host = {
        "rthl_follow_lights": (i, [vp, i]),
        "rthl_probe_light_words": (i, [vp, i, vp, sz, P(sz)]),
    }
    return entries, host


RELIGHT_ENTRIES, RELIGHT_HOST_ENTRIES = _relight_tables()


def bind_host_relight(lib):
    """Sets the signatures of the relight wrappers of librt_host.so (RELIGHT_HOST_ENTRIES) on a loaded library."""
    return _bind(lib, RELIGHT_HOST_ENTRIES)

_rtmi = None
_host = None


def load_rtmi():
    """librtmi.so: the C ABI of include/rtmi.h (HIP kernels inside)."""
    global _rtmi
    if _rtmi is not None:
        return _rtmi
    path = _build.LIBRTMI
    if not os.path.exists(path):
        _build.build_rtmi()
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    for table in FAMILIES.values():
        for name, (res, args) in table.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
    _bind(lib, UPDATE_ENTRIES)
    _bind(lib, RELIGHT_ENTRIES)
    _rtmi = lib
    return lib


def load_host():
    """librt_host.so: the C++ mirror of the reference's trait surface (links librtmi.so)."""
    global _host
    if _host is not None:
        return _host
    load_rtmi()
    path = _build.LIBHOST
    if not os.path.exists(path):
        _build.build_host()
    lib = C.CDLL(path)
    vp, d, i, u32, u64 = C.c_void_p, C.c_double, C.c_int, C.c_uint32, C.c_uint64
    sig = {
        "rth_last_error": (C.c_char_p, []),
        "rth_last_error_code": (i, []),
        "rth_free_all": (None, []),
        "rth_seed_scene_rng": (None, [u64]),
        "rth_scene_uniform": (d, []),
        "rth_philox": (None, [vp, vp, vp]),
        "rth_tex_solid": (vp, [d, d, d]),
        "rth_tex_checker": (vp, [vp, vp]),
        "rth_tex_noise": (vp, [d]),
        "rth_tex_image": (vp, [vp, u32, u32]),
        "rth_perlin_tables": (i, [vp, vp, vp]),
        "rth_mat_lambertian": (vp, [vp]),
        "rth_mat_metal": (vp, [vp, d]),
        "rth_mat_dielectric": (vp, [d]),
        "rth_mat_diffuse_light": (vp, [vp]),
        "rth_mat_isotropic": (vp, [vp]),
        "rth_sphere": (vp, [d, d, d, d, vp]),
        "rth_moving_sphere": (vp, [d] * 9 + [vp]),
        "rth_rect": (vp, [i, d, d, d, d, d, vp]),
        "rth_cube": (vp, [d] * 6 + [vp]),
        "rth_flip_normals": (vp, [vp]),
        "rth_translate": (vp, [vp, d, d, d]),
        "rth_rotate": (vp, [i, vp, d]),
        "rth_constant_medium": (vp, [vp, d, vp]),
        "rth_list_new": (vp, []),
        "rth_list_push": (i, [vp, vp]),
        "rth_bvh": (vp, [vp, i, d, d]),
        "rth_camera": (vp, [d] * 15),
        "rth_camera_lower": (i, [vp, C.POINTER(Camera)]),
        "rth_camera_state": (i, [vp, vp]),
        "rth_lower": (vp, [vp]),
        "rth_lowered_desc": (i, [vp, C.POINTER(SceneDesc)]),
        "rth_upload": (i, [vp, i]),
        "rth_render": (i, [vp, vp, C.POINTER(RenderParams), vp, vp, vp, C.POINTER(Stats)]),
        "rth_lowered_desc_f64": (i, [vp, C.POINTER(SceneF64)]),
        "rth_camera_lower_f64": (i, [vp, C.POINTER(CameraF64)]),
        "rth_attach_f64": (i, [vp]),
        "rth_render_f64": (i, [vp, vp, C.POINTER(RenderParams), d, vp, vp, vp, C.POINTER(Stats)]),
        "rth_render_adaptive": (i, [vp, vp, C.POINTER(RenderParams), C.POINTER(Adaptive), vp, vp, vp, vp, C.POINTER(Stats)]),
        "rth_render_features": (i, [vp, vp, C.POINTER(RenderParams), vp, vp, vp, vp, vp, C.POINTER(Stats)]),
        "rth_attach_lights": (i, [vp]),
        "rth_render_nee": (i, [vp, vp, C.POINTER(RenderParams), vp, vp, vp, vp, C.POINTER(Stats)]),
        "rth_attach_light_tree": (i, [vp]),
        "rth_probe_light_tree": (i, [vp, i, vp, vp, u32, vp, vp]),
        "rth_attach_env": (i, [vp, u32, u32, vp]),
        "rth_render_env": (i, [vp, vp, C.POINTER(RenderParams), C.POINTER(EnvRender), vp, vp, vp, vp, C.POINTER(Stats)]),
        "rth_probe_env": (i, [vp, i, vp, vp, u32]),
        "rth_render_adaptive_nee": (i, [vp, vp, C.POINTER(RenderParams), C.POINTER(Adaptive), vp, vp, vp, vp, C.POINTER(Stats)]),
        "rth_render_adaptive_env": (i, [vp, vp, C.POINTER(RenderParams), C.POINTER(EnvRender), C.POINTER(Adaptive), vp, vp, vp, vp,
                                        C.POINTER(Stats)]),
        "rth_render_roulette": (i, [vp, vp, C.POINTER(RenderParams), C.POINTER(Roulette), vp, vp, vp, vp, C.POINTER(Stats)]),
        "rth_render_adaptive_roulette": (i, [vp, vp, C.POINTER(RenderParams), C.POINTER(Roulette), C.POINTER(Adaptive), vp, vp,
                                             vp, vp, vp, C.POINTER(Stats)]),
        "rth_session_create": (vp, [vp, vp, C.POINTER(RenderParams), C.POINTER(SessionOpts)]),
        "rth_session_close": (i, [vp]),
        "rth_session_render": (i, [vp, u32, C.POINTER(Stats)]),
        "rth_session_refine": (i, [vp, d, d, u32, C.POINTER(Stats)]),
        "rth_session_image": (i, [vp, vp, vp, vp, vp, vp]),
        "rth_session_export": (i, [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
        "rth_session_import": (i, [vp, vp, C.c_size_t]),
        "rth_session_merge": (i, [vp, vp]),
        "rth_session_spp": (i, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "rth_frame_create": (vp, [vp, C.POINTER(RenderParams), C.POINTER(FrameOpts)]),
        "rth_frame_close": (i, [vp]),
        "rth_frame_render": (i, [vp, vp, u32, u64, C.POINTER(FrameOut), i, C.POINTER(Stats)]),
        "rth_frame_reset": (i, [vp]),
        "rth_upscaler_create": (vp, [vp, C.POINTER(RenderParams), C.POINTER(UpscalerOpts)]),
        "rth_upscaler_close": (i, [vp]),
        "rth_upscaler_render": (i, [vp, vp, u32, u64, C.POINTER(UpscalerOut), i, C.POINTER(Stats)]),
        "rth_upscaler_reset": (i, [vp]),
        "rth_trace": (i, [vp, C.POINTER(QueryParams), vp, vp, vp, C.POINTER(C.c_double)]),
        "rth_occluded": (i, [vp, C.POINTER(QueryParams), vp, vp, vp, C.POINTER(C.c_double)]),
        "rth_trace_device": (i, [vp, C.POINTER(QueryParams), vp, vp, vp, vp]),
        "rth_occluded_device": (i, [vp, C.POINTER(QueryParams), vp, vp, vp, vp]),
        "rth_radiance": (i, [vp, C.POINTER(RadianceParams), vp, vp, vp, vp, vp, C.POINTER(C.c_double)]),
        "rth_radiance_device": (i, [vp, C.POINTER(RadianceParams), vp, vp, vp, vp, vp, vp]),
        "rth_sparse_render": (i, [vp, vp, C.POINTER(RenderParams), C.POINTER(SparseParams), vp, vp, vp, vp, C.POINTER(C.c_double)]),
        "rth_sparse_render_device": (i, [vp, vp, C.POINTER(RenderParams), C.POINTER(SparseParams)] + [vp] * 7),
        "rth_sparse_refine": (i, [vp, vp, C.POINTER(RenderParams), C.POINTER(SparseParams), u32, u32, vp, vp, vp, vp, vp, u64, vp, i, vp]),
        "rth_render_pixelwise": (i, [vp, vp, C.POINTER(RenderParams), C.POINTER(PixelwiseOpts)] + [vp] * 5 + [C.POINTER(Stats)]),
        "rth_render_pixelwise_device": (i, [vp, vp, C.POINTER(RenderParams), C.POINTER(PixelwiseOpts)] + [vp] * 6 + [u64, vp]),
        "rth_render_window": (i, [vp, vp, C.POINTER(RenderParams), C.POINTER(WindowOpts)] + [vp] * 5 + [C.POINTER(Stats)]),
        "rth_render_window_device": (i, [vp, vp, C.POINTER(RenderParams), C.POINTER(WindowOpts)] + [vp] * 6 + [u64, vp]),
        "rth_gather": (i, [vp, C.POINTER(GatherParams), vp, vp, vp, vp, vp, vp, C.POINTER(C.c_double)]),
        "rth_gather_device": (i, [vp, C.POINTER(GatherParams), vp, vp, vp, vp, vp, vp, vp, C.c_uint64, vp]),
        "rth_render_device": (i, [vp, vp, C.POINTER(RenderParams), vp, vp, C.POINTER(Stats)]),
        "rth_render_prepare": (i, [vp, C.POINTER(RenderParams)]),
        "rth_scene_status": (i, [vp]),
        "rth_render_multi": (i, [vp, vp, C.POINTER(RenderParams), C.POINTER(C.c_int), u32, vp, vp, C.POINTER(Stats)]),
        "rth_partial_image": (i, [vp, C.POINTER(RenderParams), vp, vp, C.POINTER(C.c_uint32)]),
        "rth_upload_multi": (i, [vp, C.POINTER(C.c_int), u32]),
        "rth_multi_free": (i, [vp]),
        "rth_multi_collective": (i, [vp]),
        "rth_multi_prepare": (i, [vp, C.POINTER(RenderParams)]),
        "rth_multi_render": (i, [vp, vp, C.POINTER(RenderParams), vp, vp, C.POINTER(Stats)]),
        "rth_camera_render": (i, [vp, vp, u32, u32, u32, u64, u32, i, vp, vp, C.POINTER(Stats)]),
        "rth_camera_render_f64": (i, [vp, vp, u32, u32, u32, u64, u32, i, vp, vp, C.POINTER(Stats)]),
        "rth_hit": (i, [vp, vp, vp, d, d, d, u64, vp, vp]),
        "rth_bounding_box": (i, [vp, d, d, vp, vp]),
        "rth_tex_value": (i, [vp, d, d, vp, vp]),
        "rth_scatter": (i, [vp, vp, vp, d, vp, u64, vp, vp]),
        "rth_emitted": (i, [vp, d, d, vp, vp]),
        "rth_get_ray": (i, [vp, d, d, u64, vp]),
        "rth_set_sky_background": (None, [i]),
        "rth_set_face_forward": (None, [i]),
        "rth_set_uv_book": (None, [i]),
        "rth_color_sample": (i, [vp, vp, u32, u32, u32, u32, u32, u64, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _host = lib
    return lib
