//! Raw FFI of include/rtmi.h (ABI version 5): one declaration per entry point, one `#[repr(C)]` struct per
//! C struct, same field order.  UNVERIFIED SOURCE: the build image has no Rust toolchain; the layouts are
//! kept in sync with the tested ctypes binding (raytracing_rust_amd/abi.py) by tests/test_rust_binding_source.py.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_void};

pub const RTMI_ABI_VERSION: u32 = 7;
pub const RTMI_FLAG_FAST_CULL: u32 = 1;
pub const RTMI_FLAG_PATH_SIG: u32 = 2;
pub const RTMI_FLAG_PROFILE: u32 = 4;
pub const RTMI_FLAG_SYNC: u32 = 8;
pub const RTMI_FLAG_ASYNC: u32 = 16;
pub const RTMI_FLAG_SKY: u32 = 32;
pub const RTMI_FLAG_REF_TREE: u32 = 64;
pub const RTMI_FLAG_BLOCK_COOP: u32 = 32768;
pub const RTMI_SAMPLE_SLOT_BYTES: u32 = 12;
pub const RTMI_FLAG_FACE_FORWARD: u32 = 128;
pub const RTMI_FLAG_UV_BOOK: u32 = 4096;
/// opt-in: after every pass the framebuffer holds the image of the samples so far (rtmi_partial_image)
pub const RTMI_FLAG_PROGRESSIVE: u32 = 16384;
/// include/rtmi_light_coop.h: the NEE / environment entries trace on the wave-cooperative kernel (same bits)
pub const RTMI_FLAG_LIGHT_COOP: u32 = 65536;
pub const RTMI_FLAG_ROULETTE_COOP: u32 = 131072;
/// include/rtmi_light_tree.h: rtmi_render_nee picks its light by walking the light tree
pub const RTMI_FLAG_LIGHT_TREE: u32 = 262144;
pub const RTMI_OK: i32 = 0;
pub const RTMI_ERR_INVALID: i32 = 1;
pub const RTMI_ERR_UNSUPPORTED: i32 = 2;
pub const RTMI_ERR_DEVICE: i32 = 3;
pub const RTMI_ERR_NOMEM: i32 = 4;
pub const RTMI_ERR_CANCELLED: i32 = 5;
pub const RTMI_TEXEL_POISON: u32 = 0x8000_0000;
pub const RTMI_MAX_BVH_DEPTH: u32 = 24;
pub const RTMI_TILE: u32 = 8;
pub const RTMI_TEX_SOLID: i32 = 0;
pub const RTMI_TEX_CHECKER: i32 = 1;
pub const RTMI_TEX_NOISE: i32 = 2;
pub const RTMI_TEX_IMAGE: i32 = 3;
pub const RTMI_MAT_LAMBERTIAN: i32 = 0;
pub const RTMI_MAT_METAL: i32 = 1;
pub const RTMI_MAT_DIELECTRIC: i32 = 2;
pub const RTMI_MAT_DIFFUSE_LIGHT: i32 = 3;
pub const RTMI_MAT_ISOTROPIC: i32 = 4;
pub const RTMI_MATFLAG_NEEDS_UV: u32 = 1;
pub const RTMI_PRIM_SPHERE: i32 = 0;
pub const RTMI_PRIM_MSPHERE: i32 = 1;
pub const RTMI_PRIM_RECT: i32 = 2;
pub const RTMI_PRIM_CUBE: i32 = 3;
pub const RTMI_PRIMFLAG_FLIP: u32 = 1;
pub const RTMI_PRIMFLAG_PLANE_SHIFT: u32 = 8;
/// instanced primitive (rtmi.h): bits 4..7 = number of its own transforms, bits 12..31 = index of the first in xforms
pub const RTMI_PRIMFLAG_XF_COUNT_SHIFT: u32 = 4;
pub const RTMI_PRIMFLAG_XF_FIRST_SHIFT: u32 = 12;
pub const RTMI_PRIM_XF_MAX: u32 = 15;
pub const RTMI_XF_TRANSLATE: i32 = 0;
pub const RTMI_XF_ROTATE_X: i32 = 1;
pub const RTMI_XF_ROTATE_Y: i32 = 2;
pub const RTMI_XF_ROTATE_Z: i32 = 3;
/// not transforms: the two records behind the chain of a DEFERRED BVH item hold its gate box
pub const RTMI_XF_GATE_MIN: i32 = 4;
pub const RTMI_XF_GATE_MAX: i32 = 5;
/// not a transform: x = -(1/density) of the inner medium of a nested pair, behind the chain (and the gate records)
pub const RTMI_XF_INNER_MEDIUM: i32 = 6;
pub const RTMI_ITEM_LIST: i32 = 0;
pub const RTMI_ITEM_BVH: i32 = 1;
pub const RTMI_ITEMFLAG_FLIP: u32 = 1;
pub const RTMI_ITEMFLAG_MEDIUM: u32 = 2;
/// MEDIUM items: bits 8..11 = number of the item's first transforms that wrap the ConstantMedium itself
pub const RTMI_ITEMFLAG_MEDIUM_OUTER_SHIFT: u32 = 8;
/// a ConstantMedium that was a child of a BVHNode follows its BVH item as a DEFERRED item (rtmi.h): SAVE_T0 on the BVH item
/// (or on the first deferred one when the BVH holds nothing but media) remembers the closest hit before it
pub const RTMI_ITEMFLAG_SAVE_T0: u32 = 4;
pub const RTMI_ITEMFLAG_DEFERRED: u32 = 8;
/// a ConstantMedium whose boundary is a ConstantMedium: the inner density travels in an RTMI_XF_INNER_MEDIUM record
pub const RTMI_ITEMFLAG_NESTED_MEDIUM: u32 = 16;
/// a HittableList with media among its members as a BVH child: a group of DEFERRED member items and a terminator (rtmi.h)
pub const RTMI_ITEMFLAG_LISTSCAN_BEGIN: u32 = 32;
pub const RTMI_ITEMFLAG_LISTSCAN_MEMBER: u32 = 64;
pub const RTMI_ITEMFLAG_LISTSCAN_END: u32 = 128;
/// DEFERRED items: bits 12..15 = number of leading transforms that belong to the enclosing BVH item
pub const RTMI_ITEMFLAG_GATE_OUTER_SHIFT: u32 = 12;
pub const RTMI_NO_CHILD: i32 = 0x7fff_ffff;

#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiTexture {
    pub kind: i32,
    pub i0: i32,
    pub i1: i32,
    pub pad: i32,
    pub f0: f32,
    pub f1: f32,
    pub f2: f32,
    pub f3: f32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiPerlin {
    pub ranvec: [f32; 1024],
    pub perm: [i32; 768],
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiImage {
    pub offset: u64,
    pub nx: u32,
    pub ny: u32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiMaterial {
    pub kind: i32,
    pub tex: i32,
    pub param: f32,
    pub flags: u32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiPrimMeta {
    pub material: i32,
    pub flags: u32,
    pub inv_dt: f32,
    pub r#type: i32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiBvhNode {
    pub lmin: [f32; 3],
    pub lmax: [f32; 3],
    pub rmin: [f32; 3],
    pub rmax: [f32; 3],
    pub left: i32,
    pub right: i32,
    pub pad: [i32; 2],
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiBvh4Node {
    pub minx: [f32; 4],
    pub miny: [f32; 4],
    pub minz: [f32; 4],
    pub maxx: [f32; 4],
    pub maxy: [f32; 4],
    pub maxz: [f32; 4],
    pub child: [i32; 4],
    pub pad: [i32; 4],
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiXform {
    pub kind: i32,
    pub x: f32,
    pub y: f32,
    pub z: f32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiItem {
    pub kind: i32,
    pub first: i32,
    pub count: i32,
    pub flags: u32,
    pub xform_first: i32,
    pub xform_count: i32,
    pub medium_material: i32,
    pub neg_inv_density: f32,
    pub root_min: [f32; 3],
    pub root_max: [f32; 3],
    pub scale: f32,
    pub alt_first: i32,
}

#[repr(C)]
pub struct RtmiSceneDesc {
    pub abi_version: u32,
    pub n_items: u32,
    pub items: *const RtmiItem,
    pub n_prims: u32,
    pub prim_a: *const f32,
    pub prim_b: *const f32,
    pub prim_meta: *const RtmiPrimMeta,
    pub prim_gate: *const f32,
    pub alt_max_depth: u32,
    pub n_alt_nodes: u32,
    pub alt_nodes: *const RtmiBvh4Node,
    pub n_nodes: u32,
    pub nodes: *const RtmiBvhNode,
    pub n_xforms: u32,
    pub xforms: *const RtmiXform,
    pub n_materials: u32,
    pub materials: *const RtmiMaterial,
    pub n_textures: u32,
    pub textures: *const RtmiTexture,
    pub n_perlin: u32,
    pub perlin: *const RtmiPerlin,
    pub n_images: u32,
    pub images: *const RtmiImage,
    pub image_data: *const u8,
    pub image_bytes: u64,
    pub max_bvh_depth: u32,
    pub bvh_time_lo: f32,
    pub bvh_time_hi: f32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiCamera {
    pub origin: [f32; 3],
    pub lower_left_corner: [f32; 3],
    pub horizontal: [f32; 3],
    pub vertical: [f32; 3],
    pub u: [f32; 3],
    pub v: [f32; 3],
    pub time0: f32,
    pub time1: f32,
    pub lens_radius: f32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiRenderParams {
    pub nx: u32,
    pub ny: u32,
    pub ns: u32,
    pub max_depth: u32,
    pub t_min: f32,
    pub flags: u32,
    pub seed: u64,
    pub tile_rank: u32,
    pub tile_world: u32,
    pub spp_chunks: u32,
    pub shade_threshold: u32,
    pub path_sig: u64,
    pub prof: u64,
    pub sample_buffer_bytes: u64,
    /// `RtmiProgressFn` cast to an integer, or 0 (called by the blocking entry points about every 50 ms)
    pub progress_fn: u64,
    pub progress_user: u64,
}
/// `int (*)(uint64_t done, uint64_t total, void *user)`; non-zero return = cancel (RTMI_ERR_CANCELLED)
pub type RtmiProgressFn = unsafe extern "C" fn(done: u64, total: u64, user: *mut c_void) -> c_int;

#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiTexel {
    pub r: f32,
    pub g: f32,
    pub b: f32,
    pub rgb8: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct RtmiStats {
    pub kernel_ms: f64,
    pub render_ms: f64,
    pub samples: u64,
    pub tiles: u32,
    pub chunks: u32,
    pub blocks: u32,
    pub kernel: u32, // RTMI_KERNEL_*: which render kernel ran (diagnostics)
}

#[repr(C)]
pub struct RtmiScene {
    _private: [u8; 0],
}

/// opaque persistent multi-device handle (rtmi.h: rtmi_multi)
#[repr(C)]
pub struct RtmiMulti {
    _private: [u8; 0],
}

extern "C" {
    pub fn rtmi_device_count() -> c_int;
    pub fn rtmi_last_error() -> *const c_char;
    /// 16 hex digits: hash of the kernel sources, rtmi.h and the compile flags this library was built from
    pub fn rtmi_build_hash() -> *const c_char;
    pub fn rtmi_scene_create(desc: *const RtmiSceneDesc, device: c_int, out: *mut *mut RtmiScene) -> c_int;
    pub fn rtmi_scene_destroy(scene: *mut RtmiScene);
    /// frees the per-sample buffers that destroyed handles left parked (one per device) for their successors
    pub fn rtmi_release_cached();
    pub fn rtmi_local_tiles(p: *const RtmiRenderParams) -> u32;
    pub fn rtmi_render_prepare(scene: *mut RtmiScene, p: *const RtmiRenderParams) -> c_int;
    pub fn rtmi_render_device(
        scene: *mut RtmiScene,
        cam: *const RtmiCamera,
        p: *const RtmiRenderParams,
        d_texels: *mut c_void,
        stream: *mut c_void,
        stats: *mut RtmiStats,
    ) -> c_int;
    pub fn rtmi_scene_status(scene: *mut RtmiScene, overflows: *mut u32) -> c_int;
    pub fn rtmi_render_multi(
        desc: *const RtmiSceneDesc,
        devices: *const c_int,
        n_devices: u32,
        cam: *const RtmiCamera,
        p: *const RtmiRenderParams,
        out_linear_rgb: *mut f32,
        out_rgb8: *mut u8,
        stats: *mut RtmiStats,
    ) -> c_int;
    pub fn rtmi_multi_create(desc: *const RtmiSceneDesc, devices: *const c_int, n_devices: u32, out: *mut *mut RtmiMulti) -> c_int;
    pub fn rtmi_multi_prepare(m: *mut RtmiMulti, p: *const RtmiRenderParams) -> c_int;
    pub fn rtmi_multi_render(
        m: *mut RtmiMulti,
        cam: *const RtmiCamera,
        p: *const RtmiRenderParams,
        out_linear_rgb: *mut f32,
        out_rgb8: *mut u8,
        stats: *mut RtmiStats,
    ) -> c_int;
    pub fn rtmi_multi_destroy(m: *mut RtmiMulti);
    /// RTMI_COLLECTIVE_*: 0 none (one device), 1 peer copies (a device listed twice), 2 one grouped ncclGather
    pub fn rtmi_multi_collective(m: *const RtmiMulti) -> c_int;
    pub fn rtmi_render(
        scene: *mut RtmiScene,
        cam: *const RtmiCamera,
        p: *const RtmiRenderParams,
        out_linear_rgb: *mut f32,
        out_rgb8: *mut u8,
        out_path_sig: *mut u64,
        stats: *mut RtmiStats,
    ) -> c_int;
    /// RTMI_FLAG_PROGRESSIVE: only from inside the progress callback of the rtmi_render call running on `scene`
    pub fn rtmi_partial_image(
        scene: *mut RtmiScene,
        p: *const RtmiRenderParams,
        out_linear_rgb: *mut f32,
        out_rgb8: *mut u8,
        spp_done: *mut u32,
    ) -> c_int;
    pub fn rtmi_untile(
        p: *const RtmiRenderParams,
        gathered: *const RtmiTexel,
        out_linear_rgb: *mut f32,
        out_rgb8: *mut u8,
    ) -> c_int;
    pub fn rtmi_ppm_p3(nx: u32, ny: u32, rgb8: *const u8, buf: *mut c_char, cap: usize) -> usize;
    /// streaming writer: format 3 = the P3 text of `create_image`, 6 = binary P6
    pub fn rtmi_write_ppm(path: *const c_char, nx: u32, ny: u32, rgb8: *const u8, format: c_int) -> c_int;
    pub fn rtmi_probe_math(op: c_int, x: *const f32, y: *const f32, out: *mut f32, n: u32) -> c_int;
    pub fn rtmi_probe_philox(ctr: *const u32, key: *const u32, out: *mut u32, n: u32) -> c_int;
    pub fn rtmi_probe_xform(
        xforms: *const RtmiXform,
        count: u32,
        a: *const f32,
        b: *const f32,
        out: *mut f32,
        n: u32,
    ) -> c_int;
    /// ray-primitive and shading arithmetic of the render kernels (include/rtmi.h: RTMI_PROBE_GEOM_*)
    pub fn rtmi_probe_geom(
        op: c_int,
        prim_a: *const f32,
        prim_b: *const f32,
        meta: *const RtmiPrimMeta,
        n_prims: u32,
        xforms: *const RtmiXform,
        n_xforms: u32,
        input: *const f32,
        out: *mut f32,
        n: u32,
    ) -> c_int;
    /// camera rays, samplers, medium sample and transform chains over scripted words (include/rtmi.h: RTMI_PROBE_PATH_*)
    pub fn rtmi_probe_path(
        scene: *mut RtmiScene,
        op: c_int,
        cams: *const RtmiCamera,
        n_cams: u32,
        xforms: *const RtmiXform,
        n_xforms: u32,
        input: *const f32,
        words: *const u32,
        out: *mut f32,
        n: u32,
    ) -> c_int;
    /// word delivery of the Philox sources under lane divergence (include/rtmi.h)
    pub fn rtmi_probe_stream(kind: c_int, seed: u64, script: *const u8, steps: u32, out: *mut u32, n: u32) -> c_int;
}

// ---- include/rtmi_f64.h: the f64 render mode ---------------------------------------------------------------------------
// Declarations only: lowering a scene's double planes on the Rust side is not provided.

pub const RTMI_SAMPLE_SLOT_BYTES_F64: u32 = 24;

#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiSceneF64 {
    pub n_items: u32,
    pub n_prims: u32,
    pub n_nodes: u32,
    pub n_xforms: u32,
    pub n_materials: u32,
    pub n_textures: u32,
    pub n_perlin: u32,
    pub pad: u32,
    pub prim_a: *const f64,
    pub prim_b: *const f64,
    pub prim_dt: *const f64,
    pub prim_gate: *const f64,
    pub nodes: *const f64,
    pub xforms: *const f64,
    pub item_neg_inv_density: *const f64,
    pub item_root: *const f64,
    pub material_param: *const f64,
    pub texture_f: *const f64,
    pub perlin_ranvec: *const f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiCameraF64 {
    pub origin: [f64; 3],
    pub lower_left_corner: [f64; 3],
    pub horizontal: [f64; 3],
    pub vertical: [f64; 3],
    pub u: [f64; 3],
    pub v: [f64; 3],
    pub time0: f64,
    pub time1: f64,
    pub lens_radius: f64,
}

extern "C" {
    /// attaches the double planes of the scene the handle was created from
    pub fn rtmi_scene_attach_f64(scene: *mut RtmiScene, planes: *const RtmiSceneF64) -> c_int;
    /// blocking whole-image render in double; t_min as a double (0.001, color.rs:7)
    pub fn rtmi_render_f64(
        scene: *mut RtmiScene,
        cam: *const RtmiCameraF64,
        params: *const RtmiRenderParams,
        t_min: f64,
        out_linear_rgb: *mut f64,
        out_rgb8: *mut u8,
        out_path_sig: *mut u64,
        stats: *mut RtmiStats,
    ) -> c_int;
    /// the f64 kernel's sin / log / atan2 / asin / division / sqrt on the device
    pub fn rtmi_probe_math_f64(op: c_int, x: *const f64, y: *const f64, out: *mut f64, n: u32) -> c_int;
}

// ---- include/rtmi_adaptive.h: noise-targeted adaptive sampling -----------------------------------------------------------

#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiAdaptive {
    pub min_spp: u32,
    pub step_spp: u32,
    pub abs_tol: f64,
    pub rel_tol: f64,
}

extern "C" {
    /// blocking whole-image adaptive render: per-tile sample counts up to params.ns, per-pixel standard errors
    pub fn rtmi_render_adaptive(
        scene: *mut RtmiScene,
        cam: *const RtmiCamera,
        params: *const RtmiRenderParams,
        adaptive: *const RtmiAdaptive,
        out_linear: *mut f32,
        out_rgb8: *mut u8,
        out_stderr: *mut f32,
        out_spp: *mut u32,
        stats: *mut RtmiStats,
    ) -> c_int;
}

// ---- include/rtmi_features.h: first-hit albedo, normal and depth buffers for denoisers ------------------------------------

extern "C" {
    /// blocking whole-image first-hit features: albedo, normal, depth and hit count per pixel (the render's first bounce)
    pub fn rtmi_render_features(
        scene: *mut RtmiScene,
        cam: *const RtmiCamera,
        params: *const RtmiRenderParams,
        out_albedo: *mut f32,
        out_normal: *mut f32,
        out_depth: *mut f32,
        out_hits: *mut u32,
        out_path_sig: *mut u64,
        stats: *mut RtmiStats,
    ) -> c_int;
}

// ---- include/rtmi_denoise.h: the a-trous denoiser guided by first-hit features --------------------------------------------

#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiDenoiseParams {
    pub iterations: u32,
    pub normal_power: u32,
    pub sigma_l: f32,
    pub sigma_z: f32,
    pub eps_l: f32,
    pub eps_z: f32,
    pub albedo_min: f32,
    pub flags: u32,
}

extern "C" {
    /// blocking a-trous denoise of host planes (colour, albedo, normal, depth, optional standard error)
    pub fn rtmi_denoise(
        device: c_int,
        nx: u32,
        ny: u32,
        p: *const RtmiDenoiseParams,
        linear: *const f32,
        albedo: *const f32,
        normal: *const f32,
        depth: *const f32,
        stderr_rgb: *const f32,
        out_linear: *mut f32,
        out_rgb8: *mut u8,
    ) -> c_int;
    /// the filter's rtmi_expf on the device
    pub fn rtmi_probe_expf(device: c_int, x: *const f32, out: *mut f32, n: u32) -> c_int;
}

// ---- include/rtmi_nee.h: next-event estimation with MIS toward the scene's area lights ---------------------------------

#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiLight {
    pub item: i32,
    pub prim: i32,
    pub kind: i32,
    pub material: i32,
    pub area: f64,
    pub weight: f64,
    pub select_p: f64,
    pub cdf: f64,
}

extern "C" {
    /// the light table of a flat description (host code, no device): at most `cap` lights, the full count in `count`
    pub fn rtmi_lights_from_desc(desc: *const RtmiSceneDesc, out: *mut RtmiLight, cap: u32, count: *mut u32) -> c_int;
    /// derives the light table of `desc` (the handle's own description) and uploads it
    pub fn rtmi_scene_attach_lights(scene: *mut RtmiScene, desc: *const RtmiSceneDesc) -> c_int;
    /// blocking whole-image NEE render: the image, its standard errors and rtmi_render's path signature
    pub fn rtmi_render_nee(
        scene: *mut RtmiScene,
        cam: *const RtmiCamera,
        params: *const RtmiRenderParams,
        out_linear: *mut f32,
        out_rgb8: *mut u8,
        out_stderr: *mut f32,
        out_path_sig: *mut u64,
        stats: *mut RtmiStats,
    ) -> c_int;
}

// ---- include/rtmi_env.h: image-based environment lighting with importance-sampled NEE -------------------------------

pub const RTMI_ENV_MAX_SIDE: u32 = 16384;
pub const RTMI_ENV_MAX_TEXELS: u32 = 1 << 25;
pub const RTMI_ENV_PROBE_LOOKUP: c_int = 0;
pub const RTMI_ENV_PROBE_SAMPLE: c_int = 1;

/// an environment map: height * width * 3 floats, row-major, row 0 the top row (+y), finite and >= 0
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiEnvMap {
    pub width: u32,
    pub height: u32,
    pub rgb: *const f32,
}

/// the options of rtmi_render_env
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiEnvRender {
    pub nee: u32,
    pub env_select_p: f32,
}

extern "C" {
    /// the map's sampling tables (host code, no device); any output may be null
    pub fn rtmi_env_tables(
        map: *const RtmiEnvMap,
        row_cdf: *mut f32,
        row_p: *mut f32,
        col_cdf: *mut f32,
        col_p: *mut f32,
        total: *mut f64,
    ) -> c_int;
    /// uploads a map and its tables to the handle (null detaches)
    pub fn rtmi_scene_attach_env(scene: *mut RtmiScene, map: *const RtmiEnvMap) -> c_int;
    /// blocking whole-image render with the attached map: the image, its standard errors and rtmi_render's path signature
    pub fn rtmi_render_env(
        scene: *mut RtmiScene,
        cam: *const RtmiCamera,
        params: *const RtmiRenderParams,
        opts: *const RtmiEnvRender,
        out_linear: *mut f32,
        out_rgb8: *mut u8,
        out_stderr: *mut f32,
        out_path_sig: *mut u64,
        stats: *mut RtmiStats,
    ) -> c_int;
    /// the device's lookup or light sample on the attached map (RTMI_ENV_PROBE_*)
    pub fn rtmi_probe_env(scene: *mut RtmiScene, op: c_int, input: *const f32, out: *mut f32, n: u32) -> c_int;
}

// ---- include/rtmi_light_tree.h: position-aware light selection for next-event estimation ------------------------------

pub const RTMI_LIGHT_TREE_LEAF: u32 = 0x8000_0000;
pub const RTMI_LIGHT_TREE_PROBE_PICK: c_int = 0;
pub const RTMI_LIGHT_TREE_PROBE_PMF: c_int = 1;

#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiLightNode {
    pub c: [f32; 3],
    pub r2: f32,
    pub power: f32,
    pub link: u32,
    pub pad: [u32; 2],
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiLightPath {
    pub trail: u32,
    pub depth: u32,
}

extern "C" {
    /// the tree over the light table of a flat description (host code, no device): at most `cap` nodes and cap / 2 paths,
    /// the full node count (2 * lights) in `n_nodes`
    pub fn rtmi_light_tree_from_desc(
        desc: *const RtmiSceneDesc,
        nodes: *mut RtmiLightNode,
        cap: u32,
        n_nodes: *mut u32,
        paths: *mut RtmiLightPath,
    ) -> c_int;
    /// the device's walk on the host: the light of each point for each uniform, and its probability
    pub fn rtmi_light_tree_pick(
        nodes: *const RtmiLightNode,
        n_nodes: u32,
        points: *const f32,
        us: *const f32,
        n: u32,
        out_light: *mut u32,
        out_p: *mut f32,
    ) -> c_int;
    /// ... and the reverse walk: the probability of a given light from a given point
    pub fn rtmi_light_tree_pmf(
        nodes: *const RtmiLightNode,
        n_nodes: u32,
        paths: *const RtmiLightPath,
        points: *const f32,
        lights: *const u32,
        n: u32,
        out_p: *mut f32,
    ) -> c_int;
    /// attaches the light table when it is missing, builds the tree and uploads it
    pub fn rtmi_scene_attach_light_tree(scene: *mut RtmiScene, desc: *const RtmiSceneDesc) -> c_int;
    /// the device's own walk on a batch (RTMI_LIGHT_TREE_PROBE_*)
    pub fn rtmi_probe_light_tree(
        scene: *mut RtmiScene,
        op: c_int,
        points: *const f32,
        aux: *const c_void,
        n: u32,
        out_light: *mut u32,
        out_p: *mut f32,
    ) -> c_int;
}

// ---- include/rtmi_adaptive_nee.h: adaptive sampling with next-event estimation or environment lighting ---------------
extern "C" {
    /// blocking whole-image adaptive render with rtmi_render_nee's estimator: per-tile sample counts up to params.ns,
    /// per-pixel standard errors
    pub fn rtmi_render_adaptive_nee(
        scene: *mut RtmiScene,
        cam: *const RtmiCamera,
        params: *const RtmiRenderParams,
        adaptive: *const RtmiAdaptive,
        out_linear: *mut f32,
        out_rgb8: *mut u8,
        out_stderr: *mut f32,
        out_spp: *mut u32,
        stats: *mut RtmiStats,
    ) -> c_int;
    /// the same with rtmi_render_env's estimator and options on the attached map
    pub fn rtmi_render_adaptive_env(
        scene: *mut RtmiScene,
        cam: *const RtmiCamera,
        params: *const RtmiRenderParams,
        opts: *const RtmiEnvRender,
        adaptive: *const RtmiAdaptive,
        out_linear: *mut f32,
        out_rgb8: *mut u8,
        out_stderr: *mut f32,
        out_spp: *mut u32,
        stats: *mut RtmiStats,
    ) -> c_int;
}

// ---- include/rtmi_roulette.h: Russian-roulette path termination with a per-pixel bounce count --------------------------
pub const RTMI_ROULETTE_PLAIN: u32 = 0;
pub const RTMI_ROULETTE_NEE: u32 = 1;
pub const RTMI_ROULETTE_ENV: u32 = 2;
pub const RTMI_ROULETTE_ENV_NEE: u32 = 3;

/// the options of the roulette entries: whose estimator, the first depth tested, the floor of the survival probability
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiRoulette {
    pub estimator: u32,
    pub min_depth: u32,
    pub q_min: f32,
    pub env_select_p: f32,
}

extern "C" {
    /// blocking whole-image render with roulette; out_bounces: ny*nx, the scatters of the pixel's paths, summed
    pub fn rtmi_render_roulette(
        scene: *mut RtmiScene,
        cam: *const RtmiCamera,
        params: *const RtmiRenderParams,
        opts: *const RtmiRoulette,
        out_linear: *mut f32,
        out_rgb8: *mut u8,
        out_stderr: *mut f32,
        out_bounces: *mut u32,
        stats: *mut RtmiStats,
    ) -> c_int;
    /// the same under the noise target of rtmi_render_adaptive
    pub fn rtmi_render_adaptive_roulette(
        scene: *mut RtmiScene,
        cam: *const RtmiCamera,
        params: *const RtmiRenderParams,
        opts: *const RtmiRoulette,
        adaptive: *const RtmiAdaptive,
        out_linear: *mut f32,
        out_rgb8: *mut u8,
        out_stderr: *mut f32,
        out_spp: *mut u32,
        out_bounces: *mut u32,
        stats: *mut RtmiStats,
    ) -> c_int;
}

// ---- include/rtmi_query.h: ray queries (closest hit and occlusion for batches of rays) ----

/// rtmi_ray: one query ray (32 bytes); t_max = +inf or >= FLT_MAX means the render's t_max
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiRay {
    pub o: [f32; 3],
    pub t_min: f32,
    pub d: [f32; 3],
    pub t_max: f32,
}

/// rtmi_hit: the record of a closest hit (48 bytes); a miss has t = +inf, item = prim = material = -1, the rest 0
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiHit {
    pub t: f32,
    pub u: f32,
    pub v: f32,
    pub p: [f32; 3],
    pub n: [f32; 3],
    pub item: i32,
    pub prim: i32,
    pub material: i32,
}

/// rtmi_query_params: one call's batch (24 bytes); ray i draws from the Philox stream keyed seed + first_ray + i
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiQueryParams {
    pub n: u32,
    pub flags: u32,
    pub seed: u64,
    pub first_ray: u64,
}

extern "C" {
    /// optional: the places of the FlipNormals among the wrappers (bit g of an entry: between transforms g - 1 and g of the
    /// chain, outermost first), so that the zeros of rtmi_trace's normals carry the reference's signs; NULL arrays detach
    pub fn rtmi_scene_attach_flips(
        scene: *mut RtmiScene,
        prim_gaps: *const u32,
        n_prims: u32,
        item_gaps: *const u32,
        n_items: u32,
    ) -> c_int;
    /// blocking, host pointers; time: n floats or NULL (time 0); kernel_ms: optional
    pub fn rtmi_trace(
        scene: *mut RtmiScene,
        params: *const RtmiQueryParams,
        rays: *const RtmiRay,
        time: *const f32,
        hits_out: *mut RtmiHit,
        kernel_ms: *mut f64,
    ) -> c_int;
    /// occluded_out[i] = 1 iff rtmi_trace's hit i is a hit: the same predicate with the same draws
    pub fn rtmi_occluded(
        scene: *mut RtmiScene,
        params: *const RtmiQueryParams,
        rays: *const RtmiRay,
        time: *const f32,
        occluded_out: *mut u8,
        kernel_ms: *mut f64,
    ) -> c_int;
    /// asynchronous, device pointers, enqueued on `stream` (a hipStream_t); writes exactly n records
    pub fn rtmi_trace_device(
        scene: *mut RtmiScene,
        params: *const RtmiQueryParams,
        d_rays: *const c_void,
        d_time: *const c_void,
        d_hits: *mut c_void,
        stream: *mut c_void,
    ) -> c_int;
    pub fn rtmi_occluded_device(
        scene: *mut RtmiScene,
        params: *const RtmiQueryParams,
        d_rays: *const c_void,
        d_time: *const c_void,
        d_occluded: *mut c_void,
        stream: *mut c_void,
    ) -> c_int;
}

// ---- include/rtmi_radiance.h: radiance queries -------------------------------------------------------------------------

/// rtmi_radiance_params: one call's batch, estimator and Philox indices (56 bytes); path (i, s) is the render's path of
/// pixel index first_ray + i, sample first_sample + s under `seed`, its stream 0 read from word stream_skip on
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiRadianceParams {
    pub n: u32,
    pub spp: u32,
    pub estimator: u32,
    pub flags: u32,
    pub max_depth: u32,
    pub t_min: f32,
    pub seed: u64,
    pub first_ray: u64,
    pub first_sample: u32,
    pub stream_skip: u32,
    pub env_select_p: f32,
}

extern "C" {
    /// blocking, host pointers; time: n floats or NULL (time 0); each output optional, not all NULL; kernel_ms: optional
    pub fn rtmi_radiance(
        scene: *mut RtmiScene,
        params: *const RtmiRadianceParams,
        rays: *const RtmiRay,
        time: *const f32,
        out_mean: *mut f32,
        out_stderr: *mut f32,
        out_samples: *mut f32,
        kernel_ms: *mut f64,
    ) -> c_int;
    /// asynchronous, device pointers, enqueued on `stream` (a hipStream_t); d_samples (n * spp * 12 bytes) is required
    pub fn rtmi_radiance_device(
        scene: *mut RtmiScene,
        params: *const RtmiRadianceParams,
        d_rays: *const c_void,
        d_time: *const c_void,
        d_mean: *mut c_void,
        d_stderr: *mut c_void,
        d_samples: *mut c_void,
        stream: *mut c_void,
    ) -> c_int;
}

// ---- include/rtmi_gather.h: hemisphere gathers -------------------------------------------------------------------------

pub const RTMI_GATHER_COSINE: u32 = 0;
pub const RTMI_GATHER_SPHERE: u32 = 1;

/// rtmi_gather_params: one call's points, mode, estimator and Philox indices (64 bytes, seed at offset 32); direction s of
/// point i is drawn from the counter (0, first_sample + s, first_point + i, 5) under `seed`, and its path is the radiance
/// query's of ray index first_point + i, sample first_sample + s, stream_skip 0
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiGatherParams {
    pub n: u32,
    pub spp: u32,
    pub mode: u32,
    pub estimator: u32,
    pub flags: u32,
    pub max_depth: u32,
    pub t_min: f32,
    pub seed: u64,
    pub first_point: u64,
    pub first_sample: u32,
    pub slab_points: u32,
    pub env_select_p: f32,
}

extern "C" {
    /// blocking, host pointers; points n * 3 floats, normals n * 3 floats (COSINE) or NULL, time n floats or NULL;
    /// out_value, out_stderr n * 3 floats, out_sh n * 27 floats (SPHERE), each optional, not all NULL
    pub fn rtmi_gather(
        scene: *mut RtmiScene,
        params: *const RtmiGatherParams,
        points: *const f32,
        normals: *const f32,
        time: *const f32,
        out_value: *mut f32,
        out_stderr: *mut f32,
        out_sh: *mut f32,
        kernel_ms: *mut f64,
    ) -> c_int;
    /// asynchronous, device pointers, enqueued on `stream` (a hipStream_t); d_scratch holds at least 12 * spp bytes
    pub fn rtmi_gather_device(
        scene: *mut RtmiScene,
        params: *const RtmiGatherParams,
        d_points: *const c_void,
        d_normals: *const c_void,
        d_time: *const c_void,
        d_value: *mut c_void,
        d_stderr: *mut c_void,
        d_sh: *mut c_void,
        d_scratch: *mut c_void,
        scratch_bytes: u64,
        stream: *mut c_void,
    ) -> c_int;
    /// the directions of a call on the host: n * spp * 3 floats; initialises no device
    pub fn rtmi_gather_directions(
        params: *const RtmiGatherParams,
        normals: *const f32,
        n: u32,
        out_dirs: *mut f32,
    ) -> c_int;
}

// ---- include/rtmi_window.h: adaptive sampling per pixel with a neighbourhood stopping rule -----------------------------------

pub const RTMI_WINDOW_MAX_RADIUS: u32 = 16;

/// rtmi_window_opts: the steps, the estimator, the tolerances and the window radius of a windowed adaptive render (48 bytes,
/// abs_tol at offset 16, radius at offset 36)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiWindowOpts {
    pub min_spp: u32,
    pub step_spp: u32,
    pub estimator: u32,
    pub pass_spp: u32,
    pub abs_tol: f64,
    pub rel_tol: f64,
    pub env_select_p: f32,
    pub radius: u32,
    pub reserved: [u32; 2],
}

extern "C" {
    /// the bytes of the device form's scratch; pure host code, a multiple of 16
    pub fn rtmi_window_scratch_bytes(n_pixels: u64, pass_spp: u32, steps: u32) -> u64;
    /// 1 + ceil((ns - min_spp) / step_spp), 0 for bad arguments; pure host code
    pub fn rtmi_window_steps(ns: u32, min_spp: u32, step_spp: u32) -> u32;
    /// asynchronous, device pointers, every step enqueued on `stream` (a hipStream_t); the planes are each optional, not all
    /// NULL; d_counts 2 * steps words or NULL
    pub fn rtmi_render_window_device(
        scene: *mut RtmiScene,
        params: *const RtmiRenderParams,
        cam: *const RtmiCamera,
        opts: *const RtmiWindowOpts,
        d_linear: *mut c_void,
        d_rgb8: *mut c_void,
        d_stderr: *mut c_void,
        d_spp: *mut c_void,
        d_counts: *mut c_void,
        d_scratch: *mut c_void,
        scratch_bytes: u64,
        stream: *mut c_void,
    ) -> c_int;
    /// blocking, host planes, each optional, not all NULL; out_counts 2 * steps words or NULL
    pub fn rtmi_render_window(
        scene: *mut RtmiScene,
        cam: *const RtmiCamera,
        params: *const RtmiRenderParams,
        opts: *const RtmiWindowOpts,
        out_linear: *mut f32,
        out_rgb8: *mut u8,
        out_stderr: *mut f32,
        out_spp: *mut u32,
        out_counts: *mut u32,
        stats: *mut RtmiStats,
    ) -> c_int;
    /// the rule once on device planes of nx * ny bytes, enqueued on `stream`: d_active in and out, d_fail read only
    pub fn rtmi_window_spread_device(
        d_active: *mut c_void,
        d_fail: *const c_void,
        nx: u32,
        ny: u32,
        radius: u32,
        stream: *mut c_void,
    ) -> c_int;
    /// the same on host arrays, blocking (tests)
    pub fn rtmi_probe_window_spread(device: c_int, nx: u32, ny: u32, radius: u32, active: *mut u8, fail: *const u8) -> c_int;
}

// ---- include/rtmi_pixelwise.h: adaptive sampling per pixel, driven from the device -----------------------------------------

pub const RTMI_PIXELWISE_MAX_STEPS: u32 = 1024;

/// rtmi_pixelwise_opts: the steps, the estimator and the tolerances of a per-pixel adaptive render (48 bytes, abs_tol at
/// offset 16)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiPixelwiseOpts {
    pub min_spp: u32,
    pub step_spp: u32,
    pub estimator: u32,
    pub pass_spp: u32,
    pub abs_tol: f64,
    pub rel_tol: f64,
    pub env_select_p: f32,
    pub reserved: [u32; 3],
}

extern "C" {
    /// the bytes of the device form's scratch; pure host code, a multiple of 16
    pub fn rtmi_pixelwise_scratch_bytes(n_pixels: u64, pass_spp: u32, steps: u32) -> u64;
    /// 1 + ceil((ns - min_spp) / step_spp), 0 for bad arguments; pure host code
    pub fn rtmi_pixelwise_steps(ns: u32, min_spp: u32, step_spp: u32) -> u32;
    /// asynchronous, device pointers, every step enqueued on `stream` (a hipStream_t); the planes are each optional, not all
    /// NULL; d_counts 2 * steps words or NULL
    pub fn rtmi_render_pixelwise_device(
        scene: *mut RtmiScene,
        params: *const RtmiRenderParams,
        cam: *const RtmiCamera,
        opts: *const RtmiPixelwiseOpts,
        d_linear: *mut c_void,
        d_rgb8: *mut c_void,
        d_stderr: *mut c_void,
        d_spp: *mut c_void,
        d_counts: *mut c_void,
        d_scratch: *mut c_void,
        scratch_bytes: u64,
        stream: *mut c_void,
    ) -> c_int;
    /// blocking, host planes, each optional, not all NULL; out_counts 2 * steps words or NULL
    pub fn rtmi_render_pixelwise(
        scene: *mut RtmiScene,
        cam: *const RtmiCamera,
        params: *const RtmiRenderParams,
        opts: *const RtmiPixelwiseOpts,
        out_linear: *mut f32,
        out_rgb8: *mut u8,
        out_stderr: *mut f32,
        out_spp: *mut u32,
        out_counts: *mut u32,
        stats: *mut RtmiStats,
    ) -> c_int;
    /// the step kernel alone on host arrays, blocking (tests)
    pub fn rtmi_probe_pixelwise_step(
        device: c_int,
        n_pixels: u32,
        capacity: u32,
        list: *const u32,
        count: *const u32,
        samples: *const f32,
        state: *mut f64,
        n_done: u32,
        pass: u32,
        decide: u32,
        cap: u32,
        abs_tol: f64,
        rel_tol: f64,
        active: *mut u8,
        linear: *mut f32,
        rgb8: *mut u8,
        stderr_rgb: *mut f32,
        spp: *mut u32,
    ) -> c_int;
}

// ---- include/rtmi_temporal.h: temporal accumulation -------------------------------------------------------------------

pub const RTMI_TEMPORAL_NO_DEMODULATE: u32 = 1;

/// rtmi_temporal_params: the settings of a temporal history (32 bytes); defaults 32, 0, 0.05, 0.9, 1e-3, 0
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiTemporalParams {
    pub max_history: u32,
    pub alpha_min: f32,
    pub depth_tol: f32,
    pub normal_min: f32,
    pub albedo_min: f32,
    pub flags: u32,
    pub reserved: [u32; 2],
}

/// opaque device-resident history of one image size on one device (rtmi_temporal.h: rtmi_temporal)
#[repr(C)]
pub struct RtmiTemporal {
    _private: [u8; 0],
}

extern "C" {
    pub fn rtmi_temporal_create(
        device: c_int,
        nx: u32,
        ny: u32,
        params: *const RtmiTemporalParams,
        out: *mut *mut RtmiTemporal,
    ) -> c_int;
    /// blocking, host pointers; linear, albedo, normal ny * nx * 3 floats, depth ny * nx floats, stderr_rgb ny * nx * 3
    /// floats or NULL; out_linear, out_stderr ny * nx * 3 floats, out_history ny * nx, out_motion ny * nx * 2, each optional
    pub fn rtmi_temporal_push(
        h: *mut RtmiTemporal,
        cam: *const RtmiCamera,
        linear: *const f32,
        albedo: *const f32,
        normal: *const f32,
        depth: *const f32,
        stderr_rgb: *const f32,
        out_linear: *mut f32,
        out_stderr: *mut f32,
        out_history: *mut f32,
        out_motion: *mut f32,
    ) -> c_int;
    /// forgets the previous frame, keeps the allocation
    pub fn rtmi_temporal_reset(h: *mut RtmiTemporal) -> c_int;
    pub fn rtmi_temporal_destroy(h: *mut RtmiTemporal);
}

// ---- include/rtmi_sparse.h: sparse renders (select, trace and patch chosen pixels) --------------------------------------

/// rtmi_sparse_params: a list's length (host forms) or capacity (device forms), the samples per entry and the estimator
/// (32 bytes); sample s of an entry is the full render's sample first_sample + s of that pixel
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiSparseParams {
    pub n: u32,
    pub ns: u32,
    pub first_sample: u32,
    pub estimator: u32,
    pub env_select_p: f32,
    pub reserved: [u32; 3],
}

extern "C" {
    /// the bytes of scratch that serve every entry below; pure host code
    pub fn rtmi_sparse_scratch_bytes(n_pixels: u64, capacity: u32, ns: u32) -> u64;
    /// asynchronous, device pointers: the ascending list of the pixels whose byte b has b < 32 and bit b of accept_mask set;
    /// d_count receives {written, selected}
    pub fn rtmi_sparse_select_device(
        device: c_int,
        n: u32,
        d_bytes: *const c_void,
        accept_mask: u32,
        capacity: u32,
        d_list: *mut c_void,
        d_count: *mut c_void,
        d_scratch: *mut c_void,
        stream: *mut c_void,
    ) -> c_int;
    /// blocking, host pointers; pixels: sp.n indices below nx * ny; each output optional, not all NULL
    pub fn rtmi_sparse_render(
        scene: *mut RtmiScene,
        params: *const RtmiRenderParams,
        cam: *const RtmiCamera,
        sp: *const RtmiSparseParams,
        pixels: *const u32,
        out_mean: *mut f32,
        out_stderr: *mut f32,
        out_samples: *mut f32,
        kernel_ms: *mut f64,
    ) -> c_int;
    /// asynchronous, device pointers; the entries are min(d_count[0], sp.n), read by the kernels (d_count NULL: sp.n);
    /// d_samples (sp.n * ns * 12 bytes) is required
    pub fn rtmi_sparse_render_device(
        scene: *mut RtmiScene,
        params: *const RtmiRenderParams,
        cam: *const RtmiCamera,
        sp: *const RtmiSparseParams,
        d_pixels: *const c_void,
        d_count: *const c_void,
        d_mean: *mut c_void,
        d_stderr: *mut c_void,
        d_samples: *mut c_void,
        d_scratch: *mut c_void,
        stream: *mut c_void,
    ) -> c_int;
    /// asynchronous, device pointers: the records written to the planes at their pixels; each plane optional
    pub fn rtmi_sparse_patch_device(
        device: c_int,
        n_pixels: u32,
        d_list: *const c_void,
        d_count: *const c_void,
        capacity: u32,
        d_mean: *const c_void,
        d_linear: *mut c_void,
        d_rgb8: *mut c_void,
        d_bytes: *mut c_void,
        mark: u32,
        stream: *mut c_void,
    ) -> c_int;
    /// select -> sparse render -> patch enqueued in one call; sp.n is the budget of pixels
    pub fn rtmi_sparse_refine_device(
        scene: *mut RtmiScene,
        params: *const RtmiRenderParams,
        cam: *const RtmiCamera,
        sp: *const RtmiSparseParams,
        accept_mask: u32,
        mark: u32,
        d_bytes: *mut c_void,
        d_linear: *mut c_void,
        d_rgb8: *mut c_void,
        d_stderr: *mut c_void,
        d_scratch: *mut c_void,
        scratch_bytes: u64,
        d_count_out: *mut c_void,
        stream: *mut c_void,
    ) -> c_int;
    /// the blocking host-plane form; counts receives {patched, selected}
    pub fn rtmi_sparse_refine(
        scene: *mut RtmiScene,
        params: *const RtmiRenderParams,
        cam: *const RtmiCamera,
        sp: *const RtmiSparseParams,
        accept_mask: u32,
        mark: u32,
        bytes: *mut u8,
        linear: *mut f32,
        rgb8: *mut u8,
        stderr_rgb: *mut f32,
        counts: *mut u32,
    ) -> c_int;
}

// ---- include/rtmi_upscale.h: guided upscaling of a low-resolution frame ------------------------------------------------

pub const RTMI_UPSCALE_BACKGROUND: u8 = 0;
pub const RTMI_UPSCALE_GUIDED: u8 = 1;
pub const RTMI_UPSCALE_NEAREST: u8 = 2;
pub const RTMI_UPSCALE_MISMATCH: u8 = 3;

/// rtmi_upscale_params: the reconstruction's edge-stopping settings (32 bytes); defaults 32, 0.05, 1e-3, 1e-3, 1e-3, 0
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiUpscaleParams {
    pub normal_power: u32,
    pub sigma_z: f32,
    pub eps_z: f32,
    pub albedo_min: f32,
    pub w_min: f32,
    pub flags: u32,
    pub reserved: [u32; 2],
}

/// rtmi_upscale_in: the low-resolution planes (ly * lx pixels) and the full-resolution guide (ny * nx pixels) (64 bytes)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiUpscaleIn {
    pub linear_lo: *const f32,
    pub albedo_lo: *const f32,
    pub normal_lo: *const f32,
    pub depth_lo: *const f32,
    pub albedo: *const f32,
    pub normal: *const f32,
    pub depth: *const f32,
    pub reserved: *const c_void,
}

/// rtmi_upscale_out: the outputs, each optional, not all NULL (32 bytes)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiUpscaleOut {
    pub linear: *mut f32,
    pub rgb8: *mut u8,
    pub cls: *mut u8,
    pub reserved: *mut c_void,
}

/// rtmi_upscaler_opts: the low frame's options (RtmiFrameOpts, declared with rtmi_frame.h below), the reconstruction's and
/// the low size (160 bytes); guide_ns defaults to 4
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiUpscalerOpts {
    pub low: RtmiFrameOpts,
    pub up: RtmiUpscaleParams,
    pub lx: u32,
    pub ly: u32,
    pub guide_ns: u32,
    pub reserved: [u32; 5],
}

/// rtmi_upscaler_out: the full-resolution planes and the low frame's (RtmiFrameOut); a NULL plane is not copied (144 bytes)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiUpscalerOut {
    pub linear: *mut f32,
    pub rgb8: *mut u8,
    pub cls: *mut u8,
    pub albedo: *mut f32,
    pub normal: *mut f32,
    pub depth: *mut f32,
    pub low: RtmiFrameOut,
}

/// opaque upscaler handle
#[repr(C)]
pub struct RtmiUpscaler {
    _private: [u8; 0],
}

extern "C" {
    /// blocking, host pointers; 1 <= lx <= nx <= 32768, 1 <= ly <= ny <= 32768
    pub fn rtmi_upscale(
        device: c_int,
        lx: u32,
        ly: u32,
        nx: u32,
        ny: u32,
        params: *const RtmiUpscaleParams,
        input: *const RtmiUpscaleIn,
        out: *const RtmiUpscaleOut,
    ) -> c_int;
    /// asynchronous on `stream` (a hipStream_t), device pointers; float planes 16-byte aligned, rgb8 and cls 4
    pub fn rtmi_upscale_device(
        device: c_int,
        lx: u32,
        ly: u32,
        nx: u32,
        ny: u32,
        params: *const RtmiUpscaleParams,
        d_in: *const RtmiUpscaleIn,
        d_out: *const RtmiUpscaleOut,
        stream: *mut c_void,
    ) -> c_int;
    /// params fixes the full size and what the low frame reads from it; its ns and seed are not read
    pub fn rtmi_upscaler_create(
        scene: *mut RtmiScene,
        params: *const RtmiRenderParams,
        opts: *const RtmiUpscalerOpts,
        out: *mut *mut RtmiUpscaler,
    ) -> c_int;
    /// blocking; renders the low frame and the full-resolution features, reconstructs, copies the planes asked for to the host
    pub fn rtmi_upscaler_render(
        h: *mut RtmiUpscaler,
        cam: *const RtmiCamera,
        ns: u32,
        seed: u64,
        out: *const RtmiUpscalerOut,
        stats: *mut RtmiStats,
    ) -> c_int;
    /// the same with device pointers in `out`; blocking too
    pub fn rtmi_upscaler_render_device(
        h: *mut RtmiUpscaler,
        cam: *const RtmiCamera,
        ns: u32,
        seed: u64,
        out: *const RtmiUpscalerOut,
        stats: *mut RtmiStats,
    ) -> c_int;
    /// forgets the frames rendered so far, keeps the allocation
    pub fn rtmi_upscaler_reset(h: *mut RtmiUpscaler) -> c_int;
    pub fn rtmi_upscaler_destroy(h: *mut RtmiUpscaler);
}

// ---- include/rtmi_tonemap.h: tone mapping with histogram auto-exposure -------------------------------------------------

pub const RTMI_TONEMAP_CLAMP: u32 = 0;
pub const RTMI_TONEMAP_REINHARD: u32 = 1;
pub const RTMI_TONEMAP_ACES: u32 = 2;
pub const RTMI_TONEMAP_GAMMA2: u32 = 0;
pub const RTMI_TONEMAP_SRGB: u32 = 1;
pub const RTMI_TONEMAP_MANUAL: u32 = 0;
pub const RTMI_TONEMAP_AUTO: u32 = 1;

/// rtmi_tonemap_params: the operator, the transfer function and the metering (64 bytes); defaults ACES, SRGB, AUTO, 0, 0,
/// +inf, 0.18, -12, 12, 0.10, 0.95, 3, 1, log2_min, log2_max, 0
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiTonemapParams {
    pub op: u32,
    pub oetf: u32,
    pub exposure: u32,
    pub flags: u32,
    pub ev: f32,
    pub white: f32,
    pub key: f32,
    pub log2_min: f32,
    pub log2_max: f32,
    pub p_low: f32,
    pub p_high: f32,
    pub speed_up: f32,
    pub speed_down: f32,
    pub adapt_min: f32,
    pub adapt_max: f32,
    pub reserved: u32,
}

/// rtmi_tonemap_state: what one apply metered and applied (32 bytes)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiTonemapState {
    pub exposure: f32,
    pub adapted_log2: f32,
    pub metered_log2: f32,
    pub counted: u32,
    pub kept: u32,
    pub applies: u32,
    pub reserved: [u32; 2],
}

/// opaque tone mapper of one image size on one device (rtmi_tonemap.h: rtmi_tonemap)
#[repr(C)]
pub struct RtmiTonemap {
    _private: [u8; 0],
}

extern "C" {
    pub fn rtmi_tonemap_create(
        device: c_int,
        nx: u32,
        ny: u32,
        params: *const RtmiTonemapParams,
        out: *mut *mut RtmiTonemap,
    ) -> c_int;
    /// blocking, host pointers; linear ny * nx * 3 floats; out_rgb8 ny * nx * 3 bytes, out_display ny * nx * 3 floats and
    /// out_state each optional, not all NULL
    pub fn rtmi_tonemap_apply(
        h: *mut RtmiTonemap,
        linear: *const f32,
        dt: f32,
        out_rgb8: *mut u8,
        out_display: *mut f32,
        out_state: *mut RtmiTonemapState,
    ) -> c_int;
    /// asynchronous on `stream` (a hipStream_t), device pointers; d_linear and d_display 16-byte aligned, d_rgb8 and d_state 4
    pub fn rtmi_tonemap_apply_device(
        h: *mut RtmiTonemap,
        d_linear: *const c_void,
        dt: f32,
        d_rgb8: *mut c_void,
        d_display: *mut c_void,
        d_state: *mut c_void,
        stream: *mut c_void,
    ) -> c_int;
    /// the next apply is a first apply
    pub fn rtmi_tonemap_reset(h: *mut RtmiTonemap) -> c_int;
    pub fn rtmi_tonemap_destroy(h: *mut RtmiTonemap);
    /// the metering kernel alone on host data: out_bins = 256 counts
    pub fn rtmi_probe_tonemap_histogram(
        device: c_int,
        nx: u32,
        ny: u32,
        params: *const RtmiTonemapParams,
        linear: *const f32,
        out_bins: *mut u32,
    ) -> c_int;
}

// ---- include/rtmi_frame.h: the device-resident frame pipeline ---------------------------------------------------------

pub const RTMI_FRAME_NO_TEMPORAL: u32 = 1;
pub const RTMI_FRAME_NO_FILTER: u32 = 2;

/// rtmi_frame_opts: the estimator (RTMI_ROULETTE_* numbering) and the embedded temporal and filter settings (96 bytes)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiFrameOpts {
    pub estimator: u32,
    pub env_select_p: f32,
    pub temporal: RtmiTemporalParams,
    pub denoise: RtmiDenoiseParams,
    pub flags: u32,
    pub reserved: [u32; 5],
}

/// rtmi_frame_out: the planes of a frame, host pointers (rtmi_frame_render) or device pointers
/// (rtmi_frame_render_device); a NULL plane is not copied (96 bytes)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtmiFrameOut {
    pub linear: *mut f32,
    pub rgb8: *mut u8,
    pub noisy_linear: *mut f32,
    pub noisy_stderr: *mut f32,
    pub albedo: *mut f32,
    pub normal: *mut f32,
    pub depth: *mut f32,
    pub hits: *mut u32,
    pub accum_linear: *mut f32,
    pub accum_stderr: *mut f32,
    pub history: *mut f32,
    pub motion: *mut f32,
}

/// opaque frame handle
#[repr(C)]
pub struct RtmiFrame {
    _private: [u8; 0],
}

extern "C" {
    /// params fixes nx, ny, max_depth, t_min and flags; its ns and seed are not read
    pub fn rtmi_frame_create(
        scene: *mut RtmiScene,
        params: *const RtmiRenderParams,
        opts: *const RtmiFrameOpts,
        out: *mut *mut RtmiFrame,
    ) -> c_int;
    /// blocking; renders, accumulates and filters one frame and copies the planes asked for to the host
    pub fn rtmi_frame_render(
        frame: *mut RtmiFrame,
        cam: *const RtmiCamera,
        ns: u32,
        seed: u64,
        out: *const RtmiFrameOut,
        stats: *mut RtmiStats,
    ) -> c_int;
    /// the same with device pointers in `out`; blocking too
    pub fn rtmi_frame_render_device(
        frame: *mut RtmiFrame,
        cam: *const RtmiCamera,
        ns: u32,
        seed: u64,
        out: *const RtmiFrameOut,
        stats: *mut RtmiStats,
    ) -> c_int;
    /// forgets the frames rendered so far, keeps the allocation
    pub fn rtmi_frame_reset(frame: *mut RtmiFrame) -> c_int;
    pub fn rtmi_frame_destroy(frame: *mut RtmiFrame);
    /// the un-tiling kernel on the caller's host data, for tests
    pub fn rtmi_probe_frame_untile(
        device: c_int,
        nx: u32,
        ny: u32,
        tiled: *const RtmiTexel,
        tiled_stderr: *const f32,
        out_linear: *mut f32,
        out_stderr: *mut f32,
        poisoned: *mut u32,
    ) -> c_int;
}

// ---- include/rtmi_batch_coop.h: the batch modes on the wave-cooperative kernel ----------------------------------------

/// RTMI_FLAG_BATCH_COOP: a flag of rtmi_radiance, rtmi_gather, rtmi_sparse_render, rtmi_sparse_refine, rtmi_render_pixelwise
/// and rtmi_render_window (and their _device forms): the paths trace on the wave-cooperative kernel, same bits
pub const FLAG_BATCH_COOP: u32 = 2097152;

// ---- include/rtmi_update.h: edits of a resident scene (move primitives, refit the trees on the device) -----------------
// (the RTMI_SCENE_WORDS_* selectors of rtmu_probe_scene_words are 0..8 in the header's order)

extern "C" {
    /// mask[n_items]: 1 = a BVH item rtmu_scene_update_prims can refit; host code
    pub fn rtmu_refittable(desc: *const RtmiSceneDesc, mask: *mut u8) -> c_int;
    /// the refit of the items that own a primitive of [first, first + count), evaluated on the host into the caller's arrays
    pub fn rtmu_refit_desc(
        desc: *const RtmiSceneDesc,
        first: u32,
        count: u32,
        items: *mut RtmiItem,
        nodes: *mut RtmiBvhNode,
        alt_nodes: *mut RtmiBvh4Node,
        prim_gate: *mut f32,
    ) -> c_int;
    /// builds the handle's update tables ahead of its first update (which otherwise waits for the handle and allocates)
    pub fn rtmu_scene_update_prepare(scene: *mut RtmiScene) -> c_int;
    /// blocking; a, b: count * 4 floats each, b may be NULL
    pub fn rtmu_scene_update_prims(scene: *mut RtmiScene, first: u32, count: u32, a: *const f32, b: *const f32) -> c_int;
    /// the same from device memory, asynchronous on `stream`
    pub fn rtmu_scene_update_prims_device(
        scene: *mut RtmiScene,
        first: u32,
        count: u32,
        d_a: *const c_void,
        d_b: *const c_void,
        stream: *mut c_void,
    ) -> c_int;
    /// blocking; replaces transform records of item chains (and of list primitives' chains), kinds kept
    pub fn rtmu_scene_update_xforms(scene: *mut RtmiScene, first: u32, count: u32, recs: *const RtmiXform) -> c_int;
    /// test hook: one of the handle's device arrays copied to the host
    pub fn rtmu_probe_scene_words(scene: *mut RtmiScene, which: c_int, out: *mut c_void, cap: usize, need: *mut usize) -> c_int;
}

// ---- include/rtmi_relight.h: the light table and the light tree follow a scene update on the device -------------------
// (the RTML_WORDS_* selectors of rtml_probe_light_words are 0..3 in the header's order)

extern "C" {
    /// on != 0: updates that move an emitter recompute the attached table and refit the tree instead of detaching them
    pub fn rtml_scene_follow_lights(scene: *mut RtmiScene, on: c_int) -> c_int;
    /// the same rules on the host: lights[n_lights] and the tree's nodes (32 B each, or NULL with n_nodes = 0) are rewritten
    pub fn rtml_relight_desc(
        desc: *const RtmiSceneDesc,
        lights: *mut RtmiLight,
        n_lights: u32,
        nodes: *mut c_void,
        n_nodes: u32,
    ) -> c_int;
    /// test hook: one of the handle's light arrays copied to the host
    pub fn rtml_probe_light_words(scene: *mut RtmiScene, which: c_int, out: *mut c_void, cap: usize, need: *mut usize) -> c_int;
}
