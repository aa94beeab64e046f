// rtmi_host.hpp — what the host units of librtmi.so share: the scene handle, the call helpers of the
// render entry points and the estimator layer of the whole-image modes.  Hidden, not installed.  The helpers declared here
// are defined in rtmi_device.hip, which still holds these layers, and called by rtmi_multi.hip, by the entry points of
// rtmi_session.hip and by the batch modes in rtmi_batch.hip; none of them launches a kernel itself: each goes
// through a *_launch.hpp seam into the unit that instantiates the kernel.  A helper that one unit alone calls is static in
// that unit, not here.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "rtmi.h"
#include "rtmi_math.h"

#include "rtmi_bvh_coop.hpp"
#include "rtmi_shade.hpp"
#include "rtmi_f64_types.hpp"
#include "rtmi_adaptive.h"
#include "rtmi_roulette.h"
#include "rtmi_query.h"
#include "rtmi_light_coop.h"
#include "rtmi_render_launch.hpp"
#include "rtmi_adaptive_launch.hpp"
#include "rtmi_light_launch.hpp"
#include "rtmi_refit.hpp"
#include "rtmi_update_launch.hpp"
#include "rtmi_relight_launch.hpp"
#include "rtmi_hostkit.hpp"

#define HIP_TRY(expr) RTMI_HIP_TRY("", false, expr, #expr)
// sets the message of rtmi_last_error (rtmi_device.hip keeps it), returns `code`
static inline int fail(int code, const std::string &msg) { return rtmi_fail(code, msg.c_str()); }

// Every piece of device and pinned memory of the handle is an owner of rtmi_hostkit.hpp that knows its size; the members
// free themselves when rtmi_scene_destroy deletes the handle.
struct RTMI_HIDDEN rtmi_scene {
    int device = 0;
    DevScene dev{};
    DeviceList allocs;
    rtmi_scene_desc meta{}; // counts only (pointers nulled)
    DeviceBuf<double> partial; // f64 radiance sums [local tile][3][64], carried between passes
    DeviceBuf<Rad3> samples;   // per-sample radiance [local tile][pass samples][64], 12-B slots
    DeviceBuf<uint2> spill;    // global part of the cooperative traversal stacks [wavefront slot][spill_cap]
    DeviceBuf<unsigned int> status; // RTMI_STATUS_WORDS device words, see rtmi_types.hpp
    int slots = 0;                  // CUs x 16: resident wavefronts the render kernels are launched with
    bool has_alt = false;           // some BVH item carries an alternative tree
    bool all_alt = false;           // every BVH item does (and there is one): the workgroup-cooperative kernel can run
    bool all_sphere_media = true;   // every medium item is bounded by one static sphere (RTMI_ITEMFLAG_DEV_MEDIUM_SPHERE; also
                                    // true without media): with all_alt what the one-tree instantiation asks of a scene
    uint32_t last_inst = 0;         // RTMI_INST_* of the last plain render enqueued on this handle (rtmi_stats_instantiation)
    bool needs_insd = false;        // DEFERRED items, list scans, nested media: the INSTL = 2 instantiations (rtmi_kernels.hpp)
    bool has_deferred = false;      // media that were children of a BVHNode (RTMI_ITEMFLAG_DEFERRED): the asynchronous
                                    // state-machine kernel does not carry them, RTMI_FLAG_ASYNC then runs the per-lane kernel
    uint32_t last_kernel = 0;       // RTMI_KERNEL_* of the last render enqueued on this handle (rtmi_stats.kernel)
    int last_batch_kernel = -1;     // ... of the path kernel of the last batch call (rtmi_batch_coop.h); -1: none yet
    bool batch_blocking = false;    // the running batch call is a blocking one: it reads its own overflow word (batch_coop_check)
    // scratch of the blocking host API (grow-only, so a host that renders frame after frame allocates once)
    DeviceBuf<rtmi_texel> texels;
    DeviceBuf<unsigned long long> d_sig;
    DeviceBuf<uint32_t> rr_bounces;    // the bounce plane of the roulette entries (include/rtmi_roulette.h), tiled as d_sig
    PinnedBuf<rtmi_texel> h_texels;    // pinned host mirror of `texels` (hipHostMalloc: the D2H copy runs at link speed)
    PinnedBuf<rtmi_texel> h_partial;   // ... and of the partial images rtmi_partial_image fetches (RTMI_FLAG_PROGRESSIVE)
    // Thread model (rtmi.h): render calls on one handle serialise.  `mu` orders the host side (planning, scratch
    // (re)allocation, enqueue, and for the blocking calls the wait and the copy-out); `busy` chains the device side: a
    // render enqueued on ANY stream first waits for the previous render of this handle, whose kernels use the same
    // unit queue, status words and per-sample buffer.
    std::mutex mu;
    DeviceEvent busy;
    bool busy_recorded = false;
    DeviceStream stream;      // launches of the blocking API (non-blocking stream)
    DeviceStream copy_stream; // progress polls while a launch runs
    uint64_t units_total = 0; // work units of the last enqueued call (progress denominator)
    DeviceEvent ev[3];
    // f64 render mode (include/rtmi_f64.h): the attached double planes on the device, freed with the handle
    bool has_f64 = false;
    DevSceneF64 f64{};
    DeviceList f64_allocs;
    DeviceBuf<double> f64_samples; // the f64 mode's per-sample buffer (grow-only, at most RTMI_F64_MAX_BUFFER_BYTES)
    // adaptive sampling (include/rtmi_adaptive.h), grow-only, freed with the handle: sum | m | M2 per pixel and channel,
    // two active-tile lists and their count word, the standard errors and counts of the retired tiles
    DeviceBuf<double> ad_state;   // [tile][9][64]
    DeviceBuf<uint32_t> ad_lists; // [2][tiles] + count
    DeviceBuf<float> ad_stderr;   // [tile][64][3]
    DeviceBuf<uint32_t> ad_spp;   // [tile][64]
    PinnedBuf<uint32_t> h_ad_count; // pinned: the active count read back after every step
    // first-hit features (include/rtmi_features.h), grow-only, freed with the handle: the f64 sums carried between passes
    // and the four output planes
    DeviceBuf<double> ft_state; // [tile][8][64]
    DeviceBuf<float> ft_planes; // albedo [ny*nx*3] | normal [ny*nx*3] | depth [ny*nx] | hits [ny*nx] (uint32)
    // ray queries (include/rtmi_query.h), grow-only, freed with the handle: the device copies of a host-form batch
    DeviceBuf<float4> q_rays;   // [n][2]
    DeviceBuf<float> q_time;    // [n]
    DeviceBuf<float4> q_out;    // trace: [n][3] hit records; occluded: [n] bytes
    DeviceBuf<uint32_t> q_flip_gaps; // rtmi_scene_attach_flips: [n_prims] | [n_items], or empty
    // radiance queries (include/rtmi_radiance.h), grow-only, freed with the handle: the per-sample buffer and the two
    // per-ray outputs of a host-form batch (its rays go through q_rays and q_time); the chunk counter of the persistent
    // wavefronts is the word behind the status words
    DeviceBuf<Rad3> rad_samples; // [n][spp]
    DeviceBuf<float> rad_out;    // mean [n][3] | stderr [n][3]
    DeviceBuf<char> px_mem;      // per-pixel adaptive sampling, blocking form: scratch | linear | stderr | spp | rgb8
    // next-event estimation (include/rtmi_nee.h): the attached light table and per-primitive light index, freed with the
    // handle
    bool has_lights = false;
    DeviceBuf<NeeLight> nee_lights;    // [max(n, 1)]
    DeviceBuf<int32_t> nee_prim_light; // [max(n_prims, 1)]
    uint32_t nee_n = 0;
    // light tree (include/rtmi_light_tree.h): the attached nodes (64-B aligned pairs) and paths, freed with the handle
    bool has_light_tree = false;
    DeviceBuf<float4> lt_nodes; // [max(lt_n, 2)][2]
    DeviceBuf<uint2> lt_paths;  // [max(lt_n / 2, 1)]
    uint32_t lt_n = 0;          // slots: 2 * lights
    // environment lighting (include/rtmi_env.h): the attached map and its tables, freed with the handle
    bool has_env = false;
    DeviceBuf<float4> env_texels; // [h][w] {r, g, b, 0}
    DeviceBuf<float> env_tables;  // row_cdf [h] | row_p [h] | col_cdf [h][w] | col_p [h][w]
    uint32_t env_w = 0, env_h = 0;
    bool env_sampled = false;     // the map's total weight is > 0
    // scene updates (include/rtmi_update.h): the topology read back from the device on the first update — the plan of the
    // refit, per primitive its type, whether it emits and the MEDIUM item that carries a copy of it —, its device tables and
    // the scratch of the refit kernel, then the staging of the blocking form (grow-only); freed with the handle
    bool up_ready = false;
    RefitPlan up_plan;
    std::vector<uint8_t> up_type, up_emits;
    // ... and per transform record its kind, the item whose chain holds it (-1: a primitive's chain or none) and whether
    // rtmu_scene_update_xforms may replace it (UP_XF_*, rtmi_update.hip)
    std::vector<int32_t> up_xf_kind, up_xf_item, up_xf_slot; // slot: its place in that item's chain
    std::vector<uint8_t> up_xf_state;
    DeviceBuf<uint32_t> up_words;
    DeviceBuf<RefitJob> up_jobs;
    DeviceBuf<int32_t> up_medium_item; // [max(n_prims, 1)]
    DeviceBuf<float4> up_scratch;      // [max(n_nodes, 1)][2]
    uint32_t up_n_jobs = 0;
    DeviceBuf<float> up_stage;         // planes A | B of a blocking update on the device
    PinnedBuf<float> up_h_stage;       // ... and their pinned host copy
    // following lights (include/rtmi_relight.h): on, and the tables rtml_scene_follow_lights built from the attached table
    // and tree, which hold until another table or tree is attached — per primitive the light that lists it (-1: none) and
    // per light its plane and weight for the blocking update's check, then the kernel's tables; freed with the handle
    bool rl_on = false, rl_ready = false;
    std::vector<int32_t> rl_prim_light; // [n_prims]
    std::vector<int32_t> rl_plane;      // [nee_n]: NeeLight::plane
    std::vector<double> rl_weight_h;    // [nee_n]
    DeviceBuf<double> rl_weight;        // [max(nee_n, 1)]
    DeviceBuf<uint32_t> rl_words;       // the tree's slots by depth (RelightScene::words)
    DeviceBuf<double> rl_scratch;       // aw [nee_n] | box [lt_n][7]
    uint32_t rl_n_lvl = 0;              // 0: built without a tree
};

static inline uint32_t tiles_x_of(const rtmi_render_params *p) { return (p->nx + RTMI_TILE - 1) / RTMI_TILE; }
static inline uint32_t tiles_y_of(const rtmi_render_params *p) { return (p->ny + RTMI_TILE - 1) / RTMI_TILE; }
static inline uint32_t local_tiles_of(const rtmi_render_params *p, uint32_t rank) {
    const uint32_t T = tiles_x_of(p) * tiles_y_of(p);
    return rank < T ? (T - rank + p->tile_world - 1) / p->tile_world : 0;
}

// ---- host-side plumbing shared by the render entry points ------------------------------------------------------------
// records the end of a call's work on `st` on every return path after its first enqueue (thread model: `busy`)
struct BusyMark {
    rtmi_scene *s;
    hipStream_t st;
    ~BusyMark() { if (s && hipEventRecord(s->busy.e, st) == hipSuccess) s->busy_recorded = true; } // s = NULL: no call begun
};

// Grow-only device buffer of the handle: reallocated when a call needs more than it holds.  A render of this handle
// enqueued asynchronously (rtmi_render_device) may still use the old buffer: it is released after that render.
template <typename T>
static int grow(rtmi_scene *s, DeviceBuf<T> &buf, size_t want) {
    if (want <= buf.bytes) return RTMI_OK;
    if (buf.ptr) {
        if (s->busy_recorded) HIP_TRY(hipEventSynchronize(s->busy.e));
        HIP_TRY(buf.release());
    }
    HIP_TRY(buf.alloc(want));
    return RTMI_OK;
}

// what run_passes launched for a call, for rtmi_stats
struct PassCounts { uint32_t blocks = 0, chunks = 0; };

// an entry point's estimator: what it reads of the handle, and the entry's own words where the handle lacks it
struct Estimator {
    const char *name;       // the entry point, prefix of the attach refusals
    bool nee, env;          // reads the light table (rtmi_scene_attach_lights) / the map (rtmi_scene_attach_env)
    float env_select_p;     // rtmi_env_render's, read with the map only
    const char *null_scene; // the refusal of a NULL handle
    const char *no_lights;  // the refusal of a handle without the light table, after "name: "
    bool tree = false;      // reads the light tree (rtmi_scene_attach_light_tree; RTMI_FLAG_LIGHT_TREE)
};

// a blocking call's hold on the handle from begin_call to its return, and the kernel arguments of its estimator
struct RenderCall {
    std::unique_lock<std::mutex> lock;
    BusyMark busy{nullptr, nullptr};
    DevParams P;
    DevCamera C;
    DevLights L;
    DevEnv E;
    bool fast = false;
    // RTMI_FLAG_LIGHT_COOP (rtmi_light_coop.h), RTMI_FLAG_ROULETTE_COOP (rtmi_roulette_coop.h): the estimator runs on the
    // wave-cooperative kernel, with this pool form and this much dynamic LDS per block; wps: the waves per SIMD the call's
    // render kernel was compiled for
    bool coop = false, ext = false;
    size_t coop_lds = 0;
    uint32_t wps = 4u;
};

// the flags that the adaptive lighting entries, the roulette entries and the sessions accept alike
#define RTMI_ADAPTIVE_NEE_FLAGS (RTMI_FLAG_FAST_CULL | RTMI_FLAG_SYNC | RTMI_FLAG_REF_TREE | RTMI_FLAG_FACE_FORWARD | RTMI_FLAG_UV_BOOK)

// ---- the handle ------------------------------------------------------------------------------------------------------------
RTMI_HIDDEN int validate(const rtmi_scene_desc *d);
RTMI_HIDDEN int ensure_streams(rtmi_scene *s);
RTMI_HIDDEN int begin_blocking(rtmi_scene *s);

// ---- the call helpers and the plain render -------------------------------------------------------------------------------
RTMI_HIDDEN int check_params(const rtmi_render_params *p);
RTMI_HIDDEN int check_mode_params(const rtmi_render_params *p, uint32_t accepted, const char *flags_msg, const char *world_msg);
RTMI_HIDDEN int grow_host_texels(PinnedBuf<rtmi_texel> &h, size_t ntex);
RTMI_HIDDEN int reserve_texels(rtmi_scene *s, size_t ntex);
RTMI_HIDDEN int grow_adaptive(rtmi_scene *s, uint32_t T);
RTMI_HIDDEN DevCamera dev_camera(const rtmi_camera *cam);
RTMI_HIDDEN bool boxes_valid(const rtmi_scene *s, const rtmi_camera *cam);
RTMI_HIDDEN DevParams dev_params(const rtmi_scene *s, const rtmi_render_params *p);
RTMI_HIDDEN int plan_traversal(rtmi_scene *s, const rtmi_render_params *p, bool coop, DevParams &P, bool &ext);
RTMI_HIDDEN int begin_passes(rtmi_scene *s, hipStream_t stream);
RTMI_HIDDEN int check_overflow(rtmi_scene *s);
RTMI_HIDDEN void fill_stats(rtmi_scene *s, const rtmi_render_params *p, rtmi_stats *stats, float ms_render, float ms_all,
                            PassCounts counts = {});
RTMI_HIDDEN int fill_stats_from_events(rtmi_scene *s, const rtmi_render_params *p, rtmi_stats *stats, PassCounts counts = {});
RTMI_HIDDEN int plan_and_reserve(rtmi_scene *s, const rtmi_render_params *p, uint32_t ntiles_local, uint32_t &chunk_spp,
                                 uint32_t &pass_ns, size_t slot_bytes = RTMI_SAMPLE_SLOT_BYTES);
RTMI_HIDDEN int reserve_before_clock(rtmi_scene *s, const rtmi_render_params *p);
RTMI_HIDDEN int render_device_locked(rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params *p, void *d_texels,
                                     void *stream_, rtmi_stats *stats);
RTMI_HIDDEN int wait_with_progress(rtmi_scene *const *scenes, hipEvent_t *done_ev, uint32_t n, const rtmi_render_params *p);

// ---- the estimator layer ---------------------------------------------------------------------------------------------------
RTMI_HIDDEN int check_adaptive(const rtmi_render_params *p, const rtmi_adaptive *a);
RTMI_HIDDEN Estimator lit_estimator(const char *name, bool nee, bool env, float env_select_p, const char *null_scene);
RTMI_HIDDEN Estimator estimator_of(const char *name, uint32_t estimator, float env_select_p, const char *null_scene);
RTMI_HIDDEN int check_estimator(const char *name, uint32_t estimator);
RTMI_HIDDEN int check_estimator_opts(const char *name, uint32_t estimator, float env_select_p, uint32_t flags);
RTMI_HIDDEN void dev_lighting(const rtmi_scene *s, bool nee, bool env, float env_select_p, DevLights &L, DevEnv &E);
RTMI_HIDDEN int check_attached(const Estimator &m, const rtmi_scene *s);
RTMI_HIDDEN int check_attached_early(const Estimator &m, const rtmi_scene *s_in);
RTMI_HIDDEN int begin_call(RenderCall &c, const Estimator &m, rtmi_scene *s);
RTMI_HIDDEN void kernel_args(RenderCall &c, const Estimator &m, const rtmi_scene *s, const rtmi_camera *cam,
                             const rtmi_render_params &p);
RTMI_HIDDEN int plan_light_coop(RenderCall &c, rtmi_scene *s, const rtmi_render_params &p, uint32_t flag = RTMI_FLAG_LIGHT_COOP,
                                uint32_t wps = RTMI_LIGHT_COOP_WPS);
RTMI_HIDDEN uint64_t light_run_slots(const rtmi_scene *s, const RenderCall &c);
RTMI_HIDDEN int launch_light_coop(const RenderCall &c, const Estimator &m, rtmi_scene *s, bool sig, uint32_t blocks,
                                  const uint32_t *tiles);
RTMI_HIDDEN int query_check_rays(const char *name, const rtmi_ray *rays, const float *time, uint32_t n);
RTMI_HIDDEN bool query_fast(const rtmi_scene *s, const rtmi_query_params *p, bool has_time);

// An asynchronous call's hold on the handle, which it takes without waiting for the handle's previous call: the lock, what
// the estimator needs attached, the device, the caller's stream behind that previous call (a no-op when both were given the
// same stream), the busy mark.  The members are declared in RenderCall's order: the lock is taken before the mark, and the
// mark ends (records the call's end) before the lock is released.
struct AsyncCall {
    std::unique_lock<std::mutex> lock;
    BusyMark busy{nullptr, nullptr};
    hipStream_t stream = nullptr;
    int begin(const Estimator &m, rtmi_scene *s, void *stream_) {
        lock = std::unique_lock<std::mutex>(s->mu);
        if (int rc = check_attached(m, s)) return rc;
        HIP_TRY(hipSetDevice(s->device));
        stream = reinterpret_cast<hipStream_t>(stream_);
        if (s->busy_recorded) HIP_TRY(hipStreamWaitEvent(stream, s->busy.e, 0));
        busy.s = s; busy.st = stream;
        return RTMI_OK;
    }
};

// Samples [s0, s0 + count) of P.ntiles_local tiles in passes of P.pass_stride (the plan of plan_and_reserve): sets the
// pass fields of P, calls launch(blocks, first, last) for the mode's render and resolve of each pass and ends the pass.
// A pass of n items runs on min(ceil(n / items_per_block), max_blocks) blocks.  `finish`: the last pass ends the call
// (it adds the call's overflows to the sticky word that rtmi_scene_status reports).
template <typename Launch>
static int run_passes(rtmi_scene *s, DevParams &P, hipStream_t stream, uint32_t s0, uint32_t count, bool finish,
                      uint64_t max_blocks, uint32_t items_per_block, PassCounts &counts, Launch &&launch) {
    for (uint32_t k = 0; k < count; k += P.pass_stride) { // one pass unless the per-sample buffer is smaller than count samples
        P.pass_s0 = s0 + k;
        P.pass_cnt = count - k < P.pass_stride ? count - k : P.pass_stride;
        P.nchunks = (P.pass_cnt + P.chunk_spp - 1) / P.chunk_spp;
        const uint64_t nitems = (uint64_t)P.ntiles_local * P.nchunks;
        if (nitems > 0x7fffffffull) return fail(RTMI_ERR_UNSUPPORTED, "too many (tile, chunk) items in one pass");
        const uint64_t nblocks = (nitems + items_per_block - 1) / items_per_block;
        const uint32_t blocks = (uint32_t)(nblocks < max_blocks ? nblocks : max_blocks);
        counts.blocks += blocks; counts.chunks += P.nchunks;
        s->units_total += nitems;
        const bool last = k + P.pass_cnt >= count;
        if (int rc = launch(blocks, k == 0, last)) return rc;
        HIP_TRY(rtmi_render_launch_pass_end(stream, s->status.ptr, (unsigned int)nitems, P.pass_cnt, finish && last));
    }
    return RTMI_OK;
}

// Tiled -> row-major image of N components per pixel (whole-image calls): texel = tile * 64 + ly * 8 + lx, tiles
// counted from the top-left; row 0 of the output = top row
template <int N, typename T, typename U>
static void untile_to(const rtmi_render_params *p, const T *tiled, U *out) {
    const uint32_t txn = tiles_x_of(p);
    for (uint32_t row = 0; row < p->ny; row++)
        for (uint32_t px = 0; px < p->nx; px++) {
            const size_t k = (size_t)((row / RTMI_TILE) * txn + px / RTMI_TILE) * 64 + (row % RTMI_TILE) * RTMI_TILE + px % RTMI_TILE;
            const size_t o = (size_t)row * p->nx + px;
            for (int c = 0; c < N; c++) out[o * N + c] = tiled[k * N + c];
        }
}
// ... of a device buffer of `ntex` texels
template <int N, typename T, typename U>
static int download_untiled(const rtmi_render_params *p, const T *d_tiled, size_t ntex, U *out) {
    std::vector<T> h(ntex * N);
    HIP_TRY(hipMemcpy(h.data(), d_tiled, h.size() * sizeof(T), hipMemcpyDeviceToHost));
    untile_to<N>(p, h.data(), out);
    return RTMI_OK;
}
