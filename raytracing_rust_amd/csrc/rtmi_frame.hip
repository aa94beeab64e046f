// rtmi_frame.hip — translation unit of the frame pipeline (include/rtmi_frame.h): the un-tiling kernel and the host entry
// points.  The renders, the push and the filter are the existing kernels, reached through rtmi_frame_launch.hpp; this unit
// adds the one kernel that stands where the one-shot entries un-tile on the host.  Compiled with the flags of
// rtmi_temporal.hip.  See DESIGN.md §28.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <new>
#include <string>

#include "rtmi.h"
#include "rtmi_frame.h"
#include "rtmi_light_coop.h"
#include "rtmi_frame_launch.hpp"
#include "rtmi_hostkit.hpp"

namespace {

constexpr int kRowLanes = 64, kRows = 4; // a wavefront is 64 consecutive pixels of one row, a workgroup four rows of them

// The device form of rtmi_untile and untile_to<3>: one lane per output pixel.  A wavefront's stores are contiguous (768 B
// per plane) and its texel loads are eight whole 128-B lines (the eight texels of a tile row are one 16-B load each); a
// wavefront per tile would read one contiguous 1 KB but scatter its stores over eight 96-B pieces of eight rows, none of
// them a whole line.  Only pixels inside the image index the tiled buffers, so padding texels are neither read nor counted.
__global__ __launch_bounds__(kRowLanes * kRows) void rtmi_frame_untile_kernel(const uint4 *__restrict__ texels,
                                                                              const float *__restrict__ tiled_se,
                                                                              float *__restrict__ out_linear,
                                                                              float *__restrict__ out_se,
                                                                              unsigned int *__restrict__ poisoned, uint32_t nx,
                                                                              uint32_t ny, uint32_t tiles_x) {
    const uint32_t x = blockIdx.x * kRowLanes + threadIdx.x, y = blockIdx.y * kRows + threadIdx.y;
    if (x >= nx || y >= ny) return;
    const size_t k = (size_t)((y >> 3) * tiles_x + (x >> 3)) * 64 + (y & 7u) * 8 + (x & 7u);
    const size_t o = ((size_t)y * nx + x) * 3;
    const uint4 t = texels[k];
    if (t.w & RTMI_TEXEL_POISON) atomicAdd(poisoned, 1u);
    if (out_linear) {
        out_linear[o] = __uint_as_float(t.x);
        out_linear[o + 1] = __uint_as_float(t.y);
        out_linear[o + 2] = __uint_as_float(t.z);
    }
    if (out_se) {
        out_se[o] = tiled_se[k * 3];
        out_se[o + 1] = tiled_se[k * 3 + 1];
        out_se[o + 2] = tiled_se[k * 3 + 2];
    }
}

hipError_t launch_untile(hipStream_t stream, uint32_t nx, uint32_t ny, const rtmi_texel *texels, const float *tiled_se,
                         float *out_linear, float *out_se, unsigned int *poisoned) {
    const dim3 block(kRowLanes, kRows), grid((nx + kRowLanes - 1) / kRowLanes, (ny + kRows - 1) / kRows);
    hipLaunchKernelGGL(rtmi_frame_untile_kernel, grid, block, 0, stream, reinterpret_cast<const uint4 *>(texels), tiled_se,
                       out_linear, out_se, poisoned, nx, ny, (nx + 7u) / 8u);
    return hipGetLastError();
}

const uint32_t kFeatureFlags = RTMI_FLAG_FAST_CULL | RTMI_FLAG_SYNC | RTMI_FLAG_REF_TREE | RTMI_FLAG_SKY | RTMI_FLAG_FACE_FORWARD |
                               RTMI_FLAG_UV_BOOK;               // what both renders accept
const uint32_t kCoopFlags = RTMI_FLAG_LIGHT_COOP | (1u << 11); // the lit render's own (bit 11: its small-pool test knob)

#define FR_TRY(name, expr) RTMI_HIP_TRY(std::string(name) + ": ", true, expr, #expr)

} // namespace

struct RTMI_HIDDEN rtmi_frame {
    rtmi_scene *s = nullptr;
    rtmi_render_params p{}; // ns and seed are set per call
    rtmi_frame_opts o{};
    RtmiFrameLit lit{};
    bool temporal = true;
    rtmi_denoise_params filter{}; // o.denoise, with 0 iterations under RTMI_FRAME_NO_FILTER
    int device = 0;
    DeviceArena mem; // one allocation, carved in 256-B aligned pieces
    RtmiTemporalHistory hist;
    float *noisy_lin = nullptr, *noisy_se = nullptr;
    float *acc_lin = nullptr, *acc_se = nullptr, *acc_hist = nullptr;
    float2 *acc_motion = nullptr;
    RtmiDenoisePlanes work; // the filter's state, guide and gradient planes
    float *out_lin = nullptr;
    uint8_t *out_rgb = nullptr;
    unsigned int *poisoned = nullptr;   // the un-tiling's count of poisoned texels
    unsigned int *h_poisoned = nullptr; // pinned: read at the frame's final synchronise
};

static int frame_alloc(rtmi_frame *f, const char *name) {
    const size_t n = (size_t)f->p.nx * f->p.ny;
    const auto layout = [&](Carve256 &c) {
        if (f->temporal) rtmi_temporal_history_layout(f->hist, c, f->p.nx, f->p.ny);
        f->noisy_lin = c.take<float>(n * 3);
        f->noisy_se = c.take<float>(n * 3);
        if (f->temporal) {
            f->acc_lin = c.take<float>(n * 3);
            f->acc_se = c.take<float>(n * 3);
            f->acc_hist = c.take<float>(n);
            f->acc_motion = c.take<float2>(n);
        }
        rtmi_denoise_layout(f->work, c, f->p.nx, f->p.ny, f->filter.iterations);
        f->out_lin = c.take<float>(n * 3);
        f->out_rgb = c.take<uint8_t>(n * 3);
        f->poisoned = c.take<unsigned int>(1);
    };
    FR_TRY(name, f->mem.alloc(layout));
    FR_TRY(name, hipHostMalloc(reinterpret_cast<void **>(&f->h_poisoned), 64, hipHostMallocDefault));
    return RTMI_OK;
}

extern "C" void rtmi_frame_destroy(rtmi_frame *f) {
    if (!f) return;
    RtmiFrameHold *hold = nullptr; // the scene's lock and its running work, as rtmi_session_destroy
    const RtmiFrameLit plain{"rtmi_frame_destroy", false, false, 1.0f};
    (void)rtmi_frame_hold_begin(f->s, plain, &hold);
    f->mem.release();
    if (f->h_poisoned) (void)hipHostFree(f->h_poisoned);
    rtmi_frame_hold_end(hold);
    delete f;
}

extern "C" int rtmi_frame_create(rtmi_scene *s, const rtmi_render_params *p_in, const rtmi_frame_opts *o, rtmi_frame **out) {
    // every argument check comes before the first use of the handle (and of the device)
    const char *name = "rtmi_frame_create";
    if (out) *out = nullptr;
    if (!p_in || !o || !out) return fail(RTMI_ERR_INVALID, name, "NULL argument");
    const rtmi_render_params &p = *p_in;
    if (p.nx == 0 || p.ny == 0 || p.nx > 32768u || p.ny > 32768u) return fail(RTMI_ERR_INVALID, name, "nx and ny must be in [1, 32768]");
    if (p.tile_world == 0 || p.tile_rank >= p.tile_world) return fail(RTMI_ERR_INVALID, name, "bad tile_rank/tile_world");
    if (o->estimator > RTMI_ROULETTE_ENV_NEE) return fail(RTMI_ERR_INVALID, name, "estimator must be one of RTMI_ROULETTE_* (0..3)");
    if (!(o->env_select_p > 0.0f && o->env_select_p <= 1.0f)) return fail(RTMI_ERR_INVALID, name, "env_select_p must be in (0, 1]");
    int rc;
    if ((rc = rtmi_temporal_check_ranges(name, p.nx, p.ny, &o->temporal))) return rc;
    if ((rc = rtmi_denoise_check_ranges("rtmi_frame_create: ", p.nx, p.ny, &o->denoise))) return rc;
    for (uint32_t r : o->reserved)
        if (r) return fail(RTMI_ERR_INVALID, name, "reserved must be 0");
    const bool nee = o->estimator == RTMI_ROULETTE_NEE || o->estimator == RTMI_ROULETTE_ENV_NEE;
    const bool env = o->estimator == RTMI_ROULETTE_ENV || o->estimator == RTMI_ROULETTE_ENV_NEE;
    if (env && (p.flags & RTMI_FLAG_SKY)) return fail(RTMI_ERR_INVALID, name, "RTMI_FLAG_SKY is refused, the map replaces the sky");
    const uint32_t coop = (nee || env) && (p.flags & RTMI_FLAG_LIGHT_COOP) ? kCoopFlags : 0u;
    if (p.flags & ~(kFeatureFlags | coop))
        return fail(RTMI_ERR_UNSUPPORTED, name,
                    "frames accept the flags FAST_CULL, SYNC, REF_TREE, SKY, FACE_FORWARD and UV_BOOK, and LIGHT_COOP with a lit "
                    "estimator, only (not PATH_SIG, PROFILE, ASYNC, BLOCK_COOP, PROGRESSIVE, TEST_OVERFLOW, LIGHT_TREE)");
    if (o->temporal.flags & ~RTMI_TEMPORAL_NO_DEMODULATE) return fail(RTMI_ERR_UNSUPPORTED, name, "unknown temporal.flags bit");
    if (o->denoise.flags) return fail(RTMI_ERR_UNSUPPORTED, name, "denoise.flags must be 0 (reserved)");
    if (o->flags & ~(RTMI_FRAME_NO_TEMPORAL | RTMI_FRAME_NO_FILTER)) return fail(RTMI_ERR_UNSUPPORTED, name, "unknown flags bit of opts");
    if (p.tile_world != 1) return fail(RTMI_ERR_UNSUPPORTED, name, "a frame renders the whole image: tile_world must be 1");

    rtmi_frame *f = new (std::nothrow) rtmi_frame;
    if (!f) return fail(RTMI_ERR_NOMEM, name, "out of host memory");
    f->p = p;
    f->p.ns = 2u;
    f->p.seed = 0u;
    f->o = *o;
    f->lit = RtmiFrameLit{"rtmi_frame_render", nee, env, o->env_select_p};
    f->temporal = !(o->flags & RTMI_FRAME_NO_TEMPORAL);
    f->filter = o->denoise;
    if (o->flags & RTMI_FRAME_NO_FILTER) f->filter.iterations = 0u;
    RtmiFrameHold *hold = nullptr;
    const RtmiFrameLit lit{name, nee, env, o->env_select_p};
    if ((rc = rtmi_frame_hold_begin(s, lit, &hold))) { // the scene, what the estimator needs attached, the device
        delete f;
        return rc;
    }
    f->s = s;
    f->device = rtmi_frame_planes(hold, f->p).device;
    rc = frame_alloc(f, name);
    rtmi_frame_hold_end(hold);
    if (rc) {
        rtmi_frame_destroy(f);
        return rc;
    }
    *out = f;
    return RTMI_OK;
}

extern "C" int rtmi_frame_reset(rtmi_frame *f) {
    if (!f) return rtmi_fail(RTMI_ERR_INVALID, "rtmi_frame_reset: NULL handle");
    f->hist.has_prev = false;
    return RTMI_OK;
}

// the stages after the two renders, enqueued on the scene's stream, the copies of the planes asked for and the final
// synchronise
static int frame_chain(rtmi_frame *f, const char *name, const RtmiFramePlanes &R, const rtmi_camera *cam, const rtmi_frame_out &out,
                       hipMemcpyKind kind) {
    const uint32_t nx = f->p.nx, ny = f->p.ny;
    const size_t n = (size_t)nx * ny;
    hipStream_t st = R.stream;
    FR_TRY(name, hipMemsetAsync(f->poisoned, 0, sizeof(unsigned int), st));
    FR_TRY(name, launch_untile(st, nx, ny, R.texels, R.tiled_stderr, f->noisy_lin, f->noisy_se, f->poisoned));
    FR_TRY(name, hipMemcpyAsync(f->h_poisoned, f->poisoned, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    const float *lin = f->noisy_lin, *se = f->noisy_se;
    if (f->temporal) {
        FR_TRY(name, rtmi_temporal_push_launch(st, nx, ny, f->o.temporal, f->hist, cam, f->noisy_lin, R.albedo, R.normal, R.depth,
                                               f->noisy_se, f->acc_lin, f->acc_se, f->acc_hist, f->acc_motion));
        lin = f->acc_lin;
        se = f->acc_se;
    }
    FR_TRY(name, rtmi_denoise_launch(st, nx, ny, f->filter, lin, R.albedo, R.normal, R.depth, se, f->work, f->out_lin, f->out_rgb));
    const auto copy = [&](void *dst, const void *src, size_t bytes) {
        return dst ? hipMemcpyAsync(dst, src, bytes, kind, st) : hipSuccess;
    };
    FR_TRY(name, copy(out.linear, f->out_lin, n * 12));
    FR_TRY(name, copy(out.rgb8, f->out_rgb, n * 3));
    FR_TRY(name, copy(out.noisy_linear, f->noisy_lin, n * 12));
    FR_TRY(name, copy(out.noisy_stderr, f->noisy_se, n * 12));
    FR_TRY(name, copy(out.albedo, R.albedo, n * 12));
    FR_TRY(name, copy(out.normal, R.normal, n * 12));
    FR_TRY(name, copy(out.depth, R.depth, n * 4));
    FR_TRY(name, copy(out.hits, R.hits, n * 4));
    if (f->temporal) {
        FR_TRY(name, copy(out.accum_linear, f->acc_lin, n * 12));
        FR_TRY(name, copy(out.accum_stderr, f->acc_se, n * 12));
        FR_TRY(name, copy(out.history, f->acc_hist, n * 4));
        FR_TRY(name, copy(out.motion, f->acc_motion, n * 8));
    }
    FR_TRY(name, hipStreamSynchronize(st));
    if (*f->h_poisoned)
        return fail(RTMI_ERR_DEVICE, name, "framebuffer holds poisoned texels (traversal pool overflow in the launch that wrote them)");
    return RTMI_OK;
}

static int frame_render(const char *name, rtmi_frame *f, const rtmi_camera *cam, uint32_t ns, uint64_t seed, const rtmi_frame_out *out,
                        rtmi_stats *stats, hipMemcpyKind kind) {
    // every argument check comes before the first use of the handle (and of the device); the handle comes last, so that a
    // machine without a device (where no handle can exist) still answers for every other argument
    if (!cam || !out) return fail(RTMI_ERR_INVALID, name, "NULL argument");
    if (ns < 2u) return fail(RTMI_ERR_INVALID, name, "ns must be at least 2 (a standard error needs two samples)");
    float m[9];
    int rc;
    if ((rc = rtmi_temporal_camera_matrix(name, cam, m))) return rc;
    if (ns >= (1u << 26)) return fail(RTMI_ERR_UNSUPPORTED, name, "ns must be below 2^26");
    if (!f) return fail(RTMI_ERR_INVALID, name, "NULL handle");
    rtmi_render_params p = f->p;
    p.ns = ns;
    p.seed = seed;
    RtmiFrameLit lit = f->lit;
    lit.name = name;
    RtmiFrameHold *hold = nullptr;
    if ((rc = rtmi_frame_hold_begin(f->s, lit, &hold))) return rc;
    rtmi_render_params pf = p; // the features render takes no cooperative flag
    pf.flags &= ~kCoopFlags;
    if (!(rc = rtmi_frame_enqueue_lit(hold, lit, cam, p, stats)) && !(rc = rtmi_frame_enqueue_first_hits(hold, cam, pf)))
        rc = frame_chain(f, name, rtmi_frame_planes(hold, p), cam, *out, kind);
    rtmi_frame_hold_end(hold);
    if (rc) {
        f->hist.has_prev = false;
        return rc;
    }
    if (f->temporal) rtmi_temporal_history_advance(f->hist, cam, m);
    return RTMI_OK;
}

extern "C" int rtmi_frame_render(rtmi_frame *f, const rtmi_camera *cam, uint32_t ns, uint64_t seed, const rtmi_frame_out *out,
                                 rtmi_stats *stats) {
    return frame_render("rtmi_frame_render", f, cam, ns, seed, out, stats, hipMemcpyDeviceToHost);
}

extern "C" int rtmi_frame_render_device(rtmi_frame *f, const rtmi_camera *cam, uint32_t ns, uint64_t seed, const rtmi_frame_out *out,
                                        rtmi_stats *stats) {
    return frame_render("rtmi_frame_render_device", f, cam, ns, seed, out, stats, hipMemcpyDeviceToDevice);
}

extern "C" int rtmi_probe_frame_untile(int device, uint32_t nx, uint32_t ny, const rtmi_texel *tiled, const float *tiled_stderr,
                                       float *out_linear, float *out_stderr, uint32_t *poisoned) {
    const char *name = "rtmi_probe_frame_untile";
    if (nx == 0 || ny == 0 || nx > 32768u || ny > 32768u) return fail(RTMI_ERR_INVALID, name, "nx and ny must be in [1, 32768]");
    if (!tiled) return fail(RTMI_ERR_INVALID, name, "NULL argument");
    if (out_stderr && !tiled_stderr) return fail(RTMI_ERR_INVALID, name, "out_stderr needs tiled_stderr");
    if (int rc = device_ok(std::string(name) + ": ", device)) return rc;
    FR_TRY(name, hipSetDevice(device));
    const size_t n = (size_t)nx * ny, ntex = (size_t)((nx + 7u) / 8u) * ((ny + 7u) / 8u) * 64;
    rtmi_texel *d_tex;
    float *d_se, *d_lin, *d_ose;
    unsigned int *d_poison, h_poison = 0;
    const auto layout = [&](Carve256 &c) {
        d_tex = c.take<rtmi_texel>(ntex);
        d_se = c.take<float>(ntex * 3);
        d_lin = c.take<float>(n * 3);
        d_ose = c.take<float>(n * 3);
        d_poison = c.take<unsigned int>(1);
    };
    DeviceArena mem;
    FR_TRY(name, mem.alloc(layout));
    FR_TRY(name, hipMemcpy(d_tex, tiled, ntex * 16, hipMemcpyHostToDevice));
    if (tiled_stderr) FR_TRY(name, hipMemcpy(d_se, tiled_stderr, ntex * 12, hipMemcpyHostToDevice));
    FR_TRY(name, hipMemset(d_poison, 0, sizeof(unsigned int)));
    FR_TRY(name, launch_untile(nullptr, nx, ny, d_tex, tiled_stderr ? d_se : nullptr, out_linear ? d_lin : nullptr,
                               out_stderr ? d_ose : nullptr, d_poison));
    if (out_linear) FR_TRY(name, hipMemcpy(out_linear, d_lin, n * 12, hipMemcpyDeviceToHost));
    if (out_stderr) FR_TRY(name, hipMemcpy(out_stderr, d_ose, n * 12, hipMemcpyDeviceToHost));
    FR_TRY(name, hipMemcpy(&h_poison, d_poison, sizeof(unsigned int), hipMemcpyDeviceToHost));
    if (poisoned) *poisoned = h_poison;
    return RTMI_OK;
}
