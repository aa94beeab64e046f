// rtmi_batch.hip — the batch render modes (host code only): what their host paths share, radiance
// queries, hemisphere gathers, sparse renders, per-pixel and windowed adaptive sampling and their probes.  On the estimator
// layer and the call helpers, which rtmi_device.hip still holds (rtmi_host.hpp); every kernel is reached through the mode's
// *_launch.hpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "rtmi_host.hpp"
#include "rtmi_radiance.h"
#include "rtmi_radiance_launch.hpp"
#include "rtmi_gather.h"
#include "rtmi_gather_launch.hpp"
#include "rtmi_sparse.h"
#include "rtmi_sparse_launch.hpp"
#include "rtmi_pixelwise.h"
#include "rtmi_pixelwise_launch.hpp"
#include "rtmi_window.h"
#include "rtmi_window_launch.hpp"
#include "rtmi_batch_coop.h"
#include "rtmi_batch_coop_launch.hpp"

// ---- the batch modes (radiance queries, hemisphere gathers, sparse renders, per-pixel adaptive sampling) ----------------
// What their host paths share: the chunks of the persistent wavefronts (batch_take, rtmi_batch.hpp), the kernel arguments
// of a call, and the end of a blocking call that reads its records through the handle's rad_out and rad_samples.

// The chunk rule.  `total` items on the persistent grid of the per-lane render kernels (`slots` wavefronts): chunks of `cap`
// items, smaller (a multiple of 64, at least 64) for a batch that would otherwise leave wavefronts of the grid without one
// (four chunks a wavefront), and one workgroup a wavefront, no more than there are chunks.
struct BatchChunks {
    uint32_t chunk, nchunks, blocks;
};
static BatchChunks batch_chunks(const rtmi_scene *s, uint32_t total, uint32_t cap = RTMI_RADIANCE_CHUNK) {
    const uint32_t slots = (uint32_t)(s->slots / 20) * 4u * 4u;
    const uint32_t share = (uint32_t)(((uint64_t)total / ((uint64_t)slots * 4u) + 63ull) & ~63ull);
    BatchChunks c;
    c.chunk = share < 64u ? 64u : (share > cap ? cap : share);
    c.nchunks = (total + c.chunk - 1u) / c.chunk;
    c.blocks = c.nchunks < slots ? c.nchunks : slots;
    return c;
}
// RTMI_FLAG_BATCH_COOP (include/rtmi_batch_coop.h).  The bits the flag adds to a batch entry's accepted ones: itself and
// the two test knobs, bit 11 (the small pool) and TEST_OVERFLOW, which alone stay refused.
static uint32_t batch_coop_bits(uint32_t flags) {
    return (flags & RTMI_FLAG_BATCH_COOP) ? (RTMI_FLAG_BATCH_COOP | (1u << 11) | RTMI_FLAG_TEST_OVERFLOW) : 0u;
}
// The selection, evaluated once per enqueue: the flag, a call whose pruned traversal may run at all (`fast`: the entry's own
// rule, which includes FAST_CULL), a scene within the cooperative size limits and of level 0 (plan_light_coop's rule).
// Where the cooperative kernel runs: its traversal plan in P (the handle's spill buffer grown: the one allocation of a
// device form: any earlier cooperative call of the handle has made it), its pool form, the dynamic LDS of a block, and the grid.
// The grid: wavefront b spills to entries [b * spill_cap, (b + 1) * spill_cap) of the handle's buffer, which holds
// s->slots wavefronts, so blocks * WAVES_PER_BLOCK <= s->slots must hold; CUs x 4 SIMDs x the kernel's waves per SIMD
// (at most 4 of the buffer's 5) keeps it, and it is checked.  The chunks stay batch_chunks'.
struct BatchCoop {
    bool coop = false, ext = false;
    size_t lds = 0;
    uint32_t blocks = 0;
};
static int plan_batch_coop(rtmi_scene *s, const Estimator &m, uint32_t flags, bool fast, const BatchChunks &ch, DevParams &P,
                           BatchCoop &c) {
    const bool coop_ok = s->meta.n_prims < (1u << 22) && s->meta.n_nodes < (1u << 25) && s->meta.n_alt_nodes < (1u << 25);
    const bool inst = s->dev.has_prim_xf != 0u || s->dev.has_medium_outer != 0u;
    c.coop = (flags & RTMI_FLAG_BATCH_COOP) != 0u && fast && coop_ok && !inst;
    if (!c.coop) return RTMI_OK;
    rtmi_render_params rp{};
    rp.flags = flags;
    if (int rc = plan_traversal(s, &rp, true, P, c.ext)) return rc;
    if (flags & (1u << 11)) { // test knob, as in plan_light_coop: a pool this small that it spills all the time
        c.ext = true;
        P.coop_cap = 256u;
    }
    c.lds = (size_t)WAVES_PER_BLOCK * CoopLds{P.coop_cap, c.ext, false}.words() * sizeof(uint32_t);
    const uint32_t grid = (uint32_t)(s->slots / 20) * 4u * rtmi_batch_coop_wps(m.nee, m.env);
    c.blocks = ch.nchunks < grid ? ch.nchunks : grid;
    if ((uint64_t)c.blocks * WAVES_PER_BLOCK > (uint64_t)s->slots)
        return fail(RTMI_ERR_DEVICE, "the cooperative batch grid exceeds the wavefronts of the spill buffer");
    return RTMI_OK;
}
// The overflow word of a cooperative batch launch, status[0].  A blocking call owns it from its begin to its return
// (batch_blocking_begin zeroes it once, every launch of the call adds to it, batch_coop_check reads it after the wait, as
// check_overflow reads a render's): what an earlier _device call or render left in the sticky word status[2] stays there
// for rtmi_scene_status.  A _device call has nobody to read its own word: each launch starts it at zero and
// rtmi_batch_coop_end_kernel adds it to the sticky word.  Every batch entry sets s->batch_blocking under the handle's lock.
static int batch_blocking_begin(rtmi_scene *s) {
    s->batch_blocking = true;
    HIP_TRY(hipMemsetAsync(s->status.ptr, 0, sizeof(unsigned int), s->stream.s));
    return RTMI_OK;
}
static int batch_coop_begin(rtmi_scene *s, hipStream_t stream) {
    if (!s->batch_blocking) HIP_TRY(hipMemsetAsync(s->status.ptr, 0, sizeof(unsigned int), stream));
    return RTMI_OK;
}
static int batch_coop_end(rtmi_scene *s, hipStream_t stream) {
    if (!s->batch_blocking) HIP_TRY(rtmi_batch_coop_launch_end(stream, s->status.ptr));
    return RTMI_OK;
}
// the end of a blocking batch call whose kernels have finished: the call's own overflow word
static int batch_coop_check(rtmi_scene *s) {
    if (s->last_batch_kernel != (int)RTMI_KERNEL_WAVE_COOP) return RTMI_OK;
    unsigned int st = 0;
    HIP_TRY(hipMemcpy(&st, s->status.ptr, sizeof(st), hipMemcpyDeviceToHost));
    if (st != 0) {
        HIP_TRY(hipMemset(s->status.ptr, 0, sizeof(unsigned int)));
        return fail(RTMI_ERR_DEVICE, "cooperative traversal pool overflow (results invalid): run the call without RTMI_FLAG_BATCH_COOP");
    }
    return RTMI_OK;
}
// The kernel arguments of a batch call: the estimator's lights and map, and the DevParams of `rp` with no pass planned
// (ns = 1, rank 0 of 1; the pass fields stay unread) and `d_samples` as the per-sample buffer.  rp: the caller's image
// (sparse renders) or no_image (radiance queries and gathers).
struct BatchArgs {
    DevParams P;
    DevLights L;
    DevEnv E;
};
static rtmi_render_params no_image(uint32_t max_depth, float t_min, uint64_t seed, uint32_t flags) {
    rtmi_render_params rp{};
    rp.nx = 1u; rp.ny = 1u;
    rp.max_depth = max_depth; rp.t_min = t_min; rp.seed = seed; rp.flags = flags;
    return rp;
}
static BatchArgs batch_args(const rtmi_scene *s, const Estimator &m, rtmi_render_params rp, void *d_samples) {
    rp.ns = 1u; rp.tile_rank = 0u; rp.tile_world = 1u;
    BatchArgs a;
    a.P = dev_params(s, &rp);
    a.P.samples = reinterpret_cast<Rad3 *>(d_samples);
    dev_lighting(s, m.nee, m.env, m.env_select_p, a.L, a.E);
    return a;
}
// The handle's buffers of a blocking call of n entries and ns samples in all, and the end of that call, whose enqueue ran
// between ev[0] and ev[1]: the records to the host, the wait, the kernels' milliseconds.
static int batch_reserve(rtmi_scene *s, size_t n, size_t ns) {
    if (int rc = grow(s, s->rad_samples, ns * sizeof(Rad3))) return rc;
    return grow(s, s->rad_out, n * 6 * sizeof(float));
}
static int batch_finish(rtmi_scene *s, size_t n, size_t ns, float *out_mean, float *out_stderr, float *out_samples, double *kernel_ms) {
    hipStream_t stream = s->stream.s;
    if (out_mean) HIP_TRY(hipMemcpyAsync(out_mean, s->rad_out.ptr, n * 3 * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (out_stderr) HIP_TRY(hipMemcpyAsync(out_stderr, s->rad_out.ptr + n * 3, n * 3 * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (out_samples) HIP_TRY(hipMemcpyAsync(out_samples, s->rad_samples.ptr, ns * sizeof(Rad3), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (kernel_ms) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, s->ev[0].e, s->ev[1].e));
        *kernel_ms = (double)ms;
    }
    return RTMI_OK;
}

// ---- radiance queries (include/rtmi_radiance.h) -------------------------------------------------------------------------
// The checks both forms share, in this order: params, flags, the values, the ray and output pointers of a batch with rays.
// Nothing here reads the handle, so each is answered for a NULL one too; the handle and what the estimator needs attached
// follow in the entries (begin_call's rule, the one-shot entries').
#define RTMI_RADIANCE_FLAGS (RTMI_FLAG_FAST_CULL | RTMI_FLAG_SKY | RTMI_FLAG_FACE_FORWARD | RTMI_FLAG_UV_BOOK)
static int radiance_check(const char *name, const rtmi_radiance_params *p, const void *rays, bool has_out, const char *out_msg) {
    const std::string nm = std::string(name) + ": ";
    if (!p) return fail(RTMI_ERR_INVALID, nm + "params is NULL");
    if (p->flags & ~(RTMI_RADIANCE_FLAGS | batch_coop_bits(p->flags)))
        return fail(RTMI_ERR_UNSUPPORTED, nm + "radiance queries accept the flags FAST_CULL, SKY, FACE_FORWARD and UV_BOOK only");
    if (int rc = check_estimator(name, p->estimator)) return rc;
    if (p->spp == 0u) return fail(RTMI_ERR_INVALID, nm + "spp must be at least 1");
    if (p->max_depth == 0u) return fail(RTMI_ERR_INVALID, nm + "max_depth must be at least 1");
    if (!std::isfinite(p->t_min)) return fail(RTMI_ERR_INVALID, nm + "t_min must be finite");
    if (p->first_ray > (1ull << 32) || p->first_ray + p->n > (1ull << 32))
        return fail(RTMI_ERR_INVALID, nm + "first_ray + n must not exceed 2^32 (a ray index would wrap onto another ray's stream)");
    if ((uint64_t)p->first_sample + p->spp > (1ull << 32))
        return fail(RTMI_ERR_INVALID, nm + "first_sample + spp must not exceed 2^32 (a sample index would wrap onto another sample's stream)");
    if ((uint64_t)p->n * p->spp >= (1ull << 31)) return fail(RTMI_ERR_INVALID, nm + "n * spp must be below 2^31");
    if (int rc = check_estimator_opts(name, p->estimator, p->env_select_p, p->flags)) return rc;
    if (p->n == 0u) return RTMI_OK;
    if (!rays) return fail(RTMI_ERR_INVALID, nm + "rays is NULL");
    if (!has_out) return fail(RTMI_ERR_INVALID, nm + out_msg);
    return RTMI_OK;
}
// The two launches of a call on `stream`: the path kernel on the persistent grid of the per-lane render kernels, fed by the
// handle's chunk counter (zeroed here, on the call's stream: the handle serialises its calls), then the resolve.
static int radiance_enqueue(rtmi_scene *s, const Estimator &m, const rtmi_radiance_params *p, hipStream_t stream, const void *d_rays,
                            const void *d_time, void *d_mean, void *d_stderr, void *d_samples) {
    BatchArgs a = batch_args(s, m, no_image(p->max_depth, p->t_min, p->seed, p->flags), d_samples);
    RadianceBatch B{};
    B.rays = reinterpret_cast<const float4 *>(d_rays);
    B.time = reinterpret_cast<const float *>(d_time);
    B.mean = reinterpret_cast<float *>(d_mean);
    B.stderr_out = reinterpret_cast<float *>(d_stderr);
    B.queue = s->status.ptr + RTMI_STATUS_WORDS;
    B.n = p->n; B.spp = p->spp; B.total = p->n * p->spp;
    B.first_ray = (uint32_t)p->first_ray; B.first_sample = p->first_sample;
    B.skip_block = p->stream_skip >> 2; B.skip_pos = p->stream_skip & 3u;
    uint32_t cap = RTMI_RADIANCE_CHUNK;
    if (const char *e = getenv("RTMI_RADIANCE_CHUNK")) { // tuning knob of tools/radiance_timing.py: a multiple of 64 in [64, 65536]
        const long v = atol(e);
        if (v >= 64 && v <= 65536) cap = (uint32_t)v & ~63u;
    }
    const BatchChunks ch = batch_chunks(s, B.total, cap);
    B.chunk = ch.chunk; B.nchunks = ch.nchunks;
    const rtmi_query_params q{p->n, p->flags & RTMI_FLAG_FAST_CULL, 0ull, 0ull};
    const bool fast = query_fast(s, &q, d_time != nullptr);
    BatchCoop co;
    if (int rc = plan_batch_coop(s, m, p->flags, fast, ch, a.P, co)) return rc;
    s->last_batch_kernel = co.coop ? RTMI_KERNEL_WAVE_COOP : RTMI_KERNEL_PERLANE;
    HIP_TRY(hipMemsetAsync(B.queue, 0, sizeof(unsigned int), stream));
    if (co.coop) {
        if (int rc = batch_coop_begin(s, stream)) return rc;
        HIP_TRY(rtmi_batch_coop_launch_radiance(co.ext, m.nee, m.env, co.blocks, co.lds, stream, s->dev, a.P, B, a.L, a.E));
        if (int rc = batch_coop_end(s, stream)) return rc;
    } else
    HIP_TRY(rtmi_radiance_launch(fast, m.nee, m.env, ch.blocks, stream, s->dev, a.P, B, a.L, a.E));
    if (d_mean || d_stderr) HIP_TRY(rtmi_radiance_launch_resolve(stream, a.P.samples, B));
    return RTMI_OK;
}
extern "C" int rtmi_radiance(rtmi_scene *s, const rtmi_radiance_params *p, const rtmi_ray *rays, const float *time, float *out_mean,
                             float *out_stderr, float *out_samples, double *kernel_ms) {
    const char *name = "rtmi_radiance";
    int rc;
    if ((rc = radiance_check(name, p, rays, out_mean || out_stderr || out_samples, "every output is NULL"))) return rc;
    if (kernel_ms) *kernel_ms = 0.0;
    if (p->n && (rc = query_check_rays(name, rays, time, p->n))) return rc;
    const std::string null_scene = std::string(name) + ": scene is NULL";
    const Estimator m = estimator_of(name, p->estimator, p->env_select_p, null_scene.c_str());
    if (!s) return fail(RTMI_ERR_INVALID, null_scene);
    if (p->n == 0u) return RTMI_OK;
    RenderCall c;
    if ((rc = begin_call(c, m, s)) || (rc = batch_blocking_begin(s))) return rc;
    hipStream_t stream = s->stream.s;
    const size_t n = p->n, ns = n * p->spp;
    if ((rc = grow(s, s->q_rays, n * sizeof(rtmi_ray))) ||
        (time && (rc = grow(s, s->q_time, n * sizeof(float)))) || (rc = batch_reserve(s, n, ns)))
        return rc;
    float *d_mean = s->rad_out.ptr, *d_stderr = s->rad_out.ptr + n * 3;
    HIP_TRY(hipMemcpyAsync(s->q_rays.ptr, rays, n * sizeof(rtmi_ray), hipMemcpyHostToDevice, stream));
    if (time) HIP_TRY(hipMemcpyAsync(s->q_time.ptr, time, n * sizeof(float), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(s->ev[0].e, stream));
    if ((rc = radiance_enqueue(s, m, p, stream, s->q_rays.ptr, time ? s->q_time.ptr : nullptr, out_mean ? d_mean : nullptr,
                               out_stderr ? d_stderr : nullptr, s->rad_samples.ptr)))
        return rc;
    HIP_TRY(hipEventRecord(s->ev[1].e, stream));
    if ((rc = batch_finish(s, n, ns, out_mean, out_stderr, out_samples, kernel_ms))) return rc;
    return batch_coop_check(s);
}
extern "C" int rtmi_radiance_device(rtmi_scene *s, const rtmi_radiance_params *p, const void *d_rays, const void *d_time, void *d_mean,
                                    void *d_stderr, void *d_samples, void *stream_) {
    const char *name = "rtmi_radiance_device";
    if (int rc = radiance_check(name, p, d_rays, d_samples != nullptr, "d_samples is NULL (the kernel's per-sample buffer)")) return rc;
    const std::string null_scene = std::string(name) + ": scene is NULL";
    const Estimator m = estimator_of(name, p->estimator, p->env_select_p, null_scene.c_str());
    if (!s) return fail(RTMI_ERR_INVALID, null_scene);
    if (p->n == 0u) return RTMI_OK;
    AsyncCall c;
    if (int rc = c.begin(m, s, stream_)) return rc;
    s->batch_blocking = false;
    return radiance_enqueue(s, m, p, c.stream, d_rays, d_time, d_mean, d_stderr, d_samples);
}

// ---- hemisphere gathers (include/rtmi_gather.h) ---------------------------------------------------------------------------
// The checks both forms share, in radiance_check's order: params, flags, the values, then the pointers of a batch with
// points.  Nothing here reads the handle, so each is answered for a NULL one too.
static int gather_check(const char *name, const rtmi_gather_params *p, const void *points, const void *normals, bool has_out,
                        bool has_sh, const char *out_msg) {
    const std::string nm = std::string(name) + ": ";
    if (!p) return fail(RTMI_ERR_INVALID, nm + "params is NULL");
    if (p->flags & ~(RTMI_RADIANCE_FLAGS | batch_coop_bits(p->flags)))
        return fail(RTMI_ERR_UNSUPPORTED, nm + "gathers accept the flags FAST_CULL, SKY, FACE_FORWARD and UV_BOOK only");
    if (p->mode > RTMI_GATHER_SPHERE) return fail(RTMI_ERR_INVALID, nm + "mode must be RTMI_GATHER_COSINE or RTMI_GATHER_SPHERE");
    if (int rc = check_estimator(name, p->estimator)) return rc;
    if (p->spp == 0u) return fail(RTMI_ERR_INVALID, nm + "spp must be at least 1");
    if (p->spp >= (1u << 31)) return fail(RTMI_ERR_INVALID, nm + "spp must be below 2^31 (one point's samples are one slab)");
    if (p->max_depth == 0u) return fail(RTMI_ERR_INVALID, nm + "max_depth must be at least 1");
    if (!std::isfinite(p->t_min)) return fail(RTMI_ERR_INVALID, nm + "t_min must be finite");
    if (p->first_point > (1ull << 32) || p->first_point + p->n > (1ull << 32))
        return fail(RTMI_ERR_INVALID, nm + "first_point + n must not exceed 2^32 (a point index would wrap onto another point's stream)");
    if ((uint64_t)p->first_sample + p->spp > (1ull << 32))
        return fail(RTMI_ERR_INVALID, nm + "first_sample + spp must not exceed 2^32 (a sample index would wrap onto another sample's stream)");
    if (int rc = check_estimator_opts(name, p->estimator, p->env_select_p, p->flags)) return rc;
    if (p->mode == RTMI_GATHER_COSINE && has_sh)
        return fail(RTMI_ERR_INVALID, nm + "the sh output belongs to RTMI_GATHER_SPHERE (convolve a probe with sh_irradiance instead)");
    if (p->n == 0u) return RTMI_OK;
    if (!points) return fail(RTMI_ERR_INVALID, nm + "points is NULL");
    if (p->mode == RTMI_GATHER_COSINE && !normals) return fail(RTMI_ERR_INVALID, nm + "normals is NULL (RTMI_GATHER_COSINE)");
    if (!has_out) return fail(RTMI_ERR_INVALID, nm + out_msg);
    return RTMI_OK;
}
// what the host form refuses of a point; the device form takes the caller's word
static int gather_check_points(const char *name, const rtmi_gather_params *p, const float *points, const float *normals,
                               const float *time) {
    const auto bad = [&](uint32_t i, const char *what) {
        return fail(RTMI_ERR_INVALID, std::string(name) + ": point " + std::to_string(i) + " " + what);
    };
    for (uint32_t i = 0; i < p->n; i++) {
        bool finite = !time || std::isfinite(time[i]);
        for (int k = 0; k < 3; k++) finite = finite && std::isfinite(points[3 * (size_t)i + k]);
        if (!finite) return bad(i, "has a non-finite component");
        if (p->mode == RTMI_GATHER_COSINE) {
            const float l = rtmi_gather_normal_length(normals + 3 * (size_t)i);
            if (!(l > 0.0f) || !std::isfinite(l)) return bad(i, "has a zero or non-finite normal");
        }
    }
    return RTMI_OK;
}
// the points of a slab: `want` (params.slab_points, or the form's own default or capacity) held to [1, (2^31 - 1) / spp]
static uint32_t gather_slab(const rtmi_gather_params *p, uint64_t want) {
    const uint64_t most = ((1ull << 31) - 1u) / p->spp; // >= 1: spp < 2^31
    return (uint32_t)(want < 1u ? 1u : (want > most ? most : want));
}
// The launches of one slab on `stream`: points [at, at + count) of the call through pointers to the slab's records; the
// path kernel on the persistent grid of the per-lane render kernels, fed by the handle's chunk counter (zeroed here, on the
// call's stream: the handle serialises its calls and a stream its launches), then the resolve.
static int gather_enqueue(rtmi_scene *s, const Estimator &m, const rtmi_gather_params *p, hipStream_t stream, uint32_t at,
                          uint32_t count, const void *d_points, const void *d_normals, const void *d_time, void *d_value,
                          void *d_stderr, void *d_sh, void *d_scratch) {
    BatchArgs a = batch_args(s, m, no_image(p->max_depth, p->t_min, p->seed, p->flags), d_scratch);
    GatherBatch B{};
    B.points = reinterpret_cast<const float *>(d_points);
    B.normals = p->mode == RTMI_GATHER_COSINE ? reinterpret_cast<const float *>(d_normals) : nullptr;
    B.time = reinterpret_cast<const float *>(d_time);
    B.value = reinterpret_cast<float *>(d_value);
    B.stderr_out = reinterpret_cast<float *>(d_stderr);
    B.sh = reinterpret_cast<float *>(d_sh);
    B.queue = s->status.ptr + RTMI_STATUS_WORDS;
    B.n = count; B.spp = p->spp; B.total = count * p->spp;
    B.first_point = (uint32_t)(p->first_point + at); B.first_sample = p->first_sample;
    const BatchChunks ch = batch_chunks(s, B.total);
    B.chunk = ch.chunk; B.nchunks = ch.nchunks;
    const rtmi_query_params q{count, p->flags & RTMI_FLAG_FAST_CULL, 0ull, 0ull};
    const bool fast = query_fast(s, &q, d_time != nullptr);
    BatchCoop co;
    if (int rc = plan_batch_coop(s, m, p->flags, fast, ch, a.P, co)) return rc;
    s->last_batch_kernel = co.coop ? RTMI_KERNEL_WAVE_COOP : RTMI_KERNEL_PERLANE;
    HIP_TRY(hipMemsetAsync(B.queue, 0, sizeof(unsigned int), stream));
    if (co.coop) {
        if (int rc = batch_coop_begin(s, stream)) return rc;
        HIP_TRY(rtmi_batch_coop_launch_gather(co.ext, m.nee, m.env, p->mode, co.blocks, co.lds, stream, s->dev, a.P, B, a.L, a.E));
        if (int rc = batch_coop_end(s, stream)) return rc;
    } else
    HIP_TRY(rtmi_gather_launch(fast, m.nee, m.env, p->mode, ch.blocks, stream, s->dev, a.P, B, a.L, a.E));
    if (d_value || d_stderr || d_sh) HIP_TRY(rtmi_gather_launch_resolve(p->mode, stream, a.P.samples, B, a.P.key0, a.P.key1));
    return RTMI_OK;
}
extern "C" int rtmi_gather(rtmi_scene *s, const rtmi_gather_params *p, const float *points, const float *normals, const float *time,
                           float *out_value, float *out_stderr, float *out_sh, double *kernel_ms) {
    const char *name = "rtmi_gather";
    int rc;
    if ((rc = gather_check(name, p, points, normals, out_value || out_stderr || out_sh, out_sh != nullptr, "every output is NULL")))
        return rc;
    if (kernel_ms) *kernel_ms = 0.0;
    if (p->n && (rc = gather_check_points(name, p, points, normals, time))) return rc;
    const std::string null_scene = std::string(name) + ": scene is NULL";
    const Estimator m = estimator_of(name, p->estimator, p->env_select_p, null_scene.c_str());
    if (!s) return fail(RTMI_ERR_INVALID, null_scene);
    if (p->n == 0u) return RTMI_OK;
    RenderCall c;
    if ((rc = begin_call(c, m, s)) || (rc = batch_blocking_begin(s))) return rc;
    hipStream_t stream = s->stream.s;
    const bool cosine = p->mode == RTMI_GATHER_COSINE;
    const uint32_t slab = gather_slab(p, p->slab_points ? p->slab_points : (256ull << 20) / (12ull * p->spp));
    const size_t cap = slab < p->n ? slab : p->n; // points of the largest slab
    // a slab's records go through the query buffers: points | normals in q_rays, times in q_time; its outputs through rad_out
    if ((rc = grow(s, s->q_rays, cap * 6 * sizeof(float))) ||
        (time && (rc = grow(s, s->q_time, cap * sizeof(float)))) ||
        (rc = grow(s, s->rad_samples, cap * p->spp * sizeof(Rad3))) ||
        (rc = grow(s, s->rad_out, cap * 33 * sizeof(float))))
        return rc;
    float *d_points = reinterpret_cast<float *>(s->q_rays.ptr), *d_normals = d_points + cap * 3;
    float *d_value = s->rad_out.ptr, *d_stderr = s->rad_out.ptr + cap * 3, *d_sh = s->rad_out.ptr + cap * 6;
    for (uint64_t at = 0; at < p->n; at += slab) {
        const size_t cnt = p->n - at < slab ? (size_t)(p->n - at) : slab;
        HIP_TRY(hipMemcpyAsync(d_points, points + 3 * at, cnt * 3 * sizeof(float), hipMemcpyHostToDevice, stream));
        if (cosine) HIP_TRY(hipMemcpyAsync(d_normals, normals + 3 * at, cnt * 3 * sizeof(float), hipMemcpyHostToDevice, stream));
        if (time) HIP_TRY(hipMemcpyAsync(s->q_time.ptr, time + at, cnt * sizeof(float), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipEventRecord(s->ev[0].e, stream));
        if ((rc = gather_enqueue(s, m, p, stream, (uint32_t)at, (uint32_t)cnt, d_points, d_normals, time ? s->q_time.ptr : nullptr,
                                 out_value ? d_value : nullptr, out_stderr ? d_stderr : nullptr, out_sh ? d_sh : nullptr, s->rad_samples.ptr)))
            return rc;
        HIP_TRY(hipEventRecord(s->ev[1].e, stream));
        if (out_value) HIP_TRY(hipMemcpyAsync(out_value + 3 * at, d_value, cnt * 3 * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (out_stderr) HIP_TRY(hipMemcpyAsync(out_stderr + 3 * at, d_stderr, cnt * 3 * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (out_sh) HIP_TRY(hipMemcpyAsync(out_sh + 27 * at, d_sh, cnt * 27 * sizeof(float), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (kernel_ms) {
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, s->ev[0].e, s->ev[1].e));
            *kernel_ms += (double)ms;
        }
    }
    return batch_coop_check(s);
}
extern "C" int rtmi_gather_device(rtmi_scene *s, const rtmi_gather_params *p, const void *d_points, const void *d_normals,
                                  const void *d_time, void *d_value, void *d_stderr, void *d_sh, void *d_scratch,
                                  uint64_t scratch_bytes, void *stream_) {
    const char *name = "rtmi_gather_device";
    if (int rc = gather_check(name, p, d_points, d_normals, d_value || d_stderr || d_sh, d_sh != nullptr, "every output is NULL")) return rc;
    if (p->n && (!d_scratch || scratch_bytes < 12ull * p->spp))
        return fail(RTMI_ERR_INVALID, std::string(name) + ": d_scratch must hold one point's samples, scratch_bytes >= 12 * spp");
    const std::string null_scene = std::string(name) + ": scene is NULL";
    const Estimator m = estimator_of(name, p->estimator, p->env_select_p, null_scene.c_str());
    if (!s) return fail(RTMI_ERR_INVALID, null_scene);
    if (p->n == 0u) return RTMI_OK;
    AsyncCall c;
    if (int rc = c.begin(m, s, stream_)) return rc;
    s->batch_blocking = false;
    const uint64_t fits = scratch_bytes / (12ull * p->spp);
    const uint32_t slab = gather_slab(p, p->slab_points && p->slab_points < fits ? p->slab_points : fits);
    const char *pts = reinterpret_cast<const char *>(d_points), *nrm = reinterpret_cast<const char *>(d_normals);
    const char *tm = reinterpret_cast<const char *>(d_time);
    char *val = reinterpret_cast<char *>(d_value), *se = reinterpret_cast<char *>(d_stderr), *sh = reinterpret_cast<char *>(d_sh);
    for (uint64_t at = 0; at < p->n; at += slab) {
        const uint32_t cnt = p->n - at < slab ? (uint32_t)(p->n - at) : slab;
        if (int rc = gather_enqueue(s, m, p, c.stream, (uint32_t)at, cnt, pts + 12 * at, nrm ? nrm + 12 * at : nullptr,
                                    tm ? tm + 4 * at : nullptr, val ? val + 12 * at : nullptr, se ? se + 12 * at : nullptr,
                                    sh ? sh + 108 * at : nullptr, d_scratch))
            return rc;
    }
    return RTMI_OK;
}

// ---- sparse renders (include/rtmi_sparse.h) ---------------------------------------------------------------------------------
#define RTMI_SPARSE_MAX_PIXELS (32768ull * 32768ull)
// the caller's scratch, in bytes from its start: control words | per-workgroup counts | list | mean | stderr | samples
struct SparseScratch {
    uint64_t counts, list, mean, se, samples, total;
};
static SparseScratch sparse_scratch(uint64_t n_pixels, uint32_t capacity, uint32_t ns) {
    const auto up16 = [](uint64_t b) { return (b + 15ull) & ~15ull; };
    SparseScratch L;
    L.counts = 4ull * RTMI_SPARSE_HEAD_WORDS;
    L.list = L.counts + up16(4ull * ((n_pixels + RTMI_SPARSE_SPAN - 1ull) / RTMI_SPARSE_SPAN));
    L.mean = L.list + up16(4ull * capacity);
    L.se = L.mean + up16(12ull * capacity);
    L.samples = L.se + up16(12ull * capacity);
    L.total = L.samples + up16(12ull * capacity * ns);
    return L;
}
extern "C" uint64_t rtmi_sparse_scratch_bytes(uint64_t n_pixels, uint32_t capacity, uint32_t ns) {
    return sparse_scratch(n_pixels, capacity, ns).total;
}
// the end of the stateless entries' checks (select, patch, the step probe): the device
static int use_device(const std::string &nm, int device) {
    if (int rc = device_ok(nm, device)) return rc;
    HIP_TRY(hipSetDevice(device));
    return RTMI_OK;
}
extern "C" int rtmi_sparse_select_device(int device, uint32_t n, const void *d_bytes, uint32_t accept_mask, uint32_t capacity,
                                         void *d_list, void *d_count, void *d_scratch, void *stream) {
    const std::string nm = "rtmi_sparse_select_device: ";
    if (!d_bytes || !d_list || !d_count || !d_scratch) return fail(RTMI_ERR_INVALID, nm + "NULL argument");
    if (n == 0u || n > RTMI_SPARSE_MAX_PIXELS) return fail(RTMI_ERR_INVALID, nm + "n must be in 1 .. 32768^2");
    if (capacity == 0u) return fail(RTMI_ERR_INVALID, nm + "capacity must be at least 1");
    if (misaligned(d_list, 4) || misaligned(d_count, 4) || misaligned(d_scratch, 16))
        return fail(RTMI_ERR_INVALID, nm + "misaligned list, count (4 bytes) or scratch (16 bytes)");
    if (int rc = use_device(nm, device)) return rc;
    uint32_t *scratch = reinterpret_cast<uint32_t *>(d_scratch);
    HIP_TRY(rtmi_sparse_launch_select(reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const uint8_t *>(d_bytes), n, accept_mask,
                                      capacity, reinterpret_cast<uint32_t *>(d_list), reinterpret_cast<uint32_t *>(d_count),
                                      scratch + RTMI_SPARSE_HEAD_WORDS));
    return RTMI_OK;
}
extern "C" int rtmi_sparse_patch_device(int device, uint32_t n_pixels, const void *d_list, const void *d_count, uint32_t capacity,
                                        const void *d_mean, void *d_linear, void *d_rgb8, void *d_bytes, uint32_t mark, void *stream) {
    const std::string nm = "rtmi_sparse_patch_device: ";
    if (!d_list || !d_mean) return fail(RTMI_ERR_INVALID, nm + "NULL argument");
    if (!d_linear && !d_rgb8 && !d_bytes) return fail(RTMI_ERR_INVALID, nm + "every plane is NULL");
    if (n_pixels == 0u || n_pixels > RTMI_SPARSE_MAX_PIXELS) return fail(RTMI_ERR_INVALID, nm + "n_pixels must be in 1 .. 32768^2");
    if (capacity == 0u) return fail(RTMI_ERR_INVALID, nm + "capacity must be at least 1");
    if (mark > 255u) return fail(RTMI_ERR_INVALID, nm + "mark must be a byte");
    if (misaligned(d_list, 4) || misaligned(d_count, 4) || misaligned(d_mean, 4) || misaligned(d_linear, 4))
        return fail(RTMI_ERR_INVALID, nm + "misaligned list, count, mean or linear (4 bytes)");
    if (int rc = use_device(nm, device)) return rc;
    HIP_TRY(rtmi_sparse_launch_patch(reinterpret_cast<hipStream_t>(stream), n_pixels, reinterpret_cast<const uint32_t *>(d_list),
                                     reinterpret_cast<const uint32_t *>(d_count), capacity, reinterpret_cast<const float *>(d_mean),
                                     nullptr, reinterpret_cast<float *>(d_linear), reinterpret_cast<uint8_t *>(d_rgb8), nullptr,
                                     reinterpret_cast<uint8_t *>(d_bytes), mark));
    return RTMI_OK;
}
// The checks the render and refine entries share, in this order: the pointers, the outputs, the values, what the estimator
// needs attached (of a handle that is there), the reserved words, the flags.  The entry's own checks and the NULL handle
// follow in the entries, so everything here is answered for a NULL handle too.
static int sparse_check(const char *name, const rtmi_scene *s_in, const rtmi_render_params *p, const rtmi_camera *cam,
                        const rtmi_sparse_params *sp, const void *pixels, const char *pixels_msg, bool has_out, const char *out_msg) {
    const std::string nm = std::string(name) + ": ";
    if (!p || !cam || !sp) return fail(RTMI_ERR_INVALID, nm + "NULL argument (params, cam or sp)");
    if (!pixels) return fail(RTMI_ERR_INVALID, nm + pixels_msg);
    if (!has_out) return fail(RTMI_ERR_INVALID, nm + out_msg);
    if (sp->ns == 0u) return fail(RTMI_ERR_INVALID, nm + "ns must be at least 1");
    if (p->max_depth == 0u) return fail(RTMI_ERR_INVALID, nm + "max_depth must be at least 1");
    if (int rc = check_estimator(name, sp->estimator)) return rc;
    if ((uint64_t)sp->first_sample + sp->ns > (1ull << 32))
        return fail(RTMI_ERR_INVALID, nm + "first_sample + ns must not exceed 2^32 (a sample index would wrap onto another sample's stream)");
    if ((uint64_t)sp->n * sp->ns >= (1ull << 31)) return fail(RTMI_ERR_INVALID, nm + "n * ns must be below 2^31");
    if (int rc = check_estimator_opts(name, sp->estimator, sp->env_select_p, p->flags)) return rc;
    if (p->nx == 0u || p->ny == 0u || (uint64_t)p->nx * p->ny > 0xffffffffull)
        return fail(RTMI_ERR_INVALID, nm + "the image must have 1 .. 2^32 - 1 pixels");
    if (!std::isfinite(p->t_min)) return fail(RTMI_ERR_INVALID, nm + "t_min must be finite");
    if (int rc = check_attached_early(estimator_of(name, sp->estimator, sp->env_select_p, ""), s_in)) return rc;
    if (sp->reserved[0] || sp->reserved[1] || sp->reserved[2]) return fail(RTMI_ERR_INVALID, nm + "reserved words must be zero");
    if (p->flags & ~(RTMI_RADIANCE_FLAGS | batch_coop_bits(p->flags)))
        return fail(RTMI_ERR_UNSUPPORTED, nm + "sparse renders accept the flags FAST_CULL, SKY, FACE_FORWARD and UV_BOOK only");
    return RTMI_OK;
}
// The launches of a list on `stream`: the path kernel on the persistent grid of the per-lane render kernels, sized for the
// capacity sp->n and fed by `queue` (zeroed here, on the call's stream), then the resolve.  The kernels read the count.
static int sparse_enqueue(rtmi_scene *s, const Estimator &m, const rtmi_render_params *p, const rtmi_camera *cam,
                          const rtmi_sparse_params *sp, hipStream_t stream, const void *d_pixels, const void *d_count, void *d_mean,
                          void *d_stderr, void *d_samples, unsigned int *queue) {
    BatchArgs a = batch_args(s, m, *p, d_samples); // the image's nx, ny, seed, max_depth, t_min and flags
    const DevCamera C = dev_camera(cam);
    SparseBatch B{};
    B.list = reinterpret_cast<const uint32_t *>(d_pixels);
    B.count = reinterpret_cast<const uint32_t *>(d_count);
    B.mean = reinterpret_cast<float *>(d_mean);
    B.stderr_out = reinterpret_cast<float *>(d_stderr);
    B.queue = queue;
    B.n = sp->n; B.ns = sp->ns; B.first_sample = sp->first_sample;
    const BatchChunks ch = batch_chunks(s, sp->n * sp->ns); // for a full list: the kernel counts the chunks of the entries there are
    B.chunk = ch.chunk;
    const bool fast = (p->flags & RTMI_FLAG_FAST_CULL) != 0u && boxes_valid(s, cam);
    BatchCoop co;
    if (int rc = plan_batch_coop(s, m, p->flags, fast, ch, a.P, co)) return rc;
    s->last_batch_kernel = co.coop ? RTMI_KERNEL_WAVE_COOP : RTMI_KERNEL_PERLANE;
    HIP_TRY(hipMemsetAsync(queue, 0, sizeof(unsigned int), stream));
    if (co.coop) {
        if (int rc = batch_coop_begin(s, stream)) return rc;
        HIP_TRY(rtmi_batch_coop_launch_sparse(co.ext, m.nee, m.env, co.blocks, co.lds, stream, s->dev, C, a.P, B, a.L, a.E));
        if (int rc = batch_coop_end(s, stream)) return rc;
    } else
    HIP_TRY(rtmi_sparse_launch(fast, m.nee, m.env, ch.blocks, stream, s->dev, C, a.P, B, a.L, a.E));
    if (d_mean || d_stderr) HIP_TRY(rtmi_sparse_launch_resolve(stream, a.P.samples, B));
    return RTMI_OK;
}
extern "C" int rtmi_sparse_render(rtmi_scene *s, const rtmi_render_params *p, const rtmi_camera *cam, const rtmi_sparse_params *sp,
                                  const uint32_t *pixels, float *out_mean, float *out_stderr, float *out_samples, double *kernel_ms) {
    const char *name = "rtmi_sparse_render";
    int rc;
    if ((rc = sparse_check(name, s, p, cam, sp, pixels, "pixels is NULL", out_mean || out_stderr || out_samples, "every output is NULL")))
        return rc;
    if (kernel_ms) *kernel_ms = 0.0;
    const uint32_t npix = p->nx * p->ny;
    for (uint32_t k = 0; k < sp->n; k++)
        if (pixels[k] >= npix)
            return fail(RTMI_ERR_INVALID, std::string(name) + ": pixels[" + std::to_string(k) + "] = " + std::to_string(pixels[k]) +
                                              " is outside the image");
    const std::string null_scene = std::string(name) + ": scene is NULL";
    const Estimator m = estimator_of(name, sp->estimator, sp->env_select_p, null_scene.c_str());
    if (!s) return fail(RTMI_ERR_INVALID, null_scene);
    if (sp->n == 0u) return RTMI_OK;
    RenderCall c;
    if ((rc = begin_call(c, m, s)) || (rc = batch_blocking_begin(s))) return rc;
    hipStream_t stream = s->stream.s;
    const size_t n = sp->n, ns = n * sp->ns;
    if ((rc = grow(s, s->q_time, n * sizeof(uint32_t))) || (rc = batch_reserve(s, n, ns))) return rc;
    float *d_mean = s->rad_out.ptr, *d_stderr = s->rad_out.ptr + n * 3;
    HIP_TRY(hipMemcpyAsync(s->q_time.ptr, pixels, n * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(s->ev[0].e, stream));
    if ((rc = sparse_enqueue(s, m, p, cam, sp, stream, s->q_time.ptr, nullptr, out_mean ? d_mean : nullptr, out_stderr ? d_stderr : nullptr,
                             s->rad_samples.ptr, s->status.ptr + RTMI_STATUS_WORDS)))
        return rc;
    HIP_TRY(hipEventRecord(s->ev[1].e, stream));
    if ((rc = batch_finish(s, n, ns, out_mean, out_stderr, out_samples, kernel_ms))) return rc;
    return batch_coop_check(s);
}
extern "C" int rtmi_sparse_render_device(rtmi_scene *s, const rtmi_render_params *p, const rtmi_camera *cam, const rtmi_sparse_params *sp,
                                         const void *d_pixels, const void *d_count, void *d_mean, void *d_stderr, void *d_samples,
                                         void *d_scratch, void *stream_) {
    const char *name = "rtmi_sparse_render_device";
    if (int rc = sparse_check(name, s, p, cam, sp, d_pixels, "d_pixels is NULL", d_samples != nullptr,
                              "d_samples is NULL (the kernel's per-sample buffer)"))
        return rc;
    if (!d_scratch) return fail(RTMI_ERR_INVALID, std::string(name) + ": d_scratch is NULL");
    if (misaligned(d_pixels, 4) || misaligned(d_count, 4) || misaligned(d_mean, 4) || misaligned(d_stderr, 4) ||
        misaligned(d_samples, 4) || misaligned(d_scratch, 4))
        return fail(RTMI_ERR_INVALID, std::string(name) + ": misaligned pointer (4 bytes)");
    const std::string null_scene = std::string(name) + ": scene is NULL";
    const Estimator m = estimator_of(name, sp->estimator, sp->env_select_p, null_scene.c_str());
    if (!s) return fail(RTMI_ERR_INVALID, null_scene);
    if (sp->n == 0u) return RTMI_OK;
    AsyncCall c;
    if (int rc = c.begin(m, s, stream_)) return rc;
    s->batch_blocking = false;
    return sparse_enqueue(s, m, p, cam, sp, c.stream, d_pixels, d_count, d_mean, d_stderr, d_samples,
                          reinterpret_cast<unsigned int *>(d_scratch) + RTMI_SPARSE_QUEUE_WORD);
}
// the refine entries' own checks, after sparse_check: the planes, the scratch, the mark
static int sparse_refine_check(const char *name, const rtmi_render_params *p, const rtmi_sparse_params *sp, uint32_t mark,
                               bool device_form, const void *bytes, const void *linear, const void *se, const void *scratch,
                               uint64_t scratch_bytes, const void *count_out) {
    const std::string nm = std::string(name) + ": ";
    const uint64_t npix = (uint64_t)p->nx * p->ny;
    if (npix > RTMI_SPARSE_MAX_PIXELS) return fail(RTMI_ERR_INVALID, nm + "the image must have at most 32768^2 pixels");
    if (sp->n == 0u) return fail(RTMI_ERR_INVALID, nm + "sp->n, the budget of pixels, must be at least 1");
    if (mark > 255u) return fail(RTMI_ERR_INVALID, nm + "mark must be a byte");
    if (!device_form) return RTMI_OK;
    if (!scratch) return fail(RTMI_ERR_INVALID, nm + "d_scratch is NULL");
    if (misaligned(linear, 4) || misaligned(se, 4) || misaligned(count_out, 4) || misaligned(scratch, 16))
        return fail(RTMI_ERR_INVALID, nm + "misaligned linear, stderr, count (4 bytes) or scratch (16 bytes)");
    if (scratch_bytes < sparse_scratch(npix, sp->n, sp->ns).total)
        return fail(RTMI_ERR_INVALID, nm + "scratch_bytes is below rtmi_sparse_scratch_bytes(nx * ny, sp->n, sp->ns)");
    (void)bytes;
    return RTMI_OK;
}
// select -> sparse render -> patch on `stream`; the list, the counts and the records live in the scratch
static int sparse_refine_enqueue(rtmi_scene *s, const Estimator &m, const rtmi_render_params *p, const rtmi_camera *cam,
                                 const rtmi_sparse_params *sp, uint32_t accept_mask, uint32_t mark, hipStream_t stream, void *d_bytes,
                                 void *d_linear, void *d_rgb8, void *d_stderr, void *d_scratch, void *d_count_out) {
    const uint32_t npix = p->nx * p->ny;
    const SparseScratch L = sparse_scratch(npix, sp->n, sp->ns);
    char *base = reinterpret_cast<char *>(d_scratch);
    uint32_t *head = reinterpret_cast<uint32_t *>(base), *count = head + RTMI_SPARSE_COUNT_WORD;
    uint32_t *list = reinterpret_cast<uint32_t *>(base + L.list);
    float *mean = reinterpret_cast<float *>(base + L.mean), *se = reinterpret_cast<float *>(base + L.se);
    HIP_TRY(rtmi_sparse_launch_select(stream, reinterpret_cast<const uint8_t *>(d_bytes), npix, accept_mask, sp->n, list, count,
                                      reinterpret_cast<uint32_t *>(base + L.counts)));
    if (int rc = sparse_enqueue(s, m, p, cam, sp, stream, list, count, mean, se, base + L.samples, head + RTMI_SPARSE_QUEUE_WORD)) return rc;
    HIP_TRY(rtmi_sparse_launch_patch(stream, npix, list, count, sp->n, mean, se, reinterpret_cast<float *>(d_linear),
                                     reinterpret_cast<uint8_t *>(d_rgb8), reinterpret_cast<float *>(d_stderr),
                                     reinterpret_cast<uint8_t *>(d_bytes), mark));
    if (d_count_out) HIP_TRY(hipMemcpyAsync(d_count_out, count, 2 * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    return RTMI_OK;
}
extern "C" int rtmi_sparse_refine_device(rtmi_scene *s, const rtmi_render_params *p, const rtmi_camera *cam, const rtmi_sparse_params *sp,
                                         uint32_t accept_mask, uint32_t mark, void *d_bytes, void *d_linear, void *d_rgb8, void *d_stderr,
                                         void *d_scratch, uint64_t scratch_bytes, void *d_count_out, void *stream_) {
    const char *name = "rtmi_sparse_refine_device";
    int rc;
    if ((rc = sparse_check(name, s, p, cam, sp, d_bytes, "d_bytes is NULL", true, "")) ||
        (rc = sparse_refine_check(name, p, sp, mark, true, d_bytes, d_linear, d_stderr, d_scratch, scratch_bytes, d_count_out)))
        return rc;
    const std::string null_scene = std::string(name) + ": scene is NULL";
    const Estimator m = estimator_of(name, sp->estimator, sp->env_select_p, null_scene.c_str());
    if (!s) return fail(RTMI_ERR_INVALID, null_scene);
    AsyncCall c;
    if ((rc = c.begin(m, s, stream_))) return rc;
    s->batch_blocking = false;
    return sparse_refine_enqueue(s, m, p, cam, sp, accept_mask, mark, c.stream, d_bytes, d_linear, d_rgb8, d_stderr, d_scratch, d_count_out);
}
extern "C" int rtmi_sparse_refine(rtmi_scene *s, const rtmi_render_params *p, const rtmi_camera *cam, const rtmi_sparse_params *sp,
                                  uint32_t accept_mask, uint32_t mark, uint8_t *bytes, float *linear, uint8_t *rgb8, float *stderr_rgb,
                                  uint32_t *counts) {
    const char *name = "rtmi_sparse_refine";
    int rc;
    if ((rc = sparse_check(name, s, p, cam, sp, bytes, "bytes is NULL", true, "")) ||
        (rc = sparse_refine_check(name, p, sp, mark, false, bytes, linear, stderr_rgb, nullptr, 0, counts)))
        return rc;
    const std::string null_scene = std::string(name) + ": scene is NULL";
    const Estimator m = estimator_of(name, sp->estimator, sp->env_select_p, null_scene.c_str());
    RenderCall c;
    if ((rc = begin_call(c, m, s)) || (rc = batch_blocking_begin(s))) return rc;
    hipStream_t stream = s->stream.s;
    // one allocation per call: bytes | scratch | linear | stderr | rgb8
    const size_t npix = (size_t)p->nx * p->ny;
    char *d_bytes, *d_scratch, *d_linear, *d_se, *d_rgb8;
    const auto layout = [&](Carve16 &c) {
        d_bytes = c.take<char>(npix); d_scratch = c.take<char>((size_t)sparse_scratch(npix, sp->n, sp->ns).total);
        d_linear = c.take<char>(npix * 12); d_se = c.take<char>(npix * 12); d_rgb8 = c.take<char>(npix * 3);
    };
    DeviceArena mem;
    HIP_TRY(mem.alloc<16>(layout));
    HIP_TRY(hipMemcpyAsync(d_bytes, bytes, npix, hipMemcpyHostToDevice, stream));
    if (linear) HIP_TRY(hipMemcpyAsync(d_linear, linear, npix * 12, hipMemcpyHostToDevice, stream));
    if (stderr_rgb) HIP_TRY(hipMemcpyAsync(d_se, stderr_rgb, npix * 12, hipMemcpyHostToDevice, stream));
    if (rgb8) HIP_TRY(hipMemcpyAsync(d_rgb8, rgb8, npix * 3, hipMemcpyHostToDevice, stream));
    if ((rc = sparse_refine_enqueue(s, m, p, cam, sp, accept_mask, mark, stream, d_bytes, linear ? d_linear : nullptr,
                                    rgb8 ? d_rgb8 : nullptr, stderr_rgb ? d_se : nullptr, d_scratch, nullptr))) {
        (void)hipStreamSynchronize(stream);
        return rc;
    }
    hipError_t e = hipMemcpyAsync(bytes, d_bytes, npix, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess && linear) e = hipMemcpyAsync(linear, d_linear, npix * 12, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess && stderr_rgb) e = hipMemcpyAsync(stderr_rgb, d_se, npix * 12, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess && rgb8) e = hipMemcpyAsync(rgb8, d_rgb8, npix * 3, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess && counts)
        e = hipMemcpyAsync(counts, d_scratch + 4 * RTMI_SPARSE_COUNT_WORD, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    const hipError_t e2 = hipStreamSynchronize(stream); // before the allocation is freed, whatever was enqueued
    HIP_TRY(e);
    HIP_TRY(e2);
    return batch_coop_check(s);
}

// ---- per-pixel adaptive sampling (include/rtmi_pixelwise.h) -----------------------------------------------------------------
// The options of both headers' entries (rtmi_pixelwise_opts, rtmi_window_opts of include/rtmi_window.h) in one form: the
// checks and the loop below serve both.  windowed: the scratch ends with the fail plane, and the texts name that header.
struct PixelwiseForm {
    uint32_t min_spp, step_spp, estimator, pass_spp;
    double abs_tol, rel_tol;
    float env_select_p;
    uint32_t radius; // 0: each pixel alone, the launch sequence of rtmi_pixelwise.h
    bool reserved_set, windowed;
};
static PixelwiseForm pixelwise_form(const rtmi_pixelwise_opts *o) {
    return PixelwiseForm{o->min_spp, o->step_spp, o->estimator, o->pass_spp, o->abs_tol, o->rel_tol, o->env_select_p, 0u,
                         (o->reserved[0] | o->reserved[1] | o->reserved[2]) != 0u, false};
}
static PixelwiseForm pixelwise_form(const rtmi_window_opts *o) {
    return PixelwiseForm{o->min_spp, o->step_spp, o->estimator, o->pass_spp, o->abs_tol, o->rel_tol, o->env_select_p, o->radius,
                         (o->reserved[0] | o->reserved[1]) != 0u, true};
}
// the caller's scratch, in bytes from its start: control words | count slots | per-workgroup counts of the select |
// active bytes | list | state | samples, and with `windowed` | fail bytes
struct PixelwiseScratch {
    uint64_t counts, block_counts, active, list, state, samples, fail, total;
};
static PixelwiseScratch pixelwise_scratch(uint64_t n_pixels, uint32_t pass, uint32_t steps, bool windowed = false) {
    const auto up16 = [](uint64_t b) { return (b + 15ull) & ~15ull; };
    PixelwiseScratch L;
    L.counts = 4ull * RTMI_SPARSE_HEAD_WORDS;
    L.block_counts = L.counts + up16(8ull * steps);
    L.active = L.block_counts + up16(4ull * ((n_pixels + RTMI_SPARSE_SPAN - 1ull) / RTMI_SPARSE_SPAN));
    L.list = L.active + up16(n_pixels);
    L.state = L.list + up16(4ull * n_pixels);
    L.samples = L.state + up16(72ull * n_pixels);
    L.fail = L.samples + up16(12ull * n_pixels * pass);
    L.total = windowed ? L.fail + up16(n_pixels) : L.fail;
    return L;
}
extern "C" uint64_t rtmi_pixelwise_scratch_bytes(uint64_t n_pixels, uint32_t pass_spp, uint32_t steps) {
    return pixelwise_scratch(n_pixels, pass_spp, steps).total;
}
extern "C" uint32_t rtmi_pixelwise_steps(uint32_t ns, uint32_t min_spp, uint32_t step_spp) {
    if (min_spp < 2u || min_spp > ns || step_spp == 0u) return 0u;
    return 1u + (uint32_t)(((uint64_t)(ns - min_spp) + step_spp - 1ull) / step_spp);
}
// the most samples of one launch: a whole step (the first, or a later one, which the cap may shorten) or pass_spp
static uint32_t pixelwise_pass(const rtmi_render_params *p, const PixelwiseForm *o) {
    const uint32_t rest = p->ns - o->min_spp, later = o->step_spp < rest ? o->step_spp : rest;
    const uint32_t step = o->min_spp > later ? o->min_spp : later;
    return o->pass_spp == 0u || o->pass_spp > step ? step : o->pass_spp;
}
// The checks of both render forms, in the order of sparse_check (pointers, outputs, values, attachments of a handle that is
// there, flags), then this header's own: the steps and tolerances, the size of a launch, the number of steps, the scratch and
// the alignments (device form), the reserved words.  The NULL handle follows in the entries.
struct PixelwisePlanes {
    void *linear, *rgb8, *se, *spp, *counts;
};
static int pixelwise_check(const char *name, const rtmi_scene *s_in, const rtmi_render_params *p, const rtmi_camera *cam,
                           const PixelwiseForm *o, const PixelwisePlanes &out, bool device_form, const void *scratch,
                           uint64_t scratch_bytes) {
    const std::string nm = std::string(name) + ": ";
    if (!p || !cam || !o) return fail(RTMI_ERR_INVALID, nm + "NULL argument (params, cam or opts)");
    if (!out.linear && !out.rgb8 && !out.se && !out.spp) return fail(RTMI_ERR_INVALID, nm + "every plane is NULL");
    if (p->ns == 0u) return fail(RTMI_ERR_INVALID, nm + "ns, the cap, must be at least 1");
    if (p->max_depth == 0u) return fail(RTMI_ERR_INVALID, nm + "max_depth must be at least 1");
    int rc;
    if ((rc = check_estimator(name, o->estimator)) || (rc = check_estimator_opts(name, o->estimator, o->env_select_p, p->flags))) return rc;
    const uint64_t npix = (uint64_t)p->nx * p->ny;
    if (npix == 0u || npix > RTMI_SPARSE_MAX_PIXELS) return fail(RTMI_ERR_INVALID, nm + "the image must have 1 .. 32768^2 pixels");
    if (!std::isfinite(p->t_min)) return fail(RTMI_ERR_INVALID, nm + "t_min must be finite");
    if ((rc = check_attached_early(estimator_of(name, o->estimator, o->env_select_p, ""), s_in))) return rc;
    if (p->flags & ~(RTMI_RADIANCE_FLAGS | batch_coop_bits(p->flags)))
        return fail(RTMI_ERR_UNSUPPORTED, nm + (o->windowed ? "windowed" : "per-pixel") +
                                              " adaptive sampling accepts the flags FAST_CULL, SKY, FACE_FORWARD and UV_BOOK only");
    const rtmi_adaptive a{o->min_spp, o->step_spp, o->abs_tol, o->rel_tol};
    if ((rc = check_adaptive(p, &a))) { const std::string why(rtmi_last_error()); return fail(rc, nm + why); }
    if (o->radius > RTMI_WINDOW_MAX_RADIUS) return fail(RTMI_ERR_INVALID, nm + "radius must not exceed RTMI_WINDOW_MAX_RADIUS (16)");
    const uint32_t pass = pixelwise_pass(p, o);
    if (npix * pass >= (1ull << 31)) return fail(RTMI_ERR_INVALID, nm + "nx * ny * (samples of a launch) must be below 2^31: lower pass_spp");
    const uint32_t steps = rtmi_pixelwise_steps(p->ns, o->min_spp, o->step_spp);
    if (steps > RTMI_PIXELWISE_MAX_STEPS) return fail(RTMI_ERR_INVALID, nm + "more than 1024 steps");
    if (device_form) {
        if (!scratch) return fail(RTMI_ERR_INVALID, nm + "d_scratch is NULL");
        if (scratch_bytes < pixelwise_scratch(npix, pass, steps, o->windowed).total)
            return fail(RTMI_ERR_INVALID, nm + "scratch_bytes is below " + (o->windowed ? "rtmi_window" : "rtmi_pixelwise") +
                                              "_scratch_bytes(nx * ny, pass, steps)");
        if (misaligned(out.linear, 4) || misaligned(out.se, 4) || misaligned(out.spp, 4) ||
            misaligned(out.counts, 4) || misaligned(scratch, 16))
            return fail(RTMI_ERR_INVALID, nm + "misaligned linear, stderr, spp, counts (4 bytes) or scratch (16 bytes)");
    }
    if (o->reserved_set) return fail(RTMI_ERR_INVALID, nm + "reserved words must be zero");
    return RTMI_OK;
}
// Every step on `stream`: select the active pixels into the list (counts to the step's slot), then per sub-pass the path
// kernel over the list from sample n_done on and the step kernel; the last sub-pass of a step decides.  h_count (blocking
// form): pinned, the step's count is read after its select and the loop ends at the first empty step; *paths: the paths traced.
// With a radius (include/rtmi_window.h) the deciding launch writes the fail plane instead and one spread follows it: a pixel
// stays active while a pixel of its window fails.
static int pixelwise_enqueue(rtmi_scene *s, const Estimator &m, const rtmi_render_params *p, const rtmi_camera *cam,
                             const PixelwiseForm *o, hipStream_t stream, const PixelwisePlanes &out, char *base,
                             uint32_t *h_count, uint64_t *paths) {
    const uint32_t npix = p->nx * p->ny, pass = pixelwise_pass(p, o), steps = rtmi_pixelwise_steps(p->ns, o->min_spp, o->step_spp);
    const PixelwiseScratch L = pixelwise_scratch(npix, pass, steps, o->windowed);
    uint32_t *head = reinterpret_cast<uint32_t *>(base), *slots = reinterpret_cast<uint32_t *>(base + L.counts);
    uint32_t *block_counts = reinterpret_cast<uint32_t *>(base + L.block_counts), *list = reinterpret_cast<uint32_t *>(base + L.list);
    uint8_t *active = reinterpret_cast<uint8_t *>(base + L.active), *failing = reinterpret_cast<uint8_t *>(base + L.fail);
    HIP_TRY(hipMemsetAsync(active, 1, npix, stream));
    HIP_TRY(hipMemsetAsync(slots, 0, 8ull * steps, stream)); // a step that is never enqueued (blocking form) traced nothing
    rtmi_sparse_params sp{};
    sp.n = npix; sp.estimator = o->estimator; sp.env_select_p = o->env_select_p;
    PixelwiseStep S{};
    S.list = list;
    S.samples = reinterpret_cast<const Rad3 *>(base + L.samples);
    S.state = reinterpret_cast<double *>(base + L.state);
    S.active = o->radius ? failing : active; // step 0 traces every pixel: every fail byte is written before it is read
    S.linear = reinterpret_cast<float *>(out.linear); S.rgb8 = reinterpret_cast<uint8_t *>(out.rgb8);
    S.stderr_out = reinterpret_cast<float *>(out.se); S.spp = reinterpret_cast<uint32_t *>(out.spp);
    S.n_pixels = npix; S.capacity = npix; S.cap = p->ns;
    S.abs_tol = o->abs_tol; S.rel_tol = o->rel_tol;
    uint32_t n_done = 0u;
    for (uint32_t k = 0; k < steps; k++) {
        const uint32_t rest = p->ns - n_done, cnt = k == 0u ? o->min_spp : (o->step_spp < rest ? o->step_spp : rest);
        uint32_t *slot = slots + 2u * k;
        HIP_TRY(rtmi_sparse_launch_select(stream, active, npix, 2u /* byte 1 */, npix, list, slot, block_counts));
        if (h_count) {
            HIP_TRY(hipMemcpyAsync(h_count, slot, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (h_count[0] == 0u) break;
            *paths += (uint64_t)h_count[0] * cnt;
        }
        S.count = slot;
        for (uint32_t done = 0u; done < cnt;) {
            const uint32_t take = cnt - done < pass ? cnt - done : pass;
            sp.ns = take; sp.first_sample = n_done + done;
            if (int rc = sparse_enqueue(s, m, p, cam, &sp, stream, list, slot, nullptr, nullptr, base + L.samples, head + RTMI_SPARSE_QUEUE_WORD))
                return rc;
            done += take;
            S.n_done = sp.first_sample; S.pass = take; S.decide = done == cnt ? 1u : 0u;
            HIP_TRY(rtmi_pixelwise_launch_step(stream, S));
        }
        if (o->radius) HIP_TRY(rtmi_window_launch_spread(stream, active, failing, p->nx, p->ny, o->radius));
        n_done += cnt;
    }
    if (out.counts) HIP_TRY(hipMemcpyAsync(out.counts, slots, 8ull * steps, h_count ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream));
    return RTMI_OK;
}
// the device form and the blocking form of both headers' render entries; o: NULL for NULL opts
static int pixelwise_render_device(const char *name, rtmi_scene *s, const rtmi_render_params *p, const rtmi_camera *cam,
                                   const PixelwiseForm *o, const PixelwisePlanes &out, void *d_scratch, uint64_t scratch_bytes,
                                   void *stream_) {
    if (int rc = pixelwise_check(name, s, p, cam, o, out, true, d_scratch, scratch_bytes)) return rc;
    const std::string null_scene = std::string(name) + ": scene is NULL";
    const Estimator m = estimator_of(name, o->estimator, o->env_select_p, null_scene.c_str());
    if (!s) return fail(RTMI_ERR_INVALID, null_scene);
    AsyncCall c;
    if (int rc = c.begin(m, s, stream_)) return rc;
    s->batch_blocking = false;
    return pixelwise_enqueue(s, m, p, cam, o, c.stream, out, reinterpret_cast<char *>(d_scratch), nullptr, nullptr);
}
static int pixelwise_render_host(const char *name, rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params *p,
                                 const PixelwiseForm *o, float *out_linear, uint8_t *out_rgb8, float *out_stderr, uint32_t *out_spp,
                                 uint32_t *out_counts, rtmi_stats *stats) {
    int rc;
    if ((rc = pixelwise_check(name, s, p, cam, o, PixelwisePlanes{out_linear, out_rgb8, out_stderr, out_spp, out_counts}, false, nullptr, 0)))
        return rc;
    const std::string null_scene = std::string(name) + ": scene is NULL";
    const Estimator m = estimator_of(name, o->estimator, o->env_select_p, null_scene.c_str());
    RenderCall c;
    if ((rc = begin_call(c, m, s)) || (rc = batch_blocking_begin(s))) return rc;
    hipStream_t stream = s->stream.s;
    // the handle's memory, grow-only: scratch | linear | stderr | spp | rgb8
    const size_t npix = (size_t)p->nx * p->ny, up = (npix + 15u) & ~(size_t)15u;
    const size_t scratch_bytes =
        (size_t)pixelwise_scratch(npix, pixelwise_pass(p, o), rtmi_pixelwise_steps(p->ns, o->min_spp, o->step_spp), o->windowed).total;
    if ((rc = grow(s, s->px_mem, scratch_bytes + (12 + 12 + 4 + 3) * up))) return rc;
    HIP_TRY(s->h_ad_count.grow(64));
    char *d_linear = s->px_mem.ptr + scratch_bytes, *d_se = d_linear + 12 * up, *d_spp = d_se + 12 * up, *d_rgb8 = d_spp + 4 * up;
    const PixelwisePlanes out{out_linear ? d_linear : nullptr, out_rgb8 ? d_rgb8 : nullptr, out_stderr ? d_se : nullptr,
                              out_spp ? d_spp : nullptr, out_counts};
    uint64_t paths = 0;
    HIP_TRY(hipEventRecord(s->ev[0].e, stream));
    if ((rc = pixelwise_enqueue(s, m, p, cam, o, stream, out, s->px_mem.ptr, s->h_ad_count.ptr, &paths))) {
        (void)hipStreamSynchronize(stream);
        return rc;
    }
    HIP_TRY(hipEventRecord(s->ev[1].e, stream));
    if (out_linear) HIP_TRY(hipMemcpyAsync(out_linear, d_linear, npix * 12, hipMemcpyDeviceToHost, stream));
    if (out_stderr) HIP_TRY(hipMemcpyAsync(out_stderr, d_se, npix * 12, hipMemcpyDeviceToHost, stream));
    if (out_spp) HIP_TRY(hipMemcpyAsync(out_spp, d_spp, npix * 4, hipMemcpyDeviceToHost, stream));
    if (out_rgb8) HIP_TRY(hipMemcpyAsync(out_rgb8, d_rgb8, npix * 3, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (stats) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, s->ev[0].e, s->ev[1].e));
        *stats = rtmi_stats{};
        stats->kernel_ms = (double)ms;
        stats->samples = paths;
        stats->kernel = (uint32_t)s->last_batch_kernel; // every launch of the call selects alike
    }
    return batch_coop_check(s);
}
extern "C" int rtmi_render_pixelwise_device(rtmi_scene *s, const rtmi_render_params *p, const rtmi_camera *cam,
                                            const rtmi_pixelwise_opts *o, void *d_linear, void *d_rgb8, void *d_stderr, void *d_spp,
                                            void *d_counts, void *d_scratch, uint64_t scratch_bytes, void *stream_) {
    const PixelwiseForm f = o ? pixelwise_form(o) : PixelwiseForm{};
    return pixelwise_render_device("rtmi_render_pixelwise_device", s, p, cam, o ? &f : nullptr,
                                   PixelwisePlanes{d_linear, d_rgb8, d_stderr, d_spp, d_counts}, d_scratch, scratch_bytes, stream_);
}
extern "C" int rtmi_render_pixelwise(rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params *p, const rtmi_pixelwise_opts *o,
                                     float *out_linear, uint8_t *out_rgb8, float *out_stderr, uint32_t *out_spp, uint32_t *out_counts,
                                     rtmi_stats *stats) {
    const PixelwiseForm f = o ? pixelwise_form(o) : PixelwiseForm{};
    return pixelwise_render_host("rtmi_render_pixelwise", s, cam, p, o ? &f : nullptr, out_linear, out_rgb8, out_stderr, out_spp,
                                 out_counts, stats);
}
extern "C" int rtmi_probe_pixelwise_step(int device, uint32_t n_pixels, uint32_t capacity, const uint32_t *list, const uint32_t *count,
                                         const float *samples, double *state, uint32_t n_done, uint32_t pass, uint32_t decide,
                                         uint32_t cap, double abs_tol, double rel_tol, uint8_t *active, float *linear, uint8_t *rgb8,
                                         float *stderr_rgb, uint32_t *spp) {
    const std::string nm = "rtmi_probe_pixelwise_step: ";
    if (!list || !samples || !state) return fail(RTMI_ERR_INVALID, nm + "NULL argument (list, samples or state)");
    if (n_pixels == 0u || capacity == 0u || pass == 0u) return fail(RTMI_ERR_INVALID, nm + "n_pixels, capacity and pass must be at least 1");
    if ((uint64_t)capacity * pass >= (1ull << 31)) return fail(RTMI_ERR_INVALID, nm + "capacity * pass must be below 2^31");
    if (int rc = use_device(nm, device)) return rc;
    // one allocation, every part rounded up to 16 bytes: state | samples | list | count | linear | stderr | spp | rgb8 | active
    const size_t n = n_pixels, bytes[9] = {72 * n, 12 * (size_t)capacity * pass, 4 * (size_t)capacity, 8, 12 * n, 12 * n, 4 * n, 3 * n, n};
    void *host[9] = {state, const_cast<float *>(samples), const_cast<uint32_t *>(list), const_cast<uint32_t *>(count), linear, stderr_rgb,
                     spp, rgb8, active};
    char *d[9];
    const auto layout = [&](Carve16 &c) { for (int i = 0; i < 9; i++) d[i] = c.take<char>(bytes[i]); };
    DeviceArena mem;
    HIP_TRY(mem.alloc<16>(layout));
    for (int i = 0; i < 9; i++) {
        if (!host[i])
            d[i] = nullptr; // the kernel skips a plane that is not asked for
        else
            HIP_TRY(hipMemcpy(d[i], host[i], bytes[i], hipMemcpyHostToDevice));
    }
    PixelwiseStep S{};
    S.state = reinterpret_cast<double *>(d[0]); S.samples = reinterpret_cast<const Rad3 *>(d[1]);
    S.list = reinterpret_cast<const uint32_t *>(d[2]); S.count = reinterpret_cast<const uint32_t *>(d[3]);
    S.linear = reinterpret_cast<float *>(d[4]); S.stderr_out = reinterpret_cast<float *>(d[5]);
    S.spp = reinterpret_cast<uint32_t *>(d[6]); S.rgb8 = reinterpret_cast<uint8_t *>(d[7]); S.active = reinterpret_cast<uint8_t *>(d[8]);
    S.n_pixels = n_pixels; S.capacity = capacity; S.n_done = n_done; S.pass = pass; S.decide = decide ? 1u : 0u; S.cap = cap;
    S.abs_tol = abs_tol; S.rel_tol = rel_tol;
    HIP_TRY(rtmi_pixelwise_launch_step(nullptr, S));
    HIP_TRY(hipDeviceSynchronize());
    for (int i = 0; i < 9; i++)
        if (host[i] && i != 1 && i != 2 && i != 3) HIP_TRY(hipMemcpy(host[i], d[i], bytes[i], hipMemcpyDeviceToHost));
    return RTMI_OK;
}

// ---- windowed adaptive sampling (include/rtmi_window.h) -------------------------------------------------------------------
// The render entries are the per-pixel ones above with a radius: the same checks, the same loop, one spread launch per step.
static_assert(RTMI_WINDOW_MAX_RADIUS == RTMI_WINDOW_RADIUS_MAX, "the spread kernel's LDS is sized by the header's maximum");
static_assert(sizeof(rtmi_window_opts) == 48 && offsetof(rtmi_window_opts, radius) == 36, "rtmi_window_opts is 48 bytes");
extern "C" uint64_t rtmi_window_scratch_bytes(uint64_t n_pixels, uint32_t pass_spp, uint32_t steps) {
    return pixelwise_scratch(n_pixels, pass_spp, steps, true).total;
}
extern "C" uint32_t rtmi_window_steps(uint32_t ns, uint32_t min_spp, uint32_t step_spp) {
    return rtmi_pixelwise_steps(ns, min_spp, step_spp);
}
extern "C" int rtmi_render_window_device(rtmi_scene *s, const rtmi_render_params *p, const rtmi_camera *cam, const rtmi_window_opts *o,
                                         void *d_linear, void *d_rgb8, void *d_stderr, void *d_spp, void *d_counts, void *d_scratch,
                                         uint64_t scratch_bytes, void *stream_) {
    const PixelwiseForm f = o ? pixelwise_form(o) : PixelwiseForm{};
    return pixelwise_render_device("rtmi_render_window_device", s, p, cam, o ? &f : nullptr,
                                   PixelwisePlanes{d_linear, d_rgb8, d_stderr, d_spp, d_counts}, d_scratch, scratch_bytes, stream_);
}
extern "C" int rtmi_render_window(rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params *p, const rtmi_window_opts *o,
                                  float *out_linear, uint8_t *out_rgb8, float *out_stderr, uint32_t *out_spp, uint32_t *out_counts,
                                  rtmi_stats *stats) {
    const PixelwiseForm f = o ? pixelwise_form(o) : PixelwiseForm{};
    return pixelwise_render_host("rtmi_render_window", s, cam, p, o ? &f : nullptr, out_linear, out_rgb8, out_stderr, out_spp, out_counts,
                                 stats);
}
static int window_spread_check(const std::string &nm, const void *active, const void *failing, uint32_t nx, uint32_t ny, uint32_t radius) {
    if (!active || !failing) return fail(RTMI_ERR_INVALID, nm + "NULL argument (active or fail)");
    const uint64_t npix = (uint64_t)nx * ny;
    if (npix == 0u || npix > RTMI_SPARSE_MAX_PIXELS) return fail(RTMI_ERR_INVALID, nm + "the image must have 1 .. 32768^2 pixels");
    if (radius > RTMI_WINDOW_MAX_RADIUS) return fail(RTMI_ERR_INVALID, nm + "radius must not exceed RTMI_WINDOW_MAX_RADIUS (16)");
    return RTMI_OK;
}
extern "C" int rtmi_window_spread_device(void *d_active, const void *d_fail, uint32_t nx, uint32_t ny, uint32_t radius, void *stream) {
    if (int rc = window_spread_check("rtmi_window_spread_device: ", d_active, d_fail, nx, ny, radius)) return rc;
    HIP_TRY(rtmi_window_launch_spread(reinterpret_cast<hipStream_t>(stream), reinterpret_cast<uint8_t *>(d_active),
                                      reinterpret_cast<const uint8_t *>(d_fail), nx, ny, radius));
    return RTMI_OK;
}
extern "C" int rtmi_probe_window_spread(int device, uint32_t nx, uint32_t ny, uint32_t radius, uint8_t *active, const uint8_t *failing) {
    const std::string nm = "rtmi_probe_window_spread: ";
    if (int rc = window_spread_check(nm, active, failing, nx, ny, radius)) return rc;
    if (int rc = use_device(nm, device)) return rc;
    const size_t n = (size_t)nx * ny;
    uint8_t *d_active, *d_fail;
    const auto layout = [&](Carve16 &c) { d_active = c.take<uint8_t>(n); d_fail = c.take<uint8_t>(n); };
    DeviceArena mem;
    HIP_TRY(mem.alloc<16>(layout));
    HIP_TRY(hipMemcpy(d_active, active, n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_fail, failing, n, hipMemcpyHostToDevice));
    HIP_TRY(rtmi_window_launch_spread(nullptr, d_active, d_fail, nx, ny, radius));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(active, d_active, n, hipMemcpyDeviceToHost));
    return RTMI_OK;
}
