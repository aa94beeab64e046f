/* rtmi_radiance.h — radiance queries: path-traced radiance along batches of caller-supplied rays, on the MI355X (gfx950)
 * device path.  See DESIGN.md §24.
 *
 * The render entries answer "what does this camera see", rtmi_trace / rtmi_occluded (rtmi_query.h) "what does this ray
 * hit".  These entries answer the question between them: how much light arrives along a ray — for irradiance probes,
 * lightmap and vertex baking, final gathering, radiance-cache training data, or glossy look-ups of a host integrator.
 *
 * Semantics.  Sample s of ray i is one path of rtmi_render's integrator (or rtmi_render_nee's, rtmi_render_env's: the
 * estimator field) that starts with the caller's ray instead of a camera ray: T = 1, L = 0, depth = 0, no light sample
 * pending, so the first hit counts like a camera ray's (emitters at weight 1); scatter, media, depth limit and the
 * estimator's arithmetic are those of rtmi.h, rtmi_nee.h and rtmi_env.h in the fp32 contract.  No Russian roulette.
 *   Interval.  The ray's own (t_min, t_max) bounds the FIRST segment only (t_max = +inf or >= FLT_MAX: the render's
 *     FLT_MAX); every later segment and every shadow ray uses (params.t_min, FLT_MAX) as a render does.
 *   Random numbers.  The path of ray i, sample s is the render's path of pixel index first_ray + i and sample
 *     first_sample + s under the key `seed`: stream 0 has the Philox counter (block, first_sample + s, first_ray + i, 0)
 *     and is read from its 32-bit word stream_skip on (block stream_skip >> 2, position stream_skip & 3); stream 3, the
 *     light-sample stream of rtmi_nee.h, has the same two indices and is read from word 0.  first_ray + n <= 2^32 and
 *     first_sample + spp <= 2^32, so no index wraps onto another ray's stream.
 *   Equivalence.  A pinhole camera (lens_radius = 0) draws three words before its path starts: u, v and the shutter
 *     time.  With stream_skip = 3, the rays and times of such a camera in pixel-index order (index = j * nx + i) give
 *     that render's per-sample radiances bit for bit, however the batch is split into calls.
 *   Flags.  0, RTMI_FLAG_FAST_CULL (pruned traversal, same results; the rule of rtmi_query.h decides whether it may
 *     run), RTMI_FLAG_SKY (refused with a map, which replaces the sky), RTMI_FLAG_FACE_FORWARD, RTMI_FLAG_UV_BOOK.  Every
 *     other bit is RTMI_ERR_UNSUPPORTED.
 *   Attachments.  NEE and ENV_NEE read the light table (rtmi_scene_attach_lights), ENV and ENV_NEE the map
 *     (rtmi_scene_attach_env); without them RTMI_ERR_INVALID, as the one-shot entries answer.
 * Outputs, per ray, each optional in the host form (not all NULL):
 *   samples  n * spp * 3 floats: the fp32 radiance of every path, ray-major, then sample.
 *   mean     n * 3 floats: the f64 sum of the ray's samples in sample order, divided by spp, rounded once to float.
 *   stderr   n * 3 floats: the standard error of the mean by Welford's recurrence of rtmi_adaptive.h; spp == 1 writes
 *            +inf: no estimate, "never converged" in that header's sense.
 * The calls follow the handle's thread model (rtmi.h): calls on one handle serialise.  They allocate none of the
 * handle's render scratch.
 */
#ifndef RTMI_RADIANCE_H
#define RTMI_RADIANCE_H

#include "rtmi.h"
#include "rtmi_query.h"
#include "rtmi_roulette.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint32_t n;            /* rays in this call */
    uint32_t spp;          /* samples (independent paths) per ray, >= 1 */
    uint32_t estimator;    /* RTMI_ROULETTE_PLAIN / _NEE / _ENV / _ENV_NEE of rtmi_roulette.h (no roulette here) */
    uint32_t flags;        /* 0, RTMI_FLAG_FAST_CULL, _SKY, _FACE_FORWARD, _UV_BOOK; anything else RTMI_ERR_UNSUPPORTED */
    uint32_t max_depth;    /* as rtmi_render_params */
    float    t_min;        /* of every segment after the first, and of shadow rays (the render's 0.001) */
    uint64_t seed;         /* the render key */
    uint64_t first_ray;    /* index of this call's ray 0 in the caller's batch */
    uint32_t first_sample; /* index of this call's sample 0 */
    uint32_t stream_skip;  /* 32-bit words of stream 0 already consumed when the path starts */
    float    env_select_p; /* as rtmi_env_render; read by ENV_NEE only */
} rtmi_radiance_params; /* 56 B */

/* Blocking, host pointers.  rays: n records of rtmi_query.h; time: n floats, or NULL for time 0.  kernel_ms: optional,
 * the two kernels' time by HIP events.  n == 0 is RTMI_OK and launches nothing.
 * RTMI_ERR_INVALID, with the entry's name in rtmi_last_error(), for a NULL scene, params or rays, all three outputs
 * NULL, spp == 0, max_depth == 0, an estimator outside 0..3, first_ray + n > 2^32, first_sample + spp > 2^32,
 * n * spp >= 2^31, ENV_NEE with env_select_p outside (0, 1], SKY with a map estimator, a missing attachment, and for a
 * ray that rtmi_trace refuses (the message names the ray).  RTMI_ERR_UNSUPPORTED for unknown flags.  All of these are
 * answered before any device work.
 * Supported range of a caller's |d|: d.d must be a normal fp32 number (rtmi_query.h, "Supported range of |d|").  Outside it
 * the FIRST segment's scatter differs from the reference: where d.d overflows (|d| >= 2^64 always) normalize(d) is 0, so
 * a Metal reflects nothing and absorbs the path, and a Dielectric's cosine is inf / inf = NaN; where d.d is a denormal the
 * scattered direction keeps only d.d's remaining bits.  Both are pinned against the fp32 oracle bit for bit
 * (tests/test_path_contract.py, tests/test_gpu_path_contract.py).  Later segments are unaffected: scattered directions are
 * O(1).  Rescaling d by a power of two, and the interval inversely, is exact and lifts the restriction. */
int rtmi_radiance(rtmi_scene *scene, const rtmi_radiance_params *params, const rtmi_ray *rays, const float *time,
                  float *out_mean, float *out_stderr, float *out_samples, double *kernel_ms);

/* Asynchronous, DEVICE pointers on the scene's device, enqueued on `stream` (a hipStream_t) behind the handle's previous
 * call, like rtmi_trace_device.  d_samples is required: n * spp * 12 bytes, the kernel's per-sample buffer and the
 * caller's output in one, so the call allocates nothing; d_mean and d_stderr (n * 12 bytes each) are optional.  Writes
 * exactly n * spp, n and n records and nothing beyond, and takes the caller's word for the rays. */
int rtmi_radiance_device(rtmi_scene *scene, const rtmi_radiance_params *params, const void *d_rays, const void *d_time,
                         void *d_mean, void *d_stderr, void *d_samples, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RTMI_RADIANCE_H */
