/* rtmi_frame.h — a device-resident frame pipeline on the MI355X (gfx950): one call renders a frame, renders its first-hit
 * features, pushes both through a temporal history, filters and quantises, without a copy to the host between the stages.
 *
 * A frame handle is bound to a scene and an image size.  rtmi_frame_render runs, on the scene's own stream and under one
 * hold on the scene:
 *   1. the lit render with `ns` samples per pixel: rtmi_render_adaptive with min_spp == ns, step_spp == 1 and zero
 *      tolerances (RTMI_ROULETTE_PLAIN), rtmi_render_nee (_NEE) or rtmi_render_env with nee = 0 (_ENV) or 1 (_ENV_NEE);
 *   2. rtmi_render_features with the same camera, ns, seed and flags (without RTMI_FLAG_LIGHT_COOP);
 *   3. the un-tiling of the lit render's texels and standard errors into packed row-major planes (the noisy planes);
 *   4. rtmi_temporal_push of the noisy planes and the features with standard errors (the accumulated planes);
 *   5. rtmi_denoise of the accumulated linear and stderr with this frame's features (linear and rgb8).
 * The arithmetic of every stage is that stage's, as its header states it: every output plane has the bits the five calls
 * give when each is fed the previous one's host planes.  RTMI_FRAME_NO_TEMPORAL leaves out step 4 (step 5 then reads the
 * noisy planes: the chain render, features, denoise); RTMI_FRAME_NO_FILTER runs step 5 with 0 iterations (linear is the
 * accumulated image, rgb8 its quantisation).  Both together give the noisy image and its quantisation.
 *
 * Memory.  Everything the chain needs on the device is allocated by rtmi_frame_create and freed by rtmi_frame_destroy;
 * a frame call allocates nothing (the scene's own render buffers grow on first use, as for the one-shot entries).  Per
 * pixel: the history of rtmi_temporal.h, 96 B; the noisy linear and stderr, 24 B; the accumulated linear, stderr, history
 * length and motion, 36 B; the filter's two states, guide and gradient, 56 B; linear and rgb8, 15 B: 227 B per pixel with
 * every stage on (each plane rounded up to 256 B).  NO_TEMPORAL saves 132 B, NO_FILTER or iterations == 0 saves 56 B.
 *
 * Threads.  Calls on one frame must not overlap.  A frame call holds its scene for its whole length, as a blocking render
 * does: calls on frames of one scene, and other renders of that scene, serialise.  Several frames may live on one scene
 * and do not see each other.  A frame must be destroyed before its scene.  See DESIGN.md §28.
 */
#ifndef RTMI_FRAME_H
#define RTMI_FRAME_H

#include "rtmi.h"
#include "rtmi_denoise.h"
#include "rtmi_roulette.h"
#include "rtmi_temporal.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTMI_FRAME_NO_TEMPORAL 1u /* no history: linear and rgb8 are the filtered noisy image; the accumulated planes are not written */
#define RTMI_FRAME_NO_FILTER 2u   /* the filter runs with 0 iterations: linear is the accumulated image, rgb8 its quantisation */

typedef struct {
    uint32_t estimator;            /* offset  0: RTMI_ROULETTE_PLAIN / _NEE / _ENV / _ENV_NEE of rtmi_roulette.h (no roulette here) */
    float env_select_p;            /* offset  4: rtmi_env_render's, in (0, 1]; read by _ENV and _ENV_NEE; default 0.5 */
    rtmi_temporal_params temporal; /* offset  8: the history's parameters (rtmi_temporal.h), checked as rtmi_temporal_create does */
    rtmi_denoise_params denoise;   /* offset 40: the filter's parameters (rtmi_denoise.h), checked as rtmi_denoise does */
    uint32_t flags;                /* offset 72: RTMI_FRAME_*; any other bit is RTMI_ERR_UNSUPPORTED */
    uint32_t reserved[5];          /* offset 76: must be 0 */
} rtmi_frame_opts;                 /* 96 bytes */

/* The planes of a frame, all row-major with row 0 = the top row; each pointer may be NULL, and a NULL plane is not copied.
 * Host pointers for rtmi_frame_render, pointers on the scene's device for rtmi_frame_render_device. */
typedef struct {
    float *linear;         /* offset  0: ny*nx*3 floats, the frame's image */
    uint8_t *rgb8;         /* offset  8: ny*nx*3 bytes, its quantisation */
    float *noisy_linear;   /* offset 16: ny*nx*3 floats, the lit render's image */
    float *noisy_stderr;   /* offset 24: ny*nx*3 floats, its standard errors */
    float *albedo;         /* offset 32: ny*nx*3 floats (rtmi_features.h) */
    float *normal;         /* offset 40: ny*nx*3 floats */
    float *depth;          /* offset 48: ny*nx floats, +inf where no sample hit */
    uint32_t *hits;        /* offset 56: ny*nx counts */
    float *accum_linear;   /* offset 64: ny*nx*3 floats, the push's out_linear (rtmi_temporal.h) */
    float *accum_stderr;   /* offset 72: ny*nx*3 floats, its out_stderr */
    float *history;        /* offset 80: ny*nx floats, its out_history */
    float *motion;         /* offset 88: ny*nx*2 floats, its out_motion */
} rtmi_frame_out;          /* 96 bytes */

typedef struct rtmi_frame rtmi_frame;

/* `params` fixes nx, ny, max_depth, t_min, flags and the progress callback for the life of the handle; its ns and seed are
 * not read (rtmi_frame_render takes them).  Allocates all device memory of the chain.  *out is NULL after a failure.
 * Refusals, in this order and each message prefixed "rtmi_frame_create: ":
 *   RTMI_ERR_INVALID for a NULL params, opts or out; nx or ny of 0 or above 32768; tile_world of 0 or tile_rank >=
 *   tile_world; estimator above 3; env_select_p outside (0, 1]; a temporal or denoise parameter outside its header's range
 *   or a non-zero reserved word of either; a non-zero reserved word of opts; RTMI_FLAG_SKY with _ENV or _ENV_NEE (the map
 *   replaces the sky);
 *   RTMI_ERR_UNSUPPORTED for a flag of params other than FAST_CULL, SYNC, REF_TREE, SKY, FACE_FORWARD, UV_BOOK and
 *   LIGHT_COOP (which goes to the lit render only, and is refused with RTMI_ROULETTE_PLAIN, whose render is cooperative by
 *   default); an unknown bit of temporal.flags; a non-zero denoise.flags; an unknown bit of opts->flags; tile_world != 1;
 *   RTMI_ERR_INVALID for a NULL scene, a scene without the map (_ENV, _ENV_NEE) or the light table (_NEE, _ENV_NEE);
 *   RTMI_ERR_DEVICE for a failure on the device, RTMI_ERR_NOMEM when the allocation fails. */
int rtmi_frame_create(rtmi_scene *scene, const rtmi_render_params *params, const rtmi_frame_opts *opts, rtmi_frame **out);

/* Blocking.  Renders one frame under `cam` with ns samples per pixel and the seed `seed` and copies the planes asked for
 * to the host.  stats (may be NULL): the lit render's.
 * Refusals, in this order and each message prefixed "rtmi_frame_render: ": RTMI_ERR_INVALID for a NULL cam or out, ns < 2
 * (a standard error needs two samples), a non-finite camera field, a camera whose matrix (rtmi_temporal.h, step 4) is
 * singular; RTMI_ERR_UNSUPPORTED for ns >= 2^26; RTMI_ERR_INVALID for a NULL handle (checked last, so a machine without
 * a device answers for every other argument), a scene that lost what the estimator needs attached;
 * RTMI_ERR_DEVICE for a failure on the device, a traversal pool overflow among it ("framebuffer holds poisoned texels",
 * rtmi_untile's words, when the un-tiling meets poisoned texels); RTMI_ERR_CANCELLED from the progress callback.  After a
 * failure on the device or a cancellation the history is as after rtmi_frame_reset; a refused call leaves it as it was. */
int rtmi_frame_render(rtmi_frame *frame, const rtmi_camera *cam, uint32_t ns, uint64_t seed, const rtmi_frame_out *out,
                      rtmi_stats *stats);

/* The same call with `out` holding device pointers on the scene's device; no plane passes through the host.  Blocking
 * too: when it returns, the planes are complete and visible to every stream.  Messages are prefixed
 * "rtmi_frame_render_device: ". */
int rtmi_frame_render_device(rtmi_frame *frame, const rtmi_camera *cam, uint32_t ns, uint64_t seed, const rtmi_frame_out *out,
                             rtmi_stats *stats);

/* Forgets the frames rendered so far and keeps the allocation: the next frame starts a fresh history.  RTMI_ERR_INVALID
 * for a NULL handle. */
int rtmi_frame_reset(rtmi_frame *frame);

/* Frees the handle and its device memory, after the scene's running work.  NULL is allowed. */
void rtmi_frame_destroy(rtmi_frame *frame);

/* The un-tiling kernel of step 3 on the caller's (host) data, for the tests (the role rtmi_probe_expf plays for
 * rtmi_denoise.h): tiled = ceil(nx/8)*ceil(ny/8)*64 texels, texel = tile*64 + ly*8 + lx with tiles counted from the
 * top-left; tiled_stderr = that many triples (may be NULL with out_stderr); out_linear, out_stderr: ny*nx*3 floats (may be
 * NULL); *poisoned (may be NULL) = the in-image texels that carry RTMI_TEXEL_POISON.  Padding texels are neither read as
 * pixels nor counted, and nothing is written outside the planes.  RTMI_ERR_INVALID for nx or ny of 0 or above 32768, a
 * NULL tiled and out_stderr without tiled_stderr; then RTMI_ERR_DEVICE without a device or for an index out of range. */
int rtmi_probe_frame_untile(int device, uint32_t nx, uint32_t ny, const rtmi_texel *tiled, const float *tiled_stderr,
                            float *out_linear, float *out_stderr, uint32_t *poisoned);

#ifdef __cplusplus
}
#endif

#endif /* RTMI_FRAME_H */
