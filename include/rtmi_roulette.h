/* rtmi_roulette.h — Russian-roulette path termination with a per-pixel bounce count, on the MI355X (gfx950) device
 * path.  An opt-in family next to rtmi_render_nee / rtmi_render_env and their adaptive forms.  See DESIGN.md §17.
 *
 * Paths.  A roulette path is rtmi_render's path, cut short: camera, scatter and medium draws come from Philox stream 0,
 * counter (block, sample, pixel, 0), light samples from stream 3, counter (block, sample, pixel, 3), both exactly as
 * rtmi_nee.h and rtmi_env.h state them.  The roulette draws come from stream 4 and no other stream moves, so a roulette
 * path is a prefix of the path the same (seed, sample, pixel) traces without roulette: the same vertices in the same
 * order, up to the vertex where it ends.
 *
 * The test.  It is made after a scatter of any material (Lambertian, Metal, Dielectric, Isotropic) has set
 * T = T * att and raised depth to d, when d >= min_depth.  The vertex's own light sample, if it took one, is already
 * fixed with the T from before the test (its c = (T * albedo) * mis of rtmi_nee.h does not change):
 *
 *   m = max(max(T.x, T.y), T.z)
 *   if m == 0: the continuation ends (no draw)
 *   q = min(max(m, q_min), 1)
 *   if q < 1:
 *       w = word 0 of philox(counter = (d, sample, pixel, 4), key = seed)    one evaluation per test, no stream state
 *       u = u01(w)                                                           the 24-bit uniform of rtmi_math.h
 *       if !(u < q): the continuation ends
 *       else T = T / q                                                       per component, fp32, one rounding each
 *
 * (sample, pixel) are the words stream 0 uses for that path; all comparisons and max / min are fp32.  "The continuation
 * ends" means: a pending shadow ray of this vertex is still traced and counted (its item scan, its stream-3 medium
 * draws and its V), then the path is written as it stands; a vertex without a pending shadow ray ends at once.
 * Everything after a surviving test uses the rescaled T: emitter hits with their MIS weight, later light samples, the
 * map and the sky.  min_depth > max_depth makes no test (no scatter reaches that depth); q_min = 1 makes no draw and
 * leaves T alone (a throughput of exactly 0 still ends the continuation; it had nothing left to add).  The expectation
 * is unchanged: a continuation that survives with probability q is weighted 1 / q.
 *
 * Estimators.  `estimator` selects whose arithmetic the path is counted in, as the named header states it:
 *   RTMI_ROULETTE_PLAIN    rtmi_render                                              (rtmi.h)
 *   RTMI_ROULETTE_NEE      rtmi_render_nee                                          (rtmi_nee.h)
 *   RTMI_ROULETTE_ENV      rtmi_render_env with nee = 0                             (rtmi_env.h)
 *   RTMI_ROULETTE_ENV_NEE  rtmi_render_env with nee = 1 and env_select_p            (rtmi_env.h)
 * env_select_p is read by RTMI_ROULETTE_ENV_NEE only.  With no test made (min_depth > max_depth) or no draw made
 * (q_min = 1) the image and its standard errors are bit for bit those of the named entry.
 *
 * Bounce count.  out_bounces[ny*nx] (uint32, row 0 = top row) holds, per pixel, the sum over its samples of depth when
 * the path was written: the scatters it made.  Integer atomics, so the plane does not depend on the schedule.  It is
 * zeroed when a call starts and accumulates over the call's passes and adaptive steps.  Shadow rays are not bounces.
 *
 * Outputs, standard errors (Welford, as rtmi_adaptive.h), passes, progress and cancellation: those of rtmi_render_nee
 * (rtmi_render_roulette) and rtmi_render_adaptive_nee (rtmi_render_adaptive_roulette).  Results do not depend on
 * FAST_CULL, SYNC, REF_TREE, shade_threshold or sample_buffer_bytes.  Both run the per-lane kernel
 * (stats.kernel = RTMI_KERNEL_PERLANE).  include/rtmi_roulette_coop.h adds an opt-in flag that runs them on the
 * wave-cooperative kernel, with the same bits.
 *
 * Adaptive form.  rtmi_adaptive.h's steps and convergence test on the roulette estimator.  The roulette stream is keyed
 * by (seed, sample, pixel, depth) as well, so a tile that stops at n samples is bit for bit, in linear, rgb8, stderr and
 * bounces, that tile of rtmi_render_roulette with ns = n; min_spp == ns gives the fixed render.
 *
 * Errors.  RTMI_ERR_INVALID, before any device work, for a NULL scene, camera, params, opts (or adaptive), for bad
 * params, estimator > 3, min_depth == 0, q_min outside (0, 1] or not finite, env_select_p outside (0, 1] with
 * RTMI_ROULETTE_ENV_NEE, RTMI_FLAG_SKY with the two map estimators (the map replaces the sky), the adaptive checks of
 * rtmi_adaptive.h, and for a scene without a light table (NEE, ENV_NEE: rtmi_scene_attach_lights) or without a map
 * (ENV, ENV_NEE: rtmi_scene_attach_env).  RTMI_ERR_UNSUPPORTED for RTMI_FLAG_PATH_SIG (a roulette path has no
 * counterpart to compare a signature with), for PROFILE, ASYNC, BLOCK_COOP, PROGRESSIVE, TEST_OVERFLOW and any flag
 * bit not named here, and for tile_world != 1.  Accepted: FAST_CULL, SYNC, REF_TREE, SKY (PLAIN and NEE),
 * FACE_FORWARD, UV_BOOK.
 */
#ifndef RTMI_ROULETTE_H
#define RTMI_ROULETTE_H

#include "rtmi.h"
#include "rtmi_adaptive.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTMI_ROULETTE_PLAIN 0u
#define RTMI_ROULETTE_NEE 1u
#define RTMI_ROULETTE_ENV 2u
#define RTMI_ROULETTE_ENV_NEE 3u

typedef struct {
    uint32_t estimator;  /* RTMI_ROULETTE_* */
    uint32_t min_depth;  /* the first depth (scatters made) at which the test is made; >= 1 */
    float q_min;         /* floor of the survival probability, in (0, 1] */
    float env_select_p;  /* RTMI_ROULETTE_ENV_NEE: the map's share of the light samples, in (0, 1] */
} rtmi_roulette;         /* 16 B */

/* Blocking whole-image roulette render (tile_world must be 1).
 *   out_linear:  ny*nx*3 floats, the mean radiance (row 0 = top row); may be NULL
 *   out_rgb8:    ny*nx*3 bytes, quantised as rtmi_render's; may be NULL
 *   out_stderr:  ny*nx*3 floats, the standard error of the mean; may be NULL
 *   out_bounces: ny*nx, the scatters made by the pixel's paths, summed; may be NULL
 *   stats:       samples = nx*ny*ns; may be NULL */
int rtmi_render_roulette(rtmi_scene *scene, const rtmi_camera *cam, const rtmi_render_params *params,
                         const rtmi_roulette *opts, float *out_linear, uint8_t *out_rgb8, float *out_stderr,
                         uint32_t *out_bounces, rtmi_stats *stats);

/* The same under the noise target of rtmi_adaptive.h; params->ns is the cap.
 *   out_spp:     ny*nx, the sample count of each pixel's tile; may be NULL
 *   stats:       samples = the camera paths actually traced */
int rtmi_render_adaptive_roulette(rtmi_scene *scene, const rtmi_camera *cam, const rtmi_render_params *params,
                                  const rtmi_roulette *opts, const rtmi_adaptive *adaptive, float *out_linear,
                                  uint8_t *out_rgb8, float *out_stderr, uint32_t *out_spp, uint32_t *out_bounces,
                                  rtmi_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* RTMI_ROULETTE_H */
