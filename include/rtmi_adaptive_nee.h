/* rtmi_adaptive_nee.h — adaptive sampling (include/rtmi_adaptive.h) with next-event estimation (include/rtmi_nee.h) or
 * environment lighting (include/rtmi_env.h), on the MI355X (gfx950) device path.  See DESIGN.md §16.
 *
 * rtmi_render_adaptive drives rtmi_render's plain estimator.  These two entries drive the estimators of rtmi_render_nee
 * and rtmi_render_env instead: a tile gets samples in steps until its noise estimate meets the target, and the samples
 * are those of the fixed-ns entry.
 *
 * Steps, estimator, convergence test, outputs, progress and cancellation: exactly those of rtmi_adaptive.h.  Step 0
 * renders samples [0, min_spp) of every tile, each later step the next step_spp samples (fewer at the cap ns =
 * params->ns) of the tiles still active; a tile retires when every in-image pixel has, in every channel, a finite
 * stderr, a finite mean and stderr <= abs_tol + rel_tol * |mean|, or when it reaches ns.  stats.samples counts camera
 * paths (the sum of every pixel's count); shadow rays are not counted, as in rtmi_render_nee.
 *
 * Equivalence.  Both Philox streams of a path (stream 0 for the path, stream 3 for its light samples) are keyed by
 * (seed, sample, pixel), so a tile that retires with n samples is bit for bit, in linear, rgb8 and stderr, the same
 * tile of rtmi_render_nee with ns = n (rtmi_render_adaptive_nee), or of rtmi_render_env with the same opts and ns = n
 * (rtmi_render_adaptive_env).  min_spp == ns ("statistics only") therefore gives the fixed render's image and standard
 * errors.  Results do not depend on FAST_CULL, SYNC, REF_TREE, sample_buffer_bytes (sub-passes carry sum, m and M2;
 * decisions are made at step ends only) or the order of the active tiles.  Both run the per-lane kernel
 * (stats.kernel = RTMI_KERNEL_PERLANE).
 *
 * Errors.  RTMI_ERR_INVALID, before any device work, for a NULL scene, camera, params, adaptive or opts, for bad params,
 * for min_spp < 2, min_spp > ns, step_spp == 0 and tolerances that are negative or not finite; for the env form also for
 * RTMI_FLAG_SKY (the map replaces the sky), nee not 0 or 1 and env_select_p outside (0, 1].  RTMI_ERR_UNSUPPORTED for
 * the flags PATH_SIG, PROFILE, ASYNC, BLOCK_COOP, PROGRESSIVE, TEST_OVERFLOW and any flag bit not named here, and for
 * tile_world != 1.  A scene without a light table (rtmi_render_adaptive_nee; rtmi_render_adaptive_env with nee = 1) or
 * without a map (rtmi_render_adaptive_env) is RTMI_ERR_INVALID, as the fixed entries report it.  Accepted:
 * FAST_CULL, SYNC, REF_TREE, SKY (NEE form only), FACE_FORWARD, UV_BOOK.
 */
#ifndef RTMI_ADAPTIVE_NEE_H
#define RTMI_ADAPTIVE_NEE_H

#include "rtmi.h"
#include "rtmi_adaptive.h"
#include "rtmi_env.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Blocking whole-image adaptive NEE render (tile_world must be 1); params->ns is the cap.  Outputs as
 * rtmi_render_adaptive's:
 *   out_linear: ny*nx*3 floats, the mean radiance (row 0 = top row); may be NULL
 *   out_rgb8:   ny*nx*3 bytes, quantised as rtmi_render's; may be NULL
 *   out_stderr: ny*nx*3 floats, the standard error of the mean; may be NULL
 *   out_spp:    ny*nx, the sample count of each pixel's tile; may be NULL
 *   stats:      samples = the camera paths actually traced; may be NULL */
int rtmi_render_adaptive_nee(rtmi_scene *scene, const rtmi_camera *cam, const rtmi_render_params *params,
                             const rtmi_adaptive *adaptive, float *out_linear, uint8_t *out_rgb8, float *out_stderr,
                             uint32_t *out_spp, rtmi_stats *stats);

/* The same with the attached environment map and the options of rtmi_render_env. */
int rtmi_render_adaptive_env(rtmi_scene *scene, const rtmi_camera *cam, const rtmi_render_params *params,
                             const rtmi_env_render *opts, const rtmi_adaptive *adaptive, float *out_linear,
                             uint8_t *out_rgb8, float *out_stderr, uint32_t *out_spp, rtmi_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* RTMI_ADAPTIVE_NEE_H */
