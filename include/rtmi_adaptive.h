/* rtmi_adaptive.h — noise-targeted adaptive sampling with per-pixel standard errors, on the MI355X (gfx950) device path.
 *
 * rtmi_render traces exactly ns samples in every pixel (tests/test.rs:55-85).  rtmi_render_adaptive traces samples in
 * steps, per 8x8 tile, and stops a tile once its noise estimate meets a target; it also returns the estimate.  See
 * DESIGN.md §11.
 *
 * Steps.  Step 0 renders samples [0, min_spp) of every tile.  Step k renders the next step_spp samples (fewer when that
 * would pass ns = params->ns, the cap) of the tiles still active, so every active tile has the same count n and the
 * counts go min_spp, min_spp + step_spp, ..., ns.  After every step each active tile is tested and retires when
 * converged; tiles that reach ns retire as they are.
 *
 * Estimator.  Per pixel and channel, x_1..x_n are the fp32 per-sample radiances widened to double, in sample order:
 *   sum   the f64 sum of rtmi_render, same additions in the same order; the texel is sum / n, quantised as rtmi_render's
 *   m, M2 Welford in double, k = 1..n:  d = x - m;  m = m + d / k;  M2 = M2 + d * (x - m)   (no fused operations)
 *   stderr = sqrt(M2 / (n * (n - 1)))
 * A tile is converged iff every pixel of it inside the image has, in every channel, a finite stderr, a finite
 * mean = sum / n, and stderr <= abs_tol + rel_tol * |mean|.  A non-finite value is never converged.
 *
 * Equivalence.  A pixel's samples come from Philox streams keyed by (seed, sample, pixel), so a tile that retires with
 * n samples is bit for bit, in linear and rgb8, the same tile of rtmi_render with ns = n.  min_spp == ns ("statistics
 * only") is rtmi_render's image plus its standard-error plane.  Results do not depend on the kernel (default or
 * RTMI_FLAG_SYNC), on FAST_CULL, on sample_buffer_bytes (a step that does not fit is rendered in sub-passes that carry
 * sum, m and M2; decisions are made at step ends only) or on the order of the active tiles.
 */
#ifndef RTMI_ADAPTIVE_H
#define RTMI_ADAPTIVE_H

#include "rtmi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint32_t min_spp;  /* samples every tile gets first; >= 2 (a variance needs two), <= ns */
    uint32_t step_spp; /* samples added per step to each tile that is still noisy; >= 1 */
    double abs_tol;    /* a tile retires when, for every in-image pixel and channel, */
    double rel_tol;    /*   stderr <= abs_tol + rel_tol * |mean|   (both >= 0, finite) */
} rtmi_adaptive;

/* Blocking whole-image adaptive render (tile_world must be 1); params->ns is the cap.
 *   out_linear: ny*nx*3 floats, the mean radiance (row 0 = top row); may be NULL
 *   out_rgb8:   ny*nx*3 bytes, the quantisation of tests/test.rs:71-78; may be NULL
 *   out_stderr: ny*nx*3 floats, the standard error of the mean; may be NULL
 *   out_spp:    ny*nx, the sample count of each pixel's tile; may be NULL
 *   stats:      samples = the paths actually traced; may be NULL
 * RTMI_ERR_INVALID, before any device work, for a NULL scene, camera, params or adaptive, for bad params, and for
 * min_spp < 2, min_spp > ns, step_spp == 0 and tolerances that are negative or not finite.
 * RTMI_ERR_UNSUPPORTED for the flags PATH_SIG, PROFILE, ASYNC, BLOCK_COOP, PROGRESSIVE, TEST_OVERFLOW and any flag bit
 * not named here, for tile_world != 1, for multi-GPU handles (rtmi_multi has no adaptive entry) and for the f64 mode
 * (there is no adaptive form of rtmi_render_f64).  Accepted: FAST_CULL, SYNC, REF_TREE, SKY, FACE_FORWARD, UV_BOOK.
 * Scenes with instanced primitives or media inside transforms run the per-lane kernel (same image, slower).
 * The progress callback of params counts tile-samples: total = tiles x ns, the upper bound; a tile that retires at n
 * counts its remaining ns - n as done.  The call ends with done == total; a non-zero return cancels after the running
 * step (RTMI_ERR_CANCELLED, no outputs written). */
int rtmi_render_adaptive(rtmi_scene *scene, const rtmi_camera *cam, const rtmi_render_params *params,
                         const rtmi_adaptive *adaptive, float *out_linear, uint8_t *out_rgb8, float *out_stderr,
                         uint32_t *out_spp, rtmi_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* RTMI_ADAPTIVE_H */
