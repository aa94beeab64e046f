/* rtmi_features.h — first-hit albedo, normal and depth buffers for denoisers, on the MI355X (gfx950) device path.
 *
 * Image denoisers take, besides the colour, the albedo and the normal of the first surface each ray hits, and its depth.
 * rtmi_render_features returns those planes, defined as the first bounce of rtmi_render's own paths.  See DESIGN.md §12.
 *
 * Semantics.  For a pixel and a sample s in [0, ns), take the primary ray of rtmi_render's sample s: its Philox stream is
 * keyed by (seed, s, pixel) and it makes the same camera draws.  Its first interaction with the world is the interaction
 * the render's first bounce finds, including a ConstantMedium scatter event, which is decided by the render's own draws.
 * max_depth does not change any feature output.  Per sample:
 *   albedo a_s   Lambertian, Metal and Isotropic (media included): the texture value at (u, v, p), as shade_hit computes
 *                it; Dielectric: (1, 1, 1); DiffuseLight: min(emitted, 1) per channel; miss: the sky colour under
 *                RTMI_FLAG_SKY, otherwise 0.
 *   normal n_s   the normal that the material's scatter sees: the record's normal after the item and primitive transforms
 *                and FlipNormals, turned by RTMI_FLAG_FACE_FORWARD when that flag applies; not renormalised.  Medium event
 *                or miss: (0, 0, 0).
 *   distance d_s only for samples with a hit: (double)t * sqrt((double)dx*dx + (double)dy*dy + (double)dz*dz), with t the
 *                fp32 first-hit parameter and (dx, dy, dz) the fp32 world ray direction; no fused operations.
 * Per pixel, each of these is computed in f64, in sample order, and rounded to f32 once:
 *   albedo = sum(a_s) / ns    normal = sum(n_s) / ns    depth = sum(d_s) / hits, or +inf when hits == 0
 *   hits   = the number of samples with a first interaction.
 * Row 0 is the top row, as for every other output.  The planes depend on nothing in the schedule: not on the kernel
 * (default or RTMI_FLAG_SYNC), not on FAST_CULL or REF_TREE, not on sample_buffer_bytes (passes).
 */
#ifndef RTMI_FEATURES_H
#define RTMI_FEATURES_H

#include "rtmi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Blocking whole-image features render (tile_world must be 1).
 *   out_albedo:   ny*nx*3 floats; may be NULL
 *   out_normal:   ny*nx*3 floats; may be NULL
 *   out_depth:    ny*nx floats; may be NULL
 *   out_hits:     ny*nx; may be NULL
 *   out_path_sig: ny*nx, optional: per pixel, the sum of sig_mix(bits(t), depth) over the one-bounce paths traced, bit for
 *                 bit the path_sig of rtmi_render with max_depth = 0
 *   stats:        samples = nx*ny*ns; may be NULL
 * RTMI_ERR_INVALID, before any device work, for a NULL scene, camera or params and for bad params.
 * RTMI_ERR_UNSUPPORTED for the flags PROFILE, ASYNC, BLOCK_COOP, PROGRESSIVE, TEST_OVERFLOW and any flag bit not named
 * here, for tile_world != 1 and for multi-GPU handles (rtmi_multi has no features entry).  Accepted: FAST_CULL, SYNC,
 * REF_TREE, SKY, FACE_FORWARD, UV_BOOK, and PATH_SIG through out_path_sig.  The progress callback and cancellation
 * behave as in rtmi_render. */
int rtmi_render_features(rtmi_scene *scene, const rtmi_camera *cam, const rtmi_render_params *params, float *out_albedo,
                         float *out_normal, float *out_depth, uint32_t *out_hits, uint64_t *out_path_sig, rtmi_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* RTMI_FEATURES_H */
