/* rtmi_nee.h — next-event estimation with multiple importance sampling toward the scene's area lights, on the MI355X
 * (gfx950) device path.  An opt-in second estimator of rtmi_render's image.  See DESIGN.md §14.
 *
 * Paths.  rtmi_render_nee traces rtmi_render's own paths: camera, scatter and medium draws and the depth limit come from
 * Philox stream 0, counter (block, sample, pixel, 0), as in rtmi_render, so every path visits the same vertices in the
 * same order and out_path_sig is bit for bit rtmi_render's.  Only the way emission is counted along them differs.
 *
 * Light-sample randomness.  Stream 3: counter (block, sample, pixel, 3) under the render key.  Per pixel sample it is
 * read in this order: at every vertex that takes a light sample, three words (w0: the light, w1 and w2: the point on
 * it, each as a 24-bit uniform), then the medium draws of that vertex's shadow ray, as the item scan of world.hit makes
 * them; then the next such vertex.
 *
 * Eligible lights (rtmi_lights_from_desc).  A light is one occurrence (item, prim) of a primitive of a flat
 * rtmi_scene_desc such that: its material is RTMI_MAT_DIFFUSE_LIGHT; it is a RTMI_PRIM_RECT with a0 < a1 and b0 < b1 or
 * a RTMI_PRIM_SPHERE with radius > 0 (a rect with a0 >= a1 or b0 >= b1 is never hit; a RTMI_PRIM_MSPHERE whose
 * displacement is exactly 0, the form a lowering gives a static Sphere next to moving ones, is a sphere); neither the item nor the primitive
 * carries a transform chain; the item is not a medium; the primitive occurs in no other item or position of the
 * description (an occurrence is found by the index the hit reports); its weight w is > 0.  w = the largest channel of
 * a SOLID emitter texture, 1 for any other texture.  Every other emitter (under transforms, cubes, moving spheres, the
 * opt-in sky) is counted by BSDF sampling at full weight.  Selection: p_sel = area * w / sum(area * w), in f64, with a
 * CDF whose last entry is exactly 1.
 *
 * Densities (solid angle).  The Lambertian scatters toward normal + random_in_unit_sphere(): p_b(w) = (2/pi) max(0, cos)^3,
 * cos = (w . n) / (|w| |n|), n the normal its scatter sees (FlipNormals and FACE_FORWARD applied).  Isotropic:
 * p_b = 1/(4 pi).  Metal and Dielectric take no light sample.  Light: p_l = p_sel * p_L with, for a rect, a uniform point
 * q and p_L = d^2 / (|cos_l| A); for a sphere, a uniform direction in the cone it subtends from x and
 * p_L = 1 / (2 pi (1 - cos theta_max)), 1 - cos theta_max = s / (1 + sqrt(1 - s)), s = r^2 / |x - c|^2; no sample and
 * p_L = 0 from inside.
 *
 * Estimator (power heuristic, one light sample per vertex), at every Lambertian or Isotropic vertex that scatters
 * (depth < max_depth) when the table is not empty:
 *   light sample  T * albedo * Le * V * p_b p_l / (p_b^2 + p_l^2)   (nothing when p_b = 0 or p_l = 0)
 *   BSDF hit of an eligible light after such a vertex: its emission times p_b^2 / (p_b^2 + p_l^2), p_b the density of
 *                 the scatter that produced the ray, p_l evaluated from the ray's origin to the hit point.
 * Camera rays, rays after Metal or Dielectric and hits of other emitters count with weight 1, in rtmi_render's exact
 * arithmetic: with an empty light table rtmi_render_nee is rtmi_render bit for bit.  V = 1 iff world.hit of the shadow
 * ray (origin x, direction q - x, the path's time, (t_min, +inf)) returns the sampled occurrence — the item scan of a
 * path ray, media included, whose free-flight draws then come from stream 3; Le = the emitter's texture at that hit.
 *
 * Arithmetic (fp32, each operation rounded once, no fused operations; the order below is the specification, restated
 * by oracle/rt_oracle.c color_nee).  Table: area, p_sel and cdf are the f64 values above rounded once to float; the sum
 * of area * w is accumulated in table order and p_sel = (area * w) / sum.  Light choice: us = u01(w0); the first index i
 * with us < cdf[i], by binary search (lo = 0, hi = n - 1; mid = (lo + hi) >> 1; us < cdf[mid] ? hi = mid : lo = mid + 1).
 * p_b = c > 0 ? (float)(2/pi) * ((c * c) * c) : 0 with c = (w . n) / sqrt((w . w) * (n . n)), dot products summed x, y, z
 * left to right.  Rect (a, b the plane's axes, k its coordinate): q = (a0 + u1 (a1 - a0), b0 + u2 (b1 - b0)) at k,
 * p_l = (p_sel * (d2 * sqrt(d2))) / (|w_k| * area), w = q - x, d2 = w . w.  Sphere (centre c, radius r): dc = c - x,
 * dist2 = dc . dc, s = (r * r) / dist2, no sample unless s < 1; omc = s / (1 + sqrt(1 - s)); om = u1 * omc; ct = 1 - om;
 * st = sqrt(max(0, om * (2 - om))); phi = (2 * pi_f) * u2; w = dc / sqrt(dist2) per component; basis
 * sg = w.z >= 0 ? 1 : -1, a = -1 / (sg + w.z), b = (w.x * w.y) * a, t1 = (1 + ((sg * w.x) * w.x) * a, sg * b, -sg * w.x),
 * t2 = (b, sg + (w.y * w.y) * a, -w.y); d = (w * ct + t1 * (st * rtmi_cosf(phi))) + t2 * (st * rtmi_sinf(phi));
 * tq = sqrt(dist2) * ct - sqrt(max(0, r * r - dist2 * (st * st))), no sample unless tq > 0; direction d * tq;
 * p_l = p_sel / ((2 * pi_f) * omc).  The sample is taken when p_b > 0, p_l > 0 and p_l < FLT_MAX.  Weights as ratios:
 * light sample r = min / max of (p_b, p_l), r / (1 + r * r); BSDF hit p_b >= p_l ? 1 / (1 + r * r) with r = p_l / p_b,
 * else r2 / (1 + r2) with r2 = r * r, r = p_b / p_l (weight 1 when p_l = 0).  Accumulation: a BSDF hit adds
 * L = L + T * (Le * weight); a light sample adds L = L + ((T * albedo) * mis) * Le when its shadow ray hits, after the
 * vertex's own emission and before the continuation's.
 */
#ifndef RTMI_NEE_H
#define RTMI_NEE_H

#include "rtmi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One eligible light occurrence. */
typedef struct {
    int32_t item;    /* index of the item in desc->items */
    int32_t prim;    /* index of the primitive */
    int32_t kind;    /* RTMI_PRIM_RECT or RTMI_PRIM_SPHERE */
    int32_t material;
    double area;     /* rect: (a1 - a0) (b1 - b0); sphere: 4 pi r^2 */
    double weight;   /* w: the largest channel of a SOLID emitter texture, else 1 */
    double select_p; /* p_sel = area * w / sum over the table */
    double cdf;      /* sum of select_p up to and including this light; exactly 1 for the last */
} rtmi_light;        /* 48 B */

/* The light table of a description, in (item, primitive) order.  Pure host code: initialises no device.  Writes at most
 * `cap` lights to `out` (which may be NULL when cap is 0) and the full count to *count.
 * RTMI_ERR_INVALID for a NULL desc or count, a wrong ABI version, or an item or primitive outside the description. */
int rtmi_lights_from_desc(const rtmi_scene_desc *desc, rtmi_light *out, uint32_t cap, uint32_t *count);

/* Derives the light table of `desc` (the description the handle was created from) and uploads it to the handle's
 * device.  RTMI_ERR_INVALID for NULL arguments and for a desc whose counts differ from the handle's. */
int rtmi_scene_attach_lights(rtmi_scene *scene, const rtmi_scene_desc *desc);

/* Blocking whole-image NEE render (tile_world must be 1).
 *   out_linear:   ny*nx*3 floats, the mean radiance (row 0 = top row); may be NULL
 *   out_rgb8:     ny*nx*3 bytes, quantised as rtmi_render's; may be NULL
 *   out_stderr:   ny*nx*3 floats, the standard error of the mean (Welford, as include/rtmi_adaptive.h); may be NULL
 *   out_path_sig: ny*nx, optional: bit for bit rtmi_render's path_sig (shadow rays are not part of it)
 *   stats:        samples = nx*ny*ns; may be NULL
 * RTMI_ERR_INVALID, before any device work, for a NULL scene, camera or params, for bad params and for a scene without
 * attached lights (rtmi_scene_attach_lights).  RTMI_ERR_UNSUPPORTED for the flags PROFILE, ASYNC, BLOCK_COOP,
 * PROGRESSIVE, TEST_OVERFLOW and any flag bit not named here, for tile_world != 1 and for multi-GPU handles.  Accepted:
 * FAST_CULL, SYNC, REF_TREE, SKY, FACE_FORWARD, UV_BOOK, and PATH_SIG through out_path_sig.  The result does not depend
 * on FAST_CULL, SYNC, REF_TREE or sample_buffer_bytes (passes).  Progress and cancellation as in rtmi_render. */
int rtmi_render_nee(rtmi_scene *scene, const rtmi_camera *cam, const rtmi_render_params *params, float *out_linear,
                    uint8_t *out_rgb8, float *out_stderr, uint64_t *out_path_sig, rtmi_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* RTMI_NEE_H */
