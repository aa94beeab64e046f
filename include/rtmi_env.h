/* rtmi_env.h — image-based environment lighting with importance-sampled next-event estimation, on the MI355X (gfx950)
 * device path.  An opt-in estimator of rtmi_render's image in which a ray that leaves the world sees an HDR map instead of
 * black (or the RTMI_FLAG_SKY gradient).  See DESIGN.md §15.
 *
 * Map.  rtmi_env_map: width W and height H in [1, RTMI_ENV_MAX_SIDE] with W * H <= RTMI_ENV_MAX_TEXELS; rgb holds
 * H * W * 3 floats, row-major, row 0 the top row (+y), every value finite and >= 0.
 *
 * Direction -> (u, v).  The contract functions of rtmi_math.h, fp32, each operation rounded once, no fused operations.
 * A direction with a component that is not finite, or with m = max(max(|d.x|, |d.y|), |d.z|) = 0, sees nothing (env = 0,
 * pdf = 0).  Otherwise s = d / m per component; l = sqrt((s.x * s.x + s.y * s.y) + s.z * s.z); n = s / l per component;
 * phi = rtmi_atan2f(n.z, n.x); theta = rtmi_asinf(min(max(n.y, -1), 1)); u = 1 - (phi + RTMI_PI_F) / (2 * RTMI_PI_F);
 * v = (theta + RTMI_PIO2_F) / RTMI_PI_F.  This is sphere_uv's RTMI_FLAG_UV_BOOK form: the earth scene's texture used as a
 * map has that scene's orientation.
 *
 * Radiance env(d).  Bilinear: x = u * W - 0.5, y = (1 - v) * H - 0.5; x0 = floor(x), fx = x - x0, y0 = floor(y),
 * fy = y - y0; columns i0 = x0 mod W (x0 lies in [-1, W - 1]), i1 = (i0 + 1) mod W (wrap); rows j0 = clamp(y0, 0, H - 1),
 * j1 = clamp(y0 + 1, 0, H - 1) (clamp); per channel t = a + fx * (b - a) on row j0 (a at i0, b at i1), the same on row
 * j1, env = t0 + fy * (t1 - t0).  A constant map returns its constant exactly.
 *
 * Sampling tables (rtmi_env_tables; host code in f64, each output rounded once to float).  Texel weight
 * w[j][i] = (the largest channel over the 3 x 3 texels around (j, i), columns wrapped and rows clamped as the lookup does)
 * * sin((j + 0.5) * pi / H) (the cosine of the row centre's latitude).  R[j] = the sum of w[j][i] in column order,
 * total = the sum of R[j] in row order.  row_p[j] = R[j] / total, row_cdf[j] = the running sum of row_p, the last entry
 * exactly 1; col_p[j][i] = w[j][i] / R[j], col_cdf[j][i] its running sum in the row, the last entry exactly 1.  A row
 * with R[j] = 0 has col_p = 0 and col_cdf = 1; a map with total = 0 cannot be sampled (every p = 0, every cdf = 1).
 *
 * Light sample from two uniforms (u1, u2).  Row: the first j with u1 < row_cdf[j] (binary search: lo = 0, hi = H - 1;
 * mid = (lo + hi) >> 1; u1 < cdf[mid] ? hi = mid : lo = mid + 1); column: the same search of u2 in row j.  Remainders
 * fy = min((u1 - c0) / (row_cdf[j] - c0), 1 - 2^-24) with c0 = (j > 0 ? row_cdf[j - 1] : 0), fx likewise in the row.
 * u = (i + fx) / W, v = 1 - (j + fy) / H (i, j, W, H converted to float); phi = (1 - u) * (2 * RTMI_PI_F) - RTMI_PI_F;
 * theta = v * RTMI_PI_F - RTMI_PIO2_F; ct = rtmi_cosf(theta); direction (ct * rtmi_cosf(phi), rtmi_sinf(theta),
 * ct * rtmi_sinf(phi)); pdf = (((p_env * row_p[j]) * col_p[j][i]) * (float)(W * H)) / (RTMI_ENV_2PI2_F * ct).  No
 * sample unless ct > 0, pdf > 0 and pdf < FLT_MAX.  The BSDF-side pdf of a direction d is the same expression for the
 * texel i = min(floor(u * W), W - 1), j = min(floor((1 - v) * H), H - 1) of d's (u, v), with ct = rtmi_cosf(theta) of
 * d's theta; 0 when ct <= 0, when p_env = 0 or when d sees nothing.
 *
 * Estimator (rtmi_render_env).  Paths are rtmi_render's (Philox stream 0), so out_path_sig is rtmi_render's bit for bit.
 * A ray that leaves the world adds L = L + T * (env(d) * w): w = 1 for camera rays, rays after Metal or Dielectric and
 * with nee = 0; after a Lambertian or Isotropic scatter whose vertex read its three stream-3 words (below), with
 * p_b > 0, w = nee_mis_bsdf(p_b, pdf) (include/rtmi_nee.h), 1 when pdf = 0.  The weight does not ask what became of
 * that vertex's light sample: whether it aimed at the map or at an area light, had no sample, or traced no shadow ray,
 * sampling the map was a strategy available at the vertex.  nee = 1 is rtmi_render_nee (include/rtmi_nee.h) with one more light: every scattering
 * Lambertian or Isotropic vertex reads the three stream-3 words of rtmi_nee.h when the map or the light table can be
 * sampled; us = u01(w0) picks the map when us < p_env, else the area light of the table's CDF search with
 * (us - p_env) / (1 - p_env); u01(w1), u01(w2) pick the direction or the point.  p_env = env_select_p when the handle's
 * light table is not empty, 1 when it is, 0 when the map cannot be sampled; an area light's p_l (light sample and BSDF
 * hit alike) is (1 - p_env) * p_l.  The shadow ray toward the map is rtmi_render_nee's (origin x, the sampled direction,
 * the path's time, (t_min, +inf), the item scan with media, free-flight draws from stream 3); V = 1 iff it hits nothing;
 * the sample adds L = L + ((T * albedo) * mis) * env(d), mis = nee_mis_light(p_b, pdf); env(d) is looked up from the
 * sampled direction d, through "Direction -> (u, v)" again, not from the (u, v) the sample was made of.  With p_env = 0
 * the result is rtmi_render_nee's bit for bit.
 */
#ifndef RTMI_ENV_H
#define RTMI_ENV_H

#include "rtmi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTMI_ENV_MAX_SIDE 16384u
#define RTMI_ENV_MAX_TEXELS 33554432u           /* 2^25 */
#define RTMI_ENV_2PI2_F 19.739208802178716f     /* (float)(2 pi^2) */
#define RTMI_ENV_ONE_MINUS 0.99999994039535522f /* 1 - 2^-24 */

/* An environment map: height * width * 3 floats, row 0 the top row. */
typedef struct {
    uint32_t width, height;
    const float *rgb;
} rtmi_env_map; /* 16 B */

/* Options of rtmi_render_env. */
typedef struct {
    uint32_t nee;       /* 0: BSDF sampling only; 1: next-event estimation toward the map and the area lights */
    float env_select_p; /* the probability of sampling the map when the handle has area lights, in (0, 1] */
} rtmi_env_render; /* 8 B */

/* Probe operations of rtmi_probe_env */
#define RTMI_ENV_PROBE_LOOKUP 0 /* in: n directions (x, y, z); out: n x (r, g, b, pdf) */
#define RTMI_ENV_PROBE_SAMPLE 1 /* in: n pairs (u1, u2); out: n x (dx, dy, dz, pdf); all 0 when there is no sample */

/* The sampling tables of `map`.  Pure host code: initialises no device.  Writes row_cdf[H], row_p[H], col_cdf[H * W],
 * col_p[H * W] (any may be NULL) and the f64 total weight to *total (may be NULL).  RTMI_ERR_INVALID for a NULL or bad
 * map. */
int rtmi_env_tables(const rtmi_env_map *map, float *row_cdf, float *row_p, float *col_cdf, float *col_p, double *total);

/* Uploads `map` and its tables to the handle's device, replacing an attached one; NULL detaches.  Waits for the handle's
 * running render before it frees the old map; the map is freed with the handle.  RTMI_ERR_INVALID for a NULL scene or a
 * bad map, before any device work. */
int rtmi_scene_attach_env(rtmi_scene *scene, const rtmi_env_map *map);

/* Blocking whole-image render with the attached map (tile_world must be 1).  Outputs as rtmi_render_nee's.
 * RTMI_ERR_INVALID, before any device work, for a NULL scene, camera, params or opts, for bad params, for
 * RTMI_FLAG_SKY (the map replaces the sky), for nee not 0 or 1, for env_select_p outside (0, 1], for a scene without a map
 * and, with nee = 1, for a scene without a light table (rtmi_scene_attach_lights).  RTMI_ERR_UNSUPPORTED for the flags
 * PROFILE, ASYNC, BLOCK_COOP, PROGRESSIVE, TEST_OVERFLOW and any flag bit not named here, and for tile_world != 1.
 * Accepted: FAST_CULL, SYNC, REF_TREE, FACE_FORWARD, UV_BOOK, and PATH_SIG through out_path_sig.  The result does not
 * depend on FAST_CULL, SYNC, REF_TREE or sample_buffer_bytes (passes). */
int rtmi_render_env(rtmi_scene *scene, const rtmi_camera *cam, const rtmi_render_params *params, const rtmi_env_render *opts,
                    float *out_linear, uint8_t *out_rgb8, float *out_stderr, uint64_t *out_path_sig, rtmi_stats *stats);

/* The device's own code on the attached map, with p_env = 1 (0 when the map cannot be sampled): RTMI_ENV_PROBE_LOOKUP
 * gives env(d) and the BSDF-side pdf, RTMI_ENV_PROBE_SAMPLE the light sample's direction and pdf.  RTMI_ERR_INVALID for a
 * NULL argument, an unknown op or a scene without a map. */
int rtmi_probe_env(rtmi_scene *scene, int op, const float *in, float *out, uint32_t n);

#ifdef __cplusplus
}
#endif
#endif /* RTMI_ENV_H */
