/* rtmi_gather.h — hemisphere gathers: irradiance and spherical-harmonic probes at batches of caller-supplied points, on
 * the MI355X (gfx950) device path.  See DESIGN.md §26.
 *
 * rtmi_radiance (rtmi_radiance.h) answers "how much light arrives along this ray".  These entries answer the question a
 * baker asks: how much light arrives AT this point.  The caller gives points (and normals); the device draws the
 * directions, traces one path of rtmi_radiance along each, and reduces per point.  No ray is generated, stored or uploaded
 * by the host, and the scratch is bounded however large the batch.
 *
 * Modes.
 *   RTMI_GATHER_COSINE  points + normals: the irradiance E = integral of L cos(theta) over the normal's hemisphere, from spp
 *                       cosine-distributed directions per point: E = pi * mean.
 *   RTMI_GATHER_SPHERE  points only: the mean radiance over the sphere from spp uniform directions, and optionally its
 *                       projection on the 9 real spherical harmonics of bands 0..2.
 *
 * Directions (fp32, each operation rounded once, no fused operations; the order below and in the inline functions at the
 * end of this header is the specification: the kernels and rtmi_gather_directions compile those functions).
 *   Direction s of point i reads words w0 and w1 of the Philox4x32-10 block with counter
 *   (0, first_sample + s, first_point + i, 5) under the key `seed` (stream 5: no path stream of rtmi.h, rtmi_nee.h or
 *   rtmi_roulette.h has that id).  u1 = rtmi_u01(w0), u2 = rtmi_u01(w1), phi = RTMI_GATHER_2PI_F * u2,
 *   c = rtmi_cosf(phi), sn = rtmi_sinf(phi).
 *   COSINE.  r = sqrtf(u1), x = r * c, y = r * sn, z = sqrtf(1 - u1).
 *     The normal: l2 = (n.x * n.x + n.y * n.y) + n.z * n.z, l = sqrtf(l2), m = (n.x / l, n.y / l, n.z / l).  A normal whose
 *     l is zero or not finite is refused (so is one too short or too long for l2 in fp32).
 *     The frame (branch-free, after Duff et al. 2017): sign = copysignf(1, m.z), a = -1 / (sign + m.z),
 *     b = (m.x * m.y) * a, t = (1 + ((sign * m.x) * m.x) * a, sign * b, (-sign) * m.x), bt = (b, sign + (m.y * m.y) * a, -m.y).
 *     d = ((x * t) + (y * bt)) + (z * m) per component, not renormalised.
 *   SPHERE.  z = 1 - 2 * u1, r = sqrtf(max(0, 1 - z * z)), d = (r * c, r * sn, z), not renormalised.
 *
 * Paths.  Path (i, s) is the path rtmi_radiance traces for the ray (o = points[i], t_min = params.t_min, d, t_max = +inf)
 *   at time time[i] (or 0) with first_ray = first_point + i, first_sample + s, stream_skip = 0 and the same estimator,
 *   flags, max_depth, t_min, seed and env_select_p: bit for bit that call's sample.  Flags and attachments follow
 *   rtmi_radiance: 0, RTMI_FLAG_FAST_CULL, _SKY (refused with a map estimator), _FACE_FORWARD, _UV_BOOK; NEE and ENV_NEE
 *   need the light table, ENV and ENV_NEE the map.  No Russian roulette, no light tree.
 *
 * Reduction, per point, over x_s = the fp32 radiance of path (i, s), in sample order (the additions of rtmi_radiance's
 *   resolve), per channel, in f64 without fused operations:
 *     sum = sum + (double)x_s;  Welford's recurrence of rtmi_adaptive.h: dl = x - m, m = m + dl / (s + 1),
 *     M2 = M2 + dl * (x - m);  mean = sum / spp;  se = sqrt(M2 / (spp * (spp - 1))).
 *   COSINE:  value = (float)(RTMI_GATHER_PI * mean), stderr = (float)(RTMI_GATHER_PI * se).
 *   SPHERE:  value = (float)mean, stderr = (float)se, and with an sh output
 *     acc[k] = acc[k] + (double)x_s * (double)Y_k(d_s),  sh[k] = (float)((RTMI_GATHER_4PI / spp) * acc[k]),  k = 0..8,
 *     with Y_k in fp32 by rtmi_gather_sh9 from the direction d_s, which the resolve draws again from its counter: no
 *     direction is ever stored.
 *   spp == 1 writes +inf to stderr: no estimate, as the radiance query.
 *   Layouts: value and stderr n * 3 floats; sh n * 9 * 3 floats, [point][k][channel].
 *
 * Spherical harmonics.  The real basis without the Condon-Shortley phase (Ramamoorthi and Hanrahan 2001), in the order
 *   k = 0: Y00;  1, 2, 3: Y1-1 (y), Y10 (z), Y11 (x);  4..8: Y2-2 (xy), Y2-1 (yz), Y20 (3z^2 - 1), Y21 (xz), Y22 (x^2 - y^2).
 *   The irradiance of a normal m from a probe is sum_k A_band(k) * sh[k] * Y_k(m) with the cosine-lobe factors
 *   A = (pi, 2 pi / 3, pi / 4).
 *
 * Slabs.  The per-sample buffer, 12 bytes per path, is scratch.  Both forms walk the points in slabs; no output bit
 *   depends on the slab size, and neither form limits n * spp.  One point's samples are one slab's: spp < 2^31.
 *   Host form: slabs of params.slab_points points; 0 selects 256 MiB / (12 * spp).  Either is held to at least 1 and to
 *   at most (2^31 - 1) / spp.  The scratch is the grow-only per-sample buffer of the handle that rtmi_radiance uses.
 *   Device form: the largest slab that fits scratch_bytes, under the same bounds (and params.slab_points, when not 0).
 *
 * The calls follow the handle's thread model (rtmi.h): calls on one handle serialise.
 */
#ifndef RTMI_GATHER_H
#define RTMI_GATHER_H

#include "rtmi.h"
#include "rtmi_math.h"
#include "rtmi_radiance.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTMI_GATHER_COSINE 0u /* points + normals: irradiance E = integral of L cos(theta) over the normal's hemisphere */
#define RTMI_GATHER_SPHERE 1u /* points only: mean radiance over the sphere and its 9 real SH coefficients (bands 0..2) */

#define RTMI_GATHER_STREAM 5u /* the Philox stream id of the directions */

typedef struct {
    uint32_t n;            /* points in this call */
    uint32_t spp;          /* directions (independent paths) per point, 1 .. 2^31 - 1 */
    uint32_t mode;         /* RTMI_GATHER_COSINE / _SPHERE */
    uint32_t estimator;    /* RTMI_ROULETTE_PLAIN / _NEE / _ENV / _ENV_NEE of rtmi_roulette.h (no roulette here) */
    uint32_t flags;        /* as rtmi_radiance_params */
    uint32_t max_depth;    /* as rtmi_render_params */
    float    t_min;        /* of every segment, the first included, and of shadow rays (the render's 0.001) */
    uint64_t seed;         /* the render key (at offset 32) */
    uint64_t first_point;  /* index of this call's point 0 in the caller's batch */
    uint32_t first_sample; /* index of this call's sample 0 */
    uint32_t slab_points;  /* points per slab; 0: the default */
    float    env_select_p; /* as rtmi_env_render; read by ENV_NEE only */
} rtmi_gather_params; /* 64 B */

/* Blocking, host pointers.  points: n * 3 floats; normals: n * 3 floats (COSINE; ignored by SPHERE, may be NULL); time: n
 * floats, or NULL for time 0; out_value, out_stderr: n * 3 floats each, out_sh: n * 27 floats (SPHERE only), each optional,
 * not all NULL.  kernel_ms: optional, the kernels' time by HIP events, summed over the slabs.  n == 0 is RTMI_OK and
 * launches nothing.
 * RTMI_ERR_INVALID, with the entry's name in rtmi_last_error(), for a NULL scene, params or points, every output NULL,
 * spp == 0 or >= 2^31, max_depth == 0, a non-finite t_min, a mode outside 0..1, an estimator outside 0..3, COSINE without
 * normals, out_sh with COSINE, first_point + n > 2^32, first_sample + spp > 2^32, ENV_NEE with env_select_p outside
 * (0, 1], SKY with a map estimator, a missing attachment, a point or time that is not finite and a normal whose fp32 length
 * is zero or not finite (the message names the point).  RTMI_ERR_UNSUPPORTED for unknown flags.  All of these are answered
 * before any device work. */
int rtmi_gather(rtmi_scene *scene, const rtmi_gather_params *params, const float *points, const float *normals, const float *time,
                float *out_value, float *out_stderr, float *out_sh, double *kernel_ms);

/* Asynchronous, DEVICE pointers on the scene's device, enqueued on `stream` (a hipStream_t) behind the handle's previous
 * call, like rtmi_radiance_device.  d_scratch (4-byte aligned) is the per-sample buffer: scratch_bytes >= 12 * spp, else
 * RTMI_ERR_INVALID; the call allocates nothing, writes at most min(n, scratch_bytes / (12 * spp)) * spp * 12 bytes of it,
 * exactly n records to each output given and nothing beyond, and takes the caller's word for the points and normals. */
int rtmi_gather_device(rtmi_scene *scene, const rtmi_gather_params *params, const void *d_points, const void *d_normals,
                       const void *d_time, void *d_value, void *d_stderr, void *d_sh, void *d_scratch, uint64_t scratch_bytes,
                       void *stream);

/* The directions of a call on the host, compiled from the inline functions below: out_dirs receives n * spp * 3 floats,
 * [point][sample][3].  Pure host code, initialises no device.  Reads mode, spp, seed, first_point and first_sample of
 * params (params->n is not read: the count is the argument n); normals as rtmi_gather.  RTMI_ERR_INVALID for NULL
 * arguments, a bad mode, spp == 0, the two overflow rules and a refused normal. */
int rtmi_gather_directions(const rtmi_gather_params *params, const float *normals, uint32_t n, float *out_dirs);

#ifdef __cplusplus
}
#endif

/* ---- the arithmetic of the directions and of the basis: the specification, compiled by the kernels and the host ------ */

#define RTMI_GATHER_2PI_F 6.2831854820251465f /* 2 * RTMI_PI_F, exact */
#define RTMI_GATHER_PI 3.141592653589793      /* f64 pi of the reduction */
#define RTMI_GATHER_4PI 12.566370614359172    /* f64 4 pi of the SH projection */

#define RTMI_SH_Y00 0.2820947917738781f  /* 1 / (2 sqrt(pi)) */
#define RTMI_SH_Y1 0.4886025119029199f   /* sqrt(3 / (4 pi)) */
#define RTMI_SH_Y2A 1.0925484305920792f  /* sqrt(15 / (4 pi)): xy, yz, xz */
#define RTMI_SH_Y20 0.31539156525252005f /* sqrt(5 / (16 pi)) */
#define RTMI_SH_Y22 0.5462742152960396f  /* sqrt(15 / (16 pi)) */

/* The fp32 length of a normal as the frame sees it; zero or not finite: the normal is refused. */
RTMI_HD float rtmi_gather_normal_length(const float n[3]) {
    const float l2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    return __builtin_sqrtf(l2);
}

/* COSINE: the direction of the uniforms (u1, u2) about the normal n (any accepted length). */
RTMI_HD void rtmi_gather_cosine(float u1, float u2, const float n[3], float d[3]) {
    const float phi = RTMI_GATHER_2PI_F * u2;
    const float r = __builtin_sqrtf(u1);
    const float x = r * rtmi_cosf(phi), y = r * rtmi_sinf(phi);
    const float z = __builtin_sqrtf(1.0f - u1);
    const float l = rtmi_gather_normal_length(n);
    const float mx = n[0] / l, my = n[1] / l, mz = n[2] / l;
    const float sign = __builtin_copysignf(1.0f, mz);
    const float a = -1.0f / (sign + mz);
    const float b = (mx * my) * a;
    const float tx = 1.0f + ((sign * mx) * mx) * a, ty = sign * b, tz = (-sign) * mx;
    const float bx = b, by = sign + (my * my) * a, bz = -my;
    d[0] = ((x * tx) + (y * bx)) + (z * mx);
    d[1] = ((x * ty) + (y * by)) + (z * my);
    d[2] = ((x * tz) + (y * bz)) + (z * mz);
}

/* SPHERE: the uniform direction of the uniforms (u1, u2). */
RTMI_HD void rtmi_gather_sphere(float u1, float u2, float d[3]) {
    const float phi = RTMI_GATHER_2PI_F * u2;
    const float z = 1.0f - 2.0f * u1;
    const float r = __builtin_sqrtf(__builtin_fmaxf(0.0f, 1.0f - z * z));
    d[0] = r * rtmi_cosf(phi);
    d[1] = r * rtmi_sinf(phi);
    d[2] = z;
}

/* The nine real spherical harmonics of bands 0..2 at the unit direction d. */
RTMI_HD void rtmi_gather_sh9(const float d[3], float y[9]) {
    const float x = d[0], yy = d[1], z = d[2];
    y[0] = RTMI_SH_Y00;
    y[1] = RTMI_SH_Y1 * yy;
    y[2] = RTMI_SH_Y1 * z;
    y[3] = RTMI_SH_Y1 * x;
    y[4] = RTMI_SH_Y2A * (x * yy);
    y[5] = RTMI_SH_Y2A * (yy * z);
    y[6] = RTMI_SH_Y20 * (3.0f * (z * z) - 1.0f);
    y[7] = RTMI_SH_Y2A * (x * z);
    y[8] = RTMI_SH_Y22 * (x * x - yy * yy);
}

#endif /* RTMI_GATHER_H */
