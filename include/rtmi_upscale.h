/* rtmi_upscale.h — guided upscaling on the MI355X (gfx950): an image rendered at a low resolution is rebuilt at the full
 * resolution under the guidance of first-hit features (albedo, normal, depth) rendered at both resolutions.
 *
 * The lit paths are what a frame costs; the first-hit features are cheap at any size (rtmi_features.h) and the camera maps
 * [0,1]^2 to any image size.  So the lit image is rendered small and each full-resolution pixel is rebuilt from the four
 * low-resolution pixels around it: a joint bilateral upsampling (Kopf et al. 2007) of the demodulated colour (colour /
 * albedo, as rtmi_denoise.h filters it), with the bilinear weights cut by normal and depth differences between the
 * full-resolution pixel and each tap, remodulated with the full-resolution albedo.  rtmi_upscale is the reconstruction
 * alone on the caller's planes; rtmi_upscaler is a handle that renders a low-resolution frame (rtmi_frame.h) and the
 * full-resolution features and reconstructs, all on the device.  See DESIGN.md §30.
 *
 * Arithmetic.  fp32 throughout, in the order written here, with no fused operations outside rtmi_expf (rtmi_denoise.h),
 * correctly rounded / and sqrt and no denormal flushing; (float), (int) and (double) are conversions.  So a host
 * (tests/upscale_ref.py) reproduces every output bit for bit.  All planes are row-major with row 0 = the top row.
 *
 * Inputs.  Low resolution, lx x ly: linear_lo, albedo_lo, normal_lo (3 floats per pixel), depth_lo (1 float per pixel).
 * Full resolution, nx x ny, the guide: albedo, normal, depth.  1 <= lx <= nx <= 32768 and 1 <= ly <= ny <= 32768; the ratios
 * need not be integers.  A pixel of either image is a surface pixel iff its depth is finite (rtmi_denoise.h's rule).
 *
 * Per full-resolution pixel p = (x, y):
 *  1. Taps.  sx = (float)lx / (float)nx and sy = (float)ly / (float)ny, once on the host in fp32.
 *       fx = ((float)x + 0.5f)*sx - 0.5f;   x0 = (int)floorf(fx);   tx = fx - (float)x0;   the same for y
 *     x0 can be -1 and x0 + 1 can be lx.  The taps are q = (x0 + i, y0 + j), j = 0, 1 outer and i = 0, 1 inner, with
 *       b = wy_j * wx_i,   w_0 = 1.0f - t,   w_1 = t
 *     A tap outside the low image is skipped (it is not added with weight 0), and so is a tap whose b is 0: where tx is
 *     exactly 0 (every pixel when lx == nx) the column x0 + 1 does not exist for p.  "Tap" below means a tap not skipped;
 *     every p has at least one.
 *  2. p is a surface pixel: only the surface taps are used.  Per surface tap q, c = r, g, b:
 *       a'_c(q) = fmaxf(albedo_lo_c(q), albedo_min);    x_c(q) = linear_lo_c(q) / a'_c(q)
 *       w_n = 1 when normal_power == 0 or either normal has (n.x*n.x + n.y*n.y) + n.z*n.z == 0; otherwise
 *             d = (np.x*nq.x + np.y*nq.y) + np.z*nq.z and w_n = fmaxf(d, 0) squared log2(normal_power) times in succession
 *             (rtmi_denoise.h's normal weight)
 *       dz = fabsf(z_p - z_q) / (sigma_z*z_p + eps_z)
 *       e = w_n * rtmi_expf(-dz);    w = b * e
 *       W += w;   C_c += w*x_c(q)                                     (from +0, in tap order)
 *     class 1, guided:  W > w_min.   out_c = (C_c / W) * a'_c(p),   a'_c(p) = fmaxf(albedo_c(p), albedo_min)
 *     class 2, nearest-similar:  otherwise, when there is a surface tap: the surface tap with the greatest e (the first
 *       surface tap in tap order, replaced by a later one only when that one's e is greater).   out_c = x_c(q) * a'_c(p)
 *  3. p is not a surface pixel: only the non-surface taps are used, without demodulation.
 *     class 0, background:  out_c = (sum of b*linear_lo_c(q)) / (sum of b)          (both from +0, in tap order)
 *  4. class 3, mismatch: no tap of p's kind (a surface p without a surface tap, a background p without a background tap).
 *       out_c = (sum of b*linear_lo_c(q)) / (sum of b) over all taps: the plain bilinear mean
 * Outputs: linear = out; rgb8 = the quantisation of rtmi_render (tests/test.rs:71-78) of (double)out, as rtmi_denoise's:
 * g = sqrt, clamp to [0, 1] with NaN -> 0, (int)(255.99*g); cls[p] = the class number.  cls tells a caller where the low image
 * held nothing that matched: the hook for a later pass that traces those pixels again.
 * Non-finite colour, albedo or normal values and negative depths give what this arithmetic gives; they are not tested.
 *
 * The defaults below are judgement; they have not been tuned on a device.
 */
#ifndef RTMI_UPSCALE_H
#define RTMI_UPSCALE_H

#include "rtmi.h"
#include "rtmi_math.h"
#include "rtmi_denoise.h"
#include "rtmi_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTMI_UPSCALE_BACKGROUND 0u /* cls: not a surface pixel, mean of the non-surface taps */
#define RTMI_UPSCALE_GUIDED 1u     /* cls: the weighted mean of the surface taps */
#define RTMI_UPSCALE_NEAREST 2u    /* cls: the most similar surface tap alone */
#define RTMI_UPSCALE_MISMATCH 3u   /* cls: no tap of the pixel's kind, the plain bilinear mean */

typedef struct {
    uint32_t normal_power; /* offset  0: 0 (normal weight off) or a power of two <= 1024; default 32 */
    float sigma_z;         /* offset  4: >= 0, finite: the relative depth difference that costs a factor e; default 0.05 */
    float eps_z;           /* offset  8: > 0, finite; default 1e-3 */
    float albedo_min;      /* offset 12: > 0, finite; default 1e-3 */
    float w_min;           /* offset 16: >= 0, finite: at or below this total weight the pixel is not class 1; default 1e-3 */
    uint32_t flags;        /* offset 20: must be 0; any bit is RTMI_ERR_UNSUPPORTED */
    uint32_t reserved[2];  /* offset 24: must be 0 */
} rtmi_upscale_params;     /* 32 bytes */

typedef struct {
    const float *linear_lo; /* offset  0: ly*lx*3 floats, the low-resolution image */
    const float *albedo_lo; /* offset  8: ly*lx*3 floats */
    const float *normal_lo; /* offset 16: ly*lx*3 floats */
    const float *depth_lo;  /* offset 24: ly*lx floats, non-finite = no surface */
    const float *albedo;    /* offset 32: ny*nx*3 floats, the guide */
    const float *normal;    /* offset 40: ny*nx*3 floats */
    const float *depth;     /* offset 48: ny*nx floats */
    const void *reserved;   /* offset 56: must be NULL */
} rtmi_upscale_in;          /* 64 bytes */

typedef struct {
    float *linear;  /* offset  0: ny*nx*3 floats, or NULL */
    uint8_t *rgb8;  /* offset  8: ny*nx*3 bytes, or NULL */
    uint8_t *cls;   /* offset 16: ny*nx bytes, RTMI_UPSCALE_* per pixel, or NULL */
    void *reserved; /* offset 24: must be NULL */
} rtmi_upscale_out; /* 32 bytes */

/* Blocking.  Host pointers.  Device scratch (40 bytes per low-resolution and 44 per full-resolution pixel) is allocated per
 * call and freed before the call returns.
 * Refusals, in this order and each message prefixed "rtmi_upscale: ": RTMI_ERR_INVALID, before any device call, for a NULL
 * p, in, out or input plane; a size outside 1 <= lx <= nx <= 32768, 1 <= ly <= ny <= 32768; a parameter outside its range
 * above or a non-zero reserved word or pointer; every output NULL; then RTMI_ERR_UNSUPPORTED for a flag bit; then
 * RTMI_ERR_DEVICE without a device, for a device index out of range or a failure on the device. */
int rtmi_upscale(int device, uint32_t lx, uint32_t ly, uint32_t nx, uint32_t ny, const rtmi_upscale_params *p,
                 const rtmi_upscale_in *in, const rtmi_upscale_out *out);

/* Asynchronous: the same reconstruction enqueued on `stream` (a hipStream_t; NULL = the default stream) with d_in and d_out
 * (host structs) holding device pointers on `device`.  It allocates nothing and reads nothing back to the host.  It writes
 * exactly ny*nx*3 floats to linear, ny*nx*3 bytes to rgb8 and ny*nx bytes to cls, and nothing beyond.
 * The checks of rtmi_upscale in "rtmi_upscale_device: "'s name, and RTMI_ERR_INVALID (after the outputs, before the flags)
 * for a float plane that is not 16-byte aligned or an rgb8 or cls that is not 4-byte aligned. */
int rtmi_upscale_device(int device, uint32_t lx, uint32_t ly, uint32_t nx, uint32_t ny, const rtmi_upscale_params *p,
                        const rtmi_upscale_in *d_in, const rtmi_upscale_out *d_out, void *stream);

typedef struct {
    rtmi_frame_opts low;    /* offset   0: the low-resolution frame's estimator, history and filter (rtmi_frame.h) */
    rtmi_upscale_params up; /* offset  96: the reconstruction's parameters */
    uint32_t lx;            /* offset 128: the low resolution, 1 <= lx <= params->nx */
    uint32_t ly;            /* offset 132: 1 <= ly <= params->ny */
    uint32_t guide_ns;      /* offset 136: samples per pixel of the full-resolution features, >= 1; default 4 */
    uint32_t reserved[5];   /* offset 140: must be 0 */
} rtmi_upscaler_opts;       /* 160 bytes */

/* The planes of an upscaled frame; each pointer may be NULL, and a NULL plane is not copied.  Host pointers for
 * rtmi_upscaler_render, pointers on the scene's device for rtmi_upscaler_render_device. */
typedef struct {
    float *linear;      /* offset  0: ny*nx*3 floats, the reconstructed image */
    uint8_t *rgb8;      /* offset  8: ny*nx*3 bytes, its quantisation */
    uint8_t *cls;       /* offset 16: ny*nx bytes, RTMI_UPSCALE_* per pixel */
    float *albedo;      /* offset 24: ny*nx*3 floats, the full-resolution guide (rtmi_features.h) */
    float *normal;      /* offset 32: ny*nx*3 floats */
    float *depth;       /* offset 40: ny*nx floats */
    rtmi_frame_out low; /* offset 48: the low-resolution frame's planes, ly*lx pixels each.  The host form copies linear,
                           albedo, normal and depth only and refuses another plane; the device form writes every plane */
} rtmi_upscaler_out;    /* 144 bytes */

typedef struct rtmi_upscaler rtmi_upscaler;

/* Threads.  A render call takes its scene's hold twice, once for the low frame and once for the features and the
 * reconstruction; between the two another render of the scene may run, which does not touch the handle's planes.  Calls on
 * one handle serialise on a lock of the handle's own, so a second thread's render waits for the first; they, and other
 * renders of the scene, serialise on the scene as a frame's do.  Several handles may live on one scene and do not see each
 * other.  A handle must be destroyed before its scene, and not while a call on it runs. */

/* A handle bound to a scene, a full size and a low size.  `params` fixes the full size nx x ny and everything
 * rtmi_frame_create reads from it; the low-resolution frame is made by rtmi_frame_create from a copy of it with nx = lx and
 * ny = ly.  Allocates the planes the handle keeps: the low frame's linear, albedo, normal and depth (40 B per low pixel) and
 * the full-resolution linear, rgb8 and cls (16 B per full pixel), beside the low frame's own memory; a render call
 * allocates nothing (the scene's own render buffers grow on first use).  *out is NULL after a failure.
 * Refusals, in this order and each message prefixed "rtmi_upscaler_create: ": RTMI_ERR_INVALID for a NULL params, opts or
 * out; a size outside 1 <= lx <= nx <= 32768, 1 <= ly <= ny <= 32768; a field of opts->up outside its range or a non-zero
 * reserved word of it; guide_ns of 0; a non-zero reserved word of opts; RTMI_ERR_UNSUPPORTED for a bit of opts->up.flags
 * or guide_ns >= 2^26; then what rtmi_frame_create refuses for the low frame, in its order (the NULL scene last among its
 * argument checks, then the device). */
int rtmi_upscaler_create(rtmi_scene *scene, const rtmi_render_params *params, const rtmi_upscaler_opts *opts,
                         rtmi_upscaler **out);

/* Blocking.  One frame under `cam`: (1) rtmi_frame_render_device of the low frame with ns samples per pixel and `seed` into
 * the handle's planes; (2) under one hold on the scene, the first-hit features at the full size with guide_ns samples per
 * pixel, the same seed and the flags without RTMI_FLAG_LIGHT_COOP, the reconstruction on the scene's stream, and the copies
 * of the planes asked for to the host.  Every full-resolution plane has the bits of rtmi_upscale applied to the low frame's
 * linear, albedo, normal and depth and to rtmi_render_features(nx, ny, guide_ns, seed).  stats (may be NULL): the lit
 * render's.
 * Refusals, each message prefixed "rtmi_upscaler_render: ": RTMI_ERR_INVALID for a NULL cam or out and for a plane of
 * out->low other than linear, albedo, normal and depth; then what rtmi_frame_render refuses, in its order (the NULL handle
 * last among its argument checks).  After a failure on the device or a cancellation the history is as after
 * rtmi_upscaler_reset; a refused call leaves it as it was. */
int rtmi_upscaler_render(rtmi_upscaler *h, const rtmi_camera *cam, uint32_t ns, uint64_t seed, const rtmi_upscaler_out *out,
                         rtmi_stats *stats);

/* The same call with `out` holding device pointers on the scene's device; no plane passes through the host.  Blocking too.
 * Every plane of out->low may be asked for.  Messages are prefixed "rtmi_upscaler_render_device: ". */
int rtmi_upscaler_render_device(rtmi_upscaler *h, const rtmi_camera *cam, uint32_t ns, uint64_t seed,
                                const rtmi_upscaler_out *out, rtmi_stats *stats);

/* Forgets the frames rendered so far (rtmi_frame_reset of the low frame).  RTMI_ERR_INVALID for a NULL handle. */
int rtmi_upscaler_reset(rtmi_upscaler *h);

/* Frees the handle, its low frame and its device memory, after the scene's running work.  NULL is allowed.  A handle must
 * be destroyed before its scene. */
void rtmi_upscaler_destroy(rtmi_upscaler *h);

#ifdef __cplusplus
}
#endif

#endif /* RTMI_UPSCALE_H */
