/* rtmi_temporal.h — temporal accumulation on the MI355X (gfx950): reproject the previous frames into the current camera
 * and blend them with the current one, per pixel, on the device.
 *
 * The temporal half of SVGF (Schied et al. 2017) without its luminance moments: a history of the demodulated colour, its
 * per-channel variance, depth, normal and length is kept on the device; a push reprojects it through the previous camera
 * (camera motion only), rejects taps across depth and normal discontinuities and blends with weight 1/N.  The inputs are
 * what the project renders (the colour and standard error of rtmi_render_adaptive and of the NEE, env and roulette
 * renders; the albedo, normal and depth of rtmi_render_features); the outputs out_linear and out_stderr are exactly the
 * linear and stderr_rgb that rtmi_denoise (include/rtmi_denoise.h) takes.  See DESIGN.md §27.
 *
 * Arithmetic.  fp32 throughout, in the order written here, with no fused operations, correctly rounded / and sqrt and no
 * denormal flushing; so a host (tests/temporal_ref.py) reproduces every output bit for bit.  The output does not depend
 * on the schedule: a push reads one copy of the history and writes the other.  (float)k is the conversion of an integer.
 *
 * Per pixel p (column i, row r from the top; row 0 = the top row, as every other plane), c = r, g, b:
 *  1. Class.  p is a surface pixel iff depth[p] is finite (rtmi_denoise's rule).  For any other pixel out_linear is
 *     linear and out_stderr is stderr_rgb, bit for bit; N' = 0, motion = (0, 0), and its stored history has N = 0, so
 *     it is never a source.  The steps below are those of a surface pixel.
 *  2. Demodulate.  a'_c = fmaxf(albedo_c, albedo_min) (a'_c = 1 under RTMI_TEMPORAL_NO_DEMODULATE);
 *     x_c = linear_c / a'_c;  with stderr_rgb: e_c = stderr_c / a'_c, v_c = e_c*e_c.
 *  3. World position (skipped under the same-camera rule).  With the current camera (the pinhole at its lens centre;
 *     the lens is ignored):  u = ((float)i + 0.5f) / (float)nx;  v = ((float)(ny-1-r) + 0.5f) / (float)ny;
 *       d_k = ((llc_k + horizontal_k*u) + vertical_k*v) - origin_k      (k = x, y, z)
 *       len = sqrt((d_x*d_x + d_y*d_y) + d_z*d_z);  s = depth / len;  P_k = origin_k + d_k*s
 *     depth is the Euclidean distance of rtmi_render_features.
 *  4. Reprojection into the previous camera (origin o, inverse M of the matrix below):
 *       q_k = P_k - o_k;  a = (M00*q_x + M01*q_y) + M02*q_z;  b = (M10*q_x + M11*q_y) + M12*q_z;
 *       c = (M20*q_x + M21*q_y) + M22*q_z;  z_exp = sqrt((q_x*q_x + q_y*q_y) + q_z*q_z)
 *     The history is invalid unless c > 0.  Then s = a / c;  t = b / c;
 *       fx = s*(float)nx - 0.5f;  fr = (float)(ny-1) - (t*(float)ny - 0.5f)
 *     M, on the host in double at the push that made that camera the previous one: with h = horizontal, w = vertical,
 *     g = lower_left_corner - origin (each component converted to double first) and cross(a, b) =
 *     (a_y*b_z - a_z*b_y, a_z*b_x - a_x*b_z, a_x*b_y - a_y*b_x):
 *       r0 = cross(w, g);  r1 = cross(g, h);  r2 = cross(h, w);  det = (h_x*r0_x + h_y*r0_y) + h_z*r0_z
 *       M0k = (float)(r0_k / det);  M1k = (float)(r1_k / det);  M2k = (float)(r2_k / det)
 *     no fused operations; det == 0 or not finite is RTMI_ERR_INVALID.
 *     Same-camera rule: when the 84 bytes of the previous rtmi_camera equal those of the current one, steps 3 and 4
 *     are skipped: fx = (float)i, fr = (float)r and z_exp = depth exactly, so a standing camera accumulates without
 *     resampling blur.
 *     motion = (fx - (float)i, fr - (float)r) when there is a previous frame and c > 0 (or the cameras are equal);
 *     otherwise (0, 0).
 *  5. History taps.  The history is invalid unless fx and fr are finite, -1 <= fx < (float)nx and -1 <= fr < (float)ny.
 *       x0 = floorf(fx);  w_x1 = fx - x0;  w_x0 = 1 - w_x1;  y0 = floorf(fr);  w_y1 = fr - y0;  w_y0 = 1 - w_y1
 *     Taps in the order (y0, x0), (y0, x0+1), (y0+1, x0), (y0+1, x0+1) with w = w_y*w_x.  A tap is used iff w > 0, it
 *     is in the image, its stored N > 0, |z_tap - z_exp| <= depth_tol*z_exp, and the normal test passes:
 *       l_c = (n_x*n_x + n_y*n_y) + n_z*n_z of the current normal, l_t of the tap's; passes when l_c == 0 or l_t == 0
 *       (medium events, as rtmi_denoise treats zero normals); otherwise
 *       (nc_x*nt_x + nc_y*nt_y) + nc_z*nt_z >= normal_min * sqrt(l_c*l_t)
 *     From +0, in tap order, unused taps left out:  W += w;  X_c += w*x_c(tap);  V_c += (w*w)*var_c(tap);  L += w*N(tap).
 *     x_h = X_c / W;  v_h = V_c / (W*W);  N_h = L / W.  No tap used, or no previous frame: the history is invalid.
 *  6. Blend.  Valid history:  N' = fminf(N_h + 1, (float)max_history);  al = fmaxf(1 / N', alpha_min);  be = 1 - al;
 *       x'_c = be*x_h_c + al*x_c;   v'_c = (be*be)*v_h_c + (al*al)*v_c
 *     Invalid history:  N' = 1;  x' = x;  v' = v.
 *     With al = 1/N and N independent frames of equal variance s2 this keeps x' their mean and v' = s2/N.
 *  7. Store and output.  history <- (x', v', depth, normal, N');  the previous camera <- cam (after every pixel).
 *       out_linear_c = x'_c*a'_c;  out_stderr_c = sqrt(v'_c)*a'_c;  out_history = N'
 * Non-finite colour, albedo, normal or stderr values give what this arithmetic gives; they are not tested.
 */
#ifndef RTMI_TEMPORAL_H
#define RTMI_TEMPORAL_H

#include "rtmi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTMI_TEMPORAL_NO_DEMODULATE 1u /* a'_c = 1: accumulate the colour itself, not colour / albedo */

typedef struct {
    uint32_t max_history; /* 1..65535: the cap of N', so the least blend weight is 1/max_history; default 32 */
    float alpha_min;      /* [0, 1]: the least weight of the current frame; 1 makes every push a copy; default 0 */
    float depth_tol;      /* >= 0, finite: relative depth tolerance of a tap; default 0.05 */
    float normal_min;     /* [-1, 1]: the least cosine between the current and a tap's normal; default 0.9 */
    float albedo_min;     /* > 0, finite; default 1e-3 */
    uint32_t flags;       /* RTMI_TEMPORAL_NO_DEMODULATE; any other bit is RTMI_ERR_UNSUPPORTED */
    uint32_t reserved[2]; /* must be 0 */
} rtmi_temporal_params;   /* 32 bytes */

/* The device-resident history of one image size on one device.  Per pixel it holds two copies (a push reads the
 * neighbours of the previous frame while it writes the current one) of three 16-byte records, {x_r, x_g, x_b, N},
 * {n_x, n_y, n_z, depth} and {var_r, var_g, var_b, 0}: 96 bytes; and the staging of a push's host planes, 52 bytes of
 * inputs and 36 of outputs: 184 bytes per pixel in all, allocated once by rtmi_temporal_create.  Calls on one handle
 * must not overlap; different handles are independent. */
typedef struct rtmi_temporal rtmi_temporal;

/* RTMI_ERR_INVALID, before any device call, for a NULL p or out, nx or ny of 0 or above 32768, a parameter outside the
 * ranges above or a non-zero reserved word; then RTMI_ERR_UNSUPPORTED for an unknown flag bit; then RTMI_ERR_DEVICE
 * without a device, for a device index out of range or when the allocation fails.  *out is NULL after a failure. */
int rtmi_temporal_create(int device, uint32_t nx, uint32_t ny, const rtmi_temporal_params *p, rtmi_temporal **out);

/* Blocking.  Host pointers, all row-major with row 0 = the top row:
 *   cam: the camera the frame was rendered with
 *   linear, albedo, normal: ny*nx*3 floats; depth: ny*nx floats (non-finite = no surface)
 *   stderr_rgb: ny*nx*3 floats, or NULL (then no variance is kept)
 *   out_linear, out_stderr: ny*nx*3 floats; out_history: ny*nx floats; out_motion: ny*nx*2 floats (x, y), in pixels,
 *   where the pixel was in the previous frame minus where it is; each may be NULL
 * Whether standard errors are supplied is fixed by the first push after create or reset; a later push that differs is
 * RTMI_ERR_INVALID, and so is out_stderr without stderr_rgb.
 * RTMI_ERR_INVALID, before any device call and in this order, for a NULL cam or input other than stderr_rgb, a
 * non-finite camera field, a camera whose matrix (step 4) is singular, out_stderr without stderr_rgb, a NULL handle and
 * the stderr mismatch; RTMI_ERR_DEVICE for a failure on the device, after which the handle is as after a reset.  A
 * refused push leaves the history as it was. */
int rtmi_temporal_push(rtmi_temporal *h, const rtmi_camera *cam, const float *linear, const float *albedo,
                       const float *normal, const float *depth, const float *stderr_rgb, float *out_linear,
                       float *out_stderr, float *out_history, float *out_motion);

/* Forgets the previous frame and keeps the allocation: the next push is a first push (and fixes again whether standard
 * errors are supplied).  RTMI_ERR_INVALID for a NULL handle. */
int rtmi_temporal_reset(rtmi_temporal *h);

/* Frees the handle and its device memory.  NULL is allowed. */
void rtmi_temporal_destroy(rtmi_temporal *h);

#ifdef __cplusplus
}
#endif

#endif /* RTMI_TEMPORAL_H */
