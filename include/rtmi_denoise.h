/* rtmi_denoise.h — an edge-avoiding a-trous denoiser on the MI355X (gfx950), guided by first-hit features.
 *
 * The spatial filter of SVGF (Schied et al. 2017): the a-trous wavelet filter of Dammertz et al. 2010 with edge-stopping
 * weights on normal, depth and luminance, the luminance weight scaled by the propagated variance.  No temporal part.
 * The inputs are what the project renders: the colour and standard error of rtmi_render_adaptive (include/rtmi_adaptive.h)
 * and the albedo, normal and depth of rtmi_render_features (include/rtmi_features.h).  See DESIGN.md §13.
 *
 * Arithmetic.  fp32 throughout, in the order written here, with no fused operations, correctly rounded / and sqrt and no
 * denormal flushing; so a host (tests/denoise_ref.py) reproduces the device output bit for bit.  The output does not
 * depend on the schedule.
 *
 * Pixel classes.  p is a surface pixel iff depth[p] is finite.  Every other pixel is copied from linear to the output
 * unchanged (no demodulation) and never contributes to a neighbour.
 *
 * Prepass, per surface pixel p (c = r, g, b):
 *   a'_c = fmaxf(albedo_c, albedo_min)        x_c = linear_c / a'_c        l(x) = (0.2126f*x_r + 0.7152f*x_g) + 0.0722f*x_b
 *   with stderr_rgb:  s_r = 0.2126f*(stderr_r / a'_r),  s_g = 0.7152f*(stderr_g / a'_g),  s_b = 0.0722f*(stderr_b / a'_b)
 *                     var = (s_r*s_r + s_g*s_g) + s_b*s_b;   without: var = 0
 *   gx = 0.5f*(z[x+1] - z[x-1]) when both horizontal neighbours are in the image and surface pixels; otherwise
 *        z[x+1] - z[p] when that neighbour is; otherwise z[p] - z[x-1] when that one is; otherwise 0
 *   gy   the same along the column (y+1 is the row below)
 * Iteration i = 0 .. iterations-1, step s = 2^i, per surface pixel p, from the (x, var) of the previous iteration:
 *   1. gv = (sum k*var(q)) / (sum k) over the in-image surface pixels q of the 3x3 around p in row-major order, with
 *      k = k3[dy]*k3[dx], k3 = {1/4, 1/2, 1/4}; each term is (k3[dy]*k3[dx])*var(q)
 *   2. with stderr_rgb: inv_l = 1 / (sigma_l*sqrt(gv) + eps_l)
 *   3. taps (dy, dx) in [-2, 2]^2 in row-major order at q = p + s*(dx, dy); q outside the image or not a surface pixel
 *      is skipped.  h = k5[dy]*k5[dx], k5 = {1/16, 1/4, 3/8, 1/4, 1/16}.
 *        centre tap: w = h
 *        other taps: w_n = 1 when normal_power == 0 or either normal has (n.x*n.x + n.y*n.y) + n.z*n.z == 0;
 *                    otherwise d = (np.x*nq.x + np.y*nq.y) + np.z*nq.z and w_n = fmaxf(d, 0) squared log2(normal_power)
 *                    times in succession
 *                    dz = |z_p - z_q| / (sigma_z*(|gx*(float)(s*dx)| + |gy*(float)(s*dy)|) + eps_z)
 *                    dl = |l(x_p) - l(x_q)| * inv_l with stderr_rgb, otherwise 0
 *                    w  = (h*w_n) * rtmi_expf(-(dl + dz))
 *        W += w;  C_c += w*x_c(q);  V += (w*w)*var(q)            (fp32, from +0, in tap order)
 *   4. x'_c = C_c / W;  var' = V / (W*W)
 * Outputs: out_linear_c = x_c*a'_c for surface pixels (the copy of linear for the others); out_rgb8 = the quantisation of
 * rtmi_render (tests/test.rs:71-78) of (double)out_linear: g = sqrt, clamp to [0, 1] with NaN -> 0, (int)(255.99*g).
 * iterations == 0 copies linear for every pixel (no demodulation).
 * Non-finite colour, albedo, normal or stderr values give what this arithmetic gives; they are not tested.
 */
#ifndef RTMI_DENOISE_H
#define RTMI_DENOISE_H

#include "rtmi.h"
#include "rtmi_math.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint32_t iterations;   /* 0..10; 0 copies the input (no demodulation); default 5 */
    uint32_t normal_power; /* 0 (normal weight off) or a power of two <= 1024; default 128 */
    float sigma_l;         /* >= 0, finite; default 4 */
    float sigma_z;         /* >= 0, finite; default 1 */
    float eps_l;           /* > 0, finite; default 1e-10 */
    float eps_z;           /* > 0, finite; default 1e-3 */
    float albedo_min;      /* > 0, finite; default 1e-3 */
    uint32_t flags;        /* must be 0 (reserved) */
} rtmi_denoise_params;     /* 32 bytes */

/* Blocking.  Host pointers, all row-major with row 0 = the top row, as every other output:
 *   linear, albedo, normal: ny*nx*3 floats; depth: ny*nx floats (non-finite = no surface)
 *   stderr_rgb: ny*nx*3 floats (rtmi_render_adaptive's out_stderr), or NULL (then the luminance weight is omitted)
 *   out_linear: ny*nx*3 floats; out_rgb8: ny*nx*3 bytes; either may be NULL
 * Device scratch (about 100 bytes per pixel) is allocated per call and freed before the call returns.
 * RTMI_ERR_INVALID, before any device call, for a NULL p or input other than stderr_rgb, nx or ny of 0 or above 32768,
 * and any parameter outside the ranges above; then RTMI_ERR_UNSUPPORTED for any flag bit; then RTMI_ERR_DEVICE without
 * a device or for a device index out of range. */
int rtmi_denoise(int device, uint32_t nx, uint32_t ny, const rtmi_denoise_params *p, const float *linear,
                 const float *albedo, const float *normal, const float *depth, const float *stderr_rgb, float *out_linear,
                 uint8_t *out_rgb8);

/* rtmi_expf on the device, for the bit-exactness tests (the role rtmi_probe_math plays for rtmi_math.h).
 * RTMI_ERR_INVALID for NULL x or out with n > 0. */
int rtmi_probe_expf(int device, const float *x, float *out, uint32_t n);

#ifdef __cplusplus
}
#endif

#define RTMI_EXPF_LOW (-87.33654f)  /* below: +0 (no subnormal results) */
#define RTMI_EXPF_HIGH 88.72283f    /* above: +inf */

/* exp(x) (Cephes expf, under the rules of rtmi_math.h: + - * /, rint and integer operations only).
 *   n = rint(x*log2e);  r = (x - n*0.693359375f) - n*(-2.12194440e-4f)      (ln 2 in two parts)
 *   e = ((((((1.9875691500e-4f*r + 1.3981999507e-3f)*r + 8.3334519073e-3f)*r + 4.1665795894e-2f)*r
 *          + 1.6666665459e-1f)*r + 5.0000001201e-1f)*(r*r) + r) + 1
 *   result = e * 2^n, the power built from its exponent bits (n == 128: e*2, then 2^127).
 * NaN -> NaN; x < RTMI_EXPF_LOW -> +0; x > RTMI_EXPF_HIGH -> +inf; +-0 -> 1.  At most 2 ulp from the correctly rounded
 * exp on [-87.3, 0]; the filter calls it on x <= 0 only. */
RTMI_HD float rtmi_expf(float x) {
    if (x != x) return x;
    if (x < RTMI_EXPF_LOW) return 0.0f;
    if (x > RTMI_EXPF_HIGH) return rtmi_u2f(0x7f800000u);
    const float k = __builtin_rintf(x * 1.44269504088896341f);
    float r = x - k * 0.693359375f;
    r = r - k * -2.12194440e-4f;
    float p = 1.9875691500e-4f * r + 1.3981999507e-3f;
    p = p * r + 8.3334519073e-3f;
    p = p * r + 4.1665795894e-2f;
    p = p * r + 1.6666665459e-1f;
    p = p * r + 5.0000001201e-1f;
    float e = (p * (r * r) + r) + 1.0f;
    int n = (int)k;
    if (n > 127) {
        e = e * 2.0f;
        n = n - 1;
    }
    return e * rtmi_u2f((uint32_t)(n + 127) << 23);
}

#endif /* RTMI_DENOISE_H */
