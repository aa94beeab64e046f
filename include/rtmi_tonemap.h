/* rtmi_tonemap.h — tone mapping with histogram auto-exposure on the MI355X (gfx950): meter a linear image, adapt the
 * exposure over a frame sequence, apply a tone curve and an output transfer function, all on the device.
 *
 * The display transform every other entry quantises with (the reference's sqrt, a clamp and (int)(255.99*g),
 * tests/test.rs:71-78) is one setting of this one; the others serve images whose radiance is not of order one: scenes under
 * HDR maps, scenes with hundreds of lamps, and the frames of rtmi_frame.h, whose `linear` can be tone-mapped where it
 * lies.  The metering is the log-luminance histogram with percentile cut-offs of interactive renderers, the adaptation an
 * exponential approach with separate speeds toward brighter and darker, the curves Reinhard's extended operator (Reinhard
 * et al. 2002, with a white point) and Narkowicz's fit of the ACES filmic curve.  See DESIGN.md §29.
 *
 * Arithmetic.  fp32 unless it says otherwise, in the order written here, with no fused operations except inside the
 * contract functions rtmi_logf (rtmi_math.h) and rtmi_expf (rtmi_denoise.h), correctly rounded / and sqrt and no denormal
 * flushing; (double) and (float) are conversions, (uint64) and (int) truncate.  So a host (tests/tonemap_ref.py) reproduces
 * every output bit for bit.  The bins are integer counts, so the result does not depend on the schedule.
 *
 * One apply, with `a` the adapted value the handle carries (in log2 of luminance) and `linear` the image:
 *  1. Meter (RTMI_TONEMAP_AUTO only).  Per pixel:
 *       l = (0.2126f*r + 0.7152f*g) + 0.0722f*b                      (rtmi_denoise's luminance)
 *     The pixel is counted iff l is finite and l > 0.  Then
 *       e = rtmi_logf(l) * 1.44269504f
 *       t = (e - log2_min) * scale,   scale = 256.0f / (log2_max - log2_min), once on the host in fp32
 *       b = 0 if t < 0;  255 if t >= 256;  else (int)t
 *       bins[b] += 1
 *  2. Solve (RTMI_TONEMAP_AUTO only; on the device, from the bins).  n = sum of the bins (64-bit).
 *     n == 0: nothing is metered.  a' = a if an adapted value exists, else a' = 0;  metered_log2 = a';  counted = kept = 0;
 *       the handle still counts as having no adapted value if it had none.
 *     Otherwise:
 *       lo = (uint64)((double)n*(double)p_low);   hi = (uint64)((double)n*(double)p_high)
 *       if hi == lo:  when lo == n, lo = n - 1;  then hi = lo + 1
 *       K = hi - lo
 *       with c_b the count of bin b and C_b the count of all bins below it, bin b keeps
 *         k_b = max(0, min(C_b + c_b, hi) - max(C_b, lo))   samples
 *       S = sum of k_b*b in 64-bit integers
 *       m = (float)((double)log2_min + ((double)S/(double)K + 0.5) * (((double)log2_max - (double)log2_min)/256.0))
 *       first apply after create or reset, or no adapted value yet:  a' = m
 *       else  s = (m > a) ? speed_up : speed_down;   al = 1 - rtmi_expf(-(dt*s));   a' = a + (m - a)*al
 *       then  a' = fminf(fmaxf(a', adapt_min), adapt_max);  metered_log2 = m;  counted = n;  kept = K
 *     E = key * rtmi_expf((ev - a') * 0.69314718f)
 *     The solve zeroes the bins for the next call.
 *     RTMI_TONEMAP_MANUAL:  E = rtmi_expf(ev * 0.69314718f), computed on the host (ev = 0 gives exactly 1); the state reports
 *     adapted_log2 = metered_log2 = 0 and counted = kept = 0.
 *  3. Apply, per pixel and channel c:  x = linear_c * E   (E read from the handle's device state)
 *       RTMI_TONEMAP_CLAMP:     y = x
 *       RTMI_TONEMAP_REINHARD:  x = fmaxf(x, 0);  y = (x*(1 + x/w2)) / (1 + x),   w2 = white*white, once on the host in fp32
 *       RTMI_TONEMAP_ACES:      x = fmaxf(x, 0);  y = (x*(2.51f*x + 0.03f)) / (x*(2.43f*x + 0.59f) + 0.14f)
 *     then the output transfer function:
 *       RTMI_TONEMAP_GAMMA2:  the project's quantiser on (double)y:  g = sqrt((double)y), clamped to [0, 1] with NaN -> 0;
 *                             rgb8 = (uint8)(int)(255.99*g);  display = (float)g
 *       RTMI_TONEMAP_SRGB:    v = y clamped to [0, 1] with NaN -> 0;
 *                             s = 12.92f*v when v <= 0.0031308f, else
 *                             s = fminf(1.055f*rtmi_expf(rtmi_logf(v)*0.41666667f) - 0.055f, 1.0f);
 *                             rgb8 = (uint8)(int)(s*255.0f + 0.5f);  display = s
 *     fmaxf(x, 0) of a NaN is 0.  An x whose square overflows (above about 1.8e19) gives inf/inf under ACES, and under
 *     REINHARD with a finite white: y is NaN and the pixel black.
 * Consequence: MANUAL, ev = 0, CLAMP, GAMMA2 gives bit for bit the rgb8 that rtmi_denoise with iterations = 0 and the frame
 * handle give from the same linear.
 */
#ifndef RTMI_TONEMAP_H
#define RTMI_TONEMAP_H

#include "rtmi.h"
#include "rtmi_math.h"
#include "rtmi_denoise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTMI_TONEMAP_CLAMP 0u    /* op: no curve */
#define RTMI_TONEMAP_REINHARD 1u /* op: Reinhard's extended operator with the white point `white` */
#define RTMI_TONEMAP_ACES 2u     /* op: Narkowicz's fit of the ACES filmic curve */

#define RTMI_TONEMAP_GAMMA2 0u /* oetf: the reference's sqrt and (int)(255.99*g) */
#define RTMI_TONEMAP_SRGB 1u   /* oetf: the sRGB curve and round to nearest */

#define RTMI_TONEMAP_MANUAL 0u /* exposure: E = 2^ev */
#define RTMI_TONEMAP_AUTO 1u   /* exposure: metered and adapted; ev is a bias */

typedef struct {
    uint32_t op;         /* offset  0: RTMI_TONEMAP_CLAMP, _REINHARD or _ACES; default _ACES */
    uint32_t oetf;       /* offset  4: RTMI_TONEMAP_GAMMA2 or _SRGB; default _SRGB */
    uint32_t exposure;   /* offset  8: RTMI_TONEMAP_MANUAL or _AUTO; default _AUTO */
    uint32_t flags;      /* offset 12: must be 0; any bit is RTMI_ERR_UNSUPPORTED */
    float ev;            /* offset 16: stops; MANUAL: the exposure, AUTO: a bias; finite, |ev| <= 64; default 0 */
    float white;         /* offset 20: REINHARD's white point, > 0, finite or +inf; default +inf */
    float key;           /* offset 24: AUTO: the luminance the metered mean is mapped to, > 0, finite; default 0.18 */
    float log2_min;      /* offset 28: the histogram's range, finite; default -12 */
    float log2_max;      /* offset 32: finite, log2_max - log2_min >= 1; default 12 */
    float p_low;         /* offset 36: [0, 1): the share of the darkest samples left out; default 0.10 */
    float p_high;        /* offset 40: (p_low, 1]: the samples above this share are left out; default 0.95 */
    float speed_up;      /* offset 44: 1/s, >= 0, finite: adaptation toward a brighter image; default 3 */
    float speed_down;    /* offset 48: 1/s, >= 0, finite: toward a darker one; default 1 */
    float adapt_min;     /* offset 52: finite: the least adapted value; default log2_min */
    float adapt_max;     /* offset 56: finite, >= adapt_min: the greatest; default log2_max */
    uint32_t reserved;   /* offset 60: must be 0 */
} rtmi_tonemap_params;   /* 64 bytes */

typedef struct {
    float exposure;       /* offset  0: the factor E that was applied */
    float adapted_log2;   /* offset  4: a' */
    float metered_log2;   /* offset  8: m */
    uint32_t counted;     /* offset 12: n */
    uint32_t kept;        /* offset 16: K */
    uint32_t applies;     /* offset 20: applies since create or reset, this one included */
    uint32_t reserved[2]; /* offset 24: written as 0 */
} rtmi_tonemap_state;     /* 32 bytes */

/* A handle belongs to one device and one image size.  It holds 256 uint32 bins and a small state record in device memory
 * (and, after the first rtmi_tonemap_apply, the staging of that form: 27 bytes per pixel).  Calls on one handle must not
 * overlap; different handles are independent. */
typedef struct rtmi_tonemap rtmi_tonemap;

/* RTMI_ERR_INVALID, before any device call and with "rtmi_tonemap_create" in rtmi_last_error(), for a NULL p or out, nx
 * or ny of 0 or above 32768, a field outside its range above (op, oetf and exposure above their last value included;
 * fields the chosen operator or mode does not read are checked too) or a non-zero reserved word; then
 * RTMI_ERR_UNSUPPORTED for a flag bit; then RTMI_ERR_DEVICE without a device, for a device index out of range or when the
 * allocation fails.  *out is NULL after a failure. */
int rtmi_tonemap_create(int device, uint32_t nx, uint32_t ny, const rtmi_tonemap_params *p, rtmi_tonemap **out);

/* Blocking.  Host pointers: linear is ny*nx*3 floats, row-major with row 0 = the top row; out_rgb8 ny*nx*3 bytes,
 * out_display ny*nx*3 floats, out_state one record; each output may be NULL, but not all three.  dt: the seconds since the
 * previous apply (read by the adaptation only).  The device staging is allocated on the first call of this form and kept.
 * RTMI_ERR_INVALID, before any device call and in this order, for a NULL linear, a dt that is negative or not finite,
 * every output NULL, and a NULL handle (checked last, so a machine without a device answers for every other argument);
 * RTMI_ERR_DEVICE for a failure on the device, after which the handle is as after a reset.  A refused call leaves the
 * state as it was. */
int rtmi_tonemap_apply(rtmi_tonemap *h, const float *linear, float dt, uint8_t *out_rgb8, float *out_display,
                       rtmi_tonemap_state *out_state);

/* Asynchronous: the same apply enqueued on `stream` (a hipStream_t; NULL = the default stream) with device pointers on
 * the handle's device.  It allocates nothing and reads nothing back to the host.  It writes exactly ny*nx*3 bytes to
 * d_rgb8, ny*nx*3 floats to d_display and 32 bytes to d_state (each may be NULL, but not all three), and nothing beyond.
 * Successive applies on one handle must be ordered by their streams.  rtmi_tonemap_apply runs on a stream of the handle's
 * own, which waits for no other: synchronise the stream of a device-form apply before the host form, rtmi_tonemap_reset
 * aside, is used on the same handle.  After RTMI_ERR_DEVICE the handle is as after a reset, as for the host form: the
 * next apply is a first apply and zeroes the bins on its stream before it meters.
 * The checks of rtmi_tonemap_apply, and RTMI_ERR_INVALID (between the outputs and the handle) for a d_linear or d_display
 * that is not 16-byte aligned or a d_rgb8 or d_state that is not 4-byte aligned. */
int rtmi_tonemap_apply_device(rtmi_tonemap *h, const void *d_linear, float dt, void *d_rgb8, void *d_display, void *d_state,
                              void *stream);

/* The next apply is a first apply: it adopts the metered value and counts from 1.  RTMI_ERR_INVALID for a NULL handle. */
int rtmi_tonemap_reset(rtmi_tonemap *h);

/* Frees the handle and its device memory, after its enqueued work.  NULL is allowed. */
void rtmi_tonemap_destroy(rtmi_tonemap *h);

/* The metering kernel alone on the caller's (host) data, for the tests: out_bins = the 256 bins of step 1 (the probe
 * meters whatever p->exposure says).  RTMI_ERR_INVALID for a NULL p, linear or out_bins and what
 * rtmi_tonemap_create refuses; then RTMI_ERR_UNSUPPORTED; then RTMI_ERR_DEVICE. */
int rtmi_probe_tonemap_histogram(int device, uint32_t nx, uint32_t ny, const rtmi_tonemap_params *p, const float *linear,
                                 uint32_t *out_bins);

#ifdef __cplusplus
}
#endif

#endif /* RTMI_TONEMAP_H */
