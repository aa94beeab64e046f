/* rtmi_window.h — adaptive sampling per pixel with a neighbourhood stopping rule, driven from the device, on the MI355X
 * (gfx950) device path.  See DESIGN.md §33.
 *
 * The per-pixel entries of DESIGN.md §32 test every pixel alone: a pixel retires on an estimate that has not yet seen a rare
 * bright path, and the image shows it as a blotch.  rtmi_render_adaptive (rtmi_adaptive.h) keeps such a pixel alive through
 * the 63 others of its fixed 8x8 tile, and pays for it with a read-back per step.  These entries sit in between: a pixel
 * stays alive while any pixel within a Chebyshev radius r of it is still noisy.  The loop stays device-driven without a
 * read-back; the select, the path kernel and the step kernel of DESIGN.md §31 / §32 run unchanged, and one small kernel per
 * step, the spread, is added.
 *
 * The rule.  The lattice of counts, the samples, the arithmetic, the own-pixel test and the planes are those of DESIGN.md §32:
 *   the counts run min_spp, min_spp + step_spp, ..., ns = params->ns (the cap), the last step shortened; step 0 traces samples
 *   [0, min_spp) of every pixel; a pixel is tested in double, converged iff in every channel e = sqrt(M2 / (n (n - 1))) and
 *   mean = sum / n are finite and e <= abs_tol + rel_tol * |mean|.  Two byte planes per image are involved: active (1: traced
 *   by the next step) and fail.  After a step that brought the live pixels to count n, the step kernel of §32 writes, for
 *   every traced pixel q, fail[q] = !converged(q) && n < cap.  Then, for every pixel p = (x, y) of the image,
 *     active'[p] = active[p] != 0  &&  exists q = (x + dx, y + dy), |dx| <= r, |dy| <= r, 0 <= x + dx < nx,
 *                                      0 <= y + dy < ny, fail[q] != 0,
 *   written as the byte 1 or 0.  Integer logic only.
 *   - Windows are clipped at the image border; they never wrap from one row into the next.
 *   - A retired pixel stays retired.  All live pixels share one count, so the state needs no per-pixel n.
 *   - At n == cap every fail byte is 0, so everything retires.
 *   - Step 0 traces every pixel, so every fail byte is written before it is read.
 *   - A pixel's last fail write is the 0 of its retirement, so the plane is never cleared between steps.
 *   - In place is safe: a lane reads only its own active byte, and fail is read-only in the spread.
 * Consequences.
 *   1. Radius 0.  active' == fail.  The entries skip the spread and point the step kernel at active directly: the launch
 *      sequence and every output bit of the per-pixel entries of §32.
 *   2. Equivalence kept.  A pixel with spp = n has, bit for bit, the linear, rgb8 and stderr of that pixel in the estimator's
 *      fixed render with ns = n.  A pixel kept alive by a neighbour is rewritten at every step end, as §32 rewrites it.
 *   3. Monotone in r.  With everything else equal, spp_r[p] >= spp_r'[p] for r > r', at every pixel.  By induction over the
 *      steps the live set under r contains the live set under r': a pixel live in both has the same state in both; a pixel
 *      retired under r' passed its own test at its frozen count, or is at the cap; so whenever p retires under r, every
 *      pixel of its smaller window also passes under r'.
 *   4. Global rule.  For r >= max(nx, ny) - 1 every pixel stops at the same count: the first count at which all pass, or the
 *      cap.  The entries cap r at RTMI_WINDOW_MAX_RADIUS, so this is reachable on small images only.
 *   5. Tile rule.  No inclusion relation with rtmi_render_adaptive holds for r > 0: a sliding (2r + 1)^2 window and a fixed
 *      8x8 block are not nested, so neither spp bounds the other.
 *
 * params, the flags, the estimators, the planes and the counts are read and written as DESIGN.md §32 states them: linear
 *   n * 3 floats, rgb8 n * 3 bytes, stderr n * 3 floats, spp n words, n = nx * ny, row 0 the top row; counts 2 * steps words,
 *   slot k = {written, selected} of step k's select.  No Russian roulette, no light tree, no cooperative kernel, no f64.
 *
 * Scratch, the device form's, 16-byte aligned, every part rounded up to 16 bytes, in this order:
 *     16 bytes               control words
 *     8 * steps              the count slots
 *     4 * ceil(n / 4096)     the per-workgroup counts of the select
 *     n                      the active byte plane
 *     4 * n                  the list of the running step
 *     72 * n                 the state, double[9][n]
 *     12 * n * pass          the per-sample buffer of one launch; pass = pass_spp, or max(min_spp, step_spp) when pass_spp is
 *                            0 or larger than that
 *     n                      the fail byte plane
 *   that is the layout of DESIGN.md §32 byte for byte from the front, with the fail plane appended last.
 *
 * The calls that take a scene follow the handle's thread model (rtmi.h): calls on one handle serialise.
 */
#ifndef RTMI_WINDOW_H
#define RTMI_WINDOW_H

#include "rtmi.h"
#include "rtmi_adaptive.h"
#include "rtmi_roulette.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint32_t min_spp;      /* offset  0: samples every pixel gets first; >= 2, <= params->ns */
    uint32_t step_spp;     /* offset  4: samples added per step to each pixel still alive; >= 1 */
    uint32_t estimator;    /* offset  8: RTMI_ROULETTE_PLAIN / _NEE / _ENV / _ENV_NEE of rtmi_roulette.h (no roulette here) */
    uint32_t pass_spp;     /* offset 12: at most this many samples per pixel per launch; 0: a whole step */
    double   abs_tol;      /* offset 16: a pixel passes its own test when, in every channel, */
    double   rel_tol;      /* offset 24:   stderr <= abs_tol + rel_tol * |mean|   (both >= 0, finite) */
    float    env_select_p; /* offset 32: as rtmi_env_render; read by ENV_NEE only */
    uint32_t radius;       /* offset 36: r, the Chebyshev radius of the window; <= RTMI_WINDOW_MAX_RADIUS; 0: each pixel alone */
    uint32_t reserved[2];  /* offset 40: zero */
} rtmi_window_opts; /* 48 bytes */

#define RTMI_WINDOW_MAX_RADIUS 16u

/* The bytes of the layout above for an image of n_pixels pixels, launches of at most pass_spp samples per pixel and
 * `steps` steps; a multiple of 16.  Pure host code. */
uint64_t rtmi_window_scratch_bytes(uint64_t n_pixels, uint32_t pass_spp, uint32_t steps);

/* 1 + ceil((ns - min_spp) / step_spp): the steps of a render with cap ns, the rule of DESIGN.md §32.  0 for min_spp < 2,
 * min_spp > ns or step_spp == 0.  Pure host code. */
uint32_t rtmi_window_steps(uint32_t ns, uint32_t min_spp, uint32_t step_spp);

/* Asynchronous: every step is enqueued on `stream` (a hipStream_t) behind the handle's previous work; nothing is allocated
 * and nothing read back.  DEVICE pointers on the scene's device.  d_linear, d_rgb8, d_stderr, d_spp: each optional, not all
 * NULL.  d_counts: 2 * steps words or NULL.  d_scratch: scratch_bytes >= rtmi_window_scratch_bytes(nx * ny, pass, steps).
 * Refusals, before any device work, each with the entry's name in rtmi_last_error(), in this order.  RTMI_ERR_INVALID for
 * a NULL params, cam or opts; every plane NULL; ns == 0; max_depth == 0; an estimator outside 0..3; ENV_NEE with
 * env_select_p outside (0, 1]; SKY with a map estimator; an image of no or more than 32768^2 pixels; t_min not finite; a
 * missing attachment (of a handle that is there).  RTMI_ERR_UNSUPPORTED for unknown flags.  Then RTMI_ERR_INVALID for
 * (1) min_spp < 2, min_spp > ns, step_spp == 0, tolerances negative or not finite, radius > RTMI_WINDOW_MAX_RADIUS;
 * (2) nx * ny * pass >= 2^31; (3) more than 1024 steps; (4) a NULL or too small scratch; (5) a misaligned plane, counts
 * (4 bytes) or scratch (16 bytes); (6) non-zero reserved words; last, a NULL scene. */
int rtmi_render_window_device(rtmi_scene *scene, const rtmi_render_params *params, const rtmi_camera *cam,
                              const rtmi_window_opts *opts, void *d_linear, void *d_rgb8, void *d_stderr, void *d_spp,
                              void *d_counts, void *d_scratch, uint64_t scratch_bytes, void *stream);

/* Blocking, HOST planes (each optional, not all NULL); out_counts: 2 * steps words or NULL.  The device memory is the
 * handle's, grow-only.  The launches are the device form's; after each step's select the call reads that step's 8-byte
 * count and stops enqueuing at the first empty step.  stats (optional): samples = the paths traced, kernel_ms.  The
 * outputs have the bits of the device form's.  The refusals are the device form's without (4) and (5). */
int rtmi_render_window(rtmi_scene *scene, const rtmi_camera *cam, const rtmi_render_params *params,
                       const rtmi_window_opts *opts, float *out_linear, uint8_t *out_rgb8, float *out_stderr,
                       uint32_t *out_spp, uint32_t *out_counts, rtmi_stats *stats);

/* The rule applied once, asynchronously on `stream`, to DEVICE planes of nx * ny bytes each: d_active in and out, d_fail
 * read only.  A caller guards a mask of its own with it.  RTMI_ERR_INVALID for a NULL plane, an image of no or more than
 * 32768^2 pixels and a radius above RTMI_WINDOW_MAX_RADIUS.  The planes live on the device that is current. */
int rtmi_window_spread_device(void *d_active, const void *d_fail, uint32_t nx, uint32_t ny, uint32_t radius, void *stream);

/* The same on HOST arrays, blocking, for tests.  RTMI_ERR_INVALID for NULL planes, an empty image, more than 32768^2
 * pixels and a radius above the maximum; then RTMI_ERR_DEVICE for a device that does not exist. */
int rtmi_probe_window_spread(int device, uint32_t nx, uint32_t ny, uint32_t radius, uint8_t *active /* in-out */,
                             const uint8_t *fail);

#ifdef __cplusplus
}
#endif
#endif /* RTMI_WINDOW_H */
