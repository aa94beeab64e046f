/* rtmi_pixelwise.h — adaptive sampling at the granularity of one pixel, driven from the device, on the MI355X (gfx950)
 * device path.  See DESIGN.md §32.
 *
 * rtmi_render_adaptive (rtmi_adaptive.h) decides per 8x8 tile: a tile retires only when all 64 of its pixels pass the noise
 * test in the same step, and the host reads the active count back after every step.  These entries decide per PIXEL.  The
 * per-pixel state (sum | m | M2) lives on the device, the pixels still active are gathered into an ascending list by the
 * select of DESIGN.md §31, the list is traced by the path kernel of the pixel-list entries of DESIGN.md §31, and the whole
 * step loop is enqueued without a read-back: the kernels read each step's count from device memory.
 *
 * Steps.  The counts run min_spp, min_spp + step_spp, ..., ns = params->ns (the cap), the last step shortened to land on
 *   ns; rtmi_pixelwise_steps states how many there are.  Step 0 traces samples [0, min_spp) of every pixel.  After each
 *   step every pixel that was traced is tested alone, in double, as rtmi_adaptive.h tests a pixel of a tile:
 *     mean = sum / n,  e = sqrt(M2 / (n * (n - 1)));  converged iff in every channel e and mean are finite and
 *     e <= abs_tol + rel_tol * |mean|.
 *   A pixel retires when it has converged or when n == ns; otherwise the next step traces it again.  A non-finite value
 *   never converges.  A retired pixel stays retired.
 * Samples.  Sample s of pixel p is the path the estimator's full render traces for that pixel and sample (rtmi_render,
 *   rtmi_render_nee, rtmi_render_env with nee 0 or 1; the per-lane kernel, fp32 contract), a camera with a lens included.
 * Arithmetic.  The f64 sum in sample order and Welford's recurrence of rtmi_adaptive.h with k the sample's 1-based index:
 *   sum += x; d = x - m; m = m + d / k; M2 = M2 + d * (x - m).  No fused operations.
 * Equivalence.  A pixel with spp = n has, bit for bit, the linear, rgb8 and stderr of that pixel in the estimator's fixed
 *   render with ns = n (for the plain estimator rtmi_render_adaptive with min_spp = ns).  The result does not depend on
 *   pass_spp, on RTMI_FLAG_FAST_CULL, on which form ran or on repetition.  With the same steps, tolerances, seed and
 *   estimator, spp[p] <= the spp of p's tile in the tile-adaptive entry, so no more paths are traced than there.
 *
 * params is read as the pixel-list render entry of DESIGN.md §31 reads it (nx, ny, seed, max_depth, t_min, flags), and ns,
 *   the cap; the tile fields are not read.  Flags: 0, RTMI_FLAG_FAST_CULL, RTMI_FLAG_SKY (refused with a map estimator),
 *   RTMI_FLAG_FACE_FORWARD, RTMI_FLAG_UV_BOOK; every other bit is RTMI_ERR_UNSUPPORTED.  No Russian roulette, no light
 *   tree, no cooperative kernel, no f64.
 *
 * Planes.  Row 0 is the top row, as everywhere.  linear n * 3 floats, rgb8 n * 3 bytes (the quantiser of
 *   rtmi_adaptive.h: sqrt, clamp with NaN -> 0, (int)(255.99 * g)), stderr n * 3 floats, spp n words; n = nx * ny.  Every
 *   traced pixel's elements are written at every step end, so the planes hold a valid image after each step and the last
 *   write of a pixel is the one of its retirement.
 * Counts.  2 * steps words: slot k holds {written, selected} of step k's select, both the number of pixels step k traced
 *   (the list has room for every pixel).  Steps after the last active one hold {0, 0}.
 *
 * Scratch, the device form's, 16-byte aligned, every part rounded up to 16 bytes, in this order:
 *     16 bytes               control words (the chunk counter of the path kernel at byte 0)
 *     8 * steps              the count slots
 *     4 * ceil(n / 4096)     the per-workgroup counts of the select
 *     n                      the active byte plane (1: still noisy)
 *     4 * n                  the list of the running step
 *     72 * n                 the state, structure of arrays: double[9][n], rows sum r g b | m r g b | M2 r g b
 *     12 * n * pass          the per-sample buffer of one launch, entry-major; pass = the largest number of samples
 *                            of one launch: pass_spp, or max(min_spp, step_spp) when pass_spp is 0 or larger than that
 *
 * The step kernel (rtmi_probe_pixelwise_step runs it alone).  Entry k < min(count[0], capacity) of the list names pixel
 *   p = list[k] and owns records [k * pass, (k + 1) * pass) of the per-sample buffer.  The kernel loads the nine doubles
 *   of p (none when n_done == 0: the state is never cleared), folds the pass samples in sample order with
 *   k = n_done + s + 1, and stores the state.  With decide set it writes spp[p] = n_done + pass, linear[p], rgb8[p] and
 *   stderr[p] and sets active[p] = !converged && n_done + pass < cap.  The list may be unsorted (the state is then read
 *   less coalesced; the results are the same).  An entry with p >= n_pixels is skipped: nothing is read or written for
 *   it.  A list that repeats a pixel is not served: two lanes would race on one state.
 *
 * The calls that take a scene follow the handle's thread model (rtmi.h): calls on one handle serialise.
 */
#ifndef RTMI_PIXELWISE_H
#define RTMI_PIXELWISE_H

#include "rtmi.h"
#include "rtmi_adaptive.h"
#include "rtmi_roulette.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint32_t min_spp;      /* offset  0: samples every pixel gets first; >= 2, <= params->ns */
    uint32_t step_spp;     /* offset  4: samples added per step to each pixel still noisy; >= 1 */
    uint32_t estimator;    /* offset  8: RTMI_ROULETTE_PLAIN / _NEE / _ENV / _ENV_NEE of rtmi_roulette.h (no roulette here) */
    uint32_t pass_spp;     /* offset 12: at most this many samples per pixel per launch; 0: a whole step */
    double   abs_tol;      /* offset 16: a pixel retires when, in every channel, */
    double   rel_tol;      /* offset 24:   stderr <= abs_tol + rel_tol * |mean|   (both >= 0, finite) */
    float    env_select_p; /* offset 32: as rtmi_env_render; read by ENV_NEE only */
    uint32_t reserved[3];  /* offset 36: zero */
} rtmi_pixelwise_opts; /* 48 bytes */

#define RTMI_PIXELWISE_MAX_STEPS 1024u

/* The bytes of the layout above for an image of n_pixels pixels, launches of at most pass_spp samples per pixel and
 * `steps` steps; a multiple of 16.  Pure host code. */
uint64_t rtmi_pixelwise_scratch_bytes(uint64_t n_pixels, uint32_t pass_spp, uint32_t steps);

/* 1 + ceil((ns - min_spp) / step_spp): the steps of a render with cap ns.  0 for min_spp < 2, min_spp > ns or
 * step_spp == 0.  Pure host code. */
uint32_t rtmi_pixelwise_steps(uint32_t ns, uint32_t min_spp, uint32_t step_spp);

/* Asynchronous: every step is enqueued on `stream` (a hipStream_t) behind the handle's previous work; nothing is allocated
 * and nothing read back.  DEVICE pointers on the scene's device.  d_linear, d_rgb8, d_stderr, d_spp: each optional, not all
 * NULL.  d_counts: 2 * steps words or NULL.  d_scratch: scratch_bytes >= rtmi_pixelwise_scratch_bytes(nx * ny, pass, steps).
 * Refusals, before any device work, each with the entry's name in rtmi_last_error(), in this order.  RTMI_ERR_INVALID for
 * a NULL params, cam or opts; every plane NULL; ns == 0; max_depth == 0; an estimator outside 0..3; ENV_NEE with
 * env_select_p outside (0, 1]; SKY with a map estimator; an image of no or more than 32768^2 pixels; t_min not finite; a
 * missing attachment (of a handle that is there).  RTMI_ERR_UNSUPPORTED for unknown flags.  Then RTMI_ERR_INVALID for
 * (1) min_spp < 2, min_spp > ns, step_spp == 0, tolerances negative or not finite; (2) nx * ny * pass >= 2^31; (3) more
 * than RTMI_PIXELWISE_MAX_STEPS steps; (4) a NULL or too small scratch; (5) a misaligned plane, counts (4 bytes) or scratch
 * (16 bytes); (6) non-zero reserved words; last, a NULL scene. */
int rtmi_render_pixelwise_device(rtmi_scene *scene, const rtmi_render_params *params, const rtmi_camera *cam,
                                 const rtmi_pixelwise_opts *opts, void *d_linear, void *d_rgb8, void *d_stderr, void *d_spp,
                                 void *d_counts, void *d_scratch, uint64_t scratch_bytes, void *stream);

/* Blocking, HOST planes (each optional, not all NULL); out_counts: 2 * steps words or NULL.  The device memory is the
 * handle's, grow-only.  The launches are the device form's; after each step's select the call reads that step's 8-byte
 * count and stops enqueuing once no pixel is active.  stats (optional): samples = the paths traced, kernel_ms.  The
 * outputs have the bits of the device form's.  The refusals are the device form's without (4) and (5). */
int rtmi_render_pixelwise(rtmi_scene *scene, const rtmi_camera *cam, const rtmi_render_params *params,
                          const rtmi_pixelwise_opts *opts, float *out_linear, uint8_t *out_rgb8, float *out_stderr,
                          uint32_t *out_spp, uint32_t *out_counts, rtmi_stats *stats);

/* The step kernel alone on HOST arrays, blocking, for tests on crafted samples.  list: capacity words; count: 2 words or
 * NULL (capacity entries); samples: capacity * pass * 3 floats; state: 9 * n_pixels doubles, in and out (not read by
 * the kernel when n_done == 0; what it holds before the call stands where the kernel writes nothing).
 * active n_pixels bytes, linear, rgb8, stderr_rgb and spp as the planes above, each optional, in and out.
 * RTMI_ERR_INVALID for a NULL list, samples or state, n_pixels == 0, capacity == 0, pass == 0 and capacity * pass >= 2^31;
 * then RTMI_ERR_DEVICE for a device that does not exist. */
int rtmi_probe_pixelwise_step(int device, uint32_t n_pixels, uint32_t capacity, const uint32_t *list, const uint32_t *count,
                              const float *samples, double *state, uint32_t n_done, uint32_t pass, uint32_t decide, uint32_t cap,
                              double abs_tol, double rel_tol, uint8_t *active, float *linear, uint8_t *rgb8, float *stderr_rgb,
                              uint32_t *spp);

#ifdef __cplusplus
}
#endif
#endif /* RTMI_PIXELWISE_H */
