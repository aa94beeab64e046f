/* rtmi_sparse.h — sparse renders: select, trace and patch chosen pixels of an image on the MI355X (gfx950) device path.
 * See DESIGN.md §31.
 *
 * Every render entry of rtmi.h traces a whole image or whole 8x8 tiles, and rtmi_radiance (rtmi_radiance.h) takes rays,
 * not pixels.  These entries render an arbitrary LIST OF PIXELS of an image with the render's own paths, and the list
 * never has to visit the host: a byte plane on the device (a class plane of a reconstruction pass, an outlier mask, a
 * region of interest) is turned into an ascending list, the listed pixels are path-traced, and the results are written
 * back where they belong.  The three steps are entries of their own and one call (rtmi_sparse_refine_device) for all.
 *
 * Select.  Pixel p in 0..n-1 is selected when its byte b = bytes[p] satisfies b < 32 && (accept_mask >> b) & 1.  The list
 *   receives the selected indices in ascending order, at most `capacity` of them: the first `capacity` in index order.
 *   count[0] is the number written, count[1] the number selected in all, so a caller sees an overflow.  Words of the
 *   list past count[0] are not written.  A count pass, a scan of the per-workgroup counts and a scatter pass: no atomic
 *   decides a position, the result is the same bit for bit from run to run.
 *
 * Sparse render.  `params` is the rtmi_render_params of the image the pixels belong to (nx, ny, seed, max_depth, t_min,
 *   flags; ns and the tile fields are not read).  A pixel index p = row * nx + i indexes the image's planes as every entry
 *   hands them out: row 0 is the top row, the reference's j = ny - 1 - row (rtmi.h).  Sample s of list entry k is, bit for
 *   bit, the path that the estimator's full render (rtmi_render, rtmi_render_nee, rtmi_render_env with nee 0 or 1; the
 *   per-lane kernel, fp32 contract) traces for that pixel and sample first_sample + s: the render's camera sample (u, v,
 *   the lens disk and the shutter time in its draw order), the Philox indices (first_sample + s, j * nx + i) under the key
 *   `seed`, stream 3 for the light samples.  A camera with a lens is therefore served, which rtmi_radiance's stream_skip is not.
 *   No Russian roulette, no light tree, no f64.
 *   Flags.  0, RTMI_FLAG_FAST_CULL (same results; runs when the BVH boxes hold over the camera's shutter interval),
 *     RTMI_FLAG_SKY (refused with a map estimator), RTMI_FLAG_FACE_FORWARD, RTMI_FLAG_UV_BOOK: those of rtmi_radiance.h.
 *     Every other bit is RTMI_ERR_UNSUPPORTED.
 *   Outputs, per list entry k (never per pixel: an index the device form cannot check writes nowhere but its own record):
 *     samples  n * ns * 3 floats, entry-major, sample fastest: the fp32 radiance of every path.
 *     mean     n * 3 floats: the f64 sum of the entry's samples in sample order, divided by ns, rounded once.  With
 *              first_sample = 0 it is the full render's `linear` at that pixel, bit for bit.
 *     stderr   n * 3 floats: Welford's recurrence of rtmi_adaptive.h in the operation order of the render's resolve; the
 *              full render's stderr plane at that pixel, bit for bit.  ns == 1 writes +inf, as rtmi_radiance.h does.
 *   The list may be unsorted and may repeat a pixel; repeats give equal records.
 *
 * Patch.  For each of the first min(count[0], capacity) entries k with p = list[k] < n_pixels: linear[p] = mean[k];
 *   rgb8[p] = the quantiser of rtmi_denoise.h applied to (double)mean[k] (sqrt, clamp with NaN -> 0, (int)(255.99 * g));
 *   bytes[p] = mark.  An entry with p >= n_pixels is skipped; no other byte of any plane is touched.  A list that repeats
 *   a pixel with different means leaves one of them.
 *
 * Scratch.  The caller's, 16-byte aligned; rtmi_sparse_scratch_bytes states the size that serves every entry here:
 *   16 bytes of control words (the chunk counter of the path kernel at byte 0, the two counts of a refine at byte 8), the
 *   per-workgroup counts of the select (one word per 4096 pixels), and for a refine the list (capacity words), mean and
 *   stderr (capacity * 12 bytes each) and the per-sample buffer (capacity * ns * 12 bytes).
 *
 * The calls that take a scene follow the handle's thread model (rtmi.h): calls on one handle serialise.
 */
#ifndef RTMI_SPARSE_H
#define RTMI_SPARSE_H

#include "rtmi.h"
#include "rtmi_roulette.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint32_t n;            /* offset  0: entries of the list (host forms); the capacity, the budget of pixels (device forms) */
    uint32_t ns;           /* offset  4: samples (independent paths) per entry, >= 1 */
    uint32_t first_sample; /* offset  8: the render's sample index of this call's sample 0 */
    uint32_t estimator;    /* offset 12: RTMI_ROULETTE_PLAIN / _NEE / _ENV / _ENV_NEE of rtmi_roulette.h (no roulette here) */
    float    env_select_p; /* offset 16: as rtmi_env_render; read by ENV_NEE only */
    uint32_t reserved[3];  /* offset 20: zero */
} rtmi_sparse_params; /* 32 bytes */

/* The bytes of scratch that serve every entry of this header for an image of n_pixels pixels, a list of at most
 * `capacity` entries and ns samples per entry; a multiple of 16.  Pure host code. */
uint64_t rtmi_sparse_scratch_bytes(uint64_t n_pixels, uint32_t capacity, uint32_t ns);

/* Asynchronous on `stream` (a hipStream_t), DEVICE pointers on `device`; allocates nothing and reads nothing back.
 * d_bytes: n bytes, any alignment (aligned planes are read 16 bytes at a time).  d_list: capacity words, 4-byte aligned.
 * d_count: 2 words, 4-byte aligned.  d_scratch: rtmi_sparse_scratch_bytes(n, 0, 0) bytes, 16-byte aligned.
 * RTMI_ERR_INVALID, with the entry's name in rtmi_last_error(), for a NULL pointer, n == 0 or n > 32768^2, capacity == 0
 * and a misaligned list, count or scratch; then RTMI_ERR_DEVICE for a device that does not exist. */
int rtmi_sparse_select_device(int device, uint32_t n, const void *d_bytes, uint32_t accept_mask, uint32_t capacity,
                              void *d_list, void *d_count, void *d_scratch, void *stream);

/* Blocking, host pointers.  pixels: sp->n indices below nx * ny.  Each output optional, not all NULL.  kernel_ms:
 * optional, the kernels' time by HIP events.  sp->n == 0 is RTMI_OK and launches nothing.
 * RTMI_ERR_INVALID, with the entry's name, for a NULL scene, params, cam, sp or pixels, every output NULL, ns == 0,
 * max_depth == 0, an estimator outside 0..3, first_sample + ns > 2^32, n * ns >= 2^31, ENV_NEE with env_select_p outside
 * (0, 1], SKY with a map estimator, an image of no or more than 2^32 - 1 pixels, a pixel index >= nx * ny (the message
 * names the entry of the list), a missing attachment and non-zero reserved words; RTMI_ERR_UNSUPPORTED for unknown flags.
 * All of these are answered before any device work. */
int rtmi_sparse_render(rtmi_scene *scene, const rtmi_render_params *params, const rtmi_camera *cam, const rtmi_sparse_params *sp,
                       const uint32_t *pixels, float *out_mean, float *out_stderr, float *out_samples, double *kernel_ms);

/* Asynchronous, DEVICE pointers on the scene's device, enqueued on `stream` behind the handle's previous call.  The number
 * of entries is min(d_count[0], sp->n), read BY THE KERNELS: the host never learns it, the grid is sized for sp->n and a
 * wavefront that finds no chunk left leaves at once.  d_count == NULL: sp->n entries.  d_samples is required (sp->n * ns
 * * 12 bytes: the kernel's per-sample buffer and the caller's output in one), d_mean and d_stderr (sp->n * 12 bytes each)
 * are optional.  Exactly that many records of mean and stderr and that many times ns of samples are written and nothing
 * beyond.  d_scratch: 16 bytes at least, 4-byte aligned (the chunk counter, zeroed on the stream).  The call allocates
 * nothing and takes the caller's word for the indices: one out of range traces some path and writes its own record. */
int rtmi_sparse_render_device(rtmi_scene *scene, const rtmi_render_params *params, const rtmi_camera *cam,
                              const rtmi_sparse_params *sp, const void *d_pixels, const void *d_count, void *d_mean,
                              void *d_stderr, void *d_samples, void *d_scratch, void *stream);

/* Asynchronous on `stream`, DEVICE pointers on `device`.  d_list: capacity words; d_count: as above, NULL = capacity
 * entries; d_mean: capacity * 3 floats; d_linear: n_pixels * 3 floats, d_rgb8: n_pixels * 3 bytes, d_bytes: n_pixels
 * bytes, each optional, not all NULL.  RTMI_ERR_INVALID for a NULL list or mean, every plane NULL, n_pixels == 0 or
 * > 32768^2, capacity == 0, a misaligned list, count, mean or linear; then RTMI_ERR_DEVICE. */
int rtmi_sparse_patch_device(int device, uint32_t n_pixels, const void *d_list, const void *d_count, uint32_t capacity,
                             const void *d_mean, void *d_linear, void *d_rgb8, void *d_bytes, uint32_t mark, void *stream);

/* Select -> sparse render -> patch, enqueued in one call on `stream` behind the scene's previous work; nothing is read
 * back and nothing allocated.  sp->n is the capacity: the budget of pixels.  d_bytes (nx * ny bytes) is required,
 * d_linear and d_rgb8 are optional; d_stderr: nx * ny * 3 floats or NULL, patched with the entries' standard errors.
 * d_scratch: scratch_bytes >= rtmi_sparse_scratch_bytes(nx * ny, sp->n, sp->ns), 16-byte aligned.  d_count_out: 2 words
 * or NULL: {patched, selected}, copied on the stream.  The refusals of rtmi_sparse_render_device, then those of the
 * planes (image above 32768^2 pixels, misaligned linear, stderr, scratch or count), a scratch too small, mark > 255. */
int rtmi_sparse_refine_device(rtmi_scene *scene, const rtmi_render_params *params, const rtmi_camera *cam,
                              const rtmi_sparse_params *sp, uint32_t accept_mask, uint32_t mark, void *d_bytes, void *d_linear,
                              void *d_rgb8, void *d_stderr, void *d_scratch, uint64_t scratch_bytes, void *d_count_out,
                              void *stream);

/* Blocking, host planes patched in place; allocates its device memory per call and frees it.  counts: 2 words or NULL:
 * {patched, selected}. */
int rtmi_sparse_refine(rtmi_scene *scene, const rtmi_render_params *params, const rtmi_camera *cam, const rtmi_sparse_params *sp,
                       uint32_t accept_mask, uint32_t mark, uint8_t *bytes, float *linear, uint8_t *rgb8, float *stderr_rgb,
                       uint32_t *counts);

#ifdef __cplusplus
}
#endif
#endif /* RTMI_SPARSE_H */
