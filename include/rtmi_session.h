/* rtmi_session.h — render sessions: continue, refine, checkpoint and merge a render, on the MI355X (gfx950) device
 * path.  See DESIGN.md §22.
 *
 * Every other render entry starts at sample 0 and owns its accumulation state for one call.  A session owns that state
 * across calls: per 8x8 tile a sample count n, per pixel and channel the three doubles of rtmi_adaptive.h (the f64 sum,
 * Welford's m and M2, laid out [tile][9][64]: sum r,g,b | m r,g,b | M2 r,g,b, lane = pixel of the tile) and per pixel the
 * bounce count of rtmi_roulette.h ([tile][64] uint32): 76 B per tile-padded pixel, on the scene's device.  The scene's
 * scratch (per-sample buffer, unit queue) is used during a call only, under the scene's mutex like every other call, so
 * several sessions may live on one scene and calls on them serialise.  A session must be destroyed before its scene.
 *
 * Paths.  `estimator` names whose arithmetic a path is counted in, in rtmi_roulette.h's numbering: RTMI_ROULETTE_PLAIN
 * (rtmi_render), _NEE (rtmi_render_nee), _ENV (rtmi_render_env, nee = 0), _ENV_NEE (rtmi_render_env, nee = 1, with
 * env_select_p).  rr = 0: exactly those paths.  rr = 1: the roulette of rtmi_roulette.h with min_depth and q_min.
 * Sample s of a pixel uses the Philox counters the one-shot entries use for sample s, whatever call traces it.
 *
 * Kinds.  min_spp == step_spp == 0: a FIXED session; every tile holds the same count n, the samples
 * [first_sample, first_sample + n), and rtmi_session_render adds to all of them.  Otherwise a REFINE session on the
 * lattice L = {min_spp + k * step_spp}, fixed for the session's life (first_sample must be 0); tiles hold different
 * counts and rtmi_session_refine advances them.
 *
 * Continue.  After any sequence of rtmi_session_render calls with total N >= 2 and first_sample == 0,
 * rtmi_session_image is bit for bit (linear, rgb8, stderr, bounces) the one-shot entry with ns = N: rtmi_render_nee,
 * rtmi_render_env, rtmi_render_roulette (rr = 1), and for the plain estimator with rr = 0 rtmi_render_adaptive with
 * min_spp = ns.  The result does not depend on how N was split, on sample_buffer_bytes, or on FAST_CULL, SYNC, REF_TREE
 * and the two cooperative flags.  With first_sample = s0 the session holds samples [s0, s0 + N): the same Philox
 * counters, the f64 sum and Welford's recurrence (k = 1..N) in sample order starting from sample s0.
 *
 * Refine.  A call must not loosen: cap >= the previous call's cap, abs_tol and rel_tol <= the previous ones
 * (RTMI_ERR_INVALID otherwise).  After any such sequence the image is bit for bit (linear, rgb8, stderr, spp, bounces)
 * the one-shot adaptive entry of the estimator with (min_spp, step_spp, abs_tol, rel_tol, ns = cap) of the LAST call,
 * and no sample is ever traced twice.  A call proceeds by count, ascending:
 *   1. a tile parked at a count on L below the cap is tested under the new tolerances (the test of rtmi_adaptive.h)
 *      without new samples and is settled if it passes; a tile at the cap is settled;
 *   2. a tile parked off L (it stopped at an earlier, smaller cap) is not tested there: it continues;
 *   3. the unsettled tiles advance to the next stop: the next count of L, the cap, or the next count at which tiles are
 *      parked, whichever is first.  There the tiles carried from below join the tiles parked at that count, so every
 *      launch renders one sample range; all are tested at counts of L, exactly as the one-shot run decides.
 * A tighter test that passes implies the looser one passed, so the one-shot run with the last tolerances cannot have
 * retired a tile below the count where the session parked it.  stats->samples counts this call's camera paths.
 *
 * Merge.  rtmi_session_merge(dst, src): FIXED sessions whose identity (below) is equal except first_sample, with
 * src.first_sample == dst.first_sample + dst.n.  Per pixel and channel, in double, no fused operations, A = dst, B = src:
 *   sum = sumA + sumB;   n = nA + nB;   d = mB - mA;   m = mA + d * (nB / n)
 *   M2  = (M2A + M2B) + (d * d) * ((nA * nB) / n)
 * Bounces add.  nB == 0 is a no-op, nA == 0 copies; src is unchanged.  The merged image is specified by this arithmetic,
 * not by the one-shot order of additions (DESIGN.md §22 states how close the two are).
 *
 * Blob.  rtmi_session_export writes, little-endian, without padding:
 *   offset   0  char[8]   magic "RTMISESS"
 *            8  uint32    version (RTMI_SESSION_BLOB_VERSION)
 *           12  uint32    nx            16  uint32  ny            20  uint32  tiles = ceil(nx/8) * ceil(ny/8)
 *           24  uint32    kind (0 FIXED, 1 REFINE)
 *           28  rtmi_session_opts (32 B, the fields in their order)
 *           60  uint32    max_depth     64  float   t_min
 *           68  uint32    flags: the result-changing ones only (SKY, FACE_FORWARD, UV_BOOK)
 *           72  uint64    seed
 *           80  float[21] the camera: origin, lower_left_corner, horizontal, vertical, u, v, time0, time1, lens_radius
 *          164  uint32[8] the scene's counts: items, prims, nodes, materials, textures, lights, map width, map height
 *                         (lights and map: 0 unless the estimator reads them)
 *          196  uint32    the last refine call's cap (0: none yet)
 *          200  double    its abs_tol   208  double  its rel_tol   (+inf: none yet)
 *          216  uint32    n[tiles]
 *               double    state[tiles][9][64]
 *               uint32    bounces[tiles][64]
 * Bytes [0, 196) are the identity block; the three values at 196 are progress and are restored by an import.
 * rtmi_session_import into a session whose identity block differs bytewise, or with a wrong length, magic or version,
 * is RTMI_ERR_INVALID and leaves the session as it was.  The blob may be moved to another process; keeping the scene
 * the same is the caller's job beyond the counts.
 *
 * Errors.  Every argument check comes before any device work.  RTMI_ERR_INVALID for NULL arguments, bad params,
 * estimator > 3, rr > 1, the checks of rtmi_roulette.h on min_depth and q_min (rr = 1), of rtmi_env.h on env_select_p
 * (ENV_NEE) and RTMI_FLAG_SKY (ENV, ENV_NEE), of rtmi_adaptive.h on min_spp, step_spp and the tolerances, first_sample
 * != 0 in a REFINE session, a scene without a light table (NEE, ENV_NEE) or map (ENV, ENV_NEE), the wrong kind of
 * session for a call, add_spp == 0, cap < min_spp, a loosening refine call, and a count that would pass 2^31.
 * RTMI_ERR_UNSUPPORTED for PATH_SIG, PROFILE, ASYNC, BLOCK_COOP, PROGRESSIVE, TEST_OVERFLOW and any flag bit not named
 * here, for tile_world != 1, and for sample indices of 2^26 and above (rtmi_render's limit on ns).  Accepted flags:
 * FAST_CULL, SYNC, REF_TREE, SKY (PLAIN and NEE), FACE_FORWARD, UV_BOOK, and RTMI_FLAG_LIGHT_COOP /
 * RTMI_FLAG_ROULETTE_COOP: either selects the wave-cooperative kernel under the rule of its own header
 * (rtmi_light_coop.h, rtmi_roulette_coop.h); the plain estimator with rr = 0 follows rtmi_render_adaptive's rule and
 * needs no flag.  stats->kernel reports the kernel that ran.
 *
 * Progress and failure.  The progress callback of params is called as in the one-shot entries, in work units of the
 * call so far.  A call that fails or is cancelled after its device work began leaves the session FAILED: every later
 * call except rtmi_session_destroy and rtmi_session_import returns RTMI_ERR_INVALID and says so; a successful import
 * clears it.
 */
#ifndef RTMI_SESSION_H
#define RTMI_SESSION_H

#include "rtmi.h"
#include "rtmi_roulette.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTMI_SESSION_BLOB_VERSION 1u
#define RTMI_SESSION_BLOB_HEADER 216u   /* bytes before n[tiles] */
#define RTMI_SESSION_BLOB_IDENTITY 196u /* ... of which the identity block */

typedef struct {
    uint32_t estimator;    /* RTMI_ROULETTE_PLAIN / _NEE / _ENV / _ENV_NEE (rtmi_roulette.h's numbering) */
    uint32_t rr;           /* 0: no roulette (the named entry's arithmetic); 1: rtmi_roulette.h with the two fields below */
    uint32_t min_depth;    /* rr = 1: the first depth at which the test is made; >= 1 */
    float q_min;           /* rr = 1: floor of the survival probability, in (0, 1] */
    float env_select_p;    /* ENV_NEE only: the map's share of the light samples, in (0, 1] */
    uint32_t first_sample; /* the session's samples are [first_sample, first_sample + n) */
    uint32_t min_spp;      /* both 0: a FIXED session (rtmi_session_render); */
    uint32_t step_spp;     /*   else a REFINE session on this lattice (rtmi_session_refine) */
} rtmi_session_opts;       /* 32 B */

typedef struct rtmi_session rtmi_session;

/* A new, empty session on `scene`.  params->ns is not read; the camera and params are copied (the progress callback
 * included: it must stay callable while the session lives). */
int rtmi_session_create(rtmi_scene *scene, const rtmi_camera *cam, const rtmi_render_params *params,
                        const rtmi_session_opts *opts, rtmi_session **session);
void rtmi_session_destroy(rtmi_session *session);

/* FIXED sessions: add_spp more samples for every tile.  stats (may be NULL): this call's work. */
int rtmi_session_render(rtmi_session *session, uint32_t add_spp, rtmi_stats *stats);

/* REFINE sessions: advance to the noise target (abs_tol, rel_tol) under the cap, as stated above. */
int rtmi_session_refine(rtmi_session *session, double abs_tol, double rel_tol, uint32_t cap, rtmi_stats *stats);

/* The session as it stands; any pointer may be NULL.  Planes as the one-shot entries': out_linear ny*nx*3 floats = sum / n,
 * out_rgb8 ny*nx*3 bytes quantised as rtmi_render's, out_stderr ny*nx*3 floats = sqrt(M2 / (n (n - 1))) (NaN while
 * n == 1), out_spp ny*nx = the count of the pixel's tile, out_bounces ny*nx = the running sum (zeros when rr == 0).
 * RTMI_ERR_INVALID while some tile holds no sample. */
int rtmi_session_image(rtmi_session *session, float *out_linear, uint8_t *out_rgb8, float *out_stderr, uint32_t *out_spp,
                       uint32_t *out_bounces);

/* The blob: *need receives its size; it is written when buf != NULL and cap >= *need (RTMI_ERR_INVALID when buf != NULL
 * and cap is smaller). */
int rtmi_session_export(rtmi_session *session, void *buf, size_t cap, size_t *need);
int rtmi_session_import(rtmi_session *session, const void *buf, size_t len);

/* dst takes src's samples in (see Merge); src is unchanged.  Both must live on one device. */
int rtmi_session_merge(rtmi_session *dst, const rtmi_session *src);

/* the smallest and largest count over the tiles; either pointer may be NULL */
int rtmi_session_spp(rtmi_session *session, uint32_t *min_spp, uint32_t *max_spp);

#ifdef __cplusplus
}
#endif
#endif /* RTMI_SESSION_H */
