// rtmi_session.hip — translation unit of render sessions (include/rtmi_session.h): the kernels that work on a session's
// state alone, their launchers, and below them the session handle and its entry points (host code on the estimator layer,
// rtmi_host.hpp).  Compiled with the flags of rtmi_device.hip (-ffp-contract=off: no fused operations, so
// numpy restates read-out and merge bit for bit).
//
// The render kernels and the per-pass resolve of a session are the existing ones (rtmi_adaptive_resolve_kernel with
// decide = 0 writes sum, m and M2 back for every tile).  What is here streams the [tile][9][64] planes: one wavefront per
// tile, lane = pixel, so every plane access is one coalesced 512-byte row; no LDS, no scratch, memory-bound.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "rtmi.h"
#include "rtmi_session.h"
#include "rtmi_roulette_coop.h"
#include "rtmi_session_launch.hpp"
#include "rtmi_host.hpp"

// The read-out: what rtmi_adaptive_resolve_kernel writes for a tile it retires at n samples, for every tile at its own n.
__global__ __launch_bounds__(256) void rtmi_session_readout_kernel(SessionReadout R) {
    const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (tile >= R.ntiles) return; // wave-uniform
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_u = R.counts[tile];
    const double n = (double)n_u;
    const double *st = R.state + (size_t)tile * (9u * 64u) + lane;
    // the texel of rtmi_resolve_kernel with ns = n: col /= n; sqrt; clamp; (255.99*c) as i32 — tests/test.rs:71-78
    rtmi_texel tx_out;
    uint32_t q[3];
    float lin[3], se[3];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const double sum = st[ch * 64], M2 = st[(6 + ch) * 64];
        const double mm = sum / n;
        lin[ch] = (float)mm;
        double g = sqrt(mm);
        g = (g > 0.0) ? ((g < 1.0) ? g : 1.0) : 0.0; // nalgebra::clamp(val, 0, 1); NaN -> 0
        const double x = 255.99 * g;
        q[ch] = (x != x) ? 0u : (uint32_t)(int32_t)x; // `as i32`; in [0,255] after the clamp
        se[ch] = (float)sqrt(M2 / (n * (n - 1.0)));
    }
    tx_out.r = lin[0]; tx_out.g = lin[1]; tx_out.b = lin[2];
    tx_out.rgb8 = q[0] | (q[1] << 8) | (q[2] << 16);
    const size_t t = (size_t)tile * 64u + lane;
    R.texels[t] = tx_out;
    R.stderr_out[t * 3] = se[0]; R.stderr_out[t * 3 + 1] = se[1]; R.stderr_out[t * 3 + 2] = se[2];
    R.spp_out[t] = n_u;
}

// The test of rtmi_adaptive_resolve_kernel's decide step on the stored state: a ballot over the tile's in-image lanes;
// a tile that fails is appended to the next list.
__global__ __launch_bounds__(256) void rtmi_session_decide_kernel(SessionDecide D) {
    const uint32_t lpos = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (lpos >= D.n_in) return; // wave-uniform
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t tile = D.tiles_in[lpos];
    const uint32_t ty = tile / D.tiles_x, tx = tile - ty * D.tiles_x;
    const bool in_image = tx * RTMI_TILE + (lane & 7u) < D.nx && ty * RTMI_TILE + (lane >> 3) < D.ny;
    const double *st = D.state + (size_t)tile * (9u * 64u) + lane;
    const double n = (double)D.n;
    bool ok = true;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const double sum = st[ch * 64], M2 = st[(6 + ch) * 64];
        const double mean = sum / n;
        const double e = sqrt(M2 / (n * (n - 1.0)));
        ok = ok && __builtin_isfinite(e) && __builtin_isfinite(mean) && e <= D.abs_tol + D.rel_tol * fabs(mean);
    }
    if (!in_image) ok = true;
    if (__ballot(!ok) != 0ull && lane == 0u) D.tiles_out[atomicAdd(D.n_out, 1u)] = tile;
}

__global__ __launch_bounds__(256) void rtmi_session_merge_kernel(SessionMerge M) {
    const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (tile >= M.ntiles) return; // wave-uniform
    const uint32_t lane = threadIdx.x & 63u;
    double *a = M.dst + (size_t)tile * (9u * 64u) + lane;
    const double *b = M.src + (size_t)tile * (9u * 64u) + lane;
    const double n = M.nA + M.nB;
    const double wB = M.nB / n, wAB = (M.nA * M.nB) / n;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const double sumA = a[ch * 64], mA = a[(3 + ch) * 64], M2A = a[(6 + ch) * 64];
        const double sumB = b[ch * 64], mB = b[(3 + ch) * 64], M2B = b[(6 + ch) * 64];
        const double d = mB - mA;
        a[ch * 64] = sumA + sumB;
        a[(3 + ch) * 64] = mA + d * wB;
        a[(6 + ch) * 64] = (M2A + M2B) + (d * d) * wAB;
    }
    const size_t t = (size_t)tile * 64u + lane;
    M.dst_bounces[t] = M.dst_bounces[t] + M.src_bounces[t];
}

hipError_t rtmi_session_launch_readout(hipStream_t stream, const SessionReadout &R) {
    hipLaunchKernelGGL(rtmi_session_readout_kernel, dim3((R.ntiles + 3u) / 4u), dim3(256), 0, stream, R);
    return hipGetLastError();
}

hipError_t rtmi_session_launch_decide(hipStream_t stream, const SessionDecide &D) {
    hipLaunchKernelGGL(rtmi_session_decide_kernel, dim3((D.n_in + 3u) / 4u), dim3(256), 0, stream, D);
    return hipGetLastError();
}

hipError_t rtmi_session_launch_merge(hipStream_t stream, const SessionMerge &M) {
    hipLaunchKernelGGL(rtmi_session_merge_kernel, dim3((M.ntiles + 3u) / 4u), dim3(256), 0, stream, M);
    return hipGetLastError();
}

// ---- render sessions (include/rtmi_session.h) --------------------------------------------------------------------------
// A session owns what the one-shot entries keep for one call: per tile a count (on the host), the nine f64 planes and the
// bounce plane (on the scene's device).  Its calls are the host path of the one-shot entries (begin_call, kernel_args,
// plan_light_coop / plan_traversal, plan_and_reserve, run_passes, the adaptive resolve with decide = 0, which writes the
// state back for every tile) over a list of tiles that all hold the same count; the convergence test, the read-out and the
// merge are the kernels of rtmi_session.hip.
struct RTMI_HIDDEN rtmi_session {
    rtmi_scene *s = nullptr;
    rtmi_camera cam{};
    rtmi_render_params p{}; // ns = 1 (not read); the cooperative flag normalised to the one of the session's entries
    rtmi_session_opts o{};
    bool refine = false, nee = false, env = false, failed = false;
    uint32_t T = 0;
    std::vector<uint32_t> n; // [tile] the samples each tile holds
    DeviceBuf<double> state;               // [tile][9][64]
    DeviceBuf<uint32_t> bounces, d_counts; // [tile][64], [tile]
    uint32_t last_cap = 0;   // the last refine call's cap and tolerances
    double last_abs = std::numeric_limits<double>::infinity(), last_rel = std::numeric_limits<double>::infinity();
    uint32_t scene_counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

static const uint32_t SESSION_RESULT_FLAGS = RTMI_FLAG_SKY | RTMI_FLAG_FACE_FORWARD | RTMI_FLAG_UV_BOOK;
static const uint32_t SESSION_COOP_FLAGS = RTMI_FLAG_LIGHT_COOP | RTMI_FLAG_ROULETTE_COOP;

// the blob's header (include/rtmi_session.h); first_sample: written in place of the session's own (merge compares two
// sessions' identity blocks but for that field)
static std::vector<uint8_t> session_header(const rtmi_session *ss, const uint32_t *first_sample = nullptr) {
    std::vector<uint8_t> h(RTMI_SESSION_BLOB_HEADER, 0);
    size_t at = 0;
    const auto put = [&](const void *v, size_t nbytes) { std::memcpy(h.data() + at, v, nbytes); at += nbytes; };
    const uint32_t version = RTMI_SESSION_BLOB_VERSION, kind = ss->refine ? 1u : 0u, flags = ss->p.flags & SESSION_RESULT_FLAGS;
    put("RTMISESS", 8);
    put(&version, 4); put(&ss->p.nx, 4); put(&ss->p.ny, 4); put(&ss->T, 4); put(&kind, 4);
    rtmi_session_opts o = ss->o;
    if (first_sample) o.first_sample = *first_sample;
    put(&o, sizeof(rtmi_session_opts));
    put(&ss->p.max_depth, 4); put(&ss->p.t_min, 4); put(&flags, 4); put(&ss->p.seed, 8);
    put(ss->cam.origin, 12); put(ss->cam.lower_left_corner, 12); put(ss->cam.horizontal, 12); put(ss->cam.vertical, 12);
    put(ss->cam.u, 12); put(ss->cam.v, 12); put(&ss->cam.time0, 4); put(&ss->cam.time1, 4); put(&ss->cam.lens_radius, 4);
    put(ss->scene_counts, 32);
    put(&ss->last_cap, 4); put(&ss->last_abs, 8); put(&ss->last_rel, 8);
    return h; // at == RTMI_SESSION_BLOB_HEADER
}
static_assert(sizeof(rtmi_session_opts) == 32, "rtmi_session_opts is 32 bytes in the blob");
static size_t session_blob_bytes(const rtmi_session *ss) {
    return (size_t)RTMI_SESSION_BLOB_HEADER + (size_t)ss->T * (4u + 9u * 64u * 8u + 64u * 4u);
}

static Estimator session_estimator(const rtmi_session *ss, const char *name, const std::string &null_scene) {
    return lit_estimator(name, ss->nee, ss->env, ss->nee && ss->env ? ss->o.env_select_p : 1.0f, null_scene.c_str());
}

// the refusals every call on an existing session starts with
static int session_usable(const rtmi_session *ss, const std::string &nm, bool want_refine, bool any_kind = false) {
    if (!ss) return fail(RTMI_ERR_INVALID, nm + "session is NULL");
    if (ss->failed)
        return fail(RTMI_ERR_INVALID, nm + "the session is failed (an earlier call failed or was cancelled after its device work "
                                           "began): destroy it or import a checkpoint");
    if (!any_kind && ss->refine != want_refine)
        return fail(RTMI_ERR_INVALID, nm + (want_refine ? "this call needs a REFINE session: a FIXED one (min_spp == step_spp == 0) "
                                                          "advances with rtmi_session_render"
                                                        : "this call needs a FIXED session: a REFINE one advances with rtmi_session_refine"));
    return RTMI_OK;
}

extern "C" int rtmi_session_create(rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params *p_in,
                                   const rtmi_session_opts *o, rtmi_session **out) {
    // every argument check comes before the first use of the handle (and of the device)
    const char *name = "rtmi_session_create";
    const std::string nm = std::string(name) + ": ";
    if (!p_in || !cam || !o || !out) return fail(RTMI_ERR_INVALID, nm + "NULL argument");
    rtmi_render_params p = *p_in;
    p.ns = 1u; // not read
    int rc = check_params(&p);
    if (rc) return rc;
    if ((rc = check_estimator(name, o->estimator))) return rc;
    if (o->rr > 1u) return fail(RTMI_ERR_INVALID, nm + "rr must be 0 or 1");
    if (o->rr && o->min_depth == 0u) return fail(RTMI_ERR_INVALID, nm + "min_depth must be at least 1");
    if (o->rr && (!std::isfinite(o->q_min) || !(o->q_min > 0.0f && o->q_min <= 1.0f)))
        return fail(RTMI_ERR_INVALID, nm + "q_min must be in (0, 1]");
    const bool nee = o->estimator == RTMI_ROULETTE_NEE || o->estimator == RTMI_ROULETTE_ENV_NEE;
    const bool env = o->estimator == RTMI_ROULETTE_ENV || o->estimator == RTMI_ROULETTE_ENV_NEE;
    if ((rc = check_estimator_opts(name, o->estimator, o->env_select_p, p.flags))) return rc;
    if (p.flags & RTMI_FLAG_PATH_SIG) return fail(RTMI_ERR_UNSUPPORTED, nm + "PATH_SIG is refused: a session keeps no path signatures");
    const std::string flags_msg = nm + "sessions accept the flags FAST_CULL, SYNC, REF_TREE, SKY, FACE_FORWARD, UV_BOOK, LIGHT_COOP and "
                                       "ROULETTE_COOP only (not PATH_SIG, PROFILE, ASYNC, BLOCK_COOP, PROGRESSIVE, TEST_OVERFLOW)";
    const std::string world_msg = nm + "a session renders the whole image: tile_world must be 1";
    if ((rc = check_mode_params(&p, RTMI_ADAPTIVE_NEE_FLAGS | RTMI_FLAG_SKY | SESSION_COOP_FLAGS, flags_msg.c_str(), world_msg.c_str())))
        return rc;
    const bool refine = o->min_spp != 0u || o->step_spp != 0u;
    if (refine) {
        if (o->min_spp < 2u) return fail(RTMI_ERR_INVALID, nm + "min_spp must be at least 2 (a variance needs two samples)");
        if (o->step_spp == 0u) return fail(RTMI_ERR_INVALID, nm + "step_spp must be positive");
        if (o->first_sample != 0u) return fail(RTMI_ERR_INVALID, nm + "first_sample must be 0 in a REFINE session");
        if (o->min_spp >= (1u << 26)) return fail(RTMI_ERR_UNSUPPORTED, nm + "min_spp must be below 2^26");
    }
    if (o->first_sample >= (1u << 31)) return fail(RTMI_ERR_INVALID, nm + "first_sample must be below 2^31");
    if (o->first_sample >= (1u << 26)) return fail(RTMI_ERR_UNSUPPORTED, nm + "sample indices must stay below 2^26");

    rtmi_session *ss = new (std::nothrow) rtmi_session;
    if (!ss) return fail(RTMI_ERR_NOMEM, nm + "out of host memory");
    ss->s = s; ss->cam = *cam; ss->p = p; ss->o = *o;
    ss->refine = refine; ss->nee = nee; ss->env = env;
    if (!o->rr) { ss->o.min_depth = 0u; ss->o.q_min = 0.0f; } // not read: one representation in the identity block
    if (!(nee && env)) ss->o.env_select_p = 0.0f;
    if (ss->p.flags & SESSION_COOP_FLAGS)
        ss->p.flags = (ss->p.flags & ~SESSION_COOP_FLAGS) | (o->rr ? RTMI_FLAG_ROULETTE_COOP : RTMI_FLAG_LIGHT_COOP);
    ss->T = local_tiles_of(&p, 0);
    ss->n.assign(ss->T, 0u);
    const std::string null_scene = nm + "scene is NULL";
    const Estimator m = session_estimator(ss, name, null_scene);
    RenderCall c;
    if ((rc = begin_call(c, m, s))) { delete ss; return rc; }
    const uint32_t counts[8] = {s->meta.n_items, s->meta.n_prims, s->meta.n_nodes, s->meta.n_materials, s->meta.n_textures,
                                nee ? s->nee_n : 0u, env ? s->env_w : 0u, env ? s->env_h : 0u};
    std::memcpy(ss->scene_counts, counts, sizeof(counts));
    const size_t T = ss->T;
    hipError_t e = ss->state.alloc(T * 9 * 64 * sizeof(double));
    if (e == hipSuccess) e = ss->bounces.alloc(T * 64 * sizeof(uint32_t));
    if (e == hipSuccess) e = ss->d_counts.alloc(T * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemsetAsync(ss->state.ptr, 0, T * 9 * 64 * sizeof(double), s->stream.s);
    if (e == hipSuccess) e = hipMemsetAsync(ss->bounces.ptr, 0, T * 64 * sizeof(uint32_t), s->stream.s);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream.s);
    if (e != hipSuccess) {
        delete ss;
        return fail(e == hipErrorOutOfMemory ? RTMI_ERR_NOMEM : RTMI_ERR_DEVICE, nm + hipGetErrorString(e));
    }
    *out = ss;
    return RTMI_OK;
}

extern "C" void rtmi_session_destroy(rtmi_session *ss) {
    if (!ss) return;
    {
        std::lock_guard<std::mutex> lock(ss->s->mu);
        (void)hipSetDevice(ss->s->device);
        if (ss->s->busy_recorded) (void)hipEventSynchronize(ss->s->busy.e);
        (void)ss->state.release(); (void)ss->bounces.release(); (void)ss->d_counts.release();
    }
    delete ss;
}

// One render or refine call's hold on the scene and its kernel plan: begin_call, the scene's scratch for the session's
// tiles, the kernel arguments and the selection of the render kernel (the plain estimator without roulette follows
// rtmi_render_adaptive's rule, the others plan_light_coop under their entries' flag).
struct SessionCall {
    RenderCall c;
    int which = RTMI_AD_PERLANE; // the plain estimator without roulette: the kernel of rtmi_adaptive.hip
    PassCounts counts;
    uint64_t samples = 0;
    bool worked = false; // some launch was enqueued
};
static int session_begin(SessionCall &k, rtmi_session *ss, const Estimator &m) {
    rtmi_scene *s = ss->s;
    RenderCall &c = k.c;
    int rc;
    if ((rc = begin_call(c, m, s)) || (rc = reserve_texels(s, (size_t)ss->T * 64)) || (rc = grow_adaptive(s, ss->T))) return rc;
    kernel_args(c, m, s, &ss->cam, ss->p);
    const rtmi_render_params &p = ss->p;
    if (!ss->nee && !ss->env && !ss->o.rr) {
        const bool coop_ok = s->meta.n_prims < (1u << 22) && s->meta.n_nodes < (1u << 25) && s->meta.n_alt_nodes < (1u << 25);
        const bool inst = s->dev.has_prim_xf != 0u || s->dev.has_medium_outer != 0u;
        c.coop = c.fast && !(p.flags & RTMI_FLAG_SYNC) && coop_ok && !inst;
        if ((rc = plan_traversal(s, &p, c.coop, c.P, c.ext))) return rc;
        k.which = c.coop ? (c.ext ? RTMI_AD_COOP_EXT : RTMI_AD_COOP_LEAN) : (c.fast ? RTMI_AD_PERLANE_FAST : RTMI_AD_PERLANE);
        c.coop_lds = (size_t)WAVES_PER_BLOCK * CoopLds{c.P.coop_cap, c.ext, false}.words() * sizeof(uint32_t);
        c.wps = 4u;
    } else if (ss->o.rr) {
        if ((rc = plan_light_coop(c, s, p, RTMI_FLAG_ROULETTE_COOP, rtmi_roulette_coop_wps(ss->nee, ss->env)))) return rc;
    } else if ((rc = plan_light_coop(c, s, p))) {
        return rc;
    }
    s->last_kernel = c.coop ? RTMI_KERNEL_WAVE_COOP : RTMI_KERNEL_PERLANE;
    if ((rc = begin_passes(s, s->stream.s))) return rc;
    HIP_TRY(hipEventRecord(s->ev[0].e, s->stream.s));
    HIP_TRY(hipEventRecord(s->ev[2].e, s->stream.s));
    return RTMI_OK;
}
static int session_launch_render(const SessionCall &k, const rtmi_session *ss, const Estimator &m, uint32_t blocks, const uint32_t *tiles) {
    rtmi_scene *s = ss->s;
    const RenderCall &c = k.c;
    if (!ss->nee && !ss->env && !ss->o.rr) {
        HIP_TRY(rtmi_adaptive_launch_render(k.which, blocks, c.coop ? c.coop_lds : 0, s->stream.s, s->dev, c.C, c.P, tiles));
    } else if (ss->o.rr) {
        const DevRoulette R{ss->bounces.ptr, ss->o.min_depth, ss->o.q_min};
        if (c.coop)
            HIP_TRY(rtmi_roulette_coop_launch_render(c.ext, ss->nee, ss->env, blocks, c.coop_lds, s->stream.s, s->dev, c.C, c.P, tiles,
                                                     c.L, c.E, R));
        else
            HIP_TRY(rtmi_roulette_launch_render(c.fast, ss->nee, ss->env, blocks, s->stream.s, s->dev, c.C, c.P, tiles, c.L, c.E, R));
    } else if (c.coop) {
        return launch_light_coop(c, m, s, false, blocks, tiles);
    } else {
        HIP_TRY(rtmi_adaptive_nee_launch_render(c.fast, ss->nee, ss->env, blocks, s->stream.s, s->dev, c.C, c.P, tiles, c.L, c.E));
    }
    return RTMI_OK;
}
// the pixels of `tiles` that lie inside the image
static uint64_t session_pixels(const rtmi_session *ss, const std::vector<uint32_t> &tiles) {
    const uint32_t txn = tiles_x_of(&ss->p);
    uint64_t pix = 0;
    for (uint32_t t : tiles) {
        const uint32_t ty = t / txn, tx = t % txn;
        const uint32_t w = (tx * RTMI_TILE + RTMI_TILE <= ss->p.nx) ? RTMI_TILE : ss->p.nx - tx * RTMI_TILE;
        const uint32_t h = (ty * RTMI_TILE + RTMI_TILE <= ss->p.ny) ? RTMI_TILE : ss->p.ny - ty * RTMI_TILE;
        pix += (uint64_t)w * h;
    }
    return pix;
}
// Samples [from, from + cnt) of the session's sequence for the tiles of `active`, which all hold `from`: one launch range
// (pass_s0 uniform), in sub-passes when the per-sample buffer does not hold it; waits for it, reporting progress.
static int session_advance(SessionCall &k, rtmi_session *ss, const Estimator &m, const std::vector<uint32_t> &active, uint32_t from,
                           uint32_t cnt) {
    rtmi_scene *s = ss->s;
    hipStream_t stream = s->stream.s;
    DevParams &P = k.c.P;
    int rc;
    const uint32_t n_active = (uint32_t)active.size();
    HIP_TRY(hipMemcpyAsync(s->ad_lists.ptr, active.data(), (size_t)n_active * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    rtmi_render_params q = ss->p;
    q.ns = cnt;
    uint32_t chunk_spp = 0, pass_ns = 0;
    if ((rc = plan_and_reserve(s, &q, n_active, chunk_spp, pass_ns))) return rc;
    P.ntiles_local = n_active; P.chunk_spp = chunk_spp; P.pass_stride = pass_ns; P.samples = s->samples.ptr;
    AdaptiveResolve A;
    A.tiles_in = s->ad_lists.ptr; A.tiles_out = s->ad_lists.ptr + ss->T; A.n_out = s->ad_lists.ptr + 2 * (size_t)ss->T;
    A.state = ss->state.ptr; A.texels = s->texels.ptr; A.stderr_out = s->ad_stderr.ptr; A.spp_out = s->ad_spp.ptr;
    A.abs_tol = 0.0; A.rel_tol = 0.0; A.ns = 0xffffffffu;
    A.decide = 0; // never retires: sum, m and M2 go back to the session's planes after every sub-pass
    const uint32_t s0 = ss->o.first_sample;
    k.worked = true;
    rc = run_passes(s, P, stream, s0 + from, cnt, false, light_run_slots(s, k.c), 1u, k.counts,
                    [&](uint32_t blocks, bool first, bool) -> int {
                        if (int lrc = session_launch_render(k, ss, m, blocks, (const uint32_t *)s->ad_lists.ptr)) return lrc;
                        DevParams Pr = P; // the resolve counts from the session's first sample: Welford's k = 1 there
                        Pr.pass_s0 = P.pass_s0 - s0;
                        A.first = (from == 0u && first) ? 1 : 0;
                        HIP_TRY(rtmi_adaptive_launch_resolve(stream, s->samples.ptr, Pr, A));
                        return RTMI_OK;
                    });
    if (rc) return rc;
    HIP_TRY(hipEventRecord(s->ev[2].e, stream));
    rtmi_scene *one[1] = {s};
    if ((rc = wait_with_progress(one, &s->ev[2].e, 1, &ss->p))) return rc;
    for (uint32_t t : active) ss->n[t] = from + cnt;
    k.samples += session_pixels(ss, active) * cnt;
    return RTMI_OK;
}
// the end of a render or refine call whose device work began: the failed mark, the overflow word, the stats
static int session_end(SessionCall &k, rtmi_session *ss, int rc, rtmi_stats *stats) {
    rtmi_scene *s = ss->s;
    if (!rc && k.worked) rc = check_overflow(s);
    if (rc) {
        ss->failed = true;
        return rc;
    }
    if (stats) {
        float ms = 0.f;
        HIP_TRY(hipEventSynchronize(s->ev[2].e));
        HIP_TRY(hipEventElapsedTime(&ms, s->ev[0].e, s->ev[2].e));
        fill_stats(s, &ss->p, stats, ms, ms, k.counts);
        stats->samples = k.samples;
    }
    return RTMI_OK;
}
// a count the kernels can index: below 2^31 by the contract of the header, below 2^26 by the (sample, pixel) packing
static int session_check_count(const std::string &nm, uint64_t last) {
    if (last > (1ull << 31)) return fail(RTMI_ERR_INVALID, nm + "the sample count would pass 2^31");
    if (last > (1ull << 26)) return fail(RTMI_ERR_UNSUPPORTED, nm + "sample indices must stay below 2^26");
    return RTMI_OK;
}

extern "C" int rtmi_session_render(rtmi_session *ss, uint32_t add_spp, rtmi_stats *stats) {
    const char *name = "rtmi_session_render";
    const std::string nm = std::string(name) + ": ";
    int rc = session_usable(ss, nm, false);
    if (rc) return rc;
    if (add_spp == 0u) return fail(RTMI_ERR_INVALID, nm + "add_spp must be positive");
    const uint32_t from = ss->n.empty() ? 0u : ss->n[0];
    if ((rc = session_check_count(nm, (uint64_t)ss->o.first_sample + from + add_spp))) return rc;
    const std::string null_scene = nm + "scene is NULL";
    const Estimator m = session_estimator(ss, name, null_scene);
    SessionCall k;
    if ((rc = session_begin(k, ss, m))) return rc;
    std::vector<uint32_t> all(ss->T);
    for (uint32_t t = 0; t < ss->T; t++) all[t] = t;
    return session_end(k, ss, session_advance(k, ss, m, all, from, add_spp), stats);
}

// the tiles of `cand` (all at n samples) that fail the test under (abs_tol, rel_tol), in any order
static int session_test(rtmi_session *ss, std::vector<uint32_t> &cand, uint32_t n, double abs_tol, double rel_tol) {
    rtmi_scene *s = ss->s;
    hipStream_t stream = s->stream.s;
    uint32_t *in = s->ad_lists.ptr, *outl = s->ad_lists.ptr + ss->T, *count = s->ad_lists.ptr + 2 * (size_t)ss->T;
    HIP_TRY(hipMemcpyAsync(in, cand.data(), cand.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(count, 0, sizeof(uint32_t), stream));
    SessionDecide D;
    D.state = ss->state.ptr; D.tiles_in = in; D.n_in = (uint32_t)cand.size(); D.tiles_out = outl; D.n_out = count;
    D.nx = ss->p.nx; D.ny = ss->p.ny; D.tiles_x = tiles_x_of(&ss->p);
    D.n = n; D.abs_tol = abs_tol; D.rel_tol = rel_tol;
    HIP_TRY(rtmi_session_launch_decide(stream, D));
    HIP_TRY(hipStreamSynchronize(stream));
    uint32_t left = 0;
    HIP_TRY(hipMemcpy(&left, count, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (left > cand.size()) return fail(RTMI_ERR_DEVICE, "rtmi_session_refine: the test listed more tiles than it was given");
    cand.resize(left);
    if (left) HIP_TRY(hipMemcpy(cand.data(), outl, (size_t)left * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RTMI_OK;
}

extern "C" int rtmi_session_refine(rtmi_session *ss, double abs_tol, double rel_tol, uint32_t cap, rtmi_stats *stats) {
    const char *name = "rtmi_session_refine";
    const std::string nm = std::string(name) + ": ";
    int rc = session_usable(ss, nm, true);
    if (rc) return rc;
    const uint32_t min_spp = ss->o.min_spp, step = ss->o.step_spp;
    if (!std::isfinite(abs_tol) || !(abs_tol >= 0.0) || !std::isfinite(rel_tol) || !(rel_tol >= 0.0))
        return fail(RTMI_ERR_INVALID, nm + "abs_tol and rel_tol must be finite and non-negative");
    if (cap < min_spp) return fail(RTMI_ERR_INVALID, nm + "min_spp must not exceed the cap");
    if ((rc = session_check_count(nm, cap))) return rc;
    if (cap < ss->last_cap || abs_tol > ss->last_abs || rel_tol > ss->last_rel)
        return fail(RTMI_ERR_INVALID, nm + "a call must not loosen: cap >= the previous cap, abs_tol and rel_tol <= the previous ones");
    const std::string null_scene = nm + "scene is NULL";
    const Estimator m = session_estimator(ss, name, null_scene);
    SessionCall k;
    if ((rc = session_begin(k, ss, m))) return rc;

    std::map<uint32_t, std::vector<uint32_t>> parked; // count -> the tiles parked there, below the cap
    for (uint32_t t = 0; t < ss->T; t++)
        if (ss->n[t] < cap) parked[ss->n[t]].push_back(t);
    std::vector<uint32_t> active; // the unsettled tiles, all at `cur`
    uint32_t cur = 0;
    while (!rc) {
        if (active.empty()) {
            if (parked.empty()) break;
            cur = parked.begin()->first;
        }
        auto here = parked.find(cur);
        if (here != parked.end()) { // the tiles carried from below join the tiles parked at this count
            active.insert(active.end(), here->second.begin(), here->second.end());
            parked.erase(here);
        }
        const bool on_lattice = cur >= min_spp && (cur - min_spp) % step == 0u;
        if (on_lattice && (rc = session_test(ss, active, cur, abs_tol, rel_tol))) break; // off the lattice: no test, they continue
        if (active.empty()) continue;
        uint64_t next = cur < min_spp ? min_spp : (uint64_t)cur + step - (cur - min_spp) % step;
        if (next > cap) next = cap;
        if (!parked.empty() && parked.begin()->first < next) next = parked.begin()->first;
        if ((rc = session_advance(k, ss, m, active, cur, (uint32_t)next - cur))) break;
        cur = (uint32_t)next;
        if (cur >= cap) break; // settled at the cap
    }
    if (!rc) { ss->last_cap = cap; ss->last_abs = abs_tol; ss->last_rel = rel_tol; }
    return session_end(k, ss, rc, stats);
}

extern "C" int rtmi_session_spp(rtmi_session *ss, uint32_t *min_spp, uint32_t *max_spp) {
    const std::string nm = "rtmi_session_spp: ";
    if (int rc = session_usable(ss, nm, false, true)) return rc;
    std::lock_guard<std::mutex> lock(ss->s->mu);
    uint32_t lo = 0xffffffffu, hi = 0u;
    for (uint32_t v : ss->n) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
    if (min_spp) *min_spp = ss->n.empty() ? 0u : lo;
    if (max_spp) *max_spp = hi;
    return RTMI_OK;
}

extern "C" int rtmi_session_image(rtmi_session *ss, float *out_linear, uint8_t *out_rgb8, float *out_stderr, uint32_t *out_spp,
                                  uint32_t *out_bounces) {
    const char *name = "rtmi_session_image";
    const std::string nm = std::string(name) + ": ";
    int rc = session_usable(ss, nm, false, true);
    if (rc) return rc;
    rtmi_scene *s = ss->s;
    std::unique_lock<std::mutex> lock(s->mu);
    for (uint32_t v : ss->n)
        if (v == 0u) return fail(RTMI_ERR_INVALID, nm + "the session holds no samples yet");
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = begin_blocking(s))) return rc;
    BusyMark busy{s, s->stream.s};
    const size_t ntex = (size_t)ss->T * 64;
    if ((rc = reserve_texels(s, ntex)) || (rc = grow_adaptive(s, ss->T))) return rc;
    HIP_TRY(hipMemcpyAsync(ss->d_counts.ptr, ss->n.data(), (size_t)ss->T * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream.s));
    const SessionReadout R{ss->state.ptr, ss->d_counts.ptr, ss->T, s->texels.ptr, s->ad_stderr.ptr, s->ad_spp.ptr};
    HIP_TRY(rtmi_session_launch_readout(s->stream.s, R));
    HIP_TRY(hipStreamSynchronize(s->stream.s));
    HIP_TRY(hipMemcpy(s->h_texels.ptr, s->texels.ptr, ntex * sizeof(rtmi_texel), hipMemcpyDeviceToHost));
    if (out_stderr && (rc = download_untiled<3>(&ss->p, s->ad_stderr.ptr, ntex, out_stderr))) return rc;
    if (out_spp && (rc = download_untiled<1>(&ss->p, s->ad_spp.ptr, ntex, out_spp))) return rc;
    if (out_bounces && (rc = download_untiled<1>(&ss->p, ss->bounces.ptr, ntex, out_bounces))) return rc;
    return rtmi_untile(&ss->p, s->h_texels.ptr, out_linear, out_rgb8);
}

extern "C" int rtmi_session_export(rtmi_session *ss, void *buf, size_t cap, size_t *need) {
    const std::string nm = "rtmi_session_export: ";
    int rc = session_usable(ss, nm, false, true);
    if (rc) return rc;
    if (!need) return fail(RTMI_ERR_INVALID, nm + "NULL argument");
    *need = session_blob_bytes(ss);
    if (!buf) return RTMI_OK;
    if (cap < *need) return fail(RTMI_ERR_INVALID, nm + "the buffer is smaller than the blob");
    rtmi_scene *s = ss->s;
    std::lock_guard<std::mutex> lock(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    if (s->busy_recorded) HIP_TRY(hipEventSynchronize(s->busy.e));
    uint8_t *b = static_cast<uint8_t *>(buf);
    const std::vector<uint8_t> h = session_header(ss);
    std::memcpy(b, h.data(), h.size());
    size_t at = h.size();
    std::memcpy(b + at, ss->n.data(), (size_t)ss->T * 4);
    at += (size_t)ss->T * 4;
    HIP_TRY(hipMemcpy(b + at, ss->state.ptr, (size_t)ss->T * 9 * 64 * 8, hipMemcpyDeviceToHost));
    at += (size_t)ss->T * 9 * 64 * 8;
    HIP_TRY(hipMemcpy(b + at, ss->bounces.ptr, (size_t)ss->T * 64 * 4, hipMemcpyDeviceToHost));
    return RTMI_OK;
}

extern "C" int rtmi_session_import(rtmi_session *ss, const void *buf, size_t len) {
    const std::string nm = "rtmi_session_import: ";
    if (!ss || !buf) return fail(RTMI_ERR_INVALID, nm + "NULL argument");
    const uint8_t *b = static_cast<const uint8_t *>(buf);
    if (len < RTMI_SESSION_BLOB_HEADER || std::memcmp(b, "RTMISESS", 8) != 0) return fail(RTMI_ERR_INVALID, nm + "not a session blob (magic)");
    uint32_t version = 0;
    std::memcpy(&version, b + 8, 4);
    if (version != RTMI_SESSION_BLOB_VERSION) return fail(RTMI_ERR_INVALID, nm + "unknown blob version");
    const std::vector<uint8_t> h = session_header(ss);
    if (std::memcmp(b, h.data(), RTMI_SESSION_BLOB_IDENTITY) != 0)
        return fail(RTMI_ERR_INVALID, nm + "the blob's identity block differs from the session's");
    if (len != session_blob_bytes(ss)) return fail(RTMI_ERR_INVALID, nm + "wrong blob length");
    uint32_t cap = 0;
    double abs_tol = 0.0, rel_tol = 0.0;
    std::memcpy(&cap, b + 196, 4); std::memcpy(&abs_tol, b + 200, 8); std::memcpy(&rel_tol, b + 208, 8);
    std::vector<uint32_t> n(ss->T);
    size_t at = RTMI_SESSION_BLOB_HEADER;
    std::memcpy(n.data(), b + at, (size_t)ss->T * 4);
    at += (size_t)ss->T * 4;
    for (uint32_t t = 0; t < ss->T; t++) {
        if (n[t] > (1u << 26) || (!ss->refine && n[t] != n[0]) || (ss->refine && cap != 0u && n[t] > cap))
            return fail(RTMI_ERR_INVALID, nm + "the blob's counts are not a session's");
    }
    rtmi_scene *s = ss->s;
    std::lock_guard<std::mutex> lock(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    if (s->busy_recorded) HIP_TRY(hipEventSynchronize(s->busy.e));
    HIP_TRY(hipMemcpy(ss->state.ptr, b + at, (size_t)ss->T * 9 * 64 * 8, hipMemcpyHostToDevice));
    at += (size_t)ss->T * 9 * 64 * 8;
    HIP_TRY(hipMemcpy(ss->bounces.ptr, b + at, (size_t)ss->T * 64 * 4, hipMemcpyHostToDevice));
    ss->n = n;
    ss->last_cap = cap; ss->last_abs = abs_tol; ss->last_rel = rel_tol;
    ss->failed = false;
    return RTMI_OK;
}

extern "C" int rtmi_session_merge(rtmi_session *dst, const rtmi_session *src) {
    const std::string nm = "rtmi_session_merge: ";
    int rc;
    if ((rc = session_usable(dst, nm, false)) || (rc = session_usable(src, nm, false))) return rc;
    if (dst == src) return fail(RTMI_ERR_INVALID, nm + "dst and src are one session");
    const std::vector<uint8_t> ha = session_header(dst), hb = session_header(src, &dst->o.first_sample);
    if (std::memcmp(ha.data(), hb.data(), RTMI_SESSION_BLOB_IDENTITY) != 0) // equal identity except first_sample
        return fail(RTMI_ERR_INVALID, nm + "the sessions' identity blocks differ");
    const uint32_t nA = dst->n.empty() ? 0u : dst->n[0], nB = src->n.empty() ? 0u : src->n[0];
    if ((uint64_t)src->o.first_sample != (uint64_t)dst->o.first_sample + nA)
        return fail(RTMI_ERR_INVALID, nm + "the sample ranges are not adjacent: src.first_sample must equal dst.first_sample + dst's count");
    if ((rc = session_check_count(nm, (uint64_t)dst->o.first_sample + nA + nB))) return rc;
    if (dst->s->device != src->s->device)
        return fail(RTMI_ERR_UNSUPPORTED, nm + "the sessions live on different devices: export one and import it next to the other");
    if (nB == 0u) return RTMI_OK;
    rtmi_scene *s = dst->s, *s2 = src->s;
    std::unique_lock<std::mutex> l1(s->mu, std::defer_lock), l2;
    if (s2 != s) {
        l2 = std::unique_lock<std::mutex>(s2->mu, std::defer_lock);
        std::lock(l1, l2);
    } else {
        l1.lock();
    }
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = begin_blocking(s))) return rc;
    if (s2 != s && s2->busy_recorded) HIP_TRY(hipEventSynchronize(s2->busy.e));
    BusyMark busy{s, s->stream.s};
    const size_t T = dst->T;
    if (nA == 0u) {
        HIP_TRY(hipMemcpyAsync(dst->state.ptr, src->state.ptr, T * 9 * 64 * sizeof(double), hipMemcpyDeviceToDevice, s->stream.s));
        HIP_TRY(hipMemcpyAsync(dst->bounces.ptr, src->bounces.ptr, T * 64 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s->stream.s));
    } else {
        const SessionMerge M{dst->state.ptr, src->state.ptr, dst->bounces.ptr, src->bounces.ptr, dst->T, (double)nA, (double)nB};
        HIP_TRY(rtmi_session_launch_merge(s->stream.s, M));
    }
    const hipError_t e = hipStreamSynchronize(s->stream.s);
    if (e != hipSuccess) {
        dst->failed = true;
        return fail(RTMI_ERR_DEVICE, nm + hipGetErrorString(e));
    }
    dst->n.assign(dst->T, nA + nB);
    return RTMI_OK;
}
