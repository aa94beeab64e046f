// rtmi_gather.hip — translation unit of the hemisphere gathers (include/rtmi_gather.h): path-traced radiance along
// directions the device draws about batches of caller-supplied points, the per-point reduction with its spherical-harmonic
// projection, the launchers, and the host form of the directions.  Compiled with the flags of rtmi_device.hip
// (-ffp-contract=off: the directions are the header's inline functions, which numpy restates bit for bit, and the host
// function below computes what the kernels compute).
//
// The path kernel is rtmi_radiance_kernel (rtmi_radiance.hip) with another take step: the same fragments rtmi_path_lane.inc,
// rtmi_path_scan.inc, rtmi_path_traced.inc and rtmi_path_shade.inc, the same items (item k = i * spp + s is sample s of point
// i and slot k of the per-sample buffer), the same two-level refill from the handle's chunk counter (batch_take,
// rtmi_batch.hpp).  The take reads one point record (12 B, a 12-B normal for COSINE, a
// 4-B time when there is a time plane) instead of a 32-B ray, draws the direction from stream 5 and starts the path the
// radiance query starts for that ray with stream_skip = 0.  Every segment runs under (P.t_min, FLT_MAX), so the radiance
// kernel's per-lane first-segment interval is not carried.  Instantiated for FAST x NEE x ENV x SPHERE.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <type_traits>

#include "rtmi.h"
#include "rtmi_math.h"
#include "rtmi_gather.h"

#define RTMI_LEAN_TU 1 /* the plain kernels are defined in rtmi_device.hip */
#include "rtmi_kernels.hpp"
#include "rtmi_light_launch.hpp"
#include "rtmi_batch.hpp"
#include "rtmi_gather_launch.hpp"
#include "rtmi_hostkit.hpp"

static_assert(sizeof(rtmi_gather_params) == 64, "rtmi_gather_params layout");

// direction s of point i (absolute indices) in the batch's mode; n: the point's normal (COSINE)
template <bool SPHERE>
__device__ __forceinline__ void gather_direction(uint32_t k0, uint32_t k1, uint32_t sample, uint32_t point, const float n[3], float d[3]) {
    uint32_t w0, w1, w2, w3;
    philox(0u, sample, point, RTMI_GATHER_STREAM, k0, k1, w0, w1, w2, w3);
    if constexpr (SPHERE) rtmi_gather_sphere(rtmi_u01(w0), rtmi_u01(w1), d);
    else rtmi_gather_cosine(rtmi_u01(w0), rtmi_u01(w1), n, d);
}

template <bool FAST, bool NEE, bool ENV, bool SPHERE>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void rtmi_gather_kernel(DevScene sc, DevParams P, GatherBatch B, DevLights nl,
                                                                           DevEnv ev) {
    constexpr bool PROF = false, SIG = false, FEATURES = false;
    unsigned long long *prof = nullptr;
    // per wave: [0] node refs, [1] entry distances (FAST only); entry-major so lanes never bank-conflict
    __shared__ uint32_t lds_stack[WAVES_PER_BLOCK][FAST ? 2 : 1][RTMI_MAX_BVH_DEPTH][64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    uint32_t *stack = &lds_stack[wave][0][0][lane];
    unsigned long long sig = 0ull; // SIG = false: named by the fragments, never live
    BatchWork w;
    w.next = 0u; w.end = 0u;
    bool queue_empty = false;
    const uint32_t k0 = P.key0, k1 = P.key1;
    const int threshold = (int)P.shade_threshold;

    uint32_t oidx = 0u, ltile = 0u; // slot of this lane's path in the per-sample buffer (= its item)
    bool alive = false, done = false, have_hit = false;
    typename std::conditional<NEE, RngNee, RngReg>::type g;
#include "rtmi_path_lane.inc"

    for (;;) {
        // ================= phase A: trace until enough lanes hold a hit =================
        for (;;) {
            if (__ballot(!have_hit && !done) == 0ull) break;
            { // lanes whose path ended take the next (point, sample) item, or are done when there is none
                const bool want = !have_hit && !done && !alive;
                if (__ballot(want) != 0ull) {
                    if (batch_take(w, queue_empty, want, B.queue, B.chunk, B.total, B.nchunks, oidx)) {
                        const uint32_t i = oidx / B.spp, s = oidx - i * B.spp;
                        const float *pt = B.points + 3 * (size_t)i;
                        pa.ro = f3(pt[0], pt[1], pt[2]);
                        float nrm[3] = {0.0f, 0.0f, 1.0f}, d[3];
                        if constexpr (!SPHERE) {
                            const float *pn = B.normals + 3 * (size_t)i;
                            nrm[0] = pn[0]; nrm[1] = pn[1]; nrm[2] = pn[2];
                        }
                        gather_direction<SPHERE>(k0, k1, B.first_sample + s, B.first_point + i, nrm, d);
                        pa.rd = f3(d[0], d[1], d[2]);
                        pa.rtime = B.time ? B.time[i] : 0.0f;
                        pa.T = f3(1, 1, 1);
                        pa.L = f3(0, 0, 0);
                        pa.depth = 0;
                        rng_init(g, B.first_sample + s, B.first_point + i);
                        if constexpr (NEE) { rng_init(gn, B.first_sample + s, B.first_point + i); ne.pb = 0.0f; }
                        alive = true;
                    } else if (want) {
                        done = true;
                    }
                }
            }
            const bool need = !have_hit && !done;
            if (need) {
#define RTMI_SCAN_T_MIN P.t_min
#define RTMI_SCAN_T_MAX RTMI_FLT_MAX
#include "rtmi_path_scan.inc"
#undef RTMI_SCAN_T_MIN
#undef RTMI_SCAN_T_MAX
#include "rtmi_path_traced.inc"
            }
            if (__popcll(__ballot(have_hit)) >= threshold) break;
        }
        // ================= phase B: shade every lane that holds a hit =================
#define RTMI_PATH_SCRATCH &lds_stack[wave][0][0][0]
#define RTMI_PATH_INST true
#include "rtmi_path_shade.inc"
#undef RTMI_PATH_SCRATCH
#undef RTMI_PATH_INST
    }
}

// One lane per point: the f64 sum of its spp samples in sample order and Welford's recurrence (rtmi_batch_welford.inc), the
// COSINE factor pi, and for SPHERE with an sh output the projection on the nine harmonics of every sample's direction, drawn
// again from its counter: that branch spells the loop out, with the projection inside it.  spp == 1: no estimate, +inf.
template <bool SPHERE>
__global__ __launch_bounds__(256) void rtmi_gather_resolve_kernel(const Rad3 *__restrict__ samples, GatherBatch B, uint32_t k0,
                                                                 uint32_t k1) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B.n) return;
    const Rad3 *src = samples + (size_t)i * B.spp;
    double sum[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0}, M2[3] = {0.0, 0.0, 0.0};
    const double n = (double)B.spp;
    if (SPHERE && B.sh) { // wave-uniform
        double acc[9][3];
#pragma unroll
        for (int k = 0; k < 9; k++) acc[k][0] = acc[k][1] = acc[k][2] = 0.0;
        const float none[3] = {0.0f, 0.0f, 1.0f};
        for (uint32_t s = 0; s < B.spp; s++) {
            const Rad3 v = src[s];
            const double k = (double)(s + 1u);
            const double x[3] = {(double)v.r, (double)v.g, (double)v.b};
            float d[3], y[9];
            gather_direction<true>(k0, k1, B.first_sample + s, B.first_point + i, none, d);
            rtmi_gather_sh9(d, y);
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                sum[ch] += x[ch];
                const double dl = x[ch] - m[ch];
                m[ch] = m[ch] + dl / k;
                M2[ch] = M2[ch] + dl * (x[ch] - m[ch]);
#pragma unroll
                for (int q = 0; q < 9; q++) acc[q][ch] = acc[q][ch] + x[ch] * (double)y[q];
            }
        }
        const double c = RTMI_GATHER_4PI / n;
#pragma unroll
        for (int q = 0; q < 9; q++)
#pragma unroll
            for (int ch = 0; ch < 3; ch++) B.sh[27 * (size_t)i + 3 * q + ch] = (float)(c * acc[q][ch]);
    } else {
        const uint32_t ns = B.spp;
#include "rtmi_batch_welford.inc"
    }
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const double mean = sum[ch] / n;
        const double se = sqrt(M2[ch] / (n * (n - 1.0)));
        if (B.value) B.value[3 * (size_t)i + ch] = SPHERE ? (float)mean : (float)(RTMI_GATHER_PI * mean);
        if (B.stderr_out)
            B.stderr_out[3 * (size_t)i + ch] = B.spp > 1u ? (SPHERE ? (float)se : (float)(RTMI_GATHER_PI * se)) : __builtin_inff();
    }
}

hipError_t rtmi_gather_launch(bool fast, bool nee, bool env, uint32_t mode, uint32_t blocks, hipStream_t stream, const DevScene &sc,
                              const DevParams &P, const GatherBatch &B, const DevLights &L, const DevEnv &E) {
    const dim3 grid(blocks), block(64 * WAVES_PER_BLOCK);
    return rtmi_with_bools([&](auto FAST, auto NEE, auto ENV, auto SPHERE) {
        hipLaunchKernelGGL((rtmi_gather_kernel<FAST(), NEE(), ENV(), SPHERE()>), grid, block, 0, stream, sc, P, B, L, E);
        return hipGetLastError();
    }, fast, nee, env, mode == RTMI_GATHER_SPHERE);
}

hipError_t rtmi_gather_launch_resolve(uint32_t mode, hipStream_t stream, const Rad3 *samples, const GatherBatch &B, uint32_t key0,
                                      uint32_t key1) {
    const dim3 grid((B.n + 255u) / 256u), block(256);
    if (mode == RTMI_GATHER_SPHERE) hipLaunchKernelGGL(rtmi_gather_resolve_kernel<true>, grid, block, 0, stream, samples, B, key0, key1);
    else hipLaunchKernelGGL(rtmi_gather_resolve_kernel<false>, grid, block, 0, stream, samples, B, key0, key1);
    return hipGetLastError();
}

// ---- the directions on the host (include/rtmi_gather.h) -------------------------------------------------------------------
// Philox4x32-10 as rtmi_rng.hpp's device function computes it
static void philox_host(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t &o0, uint32_t &o1) {
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    o0 = c0; o1 = c1;
}

extern "C" int rtmi_gather_directions(const rtmi_gather_params *p, const float *normals, uint32_t n, float *out_dirs) {
    const std::string nm = "rtmi_gather_directions: ";
    if (!p) return rtmi_fail(RTMI_ERR_INVALID, (nm + "params is NULL").c_str());
    if (p->mode > RTMI_GATHER_SPHERE) return rtmi_fail(RTMI_ERR_INVALID, (nm + "mode must be RTMI_GATHER_COSINE or RTMI_GATHER_SPHERE").c_str());
    if (p->spp == 0u) return rtmi_fail(RTMI_ERR_INVALID, (nm + "spp must be at least 1").c_str());
    if (p->first_point > (1ull << 32) || p->first_point + n > (1ull << 32))
        return rtmi_fail(RTMI_ERR_INVALID, (nm + "first_point + n must not exceed 2^32").c_str());
    if ((uint64_t)p->first_sample + p->spp > (1ull << 32))
        return rtmi_fail(RTMI_ERR_INVALID, (nm + "first_sample + spp must not exceed 2^32").c_str());
    if (n == 0u) return RTMI_OK;
    const bool sphere = p->mode == RTMI_GATHER_SPHERE;
    if (!out_dirs) return rtmi_fail(RTMI_ERR_INVALID, (nm + "out_dirs is NULL").c_str());
    if (!sphere && !normals) return rtmi_fail(RTMI_ERR_INVALID, (nm + "normals is NULL (RTMI_GATHER_COSINE)").c_str());
    if (!sphere)
        for (uint32_t i = 0; i < n; i++) {
            const float l = rtmi_gather_normal_length(normals + 3 * (size_t)i);
            if (!(l > 0.0f) || !std::isfinite(l))
                return rtmi_fail(RTMI_ERR_INVALID, (nm + "point " + std::to_string(i) + " has a zero or non-finite normal").c_str());
        }
    const uint32_t k0 = (uint32_t)p->seed, k1 = (uint32_t)(p->seed >> 32);
    const float none[3] = {0.0f, 0.0f, 1.0f};
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t s = 0; s < p->spp; s++) {
            uint32_t w0, w1;
            philox_host(0u, p->first_sample + s, (uint32_t)p->first_point + i, RTMI_GATHER_STREAM, k0, k1, w0, w1);
            float *d = out_dirs + 3 * ((size_t)i * p->spp + s);
            if (sphere) rtmi_gather_sphere(rtmi_u01(w0), rtmi_u01(w1), d);
            else rtmi_gather_cosine(rtmi_u01(w0), rtmi_u01(w1), normals + 3 * (size_t)i, d);
        }
    return RTMI_OK;
}
