// rtmi_adaptive.hip — translation unit of adaptive sampling (include/rtmi_adaptive.h): the render kernels with the
// tile-list queue and the adaptive resolve, and their launchers.  Compiled with the flags of rtmi_device.hip
// (-ffp-contract=off: no fused operations, so numpy restates the estimator bit for bit).
//
// The render kernels are the bodies of rtmi_render_coop and rtmi_render_kernel (rtmi_kernel_coop.inc,
// rtmi_kernel_perlane.inc) with TILE_LIST = true: queue unit -> position in the active-tile list -> tile.  Only the
// instantiations the adaptive host loop launches exist: the default cooperative kernel in its lean and EXT forms and
// the per-lane kernel, exact and fast-cull.  Scenes that need the cooperative kernel's level-1/2 instantiations (instanced
// primitives, media inside transforms) run the per-lane kernel: same image, slower.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "rtmi.h"
#include "rtmi_math.h"

#define RTMI_LEAN_TU 1 /* the plain kernels are defined in rtmi_device.hip */
#include "rtmi_kernels.hpp"
#include "rtmi_adaptive_launch.hpp"

template <bool EXT>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, 4) void rtmi_adaptive_coop(DevScene sc, DevCamera cam, DevParams P,
                                                                             const uint32_t *tiles) {
    constexpr bool SIG = false, PROF = false, TILE_LIST = true, NEE = false, ENV = false, ONE_TREE = false;
    constexpr int WPS = 4, INSTL = 0;
    (void)WPS;
    const DevLights nl{};
    const DevEnv ev{};
#include "rtmi_kernel_coop.inc"
}

template <bool FAST>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void rtmi_adaptive_kernel(DevScene sc, DevCamera cam, DevParams P,
                                                                            const uint32_t *tiles) {
    constexpr bool SIG = false, PROF = false, TILE_LIST = true, FEATURES = false, NEE = false, ENV = false;
    const DevLights nl{};
    const DevEnv ev{};
#include "rtmi_kernel_perlane.inc"
}

// One wavefront per active tile, one lane per pixel (the tile's 8x8 texels).  Adds the sub-pass's samples to the f64 sum
// in sample order (the additions of rtmi_resolve_kernel) and steps Welford's recurrence; at the end of a step tests the
// tile (a ballot over its in-image lanes), then either writes its texels, standard errors and count, or appends it to
// the next active list.
__global__ __launch_bounds__(256) void rtmi_adaptive_resolve_kernel(const Rad3 *__restrict__ samples, DevParams P,
                                                                    AdaptiveResolve A) {
    const uint32_t lpos = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (lpos >= P.ntiles_local) return; // wave-uniform
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t tile = A.tiles_in[lpos];
    const uint32_t ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
    const bool in_image = tx * RTMI_TILE + (lane & 7u) < P.nx && ty * RTMI_TILE + (lane >> 3) < P.ny;
    double sum[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0}, M2[3] = {0.0, 0.0, 0.0};
    double *st = A.state + (size_t)tile * (9u * 64u) + lane;
    if (!A.first) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) { sum[ch] = st[ch * 64]; m[ch] = st[(3 + ch) * 64]; M2[ch] = st[(6 + ch) * 64]; }
    }
    if (in_image) {
        const Rad3 *src = samples + ((size_t)lpos * P.pass_stride) * 64u + lane;
        uint32_t s = 0;
        const auto add = [&](const Rad3 v, uint32_t smp) {
            const double k = (double)(P.pass_s0 + smp + 1u); // this sample's 1-based index in the pixel's sequence
            const double x[3] = {(double)v.r, (double)v.g, (double)v.b};
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                sum[ch] += x[ch];
                const double d = x[ch] - m[ch];
                m[ch] = m[ch] + d / k;
                M2[ch] = M2[ch] + d * (x[ch] - m[ch]);
            }
        };
        for (; s + 4u <= P.pass_cnt; s += 4u) { // 4 independent loads in flight, updates in sample order
            Rad3 v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = src[(size_t)(s + k) * 64u];
#pragma unroll
            for (int k = 0; k < 4; k++) add(v[k], s + (uint32_t)k);
        }
        for (; s < P.pass_cnt; s++) add(src[(size_t)s * 64u], s);
    }
    const uint32_t n_u = P.pass_s0 + P.pass_cnt; // samples every active tile holds after this sub-pass
    bool retire = false;
    float se[3] = {0.0f, 0.0f, 0.0f};
    if (A.decide) {
        const double n = (double)n_u;
        bool ok = true;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const double mean = sum[ch] / n;
            const double e = sqrt(M2[ch] / (n * (n - 1.0)));
            se[ch] = (float)e;
            ok = ok && __builtin_isfinite(e) && __builtin_isfinite(mean) && e <= A.abs_tol + A.rel_tol * fabs(mean);
        }
        if (!in_image) ok = true;
        retire = __ballot(!ok) == 0ull || n_u >= A.ns; // wave-uniform
    }
    if (!retire) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) { st[ch * 64] = sum[ch]; st[(3 + ch) * 64] = m[ch]; st[(6 + ch) * 64] = M2[ch]; }
        if (A.decide && lane == 0u) A.tiles_out[atomicAdd(A.n_out, 1u)] = tile;
        return;
    }
    // the texel of rtmi_resolve_kernel with ns = n: col /= n; sqrt; clamp; (255.99*c) as i32 — tests/test.rs:71-78
    const double n = (double)n_u;
    rtmi_texel tx_out;
    uint32_t q[3];
    float lin[3];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const double mm = sum[ch] / n;
        lin[ch] = (float)mm;
        double g = sqrt(mm);
        g = (g > 0.0) ? ((g < 1.0) ? g : 1.0) : 0.0; // nalgebra::clamp(val, 0, 1); NaN -> 0
        const double x = 255.99 * g;
        q[ch] = (x != x) ? 0u : (uint32_t)(int32_t)x; // `as i32`; in [0,255] after the clamp
    }
    tx_out.r = lin[0]; tx_out.g = lin[1]; tx_out.b = lin[2];
    tx_out.rgb8 = q[0] | (q[1] << 8) | (q[2] << 16);
    if (P.status[0] != 0u) { // a traversal-pool overflow in this call: poisoned, as rtmi_resolve_kernel does
        const float nan = __uint_as_float(0x7fc00000u);
        tx_out.r = nan; tx_out.g = nan; tx_out.b = nan;
        tx_out.rgb8 = RTMI_TEXEL_POISON;
    }
    const size_t t = (size_t)tile * 64u + lane;
    A.texels[t] = tx_out;
    A.stderr_out[t * 3] = se[0]; A.stderr_out[t * 3 + 1] = se[1]; A.stderr_out[t * 3 + 2] = se[2];
    A.spp_out[t] = n_u;
}

hipError_t rtmi_adaptive_launch_render(int which, uint32_t blocks, size_t lds, hipStream_t stream, const DevScene &sc,
                                       const DevCamera &cam, const DevParams &P, const uint32_t *tiles) {
    const dim3 grid(blocks), block(64 * WAVES_PER_BLOCK);
    if (which == RTMI_AD_COOP_EXT) {
        return rtmi_launch_lds(&rtmi_adaptive_coop<true>, grid, block, lds, stream, sc, cam, P, tiles);
    } else if (which == RTMI_AD_COOP_LEAN) {
        return rtmi_launch_lds(&rtmi_adaptive_coop<false>, grid, block, lds, stream, sc, cam, P, tiles);
    } else if (which == RTMI_AD_PERLANE_FAST) {
        hipLaunchKernelGGL(rtmi_adaptive_kernel<true>, grid, block, 0, stream, sc, cam, P, tiles);
    } else {
        hipLaunchKernelGGL(rtmi_adaptive_kernel<false>, grid, block, 0, stream, sc, cam, P, tiles);
    }
    return hipGetLastError();
}

hipError_t rtmi_adaptive_launch_resolve(hipStream_t stream, const Rad3 *samples, const DevParams &P, const AdaptiveResolve &A) {
    hipLaunchKernelGGL(rtmi_adaptive_resolve_kernel, dim3((P.ntiles_local + 3u) / 4u), dim3(256), 0, stream, samples, P, A);
    return hipGetLastError();
}
