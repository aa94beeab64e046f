// rtmi_features.hip — translation unit of the first-hit features (include/rtmi_features.h): the features kernels and
// their resolve, and the launchers.  Compiled with the flags of rtmi_device.hip (-ffp-contract=off: no fused operations,
// so the distance and the f64 sums are restated bit for bit on the host).
//
// The features kernel is the body of rtmi_render_kernel (rtmi_kernel_perlane.inc) with FEATURES = true: same work queue,
// camera_sample, item scan and two-phase schedule, so every lane finds the first interaction of the render's path of its
// (sample, pixel), media included.  Phase B ends the path there and writes a FeatSlot (albedo, normal, distance) instead
// of a radiance; a miss writes a miss slot.  Instantiated for FAST x SIG.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "rtmi.h"
#include "rtmi_math.h"

#define RTMI_LEAN_TU 1 /* the plain kernels are defined in rtmi_device.hip */
#include "rtmi_kernels.hpp"
#include "rtmi_features_launch.hpp"

template <bool FAST, bool SIG>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void rtmi_features_kernel(DevScene sc, DevCamera cam, DevParams P) {
    constexpr bool PROF = false, TILE_LIST = false, FEATURES = true, NEE = false, ENV = false;
    const DevLights nl{};
    const DevEnv ev{};
    const uint32_t *const tiles = nullptr;
#include "rtmi_kernel_perlane.inc"
}

// One wavefront per tile, one lane per pixel.  Adds the pass's slots in sample order in f64 (albedo and normal of every
// sample, distance and count of the samples with a first interaction) and, on the last pass, writes the four planes,
// each rounded to f32 once.
__global__ __launch_bounds__(256) void rtmi_features_resolve_kernel(DevParams P, FeaturesResolve R) {
    const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (tile >= P.ntiles_local) return; // wave-uniform
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
    const uint32_t col = tx * RTMI_TILE + (lane & 7u), row = ty * RTMI_TILE + (lane >> 3);
    if (col >= P.nx || row >= P.ny) return;
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double *st = R.state + (size_t)tile * (8u * 64u) + lane;
    if (!R.first) {
#pragma unroll
        for (int k = 0; k < 8; k++) acc[k] = st[k * 64];
    }
    const FeatSlot *src = R.slots + ((size_t)tile * P.pass_stride) * 64u + lane;
    const auto add = [&](const FeatSlot &v) {
#pragma unroll
        for (int c = 0; c < 3; c++) { acc[c] += (double)v.albedo[c]; acc[3 + c] += (double)v.normal[c]; }
        if (v.dist >= 0.0) { acc[6] += v.dist; acc[7] += 1.0; }
    };
    uint32_t s = 0;
    for (; s + 4u <= P.pass_cnt; s += 4u) { // 4 independent loads in flight, additions in sample order
        FeatSlot v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = src[(size_t)(s + k) * 64u];
#pragma unroll
        for (int k = 0; k < 4; k++) add(v[k]);
    }
    for (; s < P.pass_cnt; s++) add(src[(size_t)s * 64u]);
    if (!R.last) {
#pragma unroll
        for (int k = 0; k < 8; k++) st[k * 64] = acc[k];
        return;
    }
    const double ns = (double)P.ns;
    const size_t o = (size_t)row * P.nx + col;
#pragma unroll
    for (int c = 0; c < 3; c++) { R.albedo[o * 3 + c] = (float)(acc[c] / ns); R.normal[o * 3 + c] = (float)(acc[3 + c] / ns); }
    R.depth[o] = acc[7] > 0.0 ? (float)(acc[6] / acc[7]) : __builtin_inff();
    R.hits[o] = (uint32_t)acc[7];
}

hipError_t rtmi_features_launch_render(bool fast, bool sig, uint32_t blocks, hipStream_t stream, const DevScene &sc,
                                       const DevCamera &cam, const DevParams &P) {
    const dim3 grid(blocks), block(64 * WAVES_PER_BLOCK);
    if (fast && sig) hipLaunchKernelGGL((rtmi_features_kernel<true, true>), grid, block, 0, stream, sc, cam, P);
    else if (fast) hipLaunchKernelGGL((rtmi_features_kernel<true, false>), grid, block, 0, stream, sc, cam, P);
    else if (sig) hipLaunchKernelGGL((rtmi_features_kernel<false, true>), grid, block, 0, stream, sc, cam, P);
    else hipLaunchKernelGGL((rtmi_features_kernel<false, false>), grid, block, 0, stream, sc, cam, P);
    return hipGetLastError();
}

hipError_t rtmi_features_launch_resolve(hipStream_t stream, const DevParams &P, const FeaturesResolve &R) {
    hipLaunchKernelGGL(rtmi_features_resolve_kernel, dim3((P.ntiles_local + 3u) / 4u), dim3(256), 0, stream, P, R);
    return hipGetLastError();
}
