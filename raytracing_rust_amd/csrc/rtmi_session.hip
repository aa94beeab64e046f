// rtmi_session.hip — translation unit of render sessions (include/rtmi_session.h): the kernels that work on a session's
// state alone, and their launchers.  Compiled with the flags of rtmi_device.hip (-ffp-contract=off: no fused operations,
// so numpy restates read-out and merge bit for bit).
//
// The render kernels and the per-pass resolve of a session are the existing ones (rtmi_adaptive_resolve_kernel with
// decide = 0 writes sum, m and M2 back for every tile).  What is here streams the [tile][9][64] planes: one wavefront per
// tile, lane = pixel, so every plane access is one coalesced 512-byte row; no LDS, no scratch, memory-bound.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rtmi.h"
#include "rtmi_session_launch.hpp"

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
