// rtmi_pixelwise.hip — translation unit of per-pixel adaptive sampling (include/rtmi_pixelwise.h): the step kernel and its
// launcher.  Compiled with the flags of rtmi_adaptive.hip (-ffp-contract=off: no fused operations, so numpy restates the
// estimator bit for bit).  The select and the path kernel of a step are those of rtmi_sparse.hip, launched as they are by
// the entries in rtmi_batch.hip.
//
// One lane per list entry.  Entry k names pixel p = list[k] and owns records [k * pass, (k + 1) * pass) of the per-sample
// buffer.  The lane loads the nine doubles of p from the structure-of-arrays state (an ascending list reads each row nearly
// coalesced; nothing is loaded when n_done == 0, so the state is never cleared), folds the records in sample order with the
// arithmetic of rtmi_adaptive_resolve_kernel, stores the state and, when the launch ends a step, tests the pixel alone,
// writes its planes and its active byte.  All entries of a launch share n_done and pass: the state holds no count.
//
// The records of a lane are 12 * pass bytes apart; it reads them with four loads in flight, as the tile resolve does.  A
// form in which a wavefront staged the contiguous block of its 64 entries through LDS (coalesced 16-byte loads, rows padded
// to an odd number of dwords) was built and measured: 569 us against 171 us for 640 000 entries of 64 samples on an MI355X,
// so it is not here (profiles/pixelwise/step_kernel_lds_stage.patch).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rtmi.h"
#include "rtmi_math.h"

#define RTMI_LEAN_TU 1 /* the plain kernels are defined in rtmi_device.hip */
#include "rtmi_kernels.hpp"
#include "rtmi_pixelwise_launch.hpp"

__global__ __launch_bounds__(256) void rtmi_pixelwise_step_kernel(PixelwiseStep S) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t entries = S.capacity;
    if (S.count) {
        const uint32_t c = S.count[0];
        entries = c < S.capacity ? c : S.capacity;
    }
    if (k >= entries) return;
    const uint32_t p = S.list[k];
    if (p >= S.n_pixels) return;
    double sum[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0}, M2[3] = {0.0, 0.0, 0.0};
    double *st = S.state + p;
    const size_t plane = S.n_pixels;
    if (S.n_done != 0u) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) { sum[ch] = st[ch * plane]; m[ch] = st[(3 + ch) * plane]; M2[ch] = st[(6 + ch) * plane]; }
    }
    const auto add = [&](const Rad3 v, uint32_t smp) {
        const double kk = (double)(S.n_done + smp + 1u); // this sample's 1-based index in the pixel's sequence
        const double x[3] = {(double)v.r, (double)v.g, (double)v.b};
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            sum[ch] += x[ch];
            const double d = x[ch] - m[ch];
            m[ch] = m[ch] + d / kk;
            M2[ch] = M2[ch] + d * (x[ch] - m[ch]);
        }
    };
    const Rad3 *src = S.samples + (size_t)k * S.pass;
    uint32_t s = 0;
    for (; s + 4u <= S.pass; s += 4u) { // 4 independent loads in flight, updates in sample order
        Rad3 v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = src[s + j];
#pragma unroll
        for (int j = 0; j < 4; j++) add(v[j], s + (uint32_t)j);
    }
    for (; s < S.pass; s++) add(src[s], s);
#pragma unroll
    for (int ch = 0; ch < 3; ch++) { st[ch * plane] = sum[ch]; st[(3 + ch) * plane] = m[ch]; st[(6 + ch) * plane] = M2[ch]; }
    if (!S.decide) return;
    // the test and the texel of rtmi_adaptive_resolve_kernel, for one pixel
    const uint32_t n_u = S.n_done + S.pass;
    const double n = (double)n_u;
    bool ok = true;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const double mean = sum[ch] / n;
        const double e = sqrt(M2[ch] / (n * (n - 1.0)));
        ok = ok && __builtin_isfinite(e) && __builtin_isfinite(mean) && e <= S.abs_tol + S.rel_tol * fabs(mean);
        if (S.stderr_out) S.stderr_out[3 * (size_t)p + ch] = (float)e;
        if (S.linear) S.linear[3 * (size_t)p + ch] = (float)mean;
        if (S.rgb8) {
            double g = sqrt(mean);
            g = (g > 0.0) ? ((g < 1.0) ? g : 1.0) : 0.0; // NaN -> 0
            const double x = 255.99 * g;
            S.rgb8[3 * (size_t)p + ch] = (x != x) ? (uint8_t)0u : (uint8_t)(int32_t)x;
        }
    }
    if (S.spp) S.spp[p] = n_u;
    if (S.active) S.active[p] = (!ok && n_u < S.cap) ? (uint8_t)1u : (uint8_t)0u;
}

hipError_t rtmi_pixelwise_launch_step(hipStream_t stream, const PixelwiseStep &S) {
    hipLaunchKernelGGL(rtmi_pixelwise_step_kernel, dim3((S.capacity + 255u) / 256u), dim3(256), 0, stream, S);
    return hipGetLastError();
}
