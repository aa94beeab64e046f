// rtmi_relight_dev.hip — the relight kernel (include/rtmi_relight.h) and its launcher.  Compiled with the
// flags of rtmi_device.hip (-ffp-contract=off: the rules of rtmi_relight.hpp are restated bit for bit on the host, and
// the flag keeps h.x * h.x + h.y * h.y and (4 pi r) r unfused in f64 as it does in fp32).
//
// One launch, ONE workgroup.  The cdf is a serial chain by specification (the running sum of select_p in table order) and
// so is the total in front of it: no reassociated reduction gives the sequential sum's bits, so one thread adds, from LDS,
// while the others wait at the barrier; everything around the two chains — the areas, select_p, the stores, every level
// of the tree — runs on all threads.  A table is hundreds to a few thousand lights; a second workgroup could only wait.
//
// Ordering.  The launch follows the scatter and refit kernels of its update on the same stream: the moved planes are
// visible to it.  Inside the launch nothing crosses a workgroup, so none of the agent-scope hand-off machinery is needed:
// the phases are separated by __syncthreads(), and what one wave stored before the barrier another reads after it with
// plain vector loads (one CU, one L1).  Every load of a value written earlier in the launch has a per-thread address, so
// none goes through the scalar cache, which the vector stores do not refresh; the two wave-uniform values, the total and
// the chains' chunks, travel through LDS.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rtmi.h"

#include "rtmi_relight.hpp"
#include "rtmi_relight_launch.hpp"

#define RTMI_RELIGHT_CHUNK 1024 /* lights per pass of a serial chain: 8 KiB of doubles and 4 KiB of floats in LDS */

__global__ void __launch_bounds__(RTMI_RELIGHT_BLOCK) rtmi_relight_kernel(RelightScene R) {
    __shared__ double s_val[RTMI_RELIGHT_CHUNK];
    __shared__ float s_cdf[RTMI_RELIGHT_CHUNK];
    __shared__ double s_total;
    const uint32_t tid = threadIdx.x, n = R.n;

    // ---- 1. per light: geo and k from the planes, the area, aw into the scratch
    for (uint32_t i = tid; i < n; i += RTMI_RELIGHT_BLOCK) {
        float *L = R.lights + (size_t)i * 12;
        const int plane = reinterpret_cast<const int32_t *>(L)[5];
        const uint32_t prim = reinterpret_cast<const uint32_t *>(L)[7];
        const float4 A = R.prim_a[prim];
        const float k = R.prim_b[prim].x;
        const float a[4] = {A.x, A.y, A.z, A.w};
        const double area = relight_area(plane, a);
        L[0] = A.x; L[1] = A.y; L[2] = A.z; L[3] = A.w;
        L[4] = k;
        L[8] = (float)area;
        R.aw[i] = area * R.weight[i];
    }
    __syncthreads();

    // ---- 2. the total, in table order: thread 0 adds one chunk from LDS while the others have fetched it
    double run = 0.0;
    for (uint32_t base = 0; base < n; base += RTMI_RELIGHT_CHUNK) {
        const uint32_t m = n - base < RTMI_RELIGHT_CHUNK ? n - base : RTMI_RELIGHT_CHUNK;
        for (uint32_t j = tid; j < m; j += RTMI_RELIGHT_BLOCK) s_val[j] = R.aw[base + j];
        __syncthreads();
        if (tid == 0)
            for (uint32_t j = 0; j < m; j++) run += s_val[j];
        __syncthreads();
    }
    if (tid == 0) s_total = run;
    __syncthreads();
    const double total = s_total;

    // ---- 3. select_p on all threads, 4. the cdf in table order, chunk by chunk
    run = 0.0;
    for (uint32_t base = 0; base < n; base += RTMI_RELIGHT_CHUNK) {
        const uint32_t m = n - base < RTMI_RELIGHT_CHUNK ? n - base : RTMI_RELIGHT_CHUNK;
        for (uint32_t j = tid; j < m; j += RTMI_RELIGHT_BLOCK) {
            const double sp = R.aw[base + j] / total;
            s_val[j] = sp;
            R.lights[(size_t)(base + j) * 12 + 9] = (float)sp;
        }
        __syncthreads();
        if (tid == 0)
            for (uint32_t j = 0; j < m; j++) {
                run += s_val[j];
                s_cdf[j] = base + j + 1u == n ? 1.0f : (float)run;
            }
        __syncthreads();
        for (uint32_t j = tid; j < m; j += RTMI_RELIGHT_BLOCK) R.lights[(size_t)(base + j) * 12 + 10] = s_cdf[j];
    }
    if (!R.nodes) return; // (the whole workgroup)

    // ---- 5. the tree, deepest level first: a slot's f64 box and power live in the scratch
    for (uint32_t k = 0; k < R.n_lvl; k++) {
        const uint32_t lb = R.words[k], le = R.words[k + 1];
        for (uint32_t q = lb + tid; q < le; q += RTMI_RELIGHT_BLOCK) {
            const uint32_t slot = R.words[q];
            float *N = R.nodes + (size_t)slot * 8;
            const uint32_t link = reinterpret_cast<const uint32_t *>(N)[5];
            RelightBox b;
            double pw;
            if (link & RTMI_RELIGHT_LEAF) {
                const uint32_t li = link & 0x7fffffffu;
                const float *L = R.lights + (size_t)li * 12;
                const float a[4] = {L[0], L[1], L[2], L[3]};
                b = relight_leaf_box(reinterpret_cast<const int32_t *>(L)[5], a, L[4]);
                pw = R.aw[li];
            } else {
                const double *cl = R.box + (size_t)link * 7, *cr = cl + 7;
                const RelightBox bl = {{cl[0], cl[1], cl[2]}, {cl[3], cl[4], cl[5]}}, br = {{cr[0], cr[1], cr[2]}, {cr[3], cr[4], cr[5]}};
                b = relight_union(bl, br);
                pw = cl[6] + cr[6];
            }
            double *S = R.box + (size_t)slot * 7;
            for (int a = 0; a < 3; a++) { S[a] = b.lo[a]; S[3 + a] = b.hi[a]; }
            S[6] = pw;
            float f[5];
            relight_node(b, pw, f);
            for (int a = 0; a < 5; a++) N[a] = f[a];
        }
        __syncthreads();
    }
}

hipError_t rtmi_relight_launch(hipStream_t stream, const RelightScene &R) {
    if (R.n == 0) return hipSuccess;
    hipLaunchKernelGGL(rtmi_relight_kernel, dim3(1), dim3(RTMI_RELIGHT_BLOCK), 0, stream, R);
    return hipGetLastError();
}
