// rtmi_update_dev.hip — the two kernels of a scene update (include/rtmi_update.h) and their launchers.
// Compiled with the flags of rtmi_device.hip (-ffp-contract=off: the refit is restated bit for bit on the host).
//
// Scatter: one thread per primitive of the range writes the new planes into every copy the handle keeps of them.
// Refit: one workgroup per refittable BVH item that the range touches.  The rules are those of rtmi_refit.hpp, the same
// functions the host compiles.  Items are independent, so no byte crosses a workgroup inside the launch and none of the
// agent-scope hand-off machinery is needed; within the workgroup the levels of a tree are separated by __syncthreads(),
// and what one wave stored before the barrier another reads after it with plain vector loads (one CU, one L1).  Every load
// of such bytes has a per-thread address, so none goes through the scalar cache; the one value every thread needs — the
// item's pad — travels through LDS.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rtmi.h"

#include "rtmi_refit.hpp"
#include "rtmi_update_launch.hpp"

#define RTMI_UPDATE_BLOCK 256

__global__ void __launch_bounds__(RTMI_UPDATE_BLOCK) rtmi_update_scatter_kernel(UpdateScene U, uint32_t first, uint32_t count, const float *a,
                                                                                const float *b) {
    const uint32_t i = blockIdx.x * RTMI_UPDATE_BLOCK + threadIdx.x;
    if (i >= count) return;
    const uint32_t p = first + i;
    const float4 A = make_float4(a[(size_t)i * 4], a[(size_t)i * 4 + 1], a[(size_t)i * 4 + 2], a[(size_t)i * 4 + 3]);
    U.prim_a[p] = A;
    U.leaf_rec[(size_t)p * 5] = A;
    U.shade_prim[(size_t)p * 4] = A;
    if (b) {
        const float4 B = make_float4(b[(size_t)i * 4], b[(size_t)i * 4 + 1], b[(size_t)i * 4 + 2], b[(size_t)i * 4 + 3]);
        U.prim_b[p] = B;
        U.leaf_rec[(size_t)p * 5 + 1] = B;
    }
    const int32_t mi = U.medium_item[p];
    if (mi >= 0) { // RTMI_ITEMFLAG_DEV_MEDIUM_SPHERE: the item carries the sphere in root_min and root_max[0]
        float *it = reinterpret_cast<float *>(U.items + (size_t)mi * 96 + offsetof(rtmi_item, root_min));
        it[0] = A.x; it[1] = A.y; it[2] = A.z; it[3] = A.w;
    }
}

__device__ __forceinline__ RefitBox dev_leaf_box(const UpdateScene &U, int type, uint32_t p) {
    const float4 A = U.prim_a[p], B = U.prim_b[p];
    const float a[4] = {A.x, A.y, A.z, A.w}, b[4] = {B.x, B.y, B.z, B.w};
    return refit_leaf_box(type, a, b);
}
__device__ __forceinline__ RefitBox dev_leaf_extent(const UpdateScene &U, int type, uint32_t p) {
    const float4 A = U.prim_a[p], B = U.prim_b[p];
    const float a[4] = {A.x, A.y, A.z, A.w}, b[4] = {B.x, B.y, B.z, B.w};
    return refit_leaf_extent(type, a, b);
}
__device__ __forceinline__ RefitBox dev_node_box(const UpdateScene &U, uint32_t n) {
    const float4 lo = U.scratch[(size_t)n * 2], hi = U.scratch[(size_t)n * 2 + 1];
    return RefitBox{{lo.x, lo.y, lo.z}, {hi.x, hi.y, hi.z}};
}

__global__ void __launch_bounds__(RTMI_UPDATE_BLOCK) rtmi_update_refit_kernel(UpdateScene U, uint32_t first, uint32_t count) {
    __shared__ float s_pad;
    const RefitJob J = U.jobs[blockIdx.x];
    if (first >= J.prim_hi || first + count <= J.prim_lo) return; // (the whole workgroup)
    const uint32_t tid = threadIdx.x;
    // ---- the reference tree, deepest level first: the box of every node; the thread that holds the root also derives the
    // item's root box, scale and pad
    for (uint32_t k = 0; k < J.n_lvl; k++) {
        const uint32_t lb = U.words[J.lvl + k], le = U.words[J.lvl + k + 1];
        for (uint32_t q = lb + tid; q < le; q += RTMI_UPDATE_BLOCK) {
            const uint32_t n = U.words[q];
            const int32_t *ch = reinterpret_cast<const int32_t *>(U.nodes + (size_t)n * 4 + 3);
            const int32_t l = ch[0], r = ch[1];
            const RefitBox L = refit_is_leaf(l) ? dev_leaf_box(U, refit_leaf_type(l), refit_leaf_prim(l)) : dev_node_box(U, (uint32_t)l);
            const RefitBox R = refit_is_leaf(r) ? dev_leaf_box(U, refit_leaf_type(r), refit_leaf_prim(r)) : dev_node_box(U, (uint32_t)r);
            const RefitBox u = refit_union(L, R);
            U.scratch[(size_t)n * 2] = make_float4(u.mn[0], u.mn[1], u.mn[2], 0.0f);
            U.scratch[(size_t)n * 2 + 1] = make_float4(u.mx[0], u.mx[1], u.mx[2], 0.0f);
            if (n == J.root) {
                const float scale = refit_scale(u);
                float *it = reinterpret_cast<float *>(U.items + (size_t)J.item * 96 + offsetof(rtmi_item, root_min));
                for (int c = 0; c < 3; c++) { it[c] = u.mn[c]; it[3 + c] = u.mx[c]; }
                it[6] = scale;
                s_pad = refit_pad(scale);
            }
        }
        __syncthreads();
    }
    const float pad = s_pad;
    // ---- the stored boxes of every node, and the gates of the leaves it holds
    {
        const uint32_t lb = U.words[J.lvl], le = U.words[J.lvl + J.n_lvl];
        for (uint32_t q = lb + tid; q < le; q += RTMI_UPDATE_BLOCK) {
            const uint32_t n = U.words[q];
            float *N = reinterpret_cast<float *>(U.nodes + (size_t)n * 4);
            const int32_t ch[2] = {reinterpret_cast<const int32_t *>(N)[12], reinterpret_cast<const int32_t *>(N)[13]};
            const RefitBox own = dev_node_box(U, n);
            for (int c = 0; c < 2; c++) {
                RefitBox bx;
                if (refit_is_leaf(ch[c])) {
                    const uint32_t p = refit_leaf_prim(ch[c]);
                    bx = refit_widen(dev_leaf_extent(U, refit_leaf_type(ch[c]), p), pad);
                    if (U.gate) {
                        float *g = reinterpret_cast<float *>(U.gate + (size_t)p * 2), *lr = reinterpret_cast<float *>(U.leaf_rec + (size_t)p * 5 + 3);
                        for (int k = 0; k < 3; k++) { g[k] = own.mn[k]; g[4 + k] = own.mx[k]; lr[k] = own.mn[k]; lr[4 + k] = own.mx[k]; }
                    }
                } else {
                    bx = dev_node_box(U, (uint32_t)ch[c]);
                }
                for (int k = 0; k < 3; k++) { N[c * 6 + k] = bx.mn[k]; N[c * 6 + 3 + k] = bx.mx[k]; }
            }
        }
    }
    __syncthreads();
    // ---- the alternative tree, deepest level first.  Children are pool-encoded (rtmi_bvh_coop.hpp): 0xffffffff an empty
    // slot, bit 25 a leaf (type in bits 22..24, primitive below), else a node
    for (uint32_t k = 0; k < J.alt_n_lvl; k++) {
        const uint32_t lb = U.words[J.alt_lvl + k], le = U.words[J.alt_lvl + k + 1];
        for (uint32_t q = lb + tid; q < le; q += RTMI_UPDATE_BLOCK) {
            const uint32_t n = U.words[q];
            float *N = reinterpret_cast<float *>(U.nodes4 + (size_t)n * 8);
            for (int c = 0; c < 4; c++) {
                const uint32_t ref = reinterpret_cast<const uint32_t *>(N)[24 + c];
                if (ref == 0xffffffffu) continue;
                RefitBox bx;
                if (ref & (1u << 25)) {
                    bx = refit_widen(dev_leaf_extent(U, (int)((ref >> 22) & 7u), ref & 0x003fffffu), pad);
                } else {
                    const float *C = reinterpret_cast<const float *>(U.nodes4 + (size_t)ref * 8);
                    bool any = false;
                    for (int s = 0; s < 4; s++) {
                        if (reinterpret_cast<const uint32_t *>(C)[24 + s] == 0xffffffffu) continue;
                        const RefitBox sb = {{C[s], C[4 + s], C[8 + s]}, {C[12 + s], C[16 + s], C[20 + s]}};
                        bx = any ? refit_union(bx, sb) : sb;
                        any = true;
                    }
                    if (!any) continue;
                }
                N[c] = bx.mn[0]; N[4 + c] = bx.mn[1]; N[8 + c] = bx.mn[2];
                N[12 + c] = bx.mx[0]; N[16 + c] = bx.mx[1]; N[20 + c] = bx.mx[2];
            }
        }
        __syncthreads();
    }
}

hipError_t rtmi_update_scatter_launch(hipStream_t stream, const UpdateScene &U, uint32_t first, uint32_t count, const float *d_a,
                                      const float *d_b) {
    hipLaunchKernelGGL(rtmi_update_scatter_kernel, dim3((count + RTMI_UPDATE_BLOCK - 1) / RTMI_UPDATE_BLOCK), dim3(RTMI_UPDATE_BLOCK), 0, stream,
                       U, first, count, d_a, d_b);
    return hipGetLastError();
}

hipError_t rtmi_update_refit_launch(hipStream_t stream, const UpdateScene &U, uint32_t first, uint32_t count) {
    if (U.n_jobs == 0) return hipSuccess;
    hipLaunchKernelGGL(rtmi_update_refit_kernel, dim3(U.n_jobs), dim3(RTMI_UPDATE_BLOCK), 0, stream, U, first, count);
    return hipGetLastError();
}
