// rtmi_query.hip — translation unit of the ray queries (include/rtmi_query.h): closest hit and occlusion for batches of
// caller-supplied rays, and their launcher.  Compiled with the flags of rtmi_device.hip (-ffp-contract=off: the hit
// records are restated bit for bit by the fp32 oracle).
//
// One lane per ray; a wavefront takes 64 consecutive rays.  A ray record is two aligned 16-B loads per lane, a hit record
// three 16-B stores; the lanes of the n % 64 tail are masked.  Batches are dealt by grid stride over a grid of one
// wavefront per batch (capped): a wavefront lives for one batch, so the hardware dispatcher hands the next batch to
// whichever slot frees first, which is what an atomic batch counter under persistent blocks would buy — without a
// counter in device memory that every call would have to zero on the caller's stream, and that two calls on two streams
// would share.  Traversal stacks: the per-lane LDS columns of the per-lane render kernel (rtmi_kernel_perlane.inc),
// 12 KB per wavefront with the entry distances of the pruned walk, 6 KB without.
//
// trace: world_closest (rtmi_query.hpp), the world scan of rtmi_path_scan.inc, the text the per-lane render kernel traces
// its path rays with, under the ray's own (t_min, t_max), time and Philox key.  occluded: world_any (rtmi_query.hpp).
// Instantiated for FAST x {trace, occluded}; no profiling, signature or cooperative variant.  In the FAST kernels a ray
// with an infinite component of 1 / d takes the reference-topology traversal (query_ray_pruned, rtmi_query.hpp).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rtmi.h"
#include "rtmi_math.h"

#include "rtmi_query.hpp"
#include "rtmi_query_launch.hpp"

static_assert(sizeof(rtmi_ray) == 32 && sizeof(rtmi_hit) == 48 && sizeof(rtmi_query_params) == 24, "rtmi_query.h record sizes");

template <bool FAST, bool ANY>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void rtmi_query_kernel(DevScene sc, QueryBatch B) {
    // per wave: [0] node refs, [1] entry distances (FAST only); entry-major so lanes never bank-conflict
    __shared__ uint32_t lds_stack[WAVES_PER_BLOCK][FAST ? 2 : 1][RTMI_MAX_BVH_DEPTH][64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    uint32_t *stack = &lds_stack[wave][0][0][lane];
    const uint32_t nbatch = (uint32_t)(((unsigned long long)B.n + 63ull) >> 6);
    for (uint32_t b = blockIdx.x * WAVES_PER_BLOCK + wave; b < nbatch; b += gridDim.x * WAVES_PER_BLOCK) {
        const uint32_t i = b * 64u + (uint32_t)lane;
        if (i >= B.n) continue; // the tail of the last batch
        const float4 r0 = B.rays[2 * (size_t)i], r1 = B.rays[2 * (size_t)i + 1];
        QueryRay pa;
        pa.ro = f3(r0.x, r0.y, r0.z);
        pa.rd = f3(r1.x, r1.y, r1.z);
        pa.rtime = B.time ? B.time[i] : 0.0f;
        const float t_min = r0.w, t_max = r1.w < RTMI_FLT_MAX ? r1.w : RTMI_FLT_MAX; // +inf, >= FLT_MAX: the render's
        // the ray's own stream: key (seed + first_ray + i) mod 2^64, counter (0, 0, 0, 0), stream id 0
        const unsigned long long key = (((unsigned long long)B.key1 << 32) | B.key0) + i;
        const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
        RngReg g;
        rng_init(g, 0, 0);
        // an infinite component of 1 / d (d_k = +-0 or denormal): the reference-topology traversal whatever the flag says
        const bool pruned = FAST && query_ray_pruned(pa);
        if constexpr (ANY) {
            const bool any = pruned ? world_any<true>(sc, pa, t_min, t_max, stack, g, k0, k1)
                                    : world_any<false>(sc, pa, t_min, t_max, stack, g, k0, k1);
            B.occluded[i] = any ? (uint8_t)1 : (uint8_t)0;
        } else {
            float closest;
            int best_item, best_pf;
            bool best_medium;
            if (pruned) world_closest<true>(sc, pa, t_min, t_max, stack, g, k0, k1, closest, best_item, best_pf, best_medium);
            else world_closest<false>(sc, pa, t_min, t_max, stack, g, k0, k1, closest, best_item, best_pf, best_medium);
            F3 hp = f3(0, 0, 0), hn = f3(0, 0, 0);
            float ht = __builtin_inff(), hu = 0.0f, hv = 0.0f;
            int prim = -1, material = -1;
            if (best_item >= 0) {
                ht = closest;
                query_record(sc, B.prim_gaps, B.item_gaps, pa, closest, best_item, best_pf, best_medium, hp, hn, hu, hv, prim, material);
            }
            float4 *out = B.hits + 3 * (size_t)i;
            out[0] = make_float4(ht, hu, hv, hp.x);
            out[1] = make_float4(hp.y, hp.z, hn.x, hn.y);
            out[2] = make_float4(hn.z, __int_as_float(best_item), __int_as_float(prim), __int_as_float(material));
        }
    }
}

hipError_t rtmi_query_launch(bool any, bool fast, hipStream_t stream, const DevScene &sc, const QueryBatch &B) {
    const uint32_t nbatch = (uint32_t)(((unsigned long long)B.n + 63ull) >> 6);
    const uint32_t blocks = (nbatch + WAVES_PER_BLOCK - 1u) / WAVES_PER_BLOCK;
    const dim3 grid(blocks < (1u << 20) ? blocks : (1u << 20)), block(64 * WAVES_PER_BLOCK);
    if (any && fast) hipLaunchKernelGGL((rtmi_query_kernel<true, true>), grid, block, 0, stream, sc, B);
    else if (any) hipLaunchKernelGGL((rtmi_query_kernel<false, true>), grid, block, 0, stream, sc, B);
    else if (fast) hipLaunchKernelGGL((rtmi_query_kernel<true, false>), grid, block, 0, stream, sc, B);
    else hipLaunchKernelGGL((rtmi_query_kernel<false, false>), grid, block, 0, stream, sc, B);
    return hipGetLastError();
}
