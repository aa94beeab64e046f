// rtmi_batch_coop.hip — translation unit of RTMI_FLAG_BATCH_COOP (include/rtmi_batch_coop.h): the radiance queries, the
// hemisphere gathers and the sparse renders on the wave-cooperative kernel, and their launchers.  Compiled with the flags
// of rtmi_device.hip (-ffp-contract=off).
//
// Each kernel is the body of rtmi_render_coop (rtmi_kernel_coop.inc) through its two seams: the take step is
// rtmi_batch_coop_take.inc (batch_take plus the mode's ray start, the statements of the per-lane kernel of the same mode),
// and for the radiance queries the scan's interval is the lane's own on a ray's first segment.  The item scan, the fragments
// rtmi_path_lane.inc, rtmi_path_traced.inc and rtmi_path_shade.inc and the overflow report are the body's, so there is no
// second copy of any of them.  Per-lane program order is the per-lane batch kernels', so every sample has their bits.
// Instantiated for the pool form x NEE x ENV (all four estimators: the cooperative render of rtmi_device.hip knows nothing
// of batches, so the plain one is built here too), the gathers also x SPHERE; level 0 only (INSTL = 0: scenes with
// instanced primitives or media inside transforms stay on the per-lane kernels), no profiling, no signatures.  FAST is
// implied: the cooperative traversal is the fast-cull one.  rtmi_batch_coop_wps waves per SIMD
// (rtmi_batch_coop_launch.hpp): the grid the host launches.
//
// Philox.  The lean pool form (scenes without a BVH item, a non-NEE estimator) keeps the body's RngRing, the word ring in
// LDS, which is what that form is faster for (rtmi_rng.hpp); the radiance queries' stream_skip gets a seek of the ring's
// own below.  Same stream, same words, same order as rng_seek of rtmi_radiance.hip gives RngReg.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "rtmi.h"
#include "rtmi_math.h"
#include "rtmi_gather.h"

#define RTMI_LEAN_TU 1 /* the plain kernels are defined in rtmi_device.hip */
#include "rtmi_kernels.hpp"
#include "rtmi_light_launch.hpp"
#include "rtmi_batch.hpp"
#include "rtmi_radiance_launch.hpp"
#include "rtmi_gather_launch.hpp"
#include "rtmi_sparse_launch.hpp"
#include "rtmi_batch_coop_launch.hpp"

#define RTMI_BATCH_COOP_RADIANCE 0
#define RTMI_BATCH_COOP_GATHER 1
#define RTMI_BATCH_COOP_SPARSE 2

// the stream of rng_init(g, sample, pixel), read from word 4 * block + pos on (pos in 0..3; wave-uniform): rng_seek of
// rtmi_radiance.hip for the register forms ...
template <typename RngT>
__device__ __forceinline__ void batch_rng_seek(RngT &g, uint32_t k0, uint32_t k1, uint32_t block, uint32_t pos) {
    g.block = block;
    if (pos != 0u) { // inside a block: its words are the lane's current ones
        uint32_t stream = 0u;
        if constexpr (std::is_same<RngT, RngNee>::value) stream = g.stream;
        philox(block, g.sample, g.pixel, stream, k0, k1, g.b0, g.b1, g.b2, g.b3);
        g.block = block + 1u;
        g.pos = pos;
    }
}
// ... and for the ring: rd and wr count words from the start of the stream, and a block's words sit in the half of the
// ring its number selects, so a seek into a block generates that block where rng_need would have put it
__device__ __forceinline__ void batch_rng_seek(RngRing &g, uint32_t k0, uint32_t k1, uint32_t block, uint32_t pos) {
    g.wr = 4u * block;
    g.rd = g.wr + pos;
    if (pos != 0u) {
        uint32_t o0, o1, o2, o3;
        philox(block, g.sample, g.pixel, 0u, k0, k1, o0, o1, o2, o3);
        uint32_t *w = g.ring + ((g.wr & 4u) << 6);
        w[0] = o0; w[64] = o1; w[128] = o2; w[192] = o3;
        g.wr += 4u;
    }
}

// gather_direction of rtmi_gather.hip: direction s of point i (absolute indices) in the batch's mode; n: the point's
// normal (COSINE).  The header's inline functions, so the same bits.
template <bool SPHERE>
__device__ __forceinline__ void batch_gather_direction(uint32_t k0, uint32_t k1, uint32_t sample, uint32_t point, const float n[3],
                                                       float d[3]) {
    uint32_t w0, w1, w2, w3;
    philox(0u, sample, point, RTMI_GATHER_STREAM, k0, k1, w0, w1, w2, w3);
    if constexpr (SPHERE) rtmi_gather_sphere(rtmi_u01(w0), rtmi_u01(w1), d);
    else rtmi_gather_cosine(rtmi_u01(w0), rtmi_u01(w1), n, d);
}

#define RTMI_COOP_TAKE "rtmi_batch_coop_take.inc"

// ---- radiance queries: the first segment under the caller's own interval -----------------------------------------------------
template <bool EXT, bool NEE, bool ENV>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, rtmi_batch_coop_wps(NEE, ENV)) void rtmi_radiance_coop_kernel(
    DevScene sc, DevParams P, RadianceBatch B, DevLights nl, DevEnv ev) {
    constexpr bool PROF = false, SIG = false, ONE_TREE = false;
    constexpr int INSTL = 0;
    BatchWork bw;
    bw.next = 0u; bw.end = 0u;
    bool first = false;                               // the lane's ray is the caller's: its own interval
    float ray_t_min = 0.0f, ray_t_max = RTMI_FLT_MAX; // ... which is this
#define RTMI_BATCH_COOP_MODE RTMI_BATCH_COOP_RADIANCE
#define RTMI_COOP_T_MIN scan_t_min
#define RTMI_COOP_T_MAX scan_t_max
#include "rtmi_kernel_coop.inc"
#undef RTMI_COOP_T_MIN
#undef RTMI_COOP_T_MAX
#undef RTMI_BATCH_COOP_MODE
}

// ---- hemisphere gathers: (P.t_min, FLT_MAX) throughout, the body's default interval --------------------------------------------
template <bool EXT, bool NEE, bool ENV, bool SPHERE>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, rtmi_batch_coop_wps(NEE, ENV)) void rtmi_gather_coop_kernel(
    DevScene sc, DevParams P, GatherBatch B, DevLights nl, DevEnv ev) {
    constexpr bool PROF = false, SIG = false, ONE_TREE = false;
    constexpr int INSTL = 0;
    BatchWork bw;
    bw.next = 0u; bw.end = 0u;
#define RTMI_BATCH_COOP_MODE RTMI_BATCH_COOP_GATHER
#include "rtmi_kernel_coop.inc"
#undef RTMI_BATCH_COOP_MODE
}

// ---- sparse renders: the entries are min(count[0], n), read here as rtmi_sparse_kernel reads them ----------------------------
template <bool EXT, bool NEE, bool ENV>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, rtmi_batch_coop_wps(NEE, ENV)) void rtmi_sparse_coop_kernel(
    DevScene sc, DevCamera cam, DevParams P, SparseBatch B, DevLights nl, DevEnv ev) {
    constexpr bool PROF = false, SIG = false, ONE_TREE = false;
    constexpr int INSTL = 0;
    BatchWork bw;
    bw.next = 0u; bw.end = 0u;
    uint32_t entries = B.n; // wave-uniform
    if (B.count) {
        const uint32_t c = B.count[0];
        entries = c < B.n ? c : B.n;
    }
    const uint32_t total = rfl(entries * B.ns);                // < 2^31
    const uint32_t nchunks = (total + B.chunk - 1u) / B.chunk; // 0: the list is empty, every wavefront leaves at once
#define RTMI_BATCH_COOP_MODE RTMI_BATCH_COOP_SPARSE
#include "rtmi_kernel_coop.inc"
#undef RTMI_BATCH_COOP_MODE
}
#undef RTMI_COOP_TAKE

__global__ void rtmi_batch_coop_end_kernel(unsigned int *status) {
    status[2] += status[0];
    status[0] = 0u;
}

hipError_t rtmi_batch_coop_launch_radiance(bool ext, bool nee, bool env, uint32_t blocks, size_t lds, hipStream_t stream,
                                           const DevScene &sc, const DevParams &P, const RadianceBatch &B, const DevLights &L,
                                           const DevEnv &E) {
    const dim3 grid(blocks), block(64 * WAVES_PER_BLOCK);
    return rtmi_with_bools([&](auto EXT, auto NEE, auto ENV) {
        return rtmi_launch_lds(&rtmi_radiance_coop_kernel<EXT(), NEE(), ENV()>, grid, block, lds, stream, sc, P, B, L, E);
    }, ext, nee, env);
}

hipError_t rtmi_batch_coop_launch_gather(bool ext, bool nee, bool env, uint32_t mode, uint32_t blocks, size_t lds, hipStream_t stream,
                                         const DevScene &sc, const DevParams &P, const GatherBatch &B, const DevLights &L,
                                         const DevEnv &E) {
    const dim3 grid(blocks), block(64 * WAVES_PER_BLOCK);
    return rtmi_with_bools([&](auto EXT, auto NEE, auto ENV, auto SPHERE) {
        return rtmi_launch_lds(&rtmi_gather_coop_kernel<EXT(), NEE(), ENV(), SPHERE()>, grid, block, lds, stream, sc, P, B, L, E);
    }, ext, nee, env, mode == RTMI_GATHER_SPHERE);
}

hipError_t rtmi_batch_coop_launch_sparse(bool ext, bool nee, bool env, uint32_t blocks, size_t lds, hipStream_t stream,
                                         const DevScene &sc, const DevCamera &cam, const DevParams &P, const SparseBatch &B,
                                         const DevLights &L, const DevEnv &E) {
    const dim3 grid(blocks), block(64 * WAVES_PER_BLOCK);
    return rtmi_with_bools([&](auto EXT, auto NEE, auto ENV) {
        return rtmi_launch_lds(&rtmi_sparse_coop_kernel<EXT(), NEE(), ENV()>, grid, block, lds, stream, sc, cam, P, B, L, E);
    }, ext, nee, env);
}

hipError_t rtmi_batch_coop_launch_end(hipStream_t stream, unsigned int *status) {
    hipLaunchKernelGGL(rtmi_batch_coop_end_kernel, dim3(1), dim3(1), 0, stream, status);
    return hipGetLastError();
}
