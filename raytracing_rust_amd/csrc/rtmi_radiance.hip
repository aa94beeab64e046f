// rtmi_radiance.hip — translation unit of the radiance queries (include/rtmi_radiance.h): path-traced radiance along
// batches of caller-supplied rays, the resolve of their samples, and the launchers.  Compiled with the flags of
// rtmi_device.hip (-ffp-contract=off: the samples are the render's, restated bit for bit by the fp32 oracle).
//
// The path kernel is the per-lane two-phase kernel (rtmi_kernel_perlane.inc) with another take step: the fragments
// rtmi_path_lane.inc, rtmi_path_scan.inc, rtmi_path_traced.inc and rtmi_path_shade.inc are included as they are, so a path
// is traced, shaded and ended by the text the render kernels run; rtmi_path_take.inc, the one camera-specific step, is
// replaced by the batch modes' take (batch_take, rtmi_batch.hpp, which describes the items and the two-level refill) and
// the start of a caller's ray.  Instantiated for FAST x NEE x ENV; no profiling, signature, features, roulette or
// cooperative variant.
//
// Items.  Item k = i * spp + s (sample fastest) is sample s of ray i and slot k of the per-sample buffer.  The chunk
// counter is a word of the handle.  The resolve's sample loop is rtmi_batch_welford.inc.
// First segment.  A lane flag `first` selects the ray's own (t_min, t_max) for the scan; it is cleared after the lane's
// first scan, before any shadow ray can be pending, and every later scan runs under (P.t_min, FLT_MAX).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "rtmi.h"
#include "rtmi_math.h"

#define RTMI_LEAN_TU 1 /* the plain kernels are defined in rtmi_device.hip */
#include "rtmi_kernels.hpp"
#include "rtmi_light_launch.hpp"
#include "rtmi_batch.hpp"
#include "rtmi_radiance_launch.hpp"

// the stream of rng_init(g, sample, pixel), read from word 4 * block + pos on (pos in 0..3; wave-uniform)
template <typename RngT>
__device__ __forceinline__ void rng_seek(RngT &g, uint32_t k0, uint32_t k1, uint32_t block, uint32_t pos) {
    g.block = block;
    if (pos != 0u) { // inside a block: its words are the lane's current ones
        uint32_t stream = 0u;
        if constexpr (std::is_same<RngT, RngNee>::value) stream = g.stream;
        philox(block, g.sample, g.pixel, stream, k0, k1, g.b0, g.b1, g.b2, g.b3);
        g.block = block + 1u;
        g.pos = pos;
    }
}

template <bool FAST, bool NEE, bool ENV>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void rtmi_radiance_kernel(DevScene sc, DevParams P, RadianceBatch B, DevLights nl,
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
    bool first = false;                                   // the lane's ray is the caller's: its own interval
    float ray_t_min = 0.0f, ray_t_max = RTMI_FLT_MAX;     // ... which is this
    typename std::conditional<NEE, RngNee, RngReg>::type g;
#include "rtmi_path_lane.inc"

    for (;;) {
        // ================= phase A: trace until enough lanes hold a hit =================
        for (;;) {
            if (__ballot(!have_hit && !done) == 0ull) break;
            { // lanes whose path ended take the next (ray, sample) item, or are done when there is none
                const bool want = !have_hit && !done && !alive;
                if (__ballot(want) != 0ull) {
                    if (batch_take(w, queue_empty, want, B.queue, B.chunk, B.total, B.nchunks, oidx)) {
                        const uint32_t i = oidx / B.spp, s = oidx - i * B.spp;
                        const float4 r0 = B.rays[2 * (size_t)i], r1 = B.rays[2 * (size_t)i + 1];
                        pa.ro = f3(r0.x, r0.y, r0.z);
                        pa.rd = f3(r1.x, r1.y, r1.z);
                        pa.rtime = B.time ? B.time[i] : 0.0f;
                        pa.T = f3(1, 1, 1);
                        pa.L = f3(0, 0, 0);
                        pa.depth = 0;
                        ray_t_min = r0.w;
                        ray_t_max = r1.w < RTMI_FLT_MAX ? r1.w : RTMI_FLT_MAX; // +inf, >= FLT_MAX: the render's
                        first = true;
                        rng_init(g, B.first_sample + s, B.first_ray + i);
                        rng_seek(g, k0, k1, B.skip_block, B.skip_pos);
                        if constexpr (NEE) { rng_init(gn, B.first_sample + s, B.first_ray + i); ne.pb = 0.0f; }
                        alive = true;
                    } else if (want) {
                        done = true;
                    }
                }
            }
            const bool need = !have_hit && !done;
            if (need) {
#define RTMI_SCAN_T_MIN (first ? ray_t_min : P.t_min)
#define RTMI_SCAN_T_MAX (first ? ray_t_max : RTMI_FLT_MAX)
#include "rtmi_path_scan.inc"
#undef RTMI_SCAN_T_MIN
#undef RTMI_SCAN_T_MAX
                first = false;
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

// One lane per ray: the f64 sum of its spp samples in sample order and Welford's recurrence (rtmi_batch_welford.inc);
// spp == 1: no estimate, +inf.
__global__ __launch_bounds__(256) void rtmi_radiance_resolve_kernel(const Rad3 *__restrict__ samples, RadianceBatch B) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B.n) return;
    const Rad3 *src = samples + (size_t)i * B.spp;
    double sum[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0}, M2[3] = {0.0, 0.0, 0.0};
    const uint32_t ns = B.spp;
#include "rtmi_batch_welford.inc"
    const double n = (double)B.spp;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        if (B.mean) B.mean[3 * (size_t)i + ch] = (float)(sum[ch] / n);
        if (B.stderr_out) B.stderr_out[3 * (size_t)i + ch] = B.spp > 1u ? (float)sqrt(M2[ch] / (n * (n - 1.0))) : __builtin_inff();
    }
}

hipError_t rtmi_radiance_launch(bool fast, bool nee, bool env, uint32_t blocks, hipStream_t stream, const DevScene &sc,
                                const DevParams &P, const RadianceBatch &B, const DevLights &L, const DevEnv &E) {
    const dim3 grid(blocks), block(64 * WAVES_PER_BLOCK);
    return rtmi_with_bools([&](auto FAST, auto NEE, auto ENV) {
        hipLaunchKernelGGL((rtmi_radiance_kernel<FAST(), NEE(), ENV()>), grid, block, 0, stream, sc, P, B, L, E);
        return hipGetLastError();
    }, fast, nee, env);
}

hipError_t rtmi_radiance_launch_resolve(hipStream_t stream, const Rad3 *samples, const RadianceBatch &B) {
    hipLaunchKernelGGL(rtmi_radiance_resolve_kernel, dim3((B.n + 255u) / 256u), dim3(256), 0, stream, samples, B);
    return hipGetLastError();
}
