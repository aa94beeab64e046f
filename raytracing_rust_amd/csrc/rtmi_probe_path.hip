// rtmi_probe_path.hip — translation unit of the path probe (rtmi_probe_path, include/rtmi.h) and its launcher.  Compiled
// with the flags of rtmi_device.hip (-ffp-contract=off: every output is restated bit for bit by the fp32 oracle).
//
// What a path does between a hit and its next ray — camera_sample, the rejection samplers, medium_sample, the transform
// chains, and world_closest + shade_hit themselves (BOUNCE) — is templated on the word source.  The probe instantiates the production functions (rtmi_shade.hpp,
// rtmi_rng.hpp, rtmi_geom.hpp), not restatements of them, over a fourth source that exists only here: RngScript, which
// hands out the words the caller wrote down.  One case per lane, one wavefront per block; the lanes of a wavefront run
// different scripts, so they leave the rejection loops at different trials, as the lanes of a render do.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rtmi.h"
#include "rtmi_math.h"

#include "rtmi_rng.hpp"

// ---- RngScript: RTMI_PROBE_PATH_WORDS words per case, in global memory -------------------------------------------------
// `pos` is the next word of the script, `taken` the words delivered since the kernel began (rng_init rewinds the script,
// not the count).  A draw beyond the script delivers 0x80000000 — rtmi_u01 = 0.5, the samplers' p = 0, which both
// accept — and raises `exhausted`: no rejection loop outlives the script by more than one trial, whatever it holds.
struct RngScript {
    const uint32_t *w;
    uint32_t pos, taken, exhausted;
};
__device__ __forceinline__ void rng_attach(RngScript &, uint32_t *) {}
__device__ __forceinline__ void rng_init(RngScript &g, uint32_t, uint32_t) { g.pos = 0u; }
__device__ __forceinline__ uint32_t rng_word(RngScript &g) {
    uint32_t w = 0x80000000u;
    if (g.pos < (uint32_t)RTMI_PROBE_PATH_WORDS) w = g.w[g.pos];
    else g.exhausted = 1u;
    g.pos++;
    g.taken++;
    return w;
}
template <bool LOCAL = false>
__device__ __forceinline__ float rng_uniform(RngScript &g, uint32_t, uint32_t) { return rtmi_u01(rng_word(g)); }
__device__ __forceinline__ void rng_take3(RngScript &g, uint32_t, uint32_t, uint32_t &w0, uint32_t &w1, uint32_t &w2) {
    w0 = rng_word(g); w1 = rng_word(g); w2 = rng_word(g);
}
__device__ __forceinline__ void rng_take2(RngScript &g, uint32_t, uint32_t, uint32_t &w0, uint32_t &w1) {
    w0 = rng_word(g); w1 = rng_word(g);
}

#include "rtmi_query.hpp"
#include "rtmi_probe_path_launch.hpp"

__global__ void __launch_bounds__(64) rtmi_path_probe_kernel(int op, PathProbe B) {
    // BOUNCE: the traversal stack of the per-lane query kernel (rtmi_query.hip, reference-topology walk: one plane), which
    // is idle and serves as shade_hit's scratch once the trace has returned, as in rtmi_path_shade.inc
    __shared__ uint32_t lds_stack[RTMI_MAX_BVH_DEPTH][64];
    const uint32_t i = min(blockIdx.x * 64u + threadIdx.x, B.n - 1u); // tail lanes repeat the last case, write nothing
    const bool live = blockIdx.x * 64u + threadIdx.x < B.n;
    const float *a = B.in + RTMI_PROBE_PATH_IN * (size_t)i;
    float res[RTMI_PROBE_PATH_OUT];
    for (int k = 0; k < RTMI_PROBE_PATH_OUT; k++) res[k] = 0.0f;
    RngScript g;
    g.w = B.words + RTMI_PROBE_PATH_WORDS * (size_t)i;
    g.pos = 0u; g.taken = 0u; g.exhausted = 0u;
    rng_attach(g, nullptr);
    const uint32_t k0 = 0u, k1 = 0u; // the script has no key
    if (op == RTMI_PROBE_PATH_CAMERA) {
        const DevCamera cam = B.cams[__float_as_uint(a[0])];
        DevParams P{};
        P.nx = __float_as_uint(a[1]); P.ny = __float_as_uint(a[2]);
        const uint32_t px = __float_as_uint(a[3]), j = __float_as_uint(a[4]);
        Path pa;
        camera_sample(cam, P, g, k0, k1, 0u, j * P.nx + px, px, j, pa);
        res[0] = pa.ro.x; res[1] = pa.ro.y; res[2] = pa.ro.z;
        res[3] = pa.rd.x; res[4] = pa.rd.y; res[5] = pa.rd.z;
        res[6] = pa.rtime;
    } else if (op == RTMI_PROBE_PATH_SPHERE) {
        const F3 p = random_in_unit_sphere(g, k0, k1);
        res[0] = p.x; res[1] = p.y; res[2] = p.z;
    } else if (op == RTMI_PROBE_PATH_DISK) {
        const F3 p = random_in_unit_disk(g, k0, k1);
        res[0] = p.x; res[1] = p.y; res[2] = p.z;
    } else if (op == RTMI_PROBE_PATH_MEDIUM_SAMPLE) {
        float t_out = 0.0f;
        const bool taken = medium_sample(a[0], a[1], a[2], a[3], a[4], a[5], g, k0, k1, t_out);
        res[0] = taken ? 1.0f : 0.0f;
        res[1] = taken ? t_out : 0.0f;
    } else if (op == RTMI_PROBE_PATH_XFORM_ROUNDTRIP) {
        F3 o = f3(a[0], a[1], a[2]), d = f3(a[3], a[4], a[5]);
        const float t = a[6];
        const int first = __float_as_int(a[7]), count = __float_as_int(a[8]);
        F3 nn = f3(a[9], a[10], a[11]);
        xform_ray(B.xforms, first, count, o, d);
        F3 p = o + d * t; // HitRecord::p = ray.point_at_parameter(t) in the object's frame (ray.rs:23-25)
        xform_hit(B.xforms, first, count, p, nn);
        res[0] = p.x; res[1] = p.y; res[2] = p.z; res[3] = nn.x; res[4] = nn.y; res[5] = nn.z;
    } else if (op == RTMI_PROBE_PATH_BOUNCE) { // one turn of the per-lane path loop: trace, then shade (all 64 lanes call)
        QueryRay q;
        q.ro = f3(a[0], a[1], a[2]); q.rd = f3(a[3], a[4], a[5]); q.rtime = a[6];
        const float t_min = a[7], t_max = a[8] < RTMI_FLT_MAX ? a[8] : RTMI_FLT_MAX;
        float closest;
        int best_item, best_pf;
        bool best_medium;
        world_closest<false>(B.sc, q, t_min, t_max, &lds_stack[0][threadIdx.x & 63], g, k0, k1, closest, best_item, best_pf, best_medium);
        Path pa;
        pa.ro = q.ro; pa.rd = q.rd; pa.rtime = q.rtime;
        pa.T = f3(1, 1, 1); pa.L = f3(0, 0, 0);
        pa.depth = __float_as_uint(a[9]);
        const bool hit = best_item >= 0;
        const bool scattered = shade_hit<RngScript>(B.sc, B.max_depth, B.ext, g, k0, k1, hit, closest, best_item, best_pf, best_medium, pa,
                                                    reinterpret_cast<float *>(&lds_stack[0][0]));
        res[0] = hit ? closest : __builtin_inff();
        res[1] = __int_as_float(best_item);
        res[2] = __int_as_float(hit && !best_medium ? (best_pf >> 3) : -1);
        res[3] = hit && best_medium ? 1.0f : 0.0f;
        res[4] = scattered ? 1.0f : 0.0f;
        res[5] = pa.ro.x; res[6] = pa.ro.y; res[7] = pa.ro.z; res[8] = pa.rd.x; res[9] = pa.rd.y; res[10] = pa.rd.z;
        res[11] = pa.T.x; res[12] = pa.T.y; res[13] = pa.T.z; res[14] = pa.L.x; res[15] = pa.L.y; res[16] = pa.L.z;
    }
    res[RTMI_PROBE_PATH_OUT - 2] = __uint_as_float(g.taken);
    res[RTMI_PROBE_PATH_OUT - 1] = __uint_as_float(g.exhausted);
    if (live)
        for (int k = 0; k < RTMI_PROBE_PATH_OUT; k++) B.out[RTMI_PROBE_PATH_OUT * (size_t)i + k] = res[k];
}

// ---- word delivery of the Philox sources under divergence (rtmi_probe_stream, include/rtmi.h) ---------------------------
// Every lane follows its own script, so at each step the wavefront splits by draw size: rng_need's ballot then sees only
// the lanes of one branch, lanes sit at different positions of their blocks, some have just been re-initialised and some
// are idle — what a render's wavefront looks like after a few bounces.  A fixed count of steps; no loop depends on a word.
template <typename RngT>
__device__ void stream_probe_run(uint32_t *ring, uint32_t k0, uint32_t k1, const uint8_t *script, uint32_t steps, uint32_t *out, uint32_t i) {
    RngT g;
    rng_attach(g, ring);
    if constexpr (std::is_same<RngT, RngNee>::value) rng_set_stream(g, 3u);
    uint32_t sample = 0u;
    rng_init(g, sample, i);
    for (uint32_t s = 0; s < steps; s++) {
        const uint32_t op = script[(size_t)i * steps + s];
        uint32_t w0 = 0u, w1 = 0u, w2 = 0u;
        if (op == 1u) w0 = (uint32_t)(rng_uniform(g, k0, k1) * 16777216.0f) << 8; // k 2^-24 back to k: exact
        else if (op == 2u) rng_take2(g, k0, k1, w0, w1);
        else if (op == 3u) rng_take3(g, k0, k1, w0, w1, w2);
        else if (op == 4u) { sample++; rng_init(g, sample, i); }
        uint32_t *o = out + ((size_t)i * steps + s) * 3;
        o[0] = w0; o[1] = w1; o[2] = w2;
    }
}
__global__ void __launch_bounds__(64) rtmi_stream_probe_kernel(int kind, uint32_t k0, uint32_t k1, const uint8_t *script, uint32_t steps,
                                                                uint32_t *out, uint32_t n) {
    __shared__ uint32_t ring[RTMI_RNG_RING_WORDS];
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    if (kind == 0) stream_probe_run<RngRing>(ring, k0, k1, script, steps, out, i);
    else if (kind == 1) stream_probe_run<RngReg>(ring, k0, k1, script, steps, out, i);
    else stream_probe_run<RngNee>(ring, k0, k1, script, steps, out, i);
}

hipError_t rtmi_probe_stream_launch(int kind, uint32_t k0, uint32_t k1, const uint8_t *script, uint32_t steps, uint32_t *out, uint32_t n) {
    hipLaunchKernelGGL(rtmi_stream_probe_kernel, dim3((n + 63u) / 64u), dim3(64), 0, 0, kind, k0, k1, script, steps, out, n);
    return hipGetLastError();
}

hipError_t rtmi_probe_path_launch(int op, const PathProbe &B) {
    hipLaunchKernelGGL(rtmi_path_probe_kernel, dim3((B.n + 63u) / 64u), dim3(64), 0, 0, op, B);
    return hipGetLastError();
}
