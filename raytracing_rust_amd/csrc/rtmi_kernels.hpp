// rtmi_kernels.hpp — render kernels (per-lane two-phase, wave-cooperative, async state machine), resolve, probes.
// Header-only device code, included by every unit that instantiates a kernel (header-only so that every
// kernel instantiation inlines the whole path); arithmetic contract as stated in rtmi_device.hip.
#pragma once
#include "rtmi_bvh_coop.hpp"
#include "rtmi_shade.hpp"

// ----------------------------------------------------------------------------------
// render kernel, two-phase form (RTMI_FLAG_SYNC): the wavefront alternates between
//   phase A  every lane that holds no unshaded hit traces: (next camera sample if its path ended)
//            + world.hit(); a lane whose ray misses immediately starts its next sample and traces
//            again, while lanes that already found a hit wait.  The phase ends when at least
//            `P.shade_threshold` lanes hold a hit (or no lane can produce one any more).
//   phase B  all lanes holding a hit build the hit record and run the material.
// Shading (Perlin turbulence, rejection samplers, Philox refills, ...) is expensive and very
// divergent; batching it until most lanes need it runs it at high lane utilisation, at the
// price of a few partially filled tracing rounds.  Per-lane program order is unchanged, so
// results do not depend on the threshold.
// ----------------------------------------------------------------------------------
template <bool FAST, bool SIG, bool PROF>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void rtmi_render_kernel(DevScene sc, DevCamera cam, DevParams P) {
    constexpr bool TILE_LIST = false, FEATURES = false, NEE = false, ENV = false;
    const DevLights nl{};
    const DevEnv ev{};
    const uint32_t *const tiles = nullptr;
#include "rtmi_kernel_perlane.inc"
}

// ----------------------------------------------------------------------------------
// render kernel, two-phase form with wave-cooperative BVH traversal (default).
// Same schedule as rtmi_render_kernel; the item scan of phase A is executed by ALL lanes (lanes
// without a pending query are workers for the others' BVH traversals).
// ----------------------------------------------------------------------------------
// INSTL: 0 = the instantiations of the common scenes: no transform code in their loops; 1 = scenes with instanced primitives or
// media inside transforms (rtmi.h); 2 = also DEFERRED items, list scans, nested media (children of a BVHNode that are not
// primitives).  Forced on the BASELINE scenes level 2 costs 10-14 % (profiles/r04_experiments/force_inst_ab.log), hence two levels.
// ONE_TREE: the instantiation of the scenes whose every tree is gated and whose every medium is bounded by a static sphere
// (final_scene, random_spheres): one inlined copy of the traversal instead of four (rtmi_kernel_coop.inc).
template <bool SIG, bool PROF, int WPS, bool EXT, int INSTL, bool ONE_TREE = false>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, WPS) void rtmi_render_coop(DevScene sc, DevCamera cam, DevParams P) {
    constexpr bool TILE_LIST = false, NEE = false, ENV = false;
    const DevLights nl{};
    const DevEnv ev{};
    const uint32_t *const tiles = nullptr;
#include "rtmi_kernel_coop.inc"
}

#ifndef RTMI_ONE_TREE_TU
// the one-tree instantiation is compiled in rtmi_onetree.hip: a unit of its own, so that its scheduler strategy is its own
extern template __global__ void rtmi_render_coop<false, false, 4, true, 0, true>(DevScene, DevCamera, DevParams);
#endif
#ifndef RTMI_LEAN_TU
// the lean instantiations (EXT = false) are compiled in rtmi_lean.hip, with another machine-scheduler strategy
extern template __global__ void rtmi_render_coop<false, false, 4, false, 0>(DevScene, DevCamera, DevParams);
extern template __global__ void rtmi_render_coop<false, false, 4, false, 1>(DevScene, DevCamera, DevParams);
extern template __global__ void rtmi_render_coop<false, false, 4, false, 2>(DevScene, DevCamera, DevParams);
#endif

// Host: launch of a kernel whose block takes `lds` bytes of dynamic LDS.  Up to 48 KB a block gets as it is; above that
// the kernel's limit is raised first (the cooperative kernels with a deep pool).  The error of either step.  Hidden: where
// an instantiation is not inlined it is no export of librtmi.so.
template <typename... Params, typename... Args>
__attribute__((visibility("hidden"))) inline hipError_t rtmi_launch_lds(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t stream,
                                  const Args &...args) {
    if (lds > 48u * 1024u) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
    return hipGetLastError();
}

// ----------------------------------------------------------------------------------
// The workgroup-cooperative kernel (RTMI_FLAG_BLOCK_COOP) and the asynchronous state-machine kernel (RTMI_FLAG_ASYNC)
// are defined in rtmi_kernels_alt.hpp and instantiated in rtmi_alt.hip — measured slower than the default, kept as
// independent implementations for the parity tests, out of the headline translation unit.  Declarations for the launch:
// ----------------------------------------------------------------------------------
#define RTMI_BLK_WAVES 4
#define RTMI_BLK_THREADS (64 * RTMI_BLK_WAVES)
// LDS of a workgroup in uint32 words: pool [cap][2] | ctx [4][T][4] | best [T][2] | dummy [T][2] | sync [16]
#define RTMI_BLK_LDS_WORDS(cap) (2u * (cap) + RTMI_BLK_THREADS * 20u + 16u)
template <bool SIG, bool INST>
__global__ void rtmi_render_bcoop(DevScene sc, DevCamera cam, DevParams P);
template <bool FAST, bool SIG, bool PROF>
__global__ void rtmi_render_async(DevScene sc, DevCamera cam, DevParams P);
#ifndef RTMI_ALT_TU
extern template __global__ void rtmi_render_bcoop<true, false>(DevScene, DevCamera, DevParams);
extern template __global__ void rtmi_render_bcoop<false, false>(DevScene, DevCamera, DevParams);
extern template __global__ void rtmi_render_async<true, false, true>(DevScene, DevCamera, DevParams);
extern template __global__ void rtmi_render_async<false, false, true>(DevScene, DevCamera, DevParams);
extern template __global__ void rtmi_render_async<true, true, false>(DevScene, DevCamera, DevParams);
extern template __global__ void rtmi_render_async<true, false, false>(DevScene, DevCamera, DevParams);
extern template __global__ void rtmi_render_async<false, true, false>(DevScene, DevCamera, DevParams);
extern template __global__ void rtmi_render_async<false, false, false>(DevScene, DevCamera, DevParams);
#endif

#ifndef RTMI_LEAN_TU /* plain (non-template) kernels: defined once, in rtmi_device.hip */
// `col += color(..)` in sample order, then `col /= ns; sqrt; clamp; (255.99*c) as i32` — tests/test.rs:69-78,
// per local texel.  One thread per (local tile, pixel): adds this pass's samples to the f64 sum (`acc`, carried
// between passes when the per-sample buffer does not hold all ns samples at once) and, on the last pass, writes
// the texel.  A wavefront reads 1 KB contiguous per sample.
__global__ __launch_bounds__(256) void rtmi_resolve_kernel(const Rad3 *__restrict__ samples, double *__restrict__ acc,
                                                           rtmi_texel *__restrict__ out, DevParams P, int first, int last,
                                                           int partial) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= P.ntiles_local * 64u) return;
    // a traversal-pool overflow in any pass of this call invalidates its texels: poison them (rtmi_untile and
    // rtmi_scene_status report it) instead of handing out plausible numbers
    const bool poisoned = P.status[0] != 0u;
    const uint32_t ltile = tid >> 6, lane = tid & 63u;
    const uint32_t tile = ltile * P.tile_world + P.tile_rank;
    const uint32_t ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
    const bool in_image = tx * RTMI_TILE + (lane & 7u) < P.nx && ty * RTMI_TILE + (lane >> 3) < P.ny;
    double sum[3] = {0.0, 0.0, 0.0};
    double *a = acc + ((size_t)ltile * 3) * 64 + lane;
    if (!first) { sum[0] = a[0]; sum[1] = a[64]; sum[2] = a[128]; }
    if (in_image) {
        const Rad3 *src = samples + ((size_t)ltile * P.pass_stride) * 64u + lane;
        uint32_t s = 0;
        for (; s + 8u <= P.pass_cnt; s += 8u) { // 8 independent loads in flight, additions in sample order
            Rad3 v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = src[(size_t)(s + k) * 64u];
#pragma unroll
            for (int k = 0; k < 8; k++) { sum[0] += (double)v[k].r; sum[1] += (double)v[k].g; sum[2] += (double)v[k].b; }
        }
        for (; s < P.pass_cnt; s++) {
            const Rad3 v = src[(size_t)s * 64u];
            sum[0] += (double)v.r; sum[1] += (double)v.g; sum[2] += (double)v.b;
        }
    }
    if (!last) {
        a[0] = sum[0]; a[64] = sum[1]; a[128] = sum[2];
        if (!partial) return; // RTMI_FLAG_PROGRESSIVE: the texel of the samples so far is written after every pass
    }
    // col /= ns of the samples summed so far: all of them after the last pass (tests/test.rs:71)
    const double n_so_far = last ? (double)P.ns : (double)(P.pass_s0 + P.pass_cnt);
    rtmi_texel tx_out;
    uint32_t q[3];
    float lin[3];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const double m = sum[ch] / n_so_far;
        lin[ch] = (float)m;
        double g = sqrt(m);
        g = (g > 0.0) ? ((g < 1.0) ? g : 1.0) : 0.0; // nalgebra::clamp(val, 0, 1); NaN -> 0
        const double x = 255.99 * g;
        q[ch] = (x != x) ? 0u : (uint32_t)(int32_t)x; // `as i32`; in [0,255] after the clamp
    }
    tx_out.r = lin[0]; tx_out.g = lin[1]; tx_out.b = lin[2];
    tx_out.rgb8 = q[0] | (q[1] << 8) | (q[2] << 16);
    if (poisoned) {
        const float nan = __uint_as_float(0x7fc00000u);
        tx_out.r = nan; tx_out.g = nan; tx_out.b = nan;
        tx_out.rgb8 = RTMI_TEXEL_POISON;
    }
    out[tid] = tx_out;
}
// end of a pass (one thread): the unit counter goes back to zero for the next pass, the pass's units are added to
// the progress word, and after the last pass the call's overflow count joins the sticky word
__global__ void rtmi_pass_end_kernel(unsigned int *status, unsigned int units, unsigned int pass_spp, int last) {
    status[3] += units;
    status[4] += pass_spp;
    status[1] = 0u;
    if (last) status[2] += status[0];
}

// ---- device evaluation of the arithmetic contract, for parity tests --------------------
// op: 0 sin, 1 log, 2 atan2(x,y), 3 asin, 4 x/y, 5 sqrt, 6 u01(bits of x), 7 cos, 16.. instance transforms
__global__ void rtmi_math_probe_kernel(int op, const float *x, const float *y, float *out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float r;
    switch (op) {
    case 0: r = rtmi_sinf(x[i]); break;
    case 1: r = rtmi_logf(x[i]); break;
    case 2: r = rtmi_atan2f(x[i], y[i]); break;
    case 3: r = rtmi_asinf(x[i]); break;
    case 4: r = x[i] / y[i]; break;
    case 5: r = __builtin_sqrtf(x[i]); break;
    case 6: r = rtmi_u01(__float_as_uint(x[i])); break;
    case 7: r = rtmi_cosf(x[i]); break;
    default: { // 16 + 4*(axis) + which: instance transforms (rotate.rs:85-113) by sin/cos of 33 degrees
        const int axis = ((op - 16) >> 2) % 3, which = (op - 16) & 3;
        rtmi_xform X;
        X.kind = RTMI_XF_ROTATE_X + axis; X.x = 0.5446390509605408f; X.y = 0.838670551776886f; X.z = 0.0f;
        F3 o, d = f3(0, 0, 0);
        // put (x, y) into the (a, b) components of this axis: X -> (y,z), Y -> (z,x), Z -> (x,y)
        if (axis == 0) o = f3(0.25f, x[i], y[i]); else if (axis == 1) o = f3(y[i], 0.25f, x[i]); else o = f3(x[i], y[i], 0.25f);
        F3 n = o;
        if (which < 2) xform_ray(&X, 0, 1, o, d); else xform_hit(&X, 0, 1, o, n);
        if (op >= 28) o = n; // 28..39: the normal instead of the point
        const float a = axis == 0 ? o.y : (axis == 1 ? o.z : o.x), b = axis == 0 ? o.z : (axis == 1 ? o.x : o.y);
        r = (which & 1) ? b : a;
        break;
    }
    }
    out[i] = r;
}
// instance transforms exactly as the render kernels call them: xforms in global memory, runtime count
__global__ void rtmi_xform_probe_kernel(const rtmi_xform *xf, int count, const float *a, const float *b, float *out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    F3 o = f3(a[3 * i], a[3 * i + 1], a[3 * i + 2]), d = f3(b[3 * i], b[3 * i + 1], b[3 * i + 2]);
    F3 p = o, nn = d;
    const bool rot = xform_ray(xf, 0, count, o, d);
    xform_hit(xf, 0, count, p, nn);
    float *r = out + 13 * (size_t)i;
    r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = d.x; r[4] = d.y; r[5] = d.z;
    r[6] = p.x; r[7] = p.y; r[8] = p.z; r[9] = nn.x; r[10] = nn.y; r[11] = nn.z; r[12] = rot ? 1.0f : 0.0f;
}
__global__ void rtmi_philox_probe_kernel(const uint32_t *ctr, const uint32_t *key, uint32_t *out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t o0, o1, o2, o3;
    // a wavefront whose cases share one key evaluates the form with block-local round keys (philox<true>, scalar keys only)
    const uint32_t k0 = key[2 * i], k1 = key[2 * i + 1];
    const uint32_t u0 = __builtin_amdgcn_readfirstlane(k0), u1 = __builtin_amdgcn_readfirstlane(k1);
    if (__ballot(k0 != u0 || k1 != u1) == 0ull) philox<true>(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], u0, u1, o0, o1, o2, o3);
    else philox(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], k0, k1, o0, o1, o2, o3);
    out[4 * i] = o0; out[4 * i + 1] = o1; out[4 * i + 2] = o2; out[4 * i + 3] = o3;
}
// ray-primitive and shading arithmetic exactly as the render kernels call it (rtmi_probe_geom, include/rtmi.h): the
// production inline functions on a DevScene whose leaf records and transforms are laid out as rtmi_scene_create lays
// them out.  One wavefront per block; the host has checked that every 64 consecutive PRIM cases share one primitive
// index, so the index handed to prim_test_uniform is wave-uniform as in a list scan.
__global__ void __launch_bounds__(64) rtmi_geom_probe_kernel(int op, DevScene sc, const float *in, float *out, uint32_t n) {
    const uint32_t i = min(blockIdx.x * 64u + threadIdx.x, n - 1u); // tail lanes repeat the last case, write nothing
    const bool live = blockIdx.x * 64u + threadIdx.x < n;
    const float *a = in + RTMI_PROBE_GEOM_IN * (size_t)i;
    float res[RTMI_PROBE_GEOM_OUT];
    for (int k = 0; k < RTMI_PROBE_GEOM_OUT; k++) res[k] = 0.0f;
    RayF r;
    r.o = f3(a[0], a[1], a[2]);
    r.d = f3(a[3], a[4], a[5]);
    ray_derive(r);
    const float time = a[6], t_min = a[7], t_max = a[8];
    const int idx = __float_as_int(a[9]);
    if (op == RTMI_PROBE_GEOM_PRIM) {
        const PrimRec *pr = reinterpret_cast<const PrimRec *>(sc.leaf_rec + (size_t)idx * 5);
        const float4 A = pr->A, B = pr->B;
        const rtmi_prim_meta M = pr->M;
        float t0 = t_max, t1 = t_max, t2 = t_max;
        int pf0 = 0, pf1 = 0, pf2 = 0;
        const bool h0 = prim_test<true>(sc, M.type, idx, r, time, t_min, t_max, t0, pf0);
        const bool h1 = prim_test_vals<true>(sc, M.type, idx, A, B, M.inv_dt, M.flags, r, time, t_min, t_max, t1, pf1);
        const int uidx = __builtin_amdgcn_readfirstlane(idx);
        const bool h2 = prim_test_uniform<true>(sc, uidx, r, time, t_min, t_max, t2, pf2);
        res[0] = h0 ? 1.0f : 0.0f; res[1] = t0; res[2] = (float)(pf0 & 7);
        res[3] = h1 ? 1.0f : 0.0f; res[4] = t1; res[5] = (float)(pf1 & 7);
        res[6] = h2 ? 1.0f : 0.0f; res[7] = t2; res[8] = (float)(pf2 & 7);
        res[9] = (float)((pf0 >> 3) - idx) + (float)((pf1 >> 3) - idx) + (float)((pf2 >> 3) - uidx); // 0: index kept
    } else if (op == RTMI_PROBE_GEOM_AABB) {
        float te = 0.0f;
        res[0] = aabb_hit(a[10], a[11], a[12], a[13], a[14], a[15], r, t_min, t_max) ? 1.0f : 0.0f;
        res[1] = aabb_hit_t(a[10], a[11], a[12], a[13], a[14], a[15], r, t_min, t_max, te) ? 1.0f : 0.0f;
        res[2] = te;
    } else if (op == RTMI_PROBE_GEOM_MEDIUM) {
        bool h1 = false, h2 = false;
        float q1 = 0.0f, q2 = 0.0f;
        sphere_two_queries(r, reinterpret_cast<const PrimRec *>(sc.leaf_rec + (size_t)idx * 5)->A, h1, q1, h2, q2);
        res[0] = h1 ? 1.0f : 0.0f; res[1] = q1; res[2] = h2 ? 1.0f : 0.0f; res[3] = q2;
    } else if (op == RTMI_PROBE_GEOM_SHADE) { // v = ray direction, n = a[10..12], ni_over_nt = a[13], cosine = a[14], ref_idx = a[15]
        const F3 nn = f3(a[10], a[11], a[12]);
        const F3 rf = reflect(r.d, nn);
        F3 rr = f3(0.0f, 0.0f, 0.0f);
        const bool ok = refract(r.d, nn, a[13], rr);
        res[0] = rf.x; res[1] = rf.y; res[2] = rf.z;
        res[3] = ok ? 1.0f : 0.0f; res[4] = rr.x; res[5] = rr.y; res[6] = rr.z;
        res[7] = schlick(a[14], a[15]);
    } else if (op == RTMI_PROBE_GEOM_UV) { // the normal = a[10..12]; `book` read at run time, as the render reads it
        const F3 nn = f3(a[10], a[11], a[12]);
        sphere_uv(nn, a[13] != 0.0f, res[0], res[1]);
        sphere_uv(nn, a[14] != 0.0f, res[2], res[3]);
    }
    if (live)
        for (int k = 0; k < RTMI_PROBE_GEOM_OUT; k++) out[RTMI_PROBE_GEOM_OUT * (size_t)i + k] = res[k];
}
#endif // RTMI_LEAN_TU
