// rtmi_roulette_dev.hpp — what the two roulette translation units share (include/rtmi_roulette.h): the roulette test and
// the two statements a kernel body uses where a roulette kernel writes a path.  Included by rtmi_roulette.hip (the
// per-lane body) and rtmi_roulette_coop.hip (the cooperative body), both under RTMI_PATH_RR, after
// rtmi_kernels.hpp and rtmi_light_launch.hpp (DevRoulette).
#pragma once

// The roulette test of rtmi_roulette.h, after a scatter has updated pa.T and pa.depth; g is the path's stream-0 state
// (its sample and pixel words key the stateless stream-4 draw).  false: the continuation ends.
template <typename RngT>
__device__ __forceinline__ bool roulette_survives(const DevRoulette &rr, const RngT &g, uint32_t k0, uint32_t k1, Path &pa) {
    if (pa.depth < rr.min_depth) return true;
    const float m = fmaxf(fmaxf(pa.T.x, pa.T.y), pa.T.z);
    if (m == 0.0f) return false;
    const float q = fminf(fmaxf(m, rr.q_min), 1.0f);
    if (q < 1.0f) {
        uint32_t o0, o1, o2, o3;
        philox(pa.depth, g.sample, g.pixel, 4u, k0, k1, o0, o1, o2, o3);
        if (!(rtmi_u01(o0) < q)) return false;
        pa.T = vdiv(pa.T, q);
    }
    return true;
}

// the two statements the bodies use where a roulette kernel writes a path: the bounce count (tiled as the path signatures;
// a path that never scattered adds nothing) and the whole ending of a path that roulette cut
#define RTMI_RR_COUNT() \
    do { if (pa.depth != 0u) atomicAdd(rr.bounces + (size_t)ltile * 64 + (oidx & 63u), pa.depth); } while (0)
#define RTMI_RR_END_PATH() \
    do { path_end(P, oidx, pa); RTMI_RR_COUNT(); alive = false; } while (0)
