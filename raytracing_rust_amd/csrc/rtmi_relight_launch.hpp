// rtmi_relight_launch.hpp — launcher of the relight kernel (include/rtmi_relight.h), defined in rtmi_relight_dev.hip and
// called by enqueue() of rtmi_update.hip.  C++ linkage, hidden: nothing here is exported.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#define RTMI_RELIGHT_BLOCK 256 /* threads of the one workgroup */

// the device arrays of a handle that the relight reads and rewrites, and the tables rtml_scene_follow_lights built
struct RelightScene {
    const float4 *prim_a, *prim_b; // the planes, as the scatter kernel of the same update left them
    float *lights;                 // NeeLight [n], 12 words apart: geo[4], k, plane, item, prim, area, p_sel, cdf, pad
    float *nodes;                  // rtmi_light_node [2 n], 8 words apart: c[3], r2, power, link, pad[2]; NULL: no tree attached
    const double *weight;          // [n]
    const uint32_t *words;         // the tree's slots by depth, deepest first: level k = words[words[k] .. words[k + 1])
    double *aw;                    // scratch [n]: area * weight
    double *box;                   // scratch [2 n][7]: lo[3], hi[3], power of a slot
    uint32_t n, n_lvl;
};

// one workgroup of RTMI_RELIGHT_BLOCK threads; n == 0 launches nothing
__attribute__((visibility("hidden"))) hipError_t rtmi_relight_launch(hipStream_t stream, const RelightScene &R);
