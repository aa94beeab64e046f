// rtmi_query_launch.hpp — launcher of the ray-query kernels (include/rtmi_query.h), defined in rtmi_query.hip and called
// by rtmi_trace / rtmi_occluded and their _device forms in rtmi_device.hip.
#pragma once

// one batch of rays on the device
struct QueryBatch {
    const float4 *rays;   // [n][2]: {o, t_min}, {d, t_max} (rtmi_ray)
    const float *time;    // [n], or NULL: every ray at time 0
    float4 *hits;         // trace: [n][3] (rtmi_hit)
    uint8_t *occluded;    // occluded: [n]
    const uint32_t *prim_gaps, *item_gaps; // rtmi_scene_attach_flips: the flips' places in the chains, or NULL both
    uint32_t n;
    uint32_t key0, key1;  // (seed + first_ray) mod 2^64: the Philox key of ray 0; ray i adds i
};

// trace (any = false) or occluded (any = true) of the batch on `stream`; fast: the pruned closest-hit traversal
hipError_t rtmi_query_launch(bool any, bool fast, hipStream_t stream, const DevScene &sc, const QueryBatch &B);
