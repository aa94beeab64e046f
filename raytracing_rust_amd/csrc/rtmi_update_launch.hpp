// rtmi_update_launch.hpp — launchers of the scene-update kernels (include/rtmi_update.h), defined in rtmi_update_dev.hip
// and called by the entry points in rtmi_update.hip.  C++ linkage, hidden: nothing here is exported.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

// One refittable BVH item as the refit kernel reads it.  Its node lists lie in RefitTables::words: level k of the
// reference tree (deepest first) is the node indices words[lvl + k] .. words[lvl + k + 1] of the table, for k < n_lvl; the
// alternative tree likewise (alt_n_lvl = 0: none).
struct RefitJob {
    uint32_t item, root;
    uint32_t prim_lo, prim_hi; // the primitives its leaves name: the item is refit when the updated range meets them
    uint32_t lvl, n_lvl, alt_lvl, alt_n_lvl;
};
static_assert(sizeof(RefitJob) == 32, "RefitJob is read as eight words");

// the device arrays of a handle that an update rewrites, and the tables built on its first update
struct UpdateScene {
    char *items;       // DevItem [n_items], 96 B apart
    float4 *prim_a, *prim_b, *gate /* or NULL */, *nodes, *nodes4, *leaf_rec, *shade_prim;
    const uint32_t *words;       // the node lists of all jobs
    const RefitJob *jobs;        // [n_jobs]
    const int32_t *medium_item;  // [n_prims]: the MEDIUM item that carries a copy of this sphere, or -1
    float4 *scratch;             // [n_nodes][2]: the node boxes of the reference trees
    uint32_t n_jobs;
};

// planes [first, first + count) from d_a / d_b (d_b may be NULL) into every copy the handle keeps of them
__attribute__((visibility("hidden"))) hipError_t rtmi_update_scatter_launch(hipStream_t stream, const UpdateScene &U, uint32_t first,
                                                                            uint32_t count, const float *d_a, const float *d_b);
// one workgroup per job; a job whose primitives the range does not meet returns at once
__attribute__((visibility("hidden"))) hipError_t rtmi_update_refit_launch(hipStream_t stream, const UpdateScene &U, uint32_t first,
                                                                          uint32_t count);
