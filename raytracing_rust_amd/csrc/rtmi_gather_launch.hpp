// rtmi_gather_launch.hpp — launchers of the hemisphere-gather kernels (include/rtmi_gather.h), defined in rtmi_gather.hip
// and called by rtmi_gather / rtmi_gather_device in rtmi_batch.hip.
#pragma once

// one slab of points on the device; the per-sample buffer is P.samples of the launch ([n][spp] Rad3, item k = i * spp + s)
struct GatherBatch {
    const float *points;  // [n][3]
    const float *normals; // [n][3]; COSINE only
    const float *time;    // [n], or NULL: every path at time 0
    float *value;         // [n][3], or NULL
    float *stderr_out;    // [n][3], or NULL
    float *sh;            // [n][9][3], or NULL; SPHERE only
    unsigned int *queue;  // next chunk of the persistent wavefronts: the handle's word, zeroed on the call's stream
    uint32_t n, spp;
    uint32_t total;       // n * spp < 2^31
    uint32_t chunk;       // items of a chunk: consecutive items one wavefront deals to its lanes
    uint32_t nchunks;     // ceil(total / chunk)
    uint32_t first_point, first_sample; // the Philox indices of item (0, 0); no index of the batch wraps
};

// the path kernel over the slab's items on `blocks` persistent wavefronts; nee / env select the estimator, mode the
// directions (RTMI_GATHER_COSINE / _SPHERE)
hipError_t rtmi_gather_launch(bool fast, bool nee, bool env, uint32_t mode, uint32_t blocks, hipStream_t stream, const DevScene &sc,
                              const DevParams &P, const GatherBatch &B, const DevLights &L, const DevEnv &E);
// value, stderr and sh of every point from its spp slots of `samples` (any output may be NULL, not all); key0, key1: the
// Philox key of the directions, which the SH projection draws again
hipError_t rtmi_gather_launch_resolve(uint32_t mode, hipStream_t stream, const Rad3 *samples, const GatherBatch &B, uint32_t key0,
                                      uint32_t key1);
