// rtmi_radiance_launch.hpp — launchers of the radiance-query kernels (include/rtmi_radiance.h), defined in
// rtmi_radiance.hip and called by rtmi_radiance / rtmi_radiance_device in rtmi_batch.hip.
#pragma once

// one batch of rays on the device; the per-sample buffer is P.samples of the launch ([n][spp] Rad3, item k = i * spp + s)
struct RadianceBatch {
    const float4 *rays;  // [n][2]: {o, t_min}, {d, t_max} (rtmi_ray)
    const float *time;   // [n], or NULL: every ray at time 0
    float *mean;         // [n][3], or NULL
    float *stderr_out;   // [n][3], or NULL
    unsigned int *queue; // next chunk of the persistent wavefronts: the handle's word, zeroed on the call's stream
    uint32_t n, spp;
    uint32_t total;      // n * spp < 2^31
    uint32_t chunk;      // items of a chunk: consecutive items one wavefront deals to its lanes
    uint32_t nchunks;    // ceil(total / chunk)
    uint32_t first_ray, first_sample; // the Philox indices of item (0, 0); no index of the batch wraps
    uint32_t skip_block, skip_pos;    // stream 0 starts at word 4 * skip_block + skip_pos (skip_pos in 0..3)
};

// Measured: the render's unit of 1024 items lands at the render's speed; 128 is 1.05-1.5x faster on the
// scenes with a tree (the launch's tail: a wavefront ends holding at most 128 paths, not 1024) and costs 1 atomic per 128 paths
#define RTMI_RADIANCE_CHUNK 128u

// the path kernel over the batch's items on `blocks` persistent wavefronts; nee / env select the estimator
hipError_t rtmi_radiance_launch(bool fast, bool nee, bool env, uint32_t blocks, hipStream_t stream, const DevScene &sc,
                                const DevParams &P, const RadianceBatch &B, const DevLights &L, const DevEnv &E);
// mean and stderr of every ray from its spp slots of `samples` (either output may be NULL, not both)
hipError_t rtmi_radiance_launch_resolve(hipStream_t stream, const Rad3 *samples, const RadianceBatch &B);
