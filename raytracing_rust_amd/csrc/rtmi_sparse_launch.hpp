// rtmi_sparse_launch.hpp — launchers of the sparse-render kernels (include/rtmi_sparse.h), defined in rtmi_sparse.hip and
// called by the rtmi_sparse_* entries in rtmi_batch.hip.
#pragma once

// pixels of one workgroup of the select kernels: 256 lanes x 16 bytes
#define RTMI_SPARSE_SPAN 4096u
// the caller's scratch (rtmi_sparse.h): the control words, then the per-workgroup counts of the select
#define RTMI_SPARSE_QUEUE_WORD 0u  // chunk counter of the path kernel
#define RTMI_SPARSE_COUNT_WORD 2u  // {written, selected} of a refine
#define RTMI_SPARSE_HEAD_WORDS 4u

// one list of pixels on the device; the per-sample buffer is P.samples of the launch ([n][ns] Rad3, item k * ns + s)
struct SparseBatch {
    const uint32_t *list;      // [n] pixel indices row * nx + i into the image planes (row 0 the top row)
    const uint32_t *count;     // the entries are min(count[0], n), read by the kernels; NULL: n
    float *mean;               // [n][3], or NULL
    float *stderr_out;         // [n][3], or NULL
    unsigned int *queue;       // next chunk of the persistent wavefronts: a word of the caller's scratch, zeroed on the stream
    uint32_t n, ns;            // capacity of the list; n * ns < 2^31
    uint32_t chunk;            // items of a chunk: consecutive items one wavefront deals to its lanes
    uint32_t first_sample;     // no sample index of the call wraps
};

// the ascending list of the pixels of bytes[0..n) whose byte passes the mask, on `stream`: count, scan, scatter
hipError_t rtmi_sparse_launch_select(hipStream_t stream, const uint8_t *bytes, uint32_t n, uint32_t accept_mask, uint32_t capacity,
                                     uint32_t *list, uint32_t *count, uint32_t *block_counts);
// the path kernel over the list's items on `blocks` persistent wavefronts; nee / env select the estimator
hipError_t rtmi_sparse_launch(bool fast, bool nee, bool env, uint32_t blocks, hipStream_t stream, const DevScene &sc,
                              const DevCamera &cam, const DevParams &P, const SparseBatch &B, const DevLights &L, const DevEnv &E);
// mean and stderr of every entry from its ns slots of `samples` (either output may be NULL, not both)
hipError_t rtmi_sparse_launch_resolve(hipStream_t stream, const Rad3 *samples, const SparseBatch &B);
// the entries' records written to the planes at their pixels (each plane may be NULL); `se`/`stderr_plane`: the same for
// a plane of standard errors
hipError_t rtmi_sparse_launch_patch(hipStream_t stream, uint32_t n_pixels, const uint32_t *list, const uint32_t *count, uint32_t capacity,
                                    const float *mean, const float *se, float *linear, uint8_t *rgb8, float *stderr_plane,
                                    uint8_t *bytes, uint32_t mark);
