// rtmi_session_launch.hpp — launchers of the render-session kernels (include/rtmi_session.h), defined in rtmi_session.hip
// and called by the session entry points below them there.  All three work on the session's state alone, laid out
// [tile][9][64] (sum r,g,b | m r,g,b | M2 r,g,b), one wavefront per tile, lane = pixel.
#pragma once

// state + counts -> texels, standard errors and counts of all tiles
struct SessionReadout {
    const double *state;    // [tile][9][64]
    const uint32_t *counts; // [tile] the samples each tile holds (> 0)
    uint32_t ntiles;
    rtmi_texel *texels;     // [tile][64]
    float *stderr_out;      // [tile][64][3]
    uint32_t *spp_out;      // [tile][64]
};

// the convergence test of rtmi_adaptive.h on tiles that all hold n samples, without new samples
struct SessionDecide {
    const double *state;
    const uint32_t *tiles_in; // [n_in] the tiles to test
    uint32_t n_in;
    uint32_t *tiles_out;      // the tiles that fail the test, appended in any order
    uint32_t *n_out;          // ... their count (zeroed by the host before the launch)
    uint32_t nx, ny, tiles_x;
    uint32_t n;
    double abs_tol, rel_tol;
};

// dst <- dst (+) src, the pairwise combination of rtmi_session.h; every tile of dst holds nA samples, of src nB (both > 0)
struct SessionMerge {
    double *dst;
    const double *src;
    uint32_t *dst_bounces;       // [tile][64]
    const uint32_t *src_bounces;
    uint32_t ntiles;
    double nA, nB;
};

hipError_t rtmi_session_launch_readout(hipStream_t stream, const SessionReadout &R);
hipError_t rtmi_session_launch_decide(hipStream_t stream, const SessionDecide &D);
hipError_t rtmi_session_launch_merge(hipStream_t stream, const SessionMerge &M);
