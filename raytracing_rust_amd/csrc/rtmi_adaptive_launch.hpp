// rtmi_adaptive_launch.hpp — launchers of the adaptive-sampling kernels (include/rtmi_adaptive.h), defined in
// rtmi_adaptive.hip and called by the host loop in rtmi_device.hip.
#pragma once

// which render kernel an adaptive pass runs: the default cooperative kernel (lean or EXT form) or the per-lane one
enum { RTMI_AD_COOP_LEAN = 0, RTMI_AD_COOP_EXT = 1, RTMI_AD_PERLANE = 2, RTMI_AD_PERLANE_FAST = 3 };

// what the adaptive resolve of one (sub-)pass needs besides DevParams (P.ntiles_local = active tiles, P.pass_s0 = the
// samples every active tile had before this sub-pass)
struct AdaptiveResolve {
    const uint32_t *tiles_in; // [P.ntiles_local] the active tiles; position = index into the per-sample buffer
    uint32_t *tiles_out;      // the tiles still active after a decision, appended in any order
    uint32_t *n_out;          // ... their count (zeroed by the host before the step)
    double *state;            // [tile][9][64]: sum r,g,b | m r,g,b | M2 r,g,b
    rtmi_texel *texels;       // [tile][64] texels of retired tiles
    float *stderr_out;        // [tile][64][3]
    uint32_t *spp_out;        // [tile][64]
    double abs_tol, rel_tol;
    uint32_t ns;              // the cap
    int first;                // first sub-pass of the call: the state starts at zero
    int decide;               // last sub-pass of a step: test, retire or re-list every active tile
};

hipError_t rtmi_adaptive_launch_render(int which, uint32_t blocks, size_t lds, hipStream_t stream, const DevScene &sc,
                                       const DevCamera &cam, const DevParams &P, const uint32_t *tiles);
hipError_t rtmi_adaptive_launch_resolve(hipStream_t stream, const Rad3 *samples, const DevParams &P, const AdaptiveResolve &A);
