// rtmi_roulette_launch.hpp — the kernel argument and the launcher of the Russian-roulette kernels
// (include/rtmi_roulette.h), defined in rtmi_roulette.hip and called by the step loop in rtmi_device.hip.  The resolve is
// adaptive sampling's (rtmi_adaptive_launch.hpp).
#pragma once

// the roulette parameters and the bounce plane: a kernel argument of their own, as DevLights and DevEnv are (DevParams
// goes to every kernel)
struct DevRoulette {
    uint32_t *bounces;  // [local tile][64]: scatters of the pixel's written paths, summed with integer atomics
    uint32_t min_depth; // the test is made when depth >= min_depth
    float q_min;        // floor of the survival probability
};

// one pass over the P.ntiles_local active tiles of `tiles`; nee / env select the estimator (both false: the plain one)
hipError_t rtmi_roulette_launch_render(bool fast, bool nee, bool env, uint32_t blocks, hipStream_t stream, const DevScene &sc,
                                       const DevCamera &cam, const DevParams &P, const uint32_t *tiles, const DevLights &L,
                                       const DevEnv &E, const DevRoulette &R);
