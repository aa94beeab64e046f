// rtmi_adaptive_nee_launch.hpp — launcher of the adaptive NEE / environment kernels (include/rtmi_adaptive_nee.h),
// defined in rtmi_adaptive_nee.hip and called by the adaptive step loop in rtmi_device.hip.  The resolve is adaptive
// sampling's (rtmi_adaptive_launch.hpp).
#pragma once

// one pass over the P.ntiles_local active tiles of `tiles`; nee / env select the estimator (not both false)
hipError_t rtmi_adaptive_nee_launch_render(bool fast, bool nee, bool env, uint32_t blocks, hipStream_t stream, const DevScene &sc,
                                           const DevCamera &cam, const DevParams &P, const uint32_t *tiles, const DevLights &L,
                                           const DevEnv &E);
