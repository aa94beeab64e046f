// rtmi_adaptive_nee.hip — translation unit of adaptive sampling with next-event estimation or environment lighting
// (include/rtmi_adaptive_nee.h): the render kernels and their launcher.  Compiled with the flags of rtmi_device.hip
// (-ffp-contract=off).
//
// The render kernel is the body of rtmi_render_kernel (rtmi_kernel_perlane.inc) with TILE_LIST = true, as
// rtmi_adaptive_kernel, and the NEE / ENV switches of rtmi_nee_kernel and rtmi_env_kernel: queue unit -> position in the
// active-tile list -> tile, and work_take hands out the real (sample, pixel), so streams 0 and 3 are the fixed render's.
// No path signatures (SIG = false).  Instantiated for FAST x (NEE, ENV) in {(1, 0), (0, 1), (1, 1)}.  The resolve is
// adaptive sampling's (rtmi_adaptive_resolve_kernel, rtmi_adaptive.hip).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "rtmi.h"
#include "rtmi_math.h"

#define RTMI_LEAN_TU 1 /* the plain kernels are defined in rtmi_device.hip */
#include "rtmi_kernels.hpp"
#include "rtmi_light_launch.hpp"

template <bool FAST, bool NEE, bool ENV>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void rtmi_adaptive_nee_kernel(DevScene sc, DevCamera cam, DevParams P,
                                                                                const uint32_t *tiles, DevLights nl, DevEnv ev) {
    constexpr bool SIG = false, PROF = false, TILE_LIST = true, FEATURES = false;
#include "rtmi_kernel_perlane.inc"
}

hipError_t rtmi_adaptive_nee_launch_render(bool fast, bool nee, bool env, uint32_t blocks, hipStream_t stream, const DevScene &sc,
                                           const DevCamera &cam, const DevParams &P, const uint32_t *tiles, const DevLights &L,
                                           const DevEnv &E) {
    const dim3 grid(blocks), block(64 * WAVES_PER_BLOCK);
    return rtmi_with_bools([&](auto NEE, auto ENV, auto FAST) {
        if constexpr (!NEE() && !ENV()) return hipErrorInvalidValue; // the plain estimator is rtmi_adaptive_kernel's
        else {
            hipLaunchKernelGGL((rtmi_adaptive_nee_kernel<FAST(), NEE(), ENV()>), grid, block, 0, stream, sc, cam, P, tiles, L, E);
            return hipGetLastError();
        }
    }, nee, env, fast);
}
