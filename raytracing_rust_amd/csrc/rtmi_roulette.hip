// rtmi_roulette.hip — translation unit of Russian-roulette path termination (include/rtmi_roulette.h): the render kernels
// and their launcher.  Compiled with the flags of rtmi_device.hip (-ffp-contract=off).
//
// The render kernel is the body of rtmi_render_kernel (rtmi_kernel_perlane.inc) with TILE_LIST = true, the NEE / ENV
// switches of rtmi_adaptive_nee_kernel and the RR switch (RTMI_PATH_RR, a preprocessor switch: every other inclusion
// of the body is the same text as before): the roulette test after a scatter, the end-after-its-shadow-ray flag and the
// bounce count at every place a path is written.  One instantiation per FAST x estimator serves both entry points: the
// fixed render runs over the list of all tiles.  No path signatures (SIG = false).  The resolve is adaptive sampling's
// (rtmi_adaptive_resolve_kernel, rtmi_adaptive.hip).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "rtmi.h"
#include "rtmi_math.h"

#define RTMI_LEAN_TU 1 /* the plain kernels are defined in rtmi_device.hip */
#include "rtmi_kernels.hpp"
#include "rtmi_light_launch.hpp"

#include "rtmi_roulette_dev.hpp" // roulette_survives, RTMI_RR_COUNT(), RTMI_RR_END_PATH(): shared with rtmi_roulette_coop.hip

#define RTMI_PATH_RR 1
template <bool FAST, bool NEE, bool ENV>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void rtmi_roulette_kernel(DevScene sc, DevCamera cam, DevParams P,
                                                                            const uint32_t *tiles, DevLights nl, DevEnv ev,
                                                                            DevRoulette rr) {
    constexpr bool SIG = false, PROF = false, TILE_LIST = true, FEATURES = false;
#include "rtmi_kernel_perlane.inc"
}
#undef RTMI_PATH_RR

hipError_t rtmi_roulette_launch_render(bool fast, bool nee, bool env, uint32_t blocks, hipStream_t stream, const DevScene &sc,
                                       const DevCamera &cam, const DevParams &P, const uint32_t *tiles, const DevLights &L,
                                       const DevEnv &E, const DevRoulette &R) {
    const dim3 grid(blocks), block(64 * WAVES_PER_BLOCK);
    return rtmi_with_bools([&](auto NEE, auto ENV, auto FAST) {
        hipLaunchKernelGGL((rtmi_roulette_kernel<FAST(), NEE(), ENV()>), grid, block, 0, stream, sc, cam, P, tiles, L, E, R);
        return hipGetLastError();
    }, nee, env, fast);
}
