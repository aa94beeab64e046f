// rtmi_roulette_coop.hip — translation unit of RTMI_FLAG_ROULETTE_COOP (include/rtmi_roulette_coop.h): Russian-roulette
// renders on the wave-cooperative kernel, and their launcher.  Compiled with the flags of rtmi_device.hip
// (-ffp-contract=off).
//
// The kernel is the body of rtmi_render_coop (rtmi_kernel_coop.inc) with TILE_LIST = true, the NEE / ENV switches of
// rtmi_light_coop_kernel and the RR switch (RTMI_PATH_RR, a preprocessor switch: every other inclusion of the body is the
// same text as before): the statements of rtmi_roulette_kernel (rtmi_kernel_perlane.inc under RTMI_PATH_RR) at the
// same places, so per-lane program order is that kernel's and every plane, the bounce count included, has its bits.  One
// instantiation per pool form x estimator serves both entry points: the fixed render runs over the list of all tiles.
// (NEE, ENV) = (0, 0) is the plain estimator: g is RngRing (lean) or RngReg (ext), whose sample and pixel words key the
// stateless stream-4 draw; the ring does not move.  No path signatures; level 0 only (no instanced primitives, no media
// inside transforms: those scenes stay on rtmi_roulette_kernel).  The NEE / ENV forms are built for RTMI_LIGHT_COOP_WPS
// waves per SIMD as their counterparts of rtmi_light_coop.hip, the plain forms for RTMI_ROULETTE_COOP_PLAIN_WPS
// (rtmi_light_launch.hpp): the grid the host launches.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "rtmi.h"
#include "rtmi_math.h"

#define RTMI_LEAN_TU 1 /* the plain kernels are defined in rtmi_device.hip */
#include "rtmi_kernels.hpp"
#include "rtmi_light_launch.hpp"

#include "rtmi_roulette_dev.hpp" // roulette_survives, RTMI_RR_COUNT(), RTMI_RR_END_PATH(): shared with rtmi_roulette.hip

#define RTMI_PATH_RR 1
template <bool EXT, bool NEE, bool ENV>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, rtmi_roulette_coop_wps(NEE, ENV)) void rtmi_roulette_coop_kernel(
    DevScene sc, DevCamera cam, DevParams P, const uint32_t *tiles, DevLights nl, DevEnv ev, DevRoulette rr) {
    constexpr bool SIG = false, PROF = false, TILE_LIST = true, ONE_TREE = false;
    constexpr int INSTL = 0;
#include "rtmi_kernel_coop.inc"
}
#undef RTMI_PATH_RR

hipError_t rtmi_roulette_coop_launch_render(bool ext, bool nee, bool env, uint32_t blocks, size_t lds, hipStream_t stream,
                                            const DevScene &sc, const DevCamera &cam, const DevParams &P, const uint32_t *tiles,
                                            const DevLights &L, const DevEnv &E, const DevRoulette &R) {
    const dim3 grid(blocks), block(64 * WAVES_PER_BLOCK);
    return rtmi_with_bools([&](auto EXT, auto NEE, auto ENV) {
        return rtmi_launch_lds(&rtmi_roulette_coop_kernel<EXT(), NEE(), ENV()>, grid, block, lds, stream, sc, cam, P, tiles,
                               L, E, R);
    }, ext, nee, env);
}
