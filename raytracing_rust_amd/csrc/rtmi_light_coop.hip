// rtmi_light_coop.hip — translation unit of RTMI_FLAG_LIGHT_COOP (include/rtmi_light_coop.h): next-event estimation and
// environment lighting on the wave-cooperative kernel, and their launcher.  Compiled with the flags of rtmi_device.hip
// (-ffp-contract=off).
//
// The kernel is the body of rtmi_render_coop (rtmi_kernel_coop.inc) with the NEE / ENV switches of rtmi_nee_kernel and
// rtmi_env_kernel: the item scan is executed by all 64 lanes, a lane's query being its path ray or its pending shadow ray
// (NeeLane), traced with the light-sample stream swapped in for the path's; shade_hit<.., NEE, ENV> is the per-lane
// kernels'.  Per-lane program order is the per-lane kernels', so every output plane has their bits.  Instantiated for the
// fixed render (TILE_LIST = false: SIG x pool form x (NEE, ENV) in {(1, 0), (0, 1), (1, 1)}, 12 kernels) and for adaptive
// sampling's tile list (TILE_LIST = true, no signatures: 6 kernels); level 0 only (no instanced primitives, no media
// inside transforms: those scenes stay on the per-lane kernels).  FAST is implied: the cooperative traversal is the
// fast-cull one.  RTMI_LIGHT_COOP_WPS waves per SIMD (rtmi_light_launch.hpp): the grid the host launches.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "rtmi.h"
#include "rtmi_math.h"

#define RTMI_LEAN_TU 1 /* the plain kernels are defined in rtmi_device.hip */
#include "rtmi_kernels.hpp"
#include "rtmi_light_launch.hpp"

template <bool TILE_LIST, bool SIG, bool EXT, bool NEE, bool ENV>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, RTMI_LIGHT_COOP_WPS) void rtmi_light_coop_kernel(
    DevScene sc, DevCamera cam, DevParams P, const uint32_t *tiles, DevLights nl, DevEnv ev) {
    constexpr bool PROF = false, ONE_TREE = false;
    constexpr int INSTL = 0;
#include "rtmi_kernel_coop.inc"
}

hipError_t rtmi_light_coop_launch_render(bool tile_list, bool sig, bool ext, bool nee, bool env, uint32_t blocks, size_t lds,
                                         hipStream_t stream, const DevScene &sc, const DevCamera &cam, const DevParams &P,
                                         const uint32_t *tiles, const DevLights &L, const DevEnv &E) {
    const dim3 grid(blocks), block(64 * WAVES_PER_BLOCK);
    return rtmi_with_bools([&](auto TL, auto SIG, auto EXT, auto NEE, auto ENV) {
        if constexpr ((!NEE() && !ENV()) || (TL() && SIG())) return hipErrorInvalidValue; // the plain estimator is rtmi_render_coop's
        else {
            return rtmi_launch_lds(&rtmi_light_coop_kernel<TL(), SIG(), EXT(), NEE(), ENV()>, grid, block, lds, stream, sc, cam,
                                   P, tiles, L, E);
        }
    }, tile_list, sig, ext, nee, env);
}
