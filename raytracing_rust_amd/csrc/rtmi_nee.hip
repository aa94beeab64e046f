// rtmi_nee.hip — translation unit of next-event estimation (include/rtmi_nee.h): the NEE kernels and their launcher.
// Compiled with the flags of rtmi_device.hip (-ffp-contract=off).
//
// The NEE kernel is the body of rtmi_render_kernel (rtmi_kernel_perlane.inc) with NEE = true: same work queue,
// camera_sample, item scan and two-phase schedule.  Phase B of a path lane that scatters at a Lambertian or Isotropic
// vertex draws a light sample (shade_hit<.., NEE = true>) and turns the lane into a shadow ray, keeping the continuation
// aside; phase A traces it with the light-sample stream swapped in; phase B adds its contribution when the closest hit
// is the sampled light (the texture lookup is the wave-cooperative one) and restores the continuation.  Instantiated
// for FAST x SIG.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "rtmi.h"
#include "rtmi_math.h"

#define RTMI_LEAN_TU 1 /* the plain kernels are defined in rtmi_device.hip */
#include "rtmi_kernels.hpp"
#include "rtmi_light_launch.hpp"

template <bool FAST, bool SIG>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void rtmi_nee_kernel(DevScene sc, DevCamera cam, DevParams P, DevLights nl) {
    constexpr bool PROF = false, TILE_LIST = false, FEATURES = false, NEE = true, ENV = false;
    const DevEnv ev{};
    const uint32_t *const tiles = nullptr;
#include "rtmi_kernel_perlane.inc"
}

hipError_t rtmi_nee_launch_render(bool fast, bool sig, uint32_t blocks, hipStream_t stream, const DevScene &sc,
                                  const DevCamera &cam, const DevParams &P, const DevLights &L) {
    const dim3 grid(blocks), block(64 * WAVES_PER_BLOCK);
    return rtmi_with_bools([&](auto FAST, auto SIG) {
        hipLaunchKernelGGL((rtmi_nee_kernel<FAST(), SIG()>), grid, block, 0, stream, sc, cam, P, L);
        return hipGetLastError();
    }, fast, sig);
}
