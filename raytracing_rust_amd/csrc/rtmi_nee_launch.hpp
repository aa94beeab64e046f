// rtmi_nee_launch.hpp — launcher of the next-event-estimation kernels (include/rtmi_nee.h), defined in rtmi_nee.hip and
// called by rtmi_render_nee in rtmi_device.hip.  The resolve is adaptive sampling's (rtmi_adaptive_launch.hpp) over the
// list of all tiles: the render's sums plus Welford's standard errors.
#pragma once

hipError_t rtmi_nee_launch_render(bool fast, bool sig, uint32_t blocks, hipStream_t stream, const DevScene &sc,
                                  const DevCamera &cam, const DevParams &P, const DevLights &L);
