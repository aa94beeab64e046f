// rtmi_window_launch.hpp — launcher of the spread kernel of windowed adaptive sampling (include/rtmi_window.h), defined in
// rtmi_window.hip and called by the rtmi_render_window entries, rtmi_window_spread_device and the probe in rtmi_batch.hip.
#pragma once

#define RTMI_WINDOW_RADIUS_MAX 16u // RTMI_WINDOW_MAX_RADIUS of the header; the kernel's LDS is sized by it

// active[p] = active[p] != 0 && a fail byte != 0 within the clipped (2 * radius + 1)^2 window of p; nx * ny >= 1 pixels,
// radius <= RTMI_WINDOW_RADIUS_MAX (the callers check both)
hipError_t rtmi_window_launch_spread(hipStream_t stream, uint8_t *active, const uint8_t *fail, uint32_t nx, uint32_t ny, uint32_t radius);
