// rtmi_probe_path_launch.hpp — launcher of the path probe (rtmi_probe_path, include/rtmi.h), defined in
// rtmi_probe_path.hip and called by the entry point in rtmi_device.hip.  C++ linkage, hidden: nothing here is exported.
#pragma once

// the n cases of one call on the device
struct PathProbe {
    const DevCamera *cams;     // CAMERA: the cameras the cases index
    const rtmi_xform *xforms;  // XFORM_ROUNDTRIP: the chains the cases index
    const float *in;           // [n][RTMI_PROBE_PATH_IN]
    const uint32_t *words;     // [n][RTMI_PROBE_PATH_WORDS]: each case's script
    float *out;                // [n][RTMI_PROBE_PATH_OUT]
    uint32_t n;
    DevScene sc;               // BOUNCE: the uploaded scene; max_depth and ext (RTMI_EXT_*) as a render's DevParams hold them
    uint32_t max_depth, ext;
};

__attribute__((visibility("hidden"))) hipError_t rtmi_probe_path_launch(int op, const PathProbe &B);
// rtmi_probe_stream: n lanes follow script [n][steps] on the word source `kind` under the key (k0, k1); out [n][steps][3]
__attribute__((visibility("hidden"))) hipError_t rtmi_probe_stream_launch(int kind, uint32_t k0, uint32_t k1, const uint8_t *script,
                                                                          uint32_t steps, uint32_t *out, uint32_t n);
