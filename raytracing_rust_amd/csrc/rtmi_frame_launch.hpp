// rtmi_frame_launch.hpp — the seams of the frame pipeline (include/rtmi_frame.h): the device halves of the existing stages,
// defined in rtmi_device.hip, rtmi_temporal.hip and rtmi_denoise.hip and called by the frame handle in rtmi_frame.hip.  The
// one-shot entries are these halves followed by their copies to the host.  C++ linkage, hidden: nothing here is exported.
// See DESIGN.md §28.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rtmi.h"
#include "rtmi_carve.hpp"
#include "rtmi_denoise.h"
#include "rtmi_temporal.h"

#define RTMI_SEAM __attribute__((visibility("hidden")))

// ---- rtmi_device.hip: the two renders, "enqueue, wait and check overflow, result left in the scene's device buffers" ----
// the lit render of a frame: the plain estimator is rtmi_render_adaptive with min_spp == ns and step_spp == 1, the others
// are the fixed render of rtmi_render_nee and rtmi_render_env
struct RtmiFrameLit {
    const char *name;   // the entry point, prefix of the refusals
    bool nee, env;      // reads the light table / the map
    float env_select_p; // read with both
};
// One frame call's hold on its scene: the scene's lock from begin to end and the busy mark recorded at the end, so no
// other render of the scene runs between the stages.
struct RtmiFrameHold;
// begin_call of the one-shot entries: the NULL scene, the lock, what the estimator needs attached, the device, no earlier
// render of the handle running.  *hold is NULL after a failure.
RTMI_SEAM int rtmi_frame_hold_begin(rtmi_scene *s, const RtmiFrameLit &m, RtmiFrameHold **hold);
RTMI_SEAM void rtmi_frame_hold_end(RtmiFrameHold *hold); // records the busy mark on the scene's stream, unlocks; NULL allowed
// p: checked by the caller as the one-shot entries check it.  The result stays in the buffers of rtmi_frame_planes.
RTMI_SEAM int rtmi_frame_enqueue_lit(RtmiFrameHold *hold, const RtmiFrameLit &m, const rtmi_camera *cam,
                                     const rtmi_render_params &p, rtmi_stats *stats);
RTMI_SEAM int rtmi_frame_enqueue_first_hits(RtmiFrameHold *hold, const rtmi_camera *cam, const rtmi_render_params &p);
// what the two renders left on the scene's device; valid until the next call on the scene
struct RtmiFramePlanes {
    int device;
    hipStream_t stream;        // the scene's own stream
    const rtmi_texel *texels;  // [tile][64], tiles counted from the top-left
    const float *tiled_stderr; // [tile][64][3]
    const float *albedo, *normal, *depth; // packed, row-major, row 0 = top
    const uint32_t *hits;
};
RTMI_SEAM RtmiFramePlanes rtmi_frame_planes(const RtmiFrameHold *hold, const rtmi_render_params &p);

// ---- rtmi_temporal.hip: the push on device planes -------------------------------------------------------------------
// the history of rtmi_temporal.h (96 B per pixel) in memory its owner allocated, and the previous camera
struct RtmiTemporalHistory {
    float4 *col[2] = {}, *geo[2] = {}, *var[2] = {};
    int cur = 0; // the copy that holds the previous frame
    bool has_prev = false;
    rtmi_camera prev_cam{};
    float prev_m[9] = {};
};
// the six planes of H as pieces of its owner's allocation, in the order col, geo, var of copy 0, then of copy 1
RTMI_SEAM void rtmi_temporal_history_layout(RtmiTemporalHistory &H, Carve256 &c, uint32_t nx, uint32_t ny);
// the RTMI_ERR_INVALID checks of rtmi_temporal_create (sizes, ranges, reserved words) in `name`'s words; the flags are the
// caller's to check
RTMI_SEAM int rtmi_temporal_check_ranges(const char *name, uint32_t nx, uint32_t ny, const rtmi_temporal_params *p);
// the camera checks of rtmi_temporal_push (finite fields, step 4's matrix in double) in `name`'s words; m: the inverse
RTMI_SEAM int rtmi_temporal_camera_matrix(const char *name, const rtmi_camera *cam, float m[9]);
// One push, enqueued on `stream`: reads H's previous copy and the device planes, writes the other copy and the outputs
// (all on the stream's device; se and out_se NULL together).  H is advanced by rtmi_temporal_history_advance once the
// caller knows the work completed.
RTMI_SEAM hipError_t rtmi_temporal_push_launch(hipStream_t stream, uint32_t nx, uint32_t ny, const rtmi_temporal_params &params,
                                               const RtmiTemporalHistory &H, const rtmi_camera *cam, const float *linear,
                                               const float *albedo, const float *normal, const float *depth, const float *se,
                                               float *out_linear, float *out_se, float *out_hist, float2 *out_motion);
RTMI_SEAM void rtmi_temporal_history_advance(RtmiTemporalHistory &H, const rtmi_camera *cam, const float m[9]);

// ---- rtmi_denoise.hip: prepass, iterations and finish on device planes ----------------------------------------------
// the RTMI_ERR_INVALID checks of rtmi_denoise (sizes and ranges), each message after `prefix`; the flags are the caller's
RTMI_SEAM int rtmi_denoise_check_ranges(const char *prefix, uint32_t nx, uint32_t ny, const rtmi_denoise_params *p);
// the filter's working planes: the two states the iterations ping-pong between, the guide and the depth gradient
struct RtmiDenoisePlanes {
    float4 *state[2] = {}, *guide = nullptr;
    float2 *grad = nullptr;
};
// W as pieces of its owner's allocation; a filter with 0 iterations takes none and leaves W's pointers NULL
RTMI_SEAM void rtmi_denoise_layout(RtmiDenoisePlanes &W, Carve256 &c, uint32_t nx, uint32_t ny, uint32_t iterations);
// The launches of rtmi_denoise on `stream`: inputs, working planes and outputs on the stream's device; se may be NULL (no
// luminance weight), normal is read by the filter only.  out: [ny][nx][3] floats, rgb8: [ny][nx][3] bytes.
RTMI_SEAM hipError_t rtmi_denoise_launch(hipStream_t stream, uint32_t nx, uint32_t ny, const rtmi_denoise_params &p,
                                         const float *linear, const float *albedo, const float *normal, const float *depth,
                                         const float *se, const RtmiDenoisePlanes &W, float *out, uint8_t *rgb8);
