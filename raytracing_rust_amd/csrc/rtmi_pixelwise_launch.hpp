// rtmi_pixelwise_launch.hpp — launcher of the step kernel of per-pixel adaptive sampling (include/rtmi_pixelwise.h), defined in
// rtmi_pixelwise.hip and called by the rtmi_render_pixelwise entries in rtmi_batch.hip.
#pragma once

// one launch of the step kernel: the entries of a list, their pass records of the per-sample buffer, the image's state
struct PixelwiseStep {
    const uint32_t *list;  // [capacity] pixel indices into the planes
    const uint32_t *count; // the entries are min(count[0], capacity), read by the kernel; NULL: capacity
    const Rad3 *samples;   // [capacity][pass], entry-major
    double *state;         // [9][n_pixels]: sum r g b | m r g b | M2 r g b
    uint8_t *active;       // [n_pixels] or NULL, written with decide
    float *linear;         // [n_pixels][3] or NULL
    uint8_t *rgb8;         // [n_pixels][3] or NULL
    float *stderr_out;     // [n_pixels][3] or NULL
    uint32_t *spp;         // [n_pixels] or NULL
    uint32_t n_pixels, capacity;
    uint32_t n_done, pass; // samples every entry holds before this launch, and those it adds
    uint32_t decide, cap;  // decide: the launch ends a step
    double abs_tol, rel_tol;
};

hipError_t rtmi_pixelwise_launch_step(hipStream_t stream, const PixelwiseStep &S);
