// rtmi_f64_types.hpp — device views of the f64 render mode (include/rtmi_f64.h) and the launchers of its kernels.
// The kernels live in rtmi_f64.hip (rtmi_f64_kernels.hpp); the handle glue in rtmi_device.hip calls them through these.
#pragma once
#include "rtmi_types.hpp"
#include "rtmi_f64.h"

struct D3 {
    double x, y, z;
};
// the attached planes on the device (rtmi_scene_f64, same indices as the fp32 description)
struct DevSceneF64 {
    const double *prim_a, *prim_b, *prim_dt, *nodes, *xforms, *item_nid, *item_root, *mparam, *texf, *ranvec;
};
struct DevCameraF64 {
    D3 origin, llc, horizontal, vertical, u, v;
    double time0, time1, lens_radius;
};
struct DevParamsF64 {
    double t_min;
    double *samples; // [local tile][pass_stride][64] x 3 doubles (RTMI_SAMPLE_SLOT_BYTES_F64 per slot)
};

hipError_t rtmi_f64_launch_render(bool sig, uint32_t blocks, hipStream_t stream, const DevScene &sc, const DevSceneF64 &w,
                                  const DevCameraF64 &cam, const DevParams &P, const DevParamsF64 &Q);
hipError_t rtmi_f64_launch_resolve(hipStream_t stream, const double *samples, double *acc, double *out_lin, uint32_t *out_q,
                                   const DevParams &P, int first, int last);
hipError_t rtmi_f64_launch_probe(int op, const double *x, const double *y, double *out, uint32_t n);
