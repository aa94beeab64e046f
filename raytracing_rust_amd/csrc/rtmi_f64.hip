// rtmi_f64.hip — translation unit of the f64 render mode (include/rtmi_f64.h): the kernels of rtmi_f64_kernels.hpp and
// their launchers.  Compiled with the flags of the other translation units (-ffp-contract=off: no fused operations).
#include "rtmi_f64_kernels.hpp"

hipError_t rtmi_f64_launch_render(bool sig, uint32_t blocks, hipStream_t stream, const DevScene &sc, const DevSceneF64 &w,
                                  const DevCameraF64 &cam, const DevParams &P, const DevParamsF64 &Q) {
    if (sig) hipLaunchKernelGGL(rtmi_render_f64_kernel<true>, dim3(blocks), dim3(64), 0, stream, sc, w, cam, P, Q);
    else hipLaunchKernelGGL(rtmi_render_f64_kernel<false>, dim3(blocks), dim3(64), 0, stream, sc, w, cam, P, Q);
    return hipGetLastError();
}
hipError_t rtmi_f64_launch_resolve(hipStream_t stream, const double *samples, double *acc, double *out_lin, uint32_t *out_q,
                                   const DevParams &P, int first, int last) {
    const uint32_t n = P.ntiles_local * 64u;
    hipLaunchKernelGGL(rtmi_resolve_f64_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, samples, acc, out_lin, out_q, P, first, last);
    return hipGetLastError();
}
hipError_t rtmi_f64_launch_probe(int op, const double *x, const double *y, double *out, uint32_t n) {
    hipLaunchKernelGGL(rtmi_math_probe_f64_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, op, x, y, out, n);
    return hipGetLastError();
}
