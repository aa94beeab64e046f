// rtmi_render_launch.hpp — launchers of the plain render's kernels (include/rtmi.h): the render kernels, the resolve, the
// end of a pass and the four probes.  Defined in rtmi_device.hip, next to the instantiations, and called by the host side
// of the plain render (render_device_locked, the probe entries) and by run_passes (rtmi_host.hpp): the host names no kernel
// of that unit, as with every other mode's *_launch.hpp.  C++ linkage, hidden: nothing here is exported.
#pragma once

#include "rtmi_types.hpp"
#include "rtmi_hostkit.hpp"

// The choices of one plain render call, as render_device_locked computes them from the scene and the flags; the launcher
// only turns them into the kernel instantiation.
struct RenderLaunch {
    bool bcoop, coop, async; // workgroup-cooperative, wave-cooperative, asynchronous state machine; none: per-lane two-phase
    bool inst, insd;         // the INSTL = 1 / 2 instantiations of the cooperative kernel (rtmi_kernels.hpp)
    bool prof, sigf, fast;   // RTMI_FLAG_PROFILE, RTMI_FLAG_PATH_SIG, fast-cull with valid boxes
    bool ext, one_tree;      // the cooperative kernel's pool form; its one-tree instantiation (rtmi_onetree.hip)
    uint32_t wps;            // requested waves per SIMD (0 = default; 3 and 5 have instantiations)
    size_t coop_lds, bcoop_lds, dyn_lds; // dynamic LDS of a block: cooperative, workgroup-cooperative, asynchronous
};
// One pass of `blocks` workgroups on `stream`.  The cooperative kernel has no instantiation for inst with prof: the host
// refuses that call before it comes here.
RTMI_HIDDEN hipError_t rtmi_render_launch(const RenderLaunch &k, uint32_t blocks, hipStream_t stream, const DevScene &sc,
                                          const DevCamera &cam, const DevParams &P);
// the pass's samples onto the f64 sums; the texels after the last pass, or after every pass with `progressive`
RTMI_HIDDEN hipError_t rtmi_render_launch_resolve(hipStream_t stream, const Rad3 *samples, double *partial, rtmi_texel *out,
                                                  const DevParams &P, bool first, bool last, bool progressive);
// end of a pass of `units` units and `pass_spp` samples (the status words, rtmi_types.hpp); last: the call's last pass
RTMI_HIDDEN hipError_t rtmi_render_launch_pass_end(hipStream_t stream, unsigned int *status, unsigned int units,
                                                   unsigned int pass_spp, bool last);

// the probes of rtmi.h on device arrays, on the null stream
RTMI_HIDDEN hipError_t rtmi_render_launch_probe_math(int op, const float *x, const float *y, float *out, uint32_t n);
RTMI_HIDDEN hipError_t rtmi_render_launch_probe_xform(const rtmi_xform *xf, int count, const float *a, const float *b, float *out,
                                                      uint32_t n);
RTMI_HIDDEN hipError_t rtmi_render_launch_probe_philox(const uint32_t *ctr, const uint32_t *key, uint32_t *out, uint32_t n);
RTMI_HIDDEN hipError_t rtmi_render_launch_probe_geom(int op, const DevScene &sc, const float *in, float *out, uint32_t n);
