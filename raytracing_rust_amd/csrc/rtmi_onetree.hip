// rtmi_onetree.hip — translation unit of the ONE-TREE instantiation of the cooperative render kernel: the headline
// instantiation <false, false, 4, true, 0> for scenes whose every BVH item carries an alternative tree and whose every
// medium is bounded by a static sphere (final_scene, random_spheres), rendered through those trees.  Of the four inlined
// copies of coop_bvh_query the general instantiation carries (the gated 4-wide walk, the binary walk of the
// reference-topology tree and the two boundary queries of a general medium) such a scene executes the first only; here
// the other three are not compiled (ONE_TREE, rtmi_kernel_coop.inc), which leaves the register allocator and the
// scheduler a third less function to serve.  A unit of its own, as rtmi_lean.hip is, so that the
// machine-scheduler strategy can be chosen for it alone (build.py: _RTMI_UNITS).  Device code only: the host stub
// defined here is what rtmi_device.hip launches through its `extern template` declaration.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "rtmi.h"
#include "rtmi_math.h"

#define RTMI_LEAN_TU 1 /* the plain kernels are defined in rtmi_device.hip */
#define RTMI_ONE_TREE_TU 1
#include "rtmi_kernels.hpp"

template __global__ void rtmi_render_coop<false, false, 4, true, 0, true>(DevScene, DevCamera, DevParams);
