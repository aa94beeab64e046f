/* rtmi_light_coop.h — next-event estimation (include/rtmi_nee.h), environment lighting (include/rtmi_env.h) and their
 * adaptive forms (include/rtmi_adaptive_nee.h) on the wave-cooperative kernel of rtmi_render, on the MI355X (gfx950)
 * device path.  See DESIGN.md §19.
 *
 * RTMI_FLAG_LIGHT_COOP is an opt-in flag of rtmi_render_nee, rtmi_render_env, rtmi_render_adaptive_nee and
 * rtmi_render_adaptive_env.  Without it these entries run the per-lane kernel, as they always did.
 *
 * Same result.  With the flag every output plane of the four entries (linear, rgb8, stderr, spp, path signatures) is bit
 * for bit what the same call returns without it: a lane runs the per-lane kernel's program in the per-lane kernel's
 * order, only the BVH traversal inside its item scan is shared by the wavefront.  rtmi_stats.kernel and the timings
 * differ, nothing else.
 *
 * Selection.  The cooperative kernel runs (stats.kernel = RTMI_KERNEL_WAVE_COOP) when all of these hold:
 *   - the flag and RTMI_FLAG_FAST_CULL are set (the cooperative traversal is the fast-cull one);
 *   - the camera's shutter interval lies inside the scene's BVH time range;
 *   - RTMI_FLAG_SYNC is not set;
 *   - the scene is within the size limits of the cooperative kernel (n_prims < 2^22, n_nodes and n_alt_nodes < 2^25);
 *   - the scene has neither instanced primitives nor media under outer transforms or among a BVHNode's children
 *     (the rule of rtmi_render_adaptive).
 * Fallback.  Otherwise the call runs the per-lane kernel (stats.kernel = RTMI_KERNEL_PERLANE) and succeeds, with the same
 * bits.
 *
 * RTMI_FLAG_REF_TREE keeps its meaning: the cooperative kernel walks the reference-topology tree instead of the gated
 * 4-wide one.  Bit 11 of flags, the small-pool test knob of rtmi_render (a 256-entry LDS pool that spills to global memory
 * all the time), is accepted by the four entries together with this flag only; alone it is refused as before.  A
 * traversal-pool overflow is reported as rtmi_render reports it: poisoned texels and RTMI_ERR_DEVICE.
 *
 * Every other entry point answers the flag as it answers an unknown flag bit: rtmi_render_roulette,
 * rtmi_render_adaptive_roulette, rtmi_render_features and rtmi_render_adaptive return RTMI_ERR_UNSUPPORTED.
 *
 * Speed (Timing; tools/light_coop_timing.py, 64 spp on an MI355X): with the flag lit_final_scene renders
 * 1.59x faster, random_spheres under a map 1.89x (nee = 0) and 1.94x (nee = 1), scenes without a tree 1.04-1.09x, and
 * earth with nee = 0 is level.  It lost on no scene measured.  The flag is opt-in all the same; making it the default is
 * a later decision.
 */
#ifndef RTMI_LIGHT_COOP_H
#define RTMI_LIGHT_COOP_H

#include "rtmi.h"

#define RTMI_FLAG_LIGHT_COOP 65536u /* bit 16 of rtmi_render_params.flags */

#endif /* RTMI_LIGHT_COOP_H */
