/* rtmi_roulette_coop.h — Russian-roulette renders (include/rtmi_roulette.h) on the wave-cooperative kernel of rtmi_render,
 * on the MI355X (gfx950) device path.  See DESIGN.md §20.
 *
 * RTMI_FLAG_ROULETTE_COOP is an opt-in flag of rtmi_render_roulette and rtmi_render_adaptive_roulette, for all four
 * RTMI_ROULETTE_* estimators.  Without it these entries run the per-lane kernel, as they always did.  It is a bit of its
 * own: the roulette entries keep refusing RTMI_FLAG_LIGHT_COOP (include/rtmi_light_coop.h), alone or beside this flag.
 *
 * Same result.  With the flag linear, rgb8, stderr, bounces and spp are bit for bit what the same call returns without
 * it: a lane runs the per-lane roulette kernel's program in that kernel's order, the roulette test, its stream-4 draw and
 * the bounce count included; only the BVH traversal inside its item scan is shared by the wavefront.  rtmi_stats.kernel
 * and the timings differ, nothing else.
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
 * all the time), is accepted by the two entries together with this flag only; alone it is refused as before.  PATH_SIG,
 * PROFILE, ASYNC, BLOCK_COOP, PROGRESSIVE and TEST_OVERFLOW stay refused beside the flag, and every check of
 * rtmi_roulette.h keeps its order, code and text.  A traversal-pool overflow is reported as rtmi_render reports it:
 * poisoned texels and RTMI_ERR_DEVICE.
 *
 * Every other entry point answers the flag as it answers an unknown flag bit: rtmi_render_nee, rtmi_render_env,
 * rtmi_render_adaptive_nee, rtmi_render_adaptive_env, rtmi_render_features and rtmi_render_adaptive return
 * RTMI_ERR_UNSUPPORTED.
 *
 * Speed: DESIGN.md §20, Timing (tools/roulette_coop_timing.py).  The flag is opt-in; making it the default is a later
 * decision.
 */
#ifndef RTMI_ROULETTE_COOP_H
#define RTMI_ROULETTE_COOP_H

#include "rtmi.h"
#include "rtmi_roulette.h"

#define RTMI_FLAG_ROULETTE_COOP 131072u /* bit 17 of rtmi_render_params.flags */

#endif /* RTMI_ROULETTE_COOP_H */
