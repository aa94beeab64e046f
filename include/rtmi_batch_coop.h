/* rtmi_batch_coop.h — the batch modes on the wave-cooperative kernel of rtmi_render, on the MI355X (gfx950) device
 * path.  The batch modes are the entries that trace paths for a batch of items instead of an image's tiles: the
 * radiance queries along caller rays, the hemisphere gathers about caller points, the renders and refinements of a list
 * of chosen pixels, and the two per-pixel adaptive renders that drive those (each pixel alone, or with a neighbourhood
 * stopping rule).  This header names them by what they do: each of their own headers keeps its names to itself.
 * See DESIGN.md §38, which lists the twelve functions.
 *
 * RTMI_FLAG_BATCH_COOP is an opt-in flag of every one of these entries, blocking and _device form alike, in the flags
 * word each of them already reads (their params' flags, or rtmi_render_params.flags).  Without it they run the per-lane
 * kernel, as they always did.
 *
 * Same result.  With the flag every output of the call (samples, mean, stderr, value, sh, linear, rgb8, spp, counts and
 * the patched planes) is bit for bit what the same call returns without it: a lane runs the per-lane kernel's program in
 * the per-lane kernel's order, only the BVH traversal inside its item scan is shared by the wavefront.  The kernel that
 * ran and the timings differ, nothing else.
 *   In-plane rays (include/rtmi_query.h).  A ray that starts in the plane of a rect or of a cube face with an infinite
 *     1 / d_k is accepted there with t = 0 * inf = NaN.  Below a BVH, under a pruned traversal, which accepted leaf is
 *     returned can differ between the two kernels when an accepted t is NaN: the per-lane kernel folds the accepted
 *     leaves in the order it reaches them, the cooperative one takes a minimum over order-preserving keys.  The two
 *     agree whenever no accepted t is NaN.
 *
 * Selection.  The cooperative kernel runs (RTMI_KERNEL_WAVE_COOP) when all of these hold:
 *   - the flag and RTMI_FLAG_FAST_CULL are set (the cooperative traversal is the fast-cull one);
 *   - the pruned traversal may run at all for this call, by the entry's own rule, which is not changed: for the
 *     radiance queries and the gathers the scene's BVH time range contains 0 (no time plane) or is unbounded (with
 *     one); for the camera modes the shutter interval lies inside the scene's BVH time range;
 *   - the scene is within the size limits of the cooperative kernel (n_prims < 2^22, n_nodes and n_alt_nodes < 2^25);
 *   - the scene has neither instanced primitives nor media under outer transforms or among a BVHNode's children
 *     (the rule of rtmi_light_coop.h).
 * Fallback.  Otherwise the call runs the per-lane kernel (RTMI_KERNEL_PERLANE) and succeeds, with the same bits.
 *
 * RTMI_FLAG_REF_TREE stays refused by these entries: the cooperative kernel walks the gated 4-wide tree where the scene
 * has one and the reference-topology tree otherwise.  Bit 11 of flags, the small-pool test knob of rtmi_render (a
 * 256-entry LDS pool that spills to global memory all the time), and RTMI_FLAG_TEST_OVERFLOW are accepted by these
 * entries together with this flag only; alone each is refused as before.  A traversal-pool overflow is a status word, not
 * a fault: the blocking forms return RTMI_ERR_DEVICE (their outputs are invalid), and rtmi_scene_status reports and
 * clears it for the _device forms.
 *
 * Which kernel ran.  The blocking per-pixel adaptive renders report it in rtmi_stats.kernel.  The other entries have no
 * stats and this header adds no function: their results do not depend on the kernel.  (RTMI_FLAG_TEST_OVERFLOW beside
 * the flag tells the two apart where a test must know: only the cooperative kernel reports an overflow.)
 *
 * Scratch.  The cooperative kernel's stack spills to a buffer of the handle, the one rtmi_render's cooperative kernel
 * uses.  It grows on the first cooperative call for a scene: the one allocation a _device form can make with the flag.
 * A caller who needs an allocation-free enqueue makes any cooperative call on the handle first (a blocking call with
 * this flag, or rtmi_render under RTMI_FLAG_FAST_CULL without RTMI_FLAG_REF_TREE); the buffer never shrinks.
 *
 * Every other entry point answers the flag as it answers an unknown flag bit.
 *
 * Speed: DESIGN.md §38, Timing; tools/batch_coop_timing.py.  The flag is opt-in whatever the numbers say.
 */
#ifndef RTMI_BATCH_COOP_H
#define RTMI_BATCH_COOP_H

#include "rtmi.h"

#define RTMI_FLAG_BATCH_COOP 2097152u /* bit 21 of the flags word of the batch entries */

#endif /* RTMI_BATCH_COOP_H */
