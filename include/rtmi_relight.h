/* rtmi_relight.h — the light table and the light tree follow a scene update on the device.
 *
 * rtmi_update.h detaches the attached light table, and the tree over it, when an update moves an emitter: both hold copies
 * of the emitters' geometry.  A handle that FOLLOWS its lights (rtml_scene_follow_lights) keeps them attached instead: the
 * update enqueues one more kernel behind its scatter and refit kernels, on the same stream and in front of the handle's
 * busy event, which recomputes the table from the moved planes and refits the tree.  Opt-in per handle; without it every
 * byte and every answer of rtmi_update.h is what it was.
 *
 * The rules (csrc/rtmi_relight.hpp; the kernel and rtml_relight_desc compile the same functions).  All arithmetic is f64
 * from the description's floats widened; each operation is rounded once and nothing is fused.
 *   Per light: rect   area = (a1 - a0) * (b1 - b0);  sphere   area = ((4.0 * pi) * r) * r;  aw = area * weight.
 *   Table:     total = the sum of aw in table order; select_p = aw / total; cdf = the running sum of select_p in table
 *              order, the last entry exactly 1.  On the device geo and k are planes A and B of the primitive, area, p_sel
 *              and cdf the f64 values rounded once to float; plane, item, prim and the padding keep their bytes, and so does
 *              the per-primitive light index.
 *   Tree leaf: the box of the tree's build (a rect's is degenerate on its plane's axis, a sphere's is c +- r); power = aw.
 *   Interior:  lo, hi = the union of the two children's f64 boxes, left first, with min(a, b) = b < a ? b : a and
 *              max(a, b) = b > a ? b : a; power = left + right in f64.
 *   Every node: c = (float)((lo + hi) * 0.5); with h = (hi - lo) * 0.5, r2 = (float)((h.x * h.x + h.y * h.y) + h.z * h.z);
 *              the link and the padding keep their bytes.  The paths are not touched.
 *
 * What follows from them.
 *   The TABLE after an update is, byte for byte, what rtmi_scene_attach_lights uploads for the edited description whenever
 *   the membership of the table is unchanged.  The table does not depend on any topology.
 *   The TREE keeps the topology that the host build chose for the old positions.  Every topology gives a consistent pick
 *   and pmf (the probability a pick returns is the pmf of the light it returns), so the estimator stays unbiased; the tree
 *   equals a fresh build only where that build would choose the same splits.  It is DEFINED by rtml_relight_desc.
 *   A refit of unchanged planes reproduces the attached bytes: min, max and the union of boxes are exact, and the power
 *   sums run in the build's own order.  One exception: where coordinates +0 and -0 meet in a union, the sign of a zero in c
 *   may differ from the build's (which unites a set in index order).  No importance reads it differently: c enters only
 *   through (c - x)^2.
 *   Membership never changes: an emitter that was not in the table stays counted by BSDF sampling, and a listed light
 *   must stay a light (below).
 *
 * Names.  The entries carry the prefix rtml_ and their own tables in the bindings (abi.py: RELIGHT_ENTRIES; sys.rs: its own
 * block), as rtmu_ does.  The tree's nodes are passed as untyped memory: 32 bytes each, the node layout of the header that
 * declares the tree (this header includes rtmi_nee.h alone).
 */
#ifndef RTMI_RELIGHT_H
#define RTMI_RELIGHT_H

#include "rtmi_nee.h"

#ifdef __cplusplus
extern "C" {
#endif

/* on != 0: the handle follows its lights from now on.  Needs an attached light table (RTMI_ERR_INVALID without one);
 * RTMI_ERR_UNSUPPORTED for a handle with f64 planes attached (an update refuses those anyway); a multi-GPU handle has no
 * update entry and none of these (the host library answers Unsupported for a scene resident on a device list).  Does the one-time work, as
 * rtmu_scene_update_prepare does: waits for the calls enqueued on the handle, builds the update tables when they are
 * missing, reads the attached table (and the tree, when one is attached) back, builds per light its f64 weight, the tree's
 * slots by depth, deepest first, and a scratch of 7 doubles per slot, and allocates.  Idempotent.
 * While on: an rtmu_scene_update_prims / _device whose range holds an emitter keeps the table and the tree attached and
 * enqueues the relight kernel; it allocates nothing and synchronises nothing; a range without emitters enqueues nothing
 * more than before.  The blocking form also refuses, with RTMI_ERR_INVALID and before any enqueue, new planes that make a
 * listed light of the range degenerate (the list under rtml_relight_desc); in the device form that is the caller's
 * contract.  Attaching a new light table or a new tree to the handle turns following off: the tables index the old one.
 * on == 0: following off, the behaviour of rtmi_update.h. */
int rtml_scene_follow_lights(rtmi_scene *scene, int on);

/* Pure host code, initialises no device.  desc holds the ALREADY EDITED planes; lights[n_lights] is the table of the old
 * description: item, prim, kind, material and weight are kept, area, select_p and cdf are rewritten.  nodes is the old
 * tree (n_nodes = 2 * n_lights nodes of 32 bytes), or NULL with n_nodes = 0: the links are kept, c, r2 and power rewritten.
 * RTMI_ERR_INVALID for a NULL desc or table, a table entry outside the description or of another primitive type than its
 * kind, a tree that fails the checks of the host walks (a link that leaves the array, an odd or too small n_nodes) or
 * with n_nodes != 2 * n_lights, and a listed light that its new planes make degenerate: a rect with a0 >= a1 or b0 >= b1,
 * a sphere with r <= 0 or a centre that is not finite, an area * weight that is not finite. */
int rtml_relight_desc(const rtmi_scene_desc *desc, rtmi_light *lights, uint32_t n_lights, void *nodes, uint32_t n_nodes);

/* Test hook with the semantics of rtmu_probe_scene_words: copies one of the handle's light arrays to the host after the
 * calls enqueued on the handle have finished.  An array the handle does not have attached has size 0. */
enum { RTML_WORDS_LIGHTS = 0,      /* lights x 48 B: geo[4], k, plane, item, prim, area, p_sel, cdf, pad */
       RTML_WORDS_PRIM_LIGHT = 1,  /* n_prims x 4 B: the light of a primitive, or -1 */
       RTML_WORDS_TREE_NODES = 2,  /* 2 * lights x 32 B */
       RTML_WORDS_TREE_PATHS = 3 };/* lights x 8 B */
int rtml_probe_light_words(rtmi_scene *scene, int which, void *out, size_t cap, size_t *need);

#ifdef __cplusplus
}
#endif
#endif /* RTMI_RELIGHT_H */
