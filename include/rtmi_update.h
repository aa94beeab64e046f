/* rtmi_update.h — edits of a resident scene: move primitives and refit the trees on the device.
 *
 * rtmi.h calls a handle's device copy read-only after creation; these entries are the exception.  The caller supplies new
 * planes A / B (rtmi.h, "primitives") for a contiguous range of primitives; the handle rewrites every derived copy it keeps
 * of them and refits both trees of every BVH item the range touches, bottom-up, on the GPU.  Nothing is reallocated: every
 * handle that the later headers bind to the scene stays valid and sees the moved scene in its next call.
 * Primitive types, materials, flags and all topology stay fixed; only float payload changes.
 *
 * Contract.  After rtmu_scene_update_prims*, every byte of every device array of the handle equals what rtmi_scene_create
 * uploads for this description: the handle's description with the new planes written in, passed through rtmu_refit_desc with
 * the same range.  Every call that reads the scene therefore gives the bits it gives on such a fresh handle, on
 * every kernel.  The refit rules are fp32 and stated in csrc/rtmi_refit.hpp; against a fresh LOWERING of the moved geometry
 * (f64, rounded once) a box coordinate may differ by a few ulp of the item's scale — far inside the padding of the culling
 * boxes; a gate changes only for a ray that grazes a node box within that rounding.  The tree topology is kept: it is the
 * one the lowering chose for the old positions, and traversal slows as the primitives move far from them.
 *
 * What may be updated.  Primitives of LIST items, all four types (they sit under no box) — also a medium's boundary sphere
 * and emitters.  Primitives of REFITTABLE BVH items: not DEFERRED, not SAVE_T0; scale < 1e30 (prunable); an alternative tree,
 * or fewer than two primitives; every leaf a SPHERE or a CUBE without a transform chain of its own; no list as a child of a
 * node.  A touched item is refit whole; untouched items keep every byte.  A range that touches another BVH item, or a member
 * of a deferred group, is RTMI_ERR_UNSUPPORTED before any device work; so is a handle with f64 planes attached (they would go
 * stale).  An rtmi_multi handle has no update entry.
 *
 * Lights.  The light table and the light tree hold copies of the emitters' geometry.  An update whose range holds a
 * primitive with a DIFFUSE_LIGHT material detaches both; rtmi_render_nee then refuses ("no lights attached") until the
 * caller attaches them again from the refit description.  Flips and the environment map are unaffected.
 *
 * Names.  The entries carry the prefix rtmu_: they are the one family that writes to a resident scene, kept apart from the
 * render entries (rtmi_*) in name and in the binding tables (abi.py: UPDATE_ENTRIES; sys.rs: its own block).
 *
 * Ordering.  An update is a call on the handle like a render: it takes the handle's mutex, starts after the previous call
 * on the handle has finished and a later call starts after it (rtmi.h, thread model).
 */
#ifndef RTMI_UPDATE_H
#define RTMI_UPDATE_H

#include "rtmi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Which items rtmu_scene_update_prims can refit: mask[n_items], 1 = a refittable BVH item, 0 = not (LIST items are 0:
 * they need no refit).  Pure host code, initialises no device. */
int rtmu_refittable(const rtmi_scene_desc *desc, uint8_t *mask);

/* Pure host code, initialises no device.  desc holds the ALREADY EDITED prim planes and the unchanged topology; the refit
 * boxes of every refittable item that owns a primitive of [first, first + count) are written to the caller's arrays (same
 * sizes as desc's; they may be desc's own arrays): items[].root_min / root_max / scale, nodes[] boxes, alt_nodes[] boxes,
 * prim_gate[] (may be NULL when desc has none).  Everything else is left as it is.  count == 0 does nothing.
 * RTMI_ERR_INVALID for a NULL array, a range outside the primitives or a tree that leaves its array or reaches a node
 * twice; RTMI_ERR_UNSUPPORTED for a range that touches what cannot be updated (above). */
int rtmu_refit_desc(const rtmi_scene_desc *desc, uint32_t first, uint32_t count, rtmi_item *items, rtmi_bvh_node *nodes,
                    rtmi_bvh4_node *alt_nodes, float *prim_gate);

/* New planes for the primitives [first, first + count): a, b = count * 4 floats each (b may be NULL: planes B unchanged).
 * Blocking: copies through the handle's pinned staging and returns when the device arrays are rewritten.  Rejects with
 * RTMI_ERR_INVALID, before any enqueue, inside a refittable item: a non-finite value the refit reads (plane A; a cube's
 * max.y, max.z in plane B), a non-positive sphere radius and an inverted cube (min > max; with b NULL the resident plane B
 * is not read: max.y and max.z go unchecked).  The planes of list primitives are taken as rtmi_scene_create takes them. */
int rtmu_scene_update_prims(rtmi_scene *scene, uint32_t first, uint32_t count, const float *a, const float *b);
/* The first update of a handle, of either form and of the transform entry too, builds the handle's tables: it waits for
 * the calls enqueued on the handle, reads the topology back from the device and allocates.  This entry does that ahead of
 * time, so that a frame loop's first rtmu_scene_update_prims_device is as asynchronous as the later ones.  Idempotent. */
int rtmu_scene_update_prepare(rtmi_scene *scene);
/* The same from DEVICE memory (4-byte aligned), asynchronous on `stream` (a hipStream_t, may be NULL): the planes never
 * visit the host.  The buffers must stay valid and unchanged until the stream has passed the call.  After the handle's
 * first update (or rtmu_scene_update_prepare) it neither allocates nor synchronises; the first one does both (above).
 * The values are the CALLER'S CONTRACT: inside refittable items finite planes, non-zero radii and min <= max for cubes —
 * nothing on the device checks them, and boxes derived from others are meaningless.  A negative radius is the hollow
 * sphere of the reference (its node box is the inverted one of Sphere::bounding_box, its culling boxes take |r|, as in
 * the lowering); the blocking form refuses it all the same. */
int rtmu_scene_update_prims_device(rtmi_scene *scene, uint32_t first, uint32_t count, const void *d_a, const void *d_b, void *stream);

/* Replaces the transform records [first, first + count) (rtmi.h, "instance transforms"; host pointer, a handful of
 * records), blocking.  Every record must keep its kind, which must be TRANSLATE or ROTATE_*, hold finite values, and lie in
 * the chain of an item that neither heads nor belongs to a deferred group (their chains are copied in front of the group's),
 * or in the chain of a primitive of such a LIST item: RTMI_ERR_INVALID for the first three, RTMI_ERR_UNSUPPORTED for a record
 * of a deferred group, for a record of a primitive inside a BVH item (its boxes depend on it) and for a handle with f64
 * planes attached.  The item records' copies of their first two transforms follow.  No tree changes: items sit in a list,
 * not under a box. */
int rtmu_scene_update_xforms(rtmi_scene *scene, uint32_t first, uint32_t count, const rtmi_xform *recs);

/* Test hook: copies one of the handle's device arrays to the host, after the calls enqueued on the handle have finished.
 * *need (optional) receives its size in bytes; with out == NULL nothing else happens; RTMI_ERR_INVALID when cap is smaller.
 * An array the scene does not have (GATE without prim_gate, ALT_NODES without alternative trees) has size 0. */
enum { RTMI_SCENE_WORDS_ITEMS = 0,      /* n_items x 96 B: the item record and its first two transforms */
       RTMI_SCENE_WORDS_PRIM_A = 1, RTMI_SCENE_WORDS_PRIM_B = 2, /* n_prims x 16 B */
       RTMI_SCENE_WORDS_GATE = 3,       /* n_prims x 32 B */
       RTMI_SCENE_WORDS_NODES = 4,      /* n_nodes x 64 B, children pool-encoded in pad[] */
       RTMI_SCENE_WORDS_ALT_NODES = 5,  /* n_alt_nodes x 128 B, children pool-encoded, empty slots saturated */
       RTMI_SCENE_WORDS_LEAF_REC = 6,   /* n_prims x 80 B: A, B, meta, gate */
       RTMI_SCENE_WORDS_SHADE_PRIM = 7, /* n_prims x 64 B: A, material record, texture record */
       RTMI_SCENE_WORDS_XFORMS = 8 };   /* n_xforms x 16 B */
int rtmu_probe_scene_words(rtmi_scene *scene, int which, void *out, size_t cap, size_t *need);

#ifdef __cplusplus
}
#endif
#endif /* RTMI_UPDATE_H */
