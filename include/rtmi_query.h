/* rtmi_query.h — ray queries: closest hit and occlusion for batches of caller-supplied rays, on the MI355X (gfx950)
 * device path.  See DESIGN.md §23.
 *
 * Every render entry starts from the camera and returns pixels.  These entries hand out the operation all of them are
 * built on, the reference's world.hit(ray, t_min, t_max) (hittable.rs:37-47 and everything below it: the top-level list
 * scan, the BVHs, the instances and the constant media), for picking, visibility and ambient-occlusion terms, light
 * placement checks, or an integrator of the host's own on top of this traversal.
 *
 * Semantics.  For ray i of a batch, hit[i] is the Option<HitRecord> of world.hit(&Ray{o, d, time[i]}, t_min, t_max), in the
 * fp32 arithmetic contract, exactly as the render kernels evaluate it for a path ray.
 *   Random numbers.  Only ConstantMedium::hit draws.  Ray i draws from the Philox4x32-10 stream with the key
 *     (seed + first_ray + i) mod 2^64, counter (0, 0, 0, 0), stream id 0, in the order the reference's hit makes the draws:
 *     list order, BVH in-order, and the deferred / nested / list-scan media rules of rtmi.h.  first_ray makes the result
 *     independent of how a batch is split into calls.
 *   t_max.  +inf or any value >= FLT_MAX means the render's t_max, FLT_MAX.  t_min is the caller's; the render uses 0.001.
 *   Occlusion.  occluded[i] is 1 iff hit[i] is Some, bit for bit, with the same stream: the same predicate, evaluated by
 *     a scan that stops at the first accepted hit.
 *   Flags.  0 (the reference-topology traversal) and RTMI_FLAG_FAST_CULL (pruned; same results).  Every other bit is
 *     RTMI_ERR_UNSUPPORTED.  The pruned traversal needs the BVH boxes to hold at every ray time: with a time plane and a
 *     scene whose [bvh_time_lo, bvh_time_hi] is bounded, or without one when 0 lies outside that range, the exact
 *     traversal runs whatever the flag says.
 * The calls follow the handle's thread model (rtmi.h): calls on one handle serialise.  They allocate none of the
 * handle's render scratch: a handle that is only queried never gets a per-sample radiance buffer.
 */
#ifndef RTMI_QUERY_H
#define RTMI_QUERY_H

#include "rtmi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    float o[3], t_min, d[3], t_max;
} rtmi_ray; /* 32 B */

/* Miss: item = prim = material = -1, t = +inf, the rest 0.
 * Surface hit: item = the top-level item that won, prim = the primitive, material = prim_meta[prim].material, n = the
 *   record's normal after the transforms and FlipNormals, never face-forwarded, (u, v) = the record's, always computed.
 * Medium hit: prim = -1, material = items[item].medium_material, n = (1, 0, 0) handed back through the medium's outer
 *   wrappers and negated under RTMI_ITEMFLAG_FLIP, u = v = 0 (medium.rs:47-48).
 * The sign of a zero in n: negation and rotation commute in value but not in the sign of an exact zero, and the scene
 * description keeps only the parity of the FlipNormals around a primitive.  With the table of rtmi_scene_attach_flips
 * the flips are applied at their places among the Traslate / Rotate wrappers, as the reference applies them; without
 * it they are applied after all of them, and a zero component can carry the other sign. */
typedef struct {
    float t, u, v, p[3], n[3];
    int32_t item, prim, material;
} rtmi_hit; /* 48 B */

typedef struct {
    uint32_t n;         /* rays in this call */
    uint32_t flags;     /* 0 or RTMI_FLAG_FAST_CULL */
    uint64_t seed;
    uint64_t first_ray; /* index of this call's ray 0 in the caller's batch */
} rtmi_query_params; /* 24 B */

/* Optional: where the FlipNormals sit among the wrappers, so that rtmi_trace's normals have the reference's bits in
 * their zeros too.  prim_gaps[i], bit g: an odd number of flips between transforms g - 1 and g of primitive i's own chain
 * (outermost first; bit 0: outside the whole chain, where the flips of enclosing lists and tree nodes sit; bit count:
 * directly around the primitive); item_gaps[i] likewise for item i's chain, for a medium item the flips around the medium
 * only.  The parities must be those of RTMI_PRIMFLAG_FLIP and, for items that are no media, RTMI_ITEMFLAG_FLIP.  The
 * counts must be the scene's; the arrays are copied.  NULL arrays detach.  The host mirror's lowering produces the table
 * and rth_upload attaches it. */
int rtmi_scene_attach_flips(rtmi_scene *scene, const uint32_t *prim_gaps, uint32_t n_prims, const uint32_t *item_gaps,
                            uint32_t n_items);

/* Blocking, host pointers.  time: n floats, or NULL for time 0.  kernel_ms: optional, the kernel's time by HIP events.
 * n == 0 is RTMI_OK and launches nothing.  RTMI_ERR_INVALID, with the entry's name in rtmi_last_error(), for a NULL
 * scene, params, rays or output and for a ray with a non-finite component (t_max may be +inf), a zero direction or
 * t_min > t_max; the message names the ray.
 * Everything else is accepted: a direction that is not normalised, scaled by 2^-70 or 2^66, with components that are
 * exactly +-0, an origin exactly on a surface with t_min = 0, negative t_min.  Such rays return the reference's record bit
 * for bit (tests/test_gpu_query_edges.py, class A), a NaN slab value at a BVH box (0 * inf: the origin in a box plane,
 * the direction parallel to it) included.
 *   Supported range of |d|.  The hit record of a rect or cube needs no d.d and is the reference's at any scale.  Whatever
 *     normalises the direction — a sphere's discriminant, a medium's |d|, and, where a mode scatters a caller's ray, the Metal and
 *     Dielectric rules of its first segment — needs d.d = dx^2 + dy^2 + dz^2 to be a NORMAL fp32 number: 2^-63 <= |d| < 2^63
 *     is always inside, and results there are scale-free (a power of two is exact).  Outside, fp32 differs from the
 *     reference's f64, which is scale-free everywhere: where d.d overflows, d / |d| is 0; where d.d is a denormal
 *     (denormals are kept), the normalised direction keeps only the bits d.d has left.  tests/test_path_contract.py pins
 *     both (test_out_of_range_direction_magnitude_pins_documented_difference_from_the_reference), the device to the fp32
 *     oracle bit for bit.  A caller with such rays rescales d by a power of two and t_min, t_max inversely: that is exact.
 *   In-plane rays.  A ray that starts in the plane of a rect or of a cube face (o_k equal to the plane's constant) with
 *     an infinite 1 / d_k — d_k = +-0, or a denormal d_k with |d_k| <= 2^-128, whose reciprocal overflows; denormals are
 *     kept — is accepted by Rect::hit anywhere in that infinite plane, with t = 0 * inf = NaN (rect.rs:46-51), and the
 *     NaN then fails every later comparison.  Such a hit is returned as it is: t, u, v and p are
 *     NaN, the normal and the indices are the rect's.  In a scene of plain lists the record is the reference's, NaN for
 *     NaN.  Below a BVH the hit flag is the reference's, and occluded equals it; which accepted leaf is returned can
 *     differ: every leaf the reference reaches is tested, against the query's own interval, and the accepted leaves are
 *     folded in sequence from left to right (a later leaf replaces the best so far unless best.t < t, which a NaN on
 *     either side fails), where BVHNode::hit folds the two results of each node (bvh.rs:75-81).  The two agree whenever no
 *     accepted t is NaN.  A rect with x0 > x1 or y0 > y1 is left out of the device's scene (nothing but an in-plane ray
 *     could hit it): rays in its plane return the record of the world without it.
 *   RTMI_FLAG_FAST_CULL and such rays.  The pruned traversal skips a leaf whose padded box the ray misses, which would
 *     lose the acceptance above, so a ray for which a component of 1 / d is infinite takes the reference-topology
 *     traversal whatever the flag says; its result is that of flags = 0, byte for byte, at that traversal's speed
 *     (axis-aligned picking and shadow rays are such rays).  Not detected: a direction whose reciprocal is finite in
 *     every component and that a Rotate inside the scene turns into one with a zero or denormal component, by
 *     cancellation of two rounded products, for a ray that also starts exactly in a face plane of that rotated frame;
 *     under RTMI_FLAG_FAST_CULL it can miss the NaN acceptance that flags = 0 returns. */
int rtmi_trace(rtmi_scene *scene, const rtmi_query_params *params, const rtmi_ray *rays, const float *time,
               rtmi_hit *hits_out, double *kernel_ms);
int rtmi_occluded(rtmi_scene *scene, const rtmi_query_params *params, const rtmi_ray *rays, const float *time,
                  uint8_t *occluded_out, double *kernel_ms);

/* Asynchronous, DEVICE pointers on the scene's device, enqueued on `stream` (a hipStream_t) like rtmi_render_device
 * without stats.  They write exactly n records and nothing beyond, and take the caller's word for the rays. */
int rtmi_trace_device(rtmi_scene *scene, const rtmi_query_params *params, const void *d_rays, const void *d_time,
                      void *d_hits, void *stream);
int rtmi_occluded_device(rtmi_scene *scene, const rtmi_query_params *params, const void *d_rays, const void *d_time,
                         void *d_occluded, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RTMI_QUERY_H */
