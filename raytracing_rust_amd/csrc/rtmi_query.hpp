// rtmi_query.hpp — device functions of the ray queries (include/rtmi_query.h, rtmi_query.hip): the hit record of a
// closest hit, and the occlusion traversal.  Arithmetic contract as stated in rtmi_device.hip.
#pragma once
#include "rtmi_bvh.hpp"
#include "rtmi_shade.hpp"
#include "rtmi_query.h"

// the ray a query lane traces, under the names the world scan (rtmi_path_scan.inc) reads of a render's Path
struct QueryRay {
    F3 ro, rd;
    float rtime;
};

// HitRecord of the closest hit (hittable.rs:9-16): the geometric half of shade_hit (rtmi_shade.hpp), restated with
// (u, v) always evaluated (get_sphere_uv with the reference's constant, sphere.rs:9-15; rect.rs:52-56) and the material
// index kept instead of its record.  The normal is the record's after the transforms and FlipNormals (hittable.rs:78-83),
// never turned against the ray.  prim_gaps / item_gaps (rtmi_scene_attach_flips, or NULL both): the places of the flips
// among the wrappers.  Negation commutes with a rotation in value but not in the sign of an exact zero (c*0 - s*0 and
// c*(-0) - s*(-0) are both +0), so with the table the chain is walked one transform at a time, innermost first, negating
// where the reference's FlipNormals::hit does; without it the parity is applied after the transforms, as in shade_hit.
__device__ __forceinline__ void xform_hit_flips(const rtmi_xform *xf, int first, int count, uint32_t gaps, F3 &p, F3 &n) {
    for (int g = count;; g--) {
        if ((gaps >> g) & 1u) n = -n;
        if (g == 0) break;
        xform_hit_one(xf[first + g - 1], p, n);
    }
}
__device__ __forceinline__ void query_record(const DevScene &sc, const uint32_t *prim_gaps, const uint32_t *item_gaps, const QueryRay &pa,
                                             float closest, int best_item, int best_pf, bool best_medium, F3 &hp, F3 &hn, float &hu,
                                             float &hv, int &prim, int &material) {
    hu = 0.0f; hv = 0.0f;
    // of the item only {flags, xform_first, xform_count, medium_material} are needed: one 16-B fetch
    struct __attribute__((aligned(4))) ItemWords { int x, y, z, w; };
    const char *ditem = reinterpret_cast<const char *>(sc.items + best_item);
    const ItemWords IW = *reinterpret_cast<const ItemWords *>(ditem + 12);
    const rtmi_xform IX0 = *reinterpret_cast<const rtmi_xform *>(ditem + 64), IX1 = *reinterpret_cast<const rtmi_xform *>(ditem + 80);
    const uint32_t iflags = (uint32_t)IW.x;
    const int xform_first = IW.y, xform_count = IW.z;
    if (best_medium) {
        prim = -1;
        material = IW.w;               // medium_material
        hp = pa.ro + pa.rd * closest;  // ray.pointing_at(t) — medium.rs:47
        hn = f3(1.0f, 0.0f, 0.0f);     // medium.rs:48
        const int outer = (int)((iflags >> RTMI_ITEMFLAG_MEDIUM_OUTER_SHIFT) & 15u);
        F3 lo = pa.ro, ld = pa.rd;
        if (outer > 0) { // the medium sits inside `outer` wrappers: its point is taken on THEIR ray and handed back
            xform_ray(sc.xforms, xform_first, outer, lo, ld);
            hp = lo + ld * closest;
        }
        if (item_gaps) { // FlipNormals around the medium, at their places among its wrappers — hittable.rs:78-83
            xform_hit_flips(sc.xforms, xform_first, outer, item_gaps[best_item], hp, hn);
        } else {
            if (outer > 0) xform_hit(sc.xforms, xform_first, outer, hp, hn);
            if ((iflags & RTMI_ITEMFLAG_FLIP) != 0u) hn = -hn;
        }
        return;
    }
    const int idx = best_pf >> 3, face = best_pf & 7;
    const PrimRec *pr = reinterpret_cast<const PrimRec *>(sc.leaf_rec + (size_t)idx * 5);
    const float4 A = pr->A, PB = pr->B;
    const rtmi_prim_meta PM = pr->M;
    prim = idx;
    material = PM.material;
    F3 lo = pa.ro, ld = pa.rd;
    if (xform_count > 0) xform_ray_item(sc.xforms, xform_first, xform_count, IX0, IX1, lo, ld);
    // an instanced primitive's own chain, inside the item's frame (rtmi.h)
    const int pxf_count = sc.has_prim_xf ? (int)((PM.flags >> RTMI_PRIMFLAG_XF_COUNT_SHIFT) & RTMI_PRIM_XF_MAX) : 0;
    const int pxf_first = (int)(PM.flags >> RTMI_PRIMFLAG_XF_FIRST_SHIFT);
    if (pxf_count > 0) xform_ray(sc.xforms, pxf_first, pxf_count, lo, ld);
    hp = lo + ld * closest; // ray.pointing_at(t)
    if (PM.type == RTMI_PRIM_SPHERE || PM.type == RTMI_PRIM_MSPHERE) {
        F3 c = f3(A.x, A.y, A.z);
        if (PM.type == RTMI_PRIM_MSPHERE) c = moving_center(A, PB, PM.inv_dt, pa.rtime);
        hn = vdiv(hp - c, A.w); // sphere.rs:50 — outward, never face-forwarded
        sphere_uv(hn, false, hu, hv);
    } else {
        int plane;
        float x0, y0, x1, y1;
        if (PM.type == RTMI_PRIM_RECT) {
            plane = (int)((PM.flags >> RTMI_PRIMFLAG_PLANE_SHIFT) & 3u);
            x0 = A.x; y0 = A.y; x1 = A.z; y1 = A.w;
        } else { // cube face -> its rect (cube.rs:21-74)
            const float ax = A.x, ay = A.y, az = A.z, bx = A.w, by = PB.x, bz = PB.y;
            if (face < 2) { plane = 2; x0 = ax; y0 = ay; x1 = bx; y1 = by; }
            else if (face < 4) { plane = 1; x0 = az; y0 = ax; x1 = bz; y1 = bx; }
            else { plane = 0; x0 = ay; y0 = az; x1 = by; y1 = bz; }
        }
        hn = f3(plane == 0 ? 1.0f : 0.0f, plane == 1 ? 1.0f : 0.0f, plane == 2 ? 1.0f : 0.0f); // rect.rs:58-59
        // rect.rs:52-56
        const float x = plane == 0 ? lo.y + closest * ld.y : (plane == 1 ? lo.z + closest * ld.z : lo.x + closest * ld.x);
        const float y = plane == 0 ? lo.z + closest * ld.z : (plane == 1 ? lo.x + closest * ld.x : lo.y + closest * ld.y);
        hu = (x - x0) / (x1 - x0);
        hv = (y - y0) / (y1 - y0);
    }
    if (prim_gaps) { // innermost frames first, FlipNormals (hittable.rs:78-83) at their places
        xform_hit_flips(sc.xforms, pxf_first, pxf_count, prim_gaps[idx], hp, hn);
        xform_hit_flips(sc.xforms, xform_first, xform_count, item_gaps[best_item], hp, hn);
        return;
    }
    if (pxf_count > 0) xform_hit(sc.xforms, pxf_first, pxf_count, hp, hn);
    if (xform_count > 0) xform_hit_item(sc.xforms, xform_first, xform_count, IX0, IX1, hp, hn);
    if (((PM.flags ^ iflags) & 1u) != 0u) hn = -hn;
}

// Which traversal a query ray takes under RTMI_FLAG_FAST_CULL.  The pruned walk (bvh_query<true>, rtmi_bvh.hpp) skips a
// leaf whose padded box the ray misses, because no hit of the primitive lies outside that box.  One acceptance does:
// Rect::hit of a ray in the rect's plane computes t = (k - o_k) * (1 / d_k) = 0 * inf = NaN when 1 / d_k is infinite, and
// every comparison that would reject it is false (rect.rs:46-51), wherever the ray is in that infinite plane.  The
// reference reaches the leaf through its parent's box and accepts; the pruned walk would not.  A render never traces such
// a ray, a query can (the caller's shadow ray straight up, an occlusion test along a wall).  1 / d_k is infinite for
// d_k = +-0 and for every denormal |d_k| <= 2^-128, where the division overflows (denormals are kept, and
// rtmi_validate_rays accepts them), so the test is on the quotient itself, the value ray_derive hands to Rect::hit: a ray
// with an infinite component of 1 / d takes the reference-topology traversal whatever the flag says, and trace and
// occluded then evaluate the same predicate, the reference's.  (A rotation inside the scene can still produce such a
// component from a direction that has none, by exact cancellation of two rounded products; such a ray must also start
// exactly in a face plane of that rotated frame.  It is not detected here: include/rtmi_query.h.)
__device__ __forceinline__ bool query_ray_pruned(const QueryRay &pa) {
    const float ix = 1.0f / pa.rd.x, iy = 1.0f / pa.rd.y, iz = 1.0f / pa.rd.z; // aabb.rs:33, as ray_derive
    const float m = fmaxf(fmaxf(__builtin_fabsf(ix), __builtin_fabsf(iy)), __builtin_fabsf(iz));
    return m < __builtin_inff();
}

// world.hit(ray, t_min, t_max) of a query ray: the scan of rtmi_path_scan.inc, the text the per-lane render kernel traces
// its path rays with, under the ray's own interval, time and Philox key.
template <bool FAST, typename RngT>
__device__ __forceinline__ void world_closest(const DevScene &sc, const QueryRay &pa, float t_min, float t_max, uint32_t *stack, RngT &g,
                                              uint32_t k0, uint32_t k1, float &closest, int &best_item, int &best_pf,
                                              bool &best_medium) {
    constexpr bool PROF = false;
    unsigned long long *prof = nullptr;
#define RTMI_SCAN_T_MIN t_min
#define RTMI_SCAN_T_MAX t_max
#include "rtmi_path_scan.inc"
#undef RTMI_SCAN_T_MIN
#undef RTMI_SCAN_T_MAX
}

// BVHNode::hit (bvh.rs:70-89) as a predicate: does any leaf the reference reaches accept a hit in (t_min, t_max)?  The
// reference tests every box and every leaf against the query's own interval, so which leaves are reached does not
// depend on the order of the visit or on what other leaves returned: the walk needs no ordering and no entry
// distances, and stops at the first accepted leaf.  One traversal for both flag settings: the pruning of the
// closest-hit walk starts with its first hit, where this one ends.
__device__ __forceinline__ bool bvh_any(const DevScene &sc, int root, const RayF &r, float time, float t_min, float t_max,
                                        uint32_t *stack) {
    int sp = 0;
    int cur = root;
    for (;;) {
        if (cur >= 0) {
            const float4 *n = sc.nodes + (size_t)cur * 4;
            const float4 n0 = n[0], n1 = n[1], n2 = n[2], n3 = n[3];
            const int left = __float_as_int(n3.x), right = __float_as_int(n3.y);
            // a leaf child has no box test of its own (bvh.rs:72-73)
            const bool vl = left < 0 || aabb_hit(n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, r, t_min, t_max);
            bool vr = right < 0 || aabb_hit(n1.z, n1.w, n2.x, n2.y, n2.z, n2.w, r, t_min, t_max);
            if (right == left) vr = false; // BVHNode over one object: the same leaf twice, same result
            if (vl) {
                if (vr) { stack[sp * 64] = (uint32_t)right; sp++; }
                cur = left;
                continue;
            }
            if (vr) { cur = right; continue; }
        } else {
            const int type = (int)(((uint32_t)cur >> 28) & 7u);
            const int idx = (int)((uint32_t)cur & 0x0fffffffu);
            float t;
            int pf;
            if (prim_test(sc, type, idx, r, time, t_min, t_max, t, pf)) return true;
        }
        if (sp == 0) return false;
        sp--;
        cur = (int)stack[sp * 64];
    }
}

// geometry of one item against (q_min, q_max) as a predicate: HittableList scan or BVH (geom_query's, rtmi_bvh.hpp).  A
// list's scan shrinks its t_max with every hit (hittable.rs:40-44), which changes nothing before the first one.
__device__ __forceinline__ bool geom_any(const DevScene &sc, const rtmi_item &I, const RayF &r, float time, float q_min,
                                         float q_max, uint32_t *stack) {
    if (I.kind == RTMI_ITEM_BVH) {
        // BVHNode::hit of the root: its own bbox first (bvh.rs:71)
        if (!aabb_hit(I.root_min[0], I.root_min[1], I.root_min[2], I.root_max[0], I.root_max[1], I.root_max[2], r, q_min, q_max))
            return false;
        return bvh_any(sc, I.first, r, time, q_min, q_max, stack);
    }
    for (int k = 0; k < I.count; k++) {
        const int idx = I.first + k;
        const int type = reinterpret_cast<const PrimRec *>(sc.leaf_rec + (size_t)idx * 5)->M.type;
        float t;
        int pf;
        if (prim_test(sc, type, idx, r, time, q_min, q_max, t, pf)) return true;
    }
    return false;
}

// world.hit(ray, t_min, t_max).is_some(): the scan of rtmi_path_scan.inc with the closest hit so far fixed at t_max — it
// is until the first acceptance, where this scan returns.  Every acceptance condition is the closest-hit scan's, in its
// order, so the medium draws before the return are the same draws: a plain item by geom_any; a DEFERRED subtree through
// its gate, the interval it was entered with and the tie rule; a medium through both boundary queries, the nested
// interval, its draw and `tm < closest`; the members of a list scan fold their own closest hit (which later members
// and the fold at the terminator depend on), so they are traced as there and the scan returns where the fold wins.
template <bool FAST, typename RngT>
__device__ __forceinline__ bool world_any(const DevScene &sc, const QueryRay &pa, float t_min, float t_max, uint32_t *stack, RngT &g,
                                          uint32_t k0, uint32_t k1) {
    constexpr bool PROF = false;
    unsigned long long *prof = nullptr;
    RayF W;
    W.o = pa.ro; W.d = pa.rd;
    ray_derive(W);
    float closest = t_max;
    int best_item = -1, best_pf = 0;
    bool best_medium = false;
    float t0_saved = RTMI_FLT_MAX;
    int grp_first = 0x7fffffff;
    bool grp_tree = false;
    ListScan ls;
    ls.cl = RTMI_FLT_MAX; ls.item = -1; ls.pf = 0; ls.medium = false; ls.has = false;
    for (uint32_t it = 0; it < sc.n_items; it++) {
        const rtmi_item I = sc.items[it].it;
        if (I.flags & RTMI_ITEMFLAG_SAVE_T0) {
            t0_saved = closest; grp_first = (int)it; grp_tree = I.kind == RTMI_ITEM_BVH && !(I.flags & RTMI_ITEMFLAG_DEFERRED);
        }
        if (I.flags & RTMI_ITEMFLAG_LISTSCAN_END) {
            listscan_fold(ls, I.first, closest, best_item, best_pf, best_medium, grp_first, grp_tree);
            if (best_item >= 0) return true;
            continue;
        }
        if (I.flags & RTMI_ITEMFLAG_LISTSCAN_BEGIN) { ls.cl = t0_saved; ls.has = false; }
        const bool scan = (I.flags & RTMI_ITEMFLAG_LISTSCAN_MEMBER) != 0u;
        RayF R = W;
        if (I.xform_count > 0) {
            if (xform_ray(sc.xforms, I.xform_first, I.xform_count, R.o, R.d)) ray_derive(R);
        }
        if (!(I.flags & RTMI_ITEMFLAG_MEDIUM)) {
            float t;
            int pf;
            if (scan) {
                if (deferred_gate(sc, I, W, t_min, t0_saved) &&
                    geom_query<FAST, PROF>(sc, I, R, pa.rtime, t_min, ls.cl, stack, t, pf, prof, 0)) {
                    ls.cl = t; ls.item = (int)it; ls.pf = pf; ls.medium = false; ls.has = true;
                }
            } else if (I.flags & RTMI_ITEMFLAG_DEFERRED) {
                if (deferred_gate(sc, I, W, t_min, t0_saved) &&
                    geom_query<FAST, PROF>(sc, I, R, pa.rtime, t_min, t0_saved, stack, t, pf, prof, 0) &&
                    deferred_bvh_wins(I.count, t, closest, best_item, best_pf, grp_first, grp_tree))
                    return true;
            } else if (geom_any(sc, I, R, pa.rtime, t_min, closest, stack)) {
                return true;
            }
        } else {
            // ConstantMedium::hit — medium.rs:28-56
            float t1, t2, tm;
            int pf;
            const bool dfr = (I.flags & RTMI_ITEMFLAG_DEFERRED) != 0u;
            const float qmax = scan ? ls.cl : (dfr ? t0_saved : closest);
            if (!dfr || deferred_gate(sc, I, W, t_min, t0_saved)) {
                if (geom_query<FAST, PROF>(sc, I, R, pa.rtime, -RTMI_FLT_MAX, RTMI_FLT_MAX, stack, t1, pf, prof, 0)) {
                    if (geom_query<FAST, PROF>(sc, I, R, pa.rtime, t1 + 0.0001f, RTMI_FLT_MAX, stack, t2, pf, prof, 0)) {
                        const float dn = medium_dir_norm(sc, I.flags, I.xform_first, W);
                        if ((I.flags & RTMI_ITEMFLAG_NESTED_MEDIUM) && !nested_medium_interval(sc, I, dn, g, k0, k1, t1, t2)) {
                            // the inner medium returned no hit to one of the outer medium's two queries
                        } else if (medium_sample(t1, t2, t_min, qmax, dn, I.neg_inv_density, g, k0, k1, tm)) {
                            if (scan) { ls.cl = tm; ls.item = (int)it; ls.medium = true; ls.has = true; }
                            else if (!dfr || tm < closest) return true;
                        }
                    }
                }
            }
        }
    }
    return false;
}
