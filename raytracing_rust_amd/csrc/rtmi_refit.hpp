// rtmi_refit.hpp — the refit of a scene's trees after its primitives have moved (include/rtmi_update.h).
// This header is the specification.  Its first part states the per-primitive and per-node rules once, as functions that
// the refit kernel (rtmi_update_dev.hip) and the host evaluation (rtmu_refit_desc) both compile; its second part, host
// only, reads the topology of a description into a RefitPlan — which items can be refit, their nodes by level, which
// primitives they own — and evaluates the rules over it.  Plain C++: the host part needs no HIP and is compiled alone by the
// tests (under sanitizers).
//
// Arithmetic: fp32, every operation rounded once, nothing fused (the units are compiled with -ffp-contract=off).
//   refit_min(a, b) = b < a ? b : a, refit_max(a, b) = b > a ? b : a: fminf / fmaxf for finite values, with the result of a
//                     tie between -0 and +0 fixed (the first argument), so that host and device agree in every bit
//   leaf box        SPHERE: c_k - r, c_k + r with the radius as it stands (Sphere::bounding_box: inverted for the negative radius
//                   of a hollow sphere);  CUBE: its planes (min.xyz = A.xyz, max = A.w, B.x, B.y)
//   leaf extent     what the primitive can report (true_bounds of the lowering): SPHERE: c_k - |r|, c_k + |r|;  CUBE: its planes
//   node box        the union (refit_min / refit_max per component) of its two children's boxes, left first; a node over one
//                   element (left == right) unites the box with itself
//   root, scale     item.root_min / root_max = the root node's box; scale = the largest |coordinate| of those six, taken in
//                   the order min.xyz, max.xyz; pad = scale / 8192
//   nodes[]         an internal child's box = that child's node box; a leaf child's = the leaf EXTENT widened by pad
//                   (min - pad, max + pad)
//   prim_gate[p]    the node box of the node that holds leaf p (w components untouched)
//   alt_nodes[]     a leaf slot = the leaf extent widened by pad; a node slot = the union of that node's own non-empty slots, in
//                   slot order; an empty slot is left alone
// Against the lowering (host/rt_host.cpp): it evaluates the same quantities in f64 from the f64 geometry and rounds once;
// the refit starts from the fp32 planes.  Refitting unchanged planes may therefore move a box coordinate by a few ulp of
// `scale` (at most 2^-22 scale: two inputs off by 2^-24 scale each, and one rounding on either side).  pad is 2^-13 scale,
// so culling stays conservative; a gate can change only for a ray that grazes a node box within that rounding.  The updated
// scene is DEFINED by these rules (rtmu_refit_desc), not by a fresh lowering.
#pragma once

#include <stdint.h>

#include "rtmi.h"

#if defined(__HIPCC__)
#define RTMI_REFIT_HD __host__ __device__ inline
#else
#define RTMI_REFIT_HD inline
#endif

struct RefitBox {
    float mn[3], mx[3];
};

RTMI_REFIT_HD float refit_min(float a, float b) { return b < a ? b : a; }
RTMI_REFIT_HD float refit_max(float a, float b) { return b > a ? b : a; }
RTMI_REFIT_HD bool refit_is_leaf(int32_t ref) { return ref < 0; }
RTMI_REFIT_HD int refit_leaf_type(int32_t ref) { return (int)(((uint32_t)ref >> 28) & 7u); }
RTMI_REFIT_HD uint32_t refit_leaf_prim(int32_t ref) { return (uint32_t)ref & 0x0fffffffu; }

// A, B: the primitive's planes (4 floats each)
RTMI_REFIT_HD RefitBox refit_leaf_box(int type, const float *A, const float *B) {
    RefitBox b;
    if (type == RTMI_PRIM_CUBE) {
        b.mn[0] = A[0]; b.mn[1] = A[1]; b.mn[2] = A[2];
        b.mx[0] = A[3]; b.mx[1] = B[0]; b.mx[2] = B[1];
    } else { // RTMI_PRIM_SPHERE
        for (int k = 0; k < 3; k++) { b.mn[k] = A[k] - A[3]; b.mx[k] = A[k] + A[3]; }
    }
    return b;
}
// what the primitive can report: the culling boxes (a leaf child's box in nodes[], a leaf slot of alt_nodes[]) bound this
RTMI_REFIT_HD RefitBox refit_leaf_extent(int type, const float *A, const float *B) {
    if (type == RTMI_PRIM_CUBE) return refit_leaf_box(type, A, B);
    const float r = A[3] < 0.0f ? -A[3] : A[3];
    RefitBox b;
    for (int k = 0; k < 3; k++) { b.mn[k] = A[k] - r; b.mx[k] = A[k] + r; }
    return b;
}
RTMI_REFIT_HD RefitBox refit_union(const RefitBox &a, const RefitBox &b) {
    RefitBox u;
    for (int k = 0; k < 3; k++) { u.mn[k] = refit_min(a.mn[k], b.mn[k]); u.mx[k] = refit_max(a.mx[k], b.mx[k]); }
    return u;
}
RTMI_REFIT_HD float refit_abs(float v) { return v < 0.0f ? -v : (v == 0.0f ? 0.0f : v); }
RTMI_REFIT_HD float refit_scale(const RefitBox &root) {
    float s = 0.0f;
    for (int k = 0; k < 3; k++) s = refit_max(s, refit_abs(root.mn[k]));
    for (int k = 0; k < 3; k++) s = refit_max(s, refit_abs(root.mx[k]));
    return s;
}
RTMI_REFIT_HD float refit_pad(float scale) { return scale / 8192.0f; }
RTMI_REFIT_HD RefitBox refit_widen(const RefitBox &b, float pad) {
    RefitBox w;
    for (int k = 0; k < 3; k++) { w.mn[k] = b.mn[k] - pad; w.mx[k] = b.mx[k] + pad; }
    return w;
}


// ---- host: the topology of a description ------------------------------------------------------------------------------------
#include <string>
#include <vector>

// One item of the description.  A BVH item owns the primitives its leaves name, [prim_lo, prim_hi); a LIST item its run.
// order / lvl: the nodes of the reference tree, deepest level first; level k = order[lvl[k] .. lvl[k + 1]).  alt_*: the same
// of the alternative tree.  Filled for every BVH item, refittable or not.
struct RefitPlanItem {
    bool bvh = false, refittable = false;
    bool frozen = false; // a LIST item of a deferred group: its gate is a box of the enclosing tree
    const char *why = ""; // what keeps a BVH item from being refit
    uint32_t prim_lo = 0, prim_hi = 0;
    std::vector<uint32_t> order, lvl, alt_order, alt_lvl;
};
struct RefitPlan {
    std::vector<RefitPlanItem> items;
    std::vector<int32_t> prim_item; // the item that owns each primitive (-1: none)
    std::string err;
};

// nodes of one tree by level; `kids(n, out)` lists the node's children (references).  false: malformed (a child outside
// the array, a node reached twice — which also ends every cycle —, deeper than the array is long)
template <typename Kids>
static inline bool refit_levels(int32_t root, uint32_t n_nodes, std::vector<uint8_t> &seen, Kids &&kids, std::vector<uint32_t> &order,
                                std::vector<uint32_t> &lvl, std::vector<int32_t> &leaves) {
    std::vector<std::vector<uint32_t>> by_depth;
    std::vector<std::pair<uint32_t, uint32_t>> stack;
    if (root < 0 || (uint32_t)root >= n_nodes) return false;
    stack.push_back({(uint32_t)root, 0u});
    while (!stack.empty()) {
        const uint32_t n = stack.back().first, depth = stack.back().second;
        stack.pop_back();
        if (seen[n]) return false;
        seen[n] = 1;
        if (by_depth.size() <= depth) by_depth.resize(depth + 1);
        by_depth[depth].push_back(n);
        int32_t ch[4];
        const int nch = kids(n, ch);
        for (int c = 0; c < nch; c++) {
            if (c > 0 && ch[c] == ch[c - 1]) continue; // a node over one element names it twice
            if (refit_is_leaf(ch[c])) { leaves.push_back(ch[c]); continue; }
            if ((uint32_t)ch[c] >= n_nodes) return false;
            stack.push_back({(uint32_t)ch[c], depth + 1});
        }
    }
    order.clear(); lvl.clear();
    for (size_t d = by_depth.size(); d-- > 0;) {
        lvl.push_back((uint32_t)order.size());
        order.insert(order.end(), by_depth[d].begin(), by_depth[d].end());
    }
    lvl.push_back((uint32_t)order.size());
    return true;
}

static inline int refit_plan_build(const rtmi_scene_desc *d, RefitPlan &plan) {
    const float big = 3.40282346638528859811704183484516925e+38f;
    if (!d || (d->n_items && !d->items) || (d->n_prims && !d->prim_meta) || (d->n_nodes && !d->nodes) ||
        (d->n_alt_nodes && !d->alt_nodes)) {
        plan.err = "a NULL array in the description";
        return RTMI_ERR_INVALID;
    }
    plan.items.assign(d->n_items, RefitPlanItem());
    plan.prim_item.assign(d->n_prims, -1);
    std::vector<uint8_t> seen(d->n_nodes, 0), seen_alt(d->n_alt_nodes, 0), is_leaf(d->n_prims, 0);
    for (uint32_t i = 0; i < d->n_items; i++) {
        const rtmi_item &it = d->items[i];
        RefitPlanItem &P = plan.items[i];
        if (it.kind == RTMI_ITEM_LIST) {
            if (it.count < 0 || it.first < 0 || (uint64_t)it.first + (uint64_t)it.count > d->n_prims) {
                if (it.flags & RTMI_ITEMFLAG_LISTSCAN_END) continue; // the terminator of a list scan: `first` is a count
                plan.err = "a LIST item outside the primitives";
                return RTMI_ERR_INVALID;
            }
            if (it.flags & RTMI_ITEMFLAG_LISTSCAN_END) continue;
            P.prim_lo = (uint32_t)it.first; P.prim_hi = (uint32_t)(it.first + it.count);
            P.frozen = (it.flags & (RTMI_ITEMFLAG_DEFERRED | RTMI_ITEMFLAG_LISTSCAN_MEMBER)) != 0u;
            for (uint32_t p = P.prim_lo; p < P.prim_hi; p++) plan.prim_item[p] = (int32_t)i;
            continue;
        }
        if (it.kind != RTMI_ITEM_BVH) { plan.err = "bad item kind"; return RTMI_ERR_INVALID; }
        P.bvh = true;
        std::vector<int32_t> leaves, alt_leaves;
        if (!refit_levels(it.first, d->n_nodes, seen, [&](uint32_t n, int32_t *ch) { ch[0] = d->nodes[n].left; ch[1] = d->nodes[n].right; return 2; },
                          P.order, P.lvl, leaves)) {
            plan.err = "a BVH item's tree leaves the node array or reaches a node twice";
            return RTMI_ERR_INVALID;
        }
        P.prim_lo = 0xffffffffu; P.prim_hi = 0u;
        for (int32_t ref : leaves) {
            const uint32_t p = refit_leaf_prim(ref);
            if (p >= d->n_prims) { plan.err = "a leaf outside the primitives"; return RTMI_ERR_INVALID; }
            P.prim_lo = p < P.prim_lo ? p : P.prim_lo;
            P.prim_hi = p + 1 > P.prim_hi ? p + 1 : P.prim_hi;
        }
        for (uint32_t p = P.prim_lo; p < P.prim_hi; p++) plan.prim_item[p] = (int32_t)i;
        if (it.alt_first >= 0 &&
            !refit_levels(it.alt_first, d->n_alt_nodes, seen_alt,
                          [&](uint32_t n, int32_t *ch) {
                              int k = 0;
                              for (int c = 0; c < 4; c++)
                                  if (d->alt_nodes[n].child[c] != RTMI_NO_CHILD) ch[k++] = d->alt_nodes[n].child[c];
                              return k;
                          },
                          P.alt_order, P.alt_lvl, alt_leaves)) {
            plan.err = "a BVH item's alternative tree leaves the node array or reaches a node twice";
            return RTMI_ERR_INVALID;
        }
        // ---- can it be refit? ----
        P.refittable = true;
        const auto no = [&](const char *why) { P.refittable = false; if (!P.why[0]) P.why = why; };
        if (it.flags & (RTMI_ITEMFLAG_DEFERRED | RTMI_ITEMFLAG_SAVE_T0)) no("the item heads or belongs to a deferred group");
        if (!(it.scale < 1e30f)) no("the lowering found the tree not prunable (scale = 1e30)");
        for (int32_t ref : leaves) {
            const uint32_t p = refit_leaf_prim(ref);
            const rtmi_prim_meta &m = d->prim_meta[p];
            if (m.type != refit_leaf_type(ref) || (m.type != RTMI_PRIM_SPHERE && m.type != RTMI_PRIM_CUBE)) no("a leaf is not a static sphere or a cube");
            if ((m.flags >> RTMI_PRIMFLAG_XF_COUNT_SHIFT) & RTMI_PRIM_XF_MAX) no("a leaf carries a transform chain of its own");
            is_leaf[p] = 1;
        }
        for (uint32_t n : P.order) { // a list as a BVH child: nodes whose boxes pass every ray (lower_list_leaf)
            const rtmi_bvh_node &N = d->nodes[n];
            if (!refit_is_leaf(N.left) && N.lmin[0] == -big && N.lmax[0] == big) no("a list is a child of a node of the tree");
            if (!refit_is_leaf(N.right) && N.rmin[0] == -big && N.rmax[0] == big) no("a list is a child of a node of the tree");
        }
        uint32_t distinct = 0;
        for (uint32_t p = P.prim_lo; p < P.prim_hi; p++) distinct += is_leaf[p] != 0 ? 1u : 0u;
        if (distinct != P.prim_hi - P.prim_lo) no("the item's primitives are not the run its leaves name");
        if (it.alt_first < 0) {
            if (distinct >= 2) no("no alternative tree");
        } else {
            uint32_t alt_distinct = 0;
            for (int32_t ref : alt_leaves) {
                const uint32_t p = refit_leaf_prim(ref);
                if (p >= d->n_prims) { plan.err = "a leaf of an alternative tree outside the primitives"; return RTMI_ERR_INVALID; }
                if (p < P.prim_lo || p >= P.prim_hi || is_leaf[p] != 1) { no("the alternative tree holds other primitives than the tree"); continue; }
                is_leaf[p] = 2;
                alt_distinct++;
            }
            if (alt_distinct != distinct || alt_leaves.size() != distinct) no("the alternative tree holds other primitives than the tree");
        }
    }
    return RTMI_OK;
}

// Which items the range [first, first + count) touches: touched[i] = 1.  RTMI_ERR_UNSUPPORTED (plan.err says why) when one of
// them is a BVH item that cannot be refit or belongs to a deferred group.
static inline int refit_touched(RefitPlan &plan, uint32_t first, uint32_t count, std::vector<uint8_t> &touched) {
    touched.assign(plan.items.size(), 0);
    for (size_t i = 0; i < plan.items.size(); i++) {
        const RefitPlanItem &P = plan.items[i];
        if (P.prim_hi <= P.prim_lo || first >= P.prim_hi || first + count <= P.prim_lo) continue;
        if (P.bvh && !P.refittable) {
            plan.err = std::string("the range touches a BVH item that cannot be refit: ") + P.why;
            return RTMI_ERR_UNSUPPORTED;
        }
        if (P.frozen) {
            plan.err = "the range touches a member of a deferred group";
            return RTMI_ERR_UNSUPPORTED;
        }
        touched[i] = 1;
    }
    return RTMI_OK;
}

// the rules over one refittable item; `box` is scratch of n_nodes boxes
static inline void refit_item_host(const rtmi_scene_desc *d, const RefitPlanItem &P, uint32_t i, std::vector<RefitBox> &box, rtmi_item *items,
                                   rtmi_bvh_node *nodes, rtmi_bvh4_node *alt_nodes, float *prim_gate) {
    const auto leaf = [&](int32_t ref) {
        const uint32_t p = refit_leaf_prim(ref);
        return refit_leaf_box(d->prim_meta[p].type, d->prim_a + (size_t)p * 4, d->prim_b + (size_t)p * 4);
    };
    const auto extent = [&](int32_t ref) {
        const uint32_t p = refit_leaf_prim(ref);
        return refit_leaf_extent(d->prim_meta[p].type, d->prim_a + (size_t)p * 4, d->prim_b + (size_t)p * 4);
    };
    const auto child = [&](int32_t ref) { return refit_is_leaf(ref) ? leaf(ref) : box[(size_t)ref]; };
    for (uint32_t n : P.order) box[n] = refit_union(child(d->nodes[n].left), child(d->nodes[n].right));
    const RefitBox root = box[(size_t)d->items[i].first];
    const float scale = refit_scale(root), pad = refit_pad(scale);
    for (int k = 0; k < 3; k++) { items[i].root_min[k] = root.mn[k]; items[i].root_max[k] = root.mx[k]; }
    items[i].scale = scale;
    for (uint32_t n : P.order) {
        const int32_t ch[2] = {d->nodes[n].left, d->nodes[n].right};
        for (int c = 0; c < 2; c++) {
            const RefitBox b = refit_is_leaf(ch[c]) ? refit_widen(extent(ch[c]), pad) : box[(size_t)ch[c]];
            float *mn = c == 0 ? nodes[n].lmin : nodes[n].rmin, *mx = c == 0 ? nodes[n].lmax : nodes[n].rmax;
            for (int k = 0; k < 3; k++) { mn[k] = b.mn[k]; mx[k] = b.mx[k]; }
            if (refit_is_leaf(ch[c]) && prim_gate) {
                float *g = prim_gate + (size_t)refit_leaf_prim(ch[c]) * 8;
                for (int k = 0; k < 3; k++) { g[k] = box[n].mn[k]; g[4 + k] = box[n].mx[k]; }
            }
        }
    }
    for (uint32_t n : P.alt_order) {
        for (int c = 0; c < 4; c++) {
            const int32_t ref = d->alt_nodes[n].child[c];
            if (ref == RTMI_NO_CHILD) continue;
            RefitBox b;
            if (refit_is_leaf(ref)) {
                b = refit_widen(extent(ref), pad);
            } else {
                const rtmi_bvh4_node &C = alt_nodes[(size_t)ref]; // refit already: a deeper level
                bool any = false;
                for (int q = 0; q < 4; q++) {
                    if (d->alt_nodes[(size_t)ref].child[q] == RTMI_NO_CHILD) continue;
                    const RefitBox s = {{C.minx[q], C.miny[q], C.minz[q]}, {C.maxx[q], C.maxy[q], C.maxz[q]}};
                    b = any ? refit_union(b, s) : s;
                    any = true;
                }
                if (!any) continue; // a node without a slot: nothing to bound
            }
            rtmi_bvh4_node &N = alt_nodes[n];
            N.minx[c] = b.mn[0]; N.miny[c] = b.mn[1]; N.minz[c] = b.mn[2];
            N.maxx[c] = b.mx[0]; N.maxy[c] = b.mx[1]; N.maxz[c] = b.mx[2];
        }
    }
}

// rtmu_refittable and rtmu_refit_desc (include/rtmi_update.h) up to the error message, which `err` receives
static inline int refit_refittable(const rtmi_scene_desc *d, uint8_t *mask, std::string &err) {
    if (!mask) { err = "mask is NULL"; return RTMI_ERR_INVALID; }
    RefitPlan plan;
    if (int rc = refit_plan_build(d, plan)) { err = plan.err; return rc; }
    for (size_t i = 0; i < plan.items.size(); i++) mask[i] = plan.items[i].bvh && plan.items[i].refittable ? 1 : 0;
    return RTMI_OK;
}
static inline int refit_desc(const rtmi_scene_desc *d, uint32_t first, uint32_t count, rtmi_item *items, rtmi_bvh_node *nodes,
                             rtmi_bvh4_node *alt_nodes, float *prim_gate, std::string &err) {
    RefitPlan plan;
    if (int rc = refit_plan_build(d, plan)) { err = plan.err; return rc; }
    if ((uint64_t)first + (uint64_t)count > d->n_prims) { err = "the range leaves the primitives"; return RTMI_ERR_INVALID; }
    if (count == 0) return RTMI_OK;
    if (!d->prim_a || !d->prim_b) { err = "a NULL array in the description"; return RTMI_ERR_INVALID; }
    if (!items || (d->n_nodes && !nodes) || (d->n_alt_nodes && !alt_nodes)) { err = "an output array is NULL"; return RTMI_ERR_INVALID; }
    std::vector<uint8_t> touched;
    if (int rc = refit_touched(plan, first, count, touched)) { err = plan.err; return rc; }
    std::vector<RefitBox> box(d->n_nodes);
    for (uint32_t i = 0; i < d->n_items; i++)
        if (touched[i] && plan.items[i].bvh) refit_item_host(d, plan.items[i], i, box, items, nodes, alt_nodes, d->prim_gate ? prim_gate : nullptr);
    return RTMI_OK;
}

