// rtmi_relight.hpp — the light table and the light tree after the emitters have moved (include/rtmi_relight.h; DESIGN.md
// §44).  This header is the specification.  Its first part states the per-light and per-node rules once, as functions that
// the relight kernel (rtmi_relight_dev.hip) and the host evaluation (rtml_relight_desc) both compile; its second part, host
// only, checks a table and a tree against a description and evaluates the rules over them.  Plain C++: the host part needs
// no HIP and is compiled alone by the tests (under sanitizers).
//
// Arithmetic: f64 from the planes' floats widened, every operation rounded once, nothing fused (the units are compiled with
// -ffp-contract=off, which holds for every floating type).  The rules are read off nee_lights_of (rtmi_device.hip) and
// TreeBuild::fill (rtmi_light_tree.hip) and give their bits:
//   area        RECT: (a1 - a0) * (b1 - b0);  SPHERE: ((4.0 * pi) * r) * r
//   aw          area * weight; total = the sum of aw in table order; select_p = aw / total; cdf = the running sum of
//               select_p in table order, its last entry exactly 1
//   leaf box    RECT of plane 0 = YZ (a = y, b = z), 1 = ZX (a = z, b = x), 2 = XY (a = x, b = y): [a0, a1] x [b0, b1] at k,
//               degenerate on the plane's axis;  SPHERE: c - r, c + r per axis
//   node box    the union of its children's boxes, left first: relight_min(a, b) = b < a ? b : a, relight_max(a, b) = b > a ? b : a
//               (std::min / std::max of the build, with the result of a tie between -0 and +0 fixed: the first argument)
//   node        c = (float)((lo + hi) * 0.5); h = (hi - lo) * 0.5; r2 = (float)((h.x * h.x + h.y * h.y) + h.z * h.z);
//               power = (float)(left + right), a leaf's = (float)aw
#pragma once

#include <stdint.h>

#include "rtmi.h"

#if defined(__HIPCC__)
#define RTMI_RELIGHT_HD __host__ __device__ inline
#else
#define RTMI_RELIGHT_HD inline
#endif

#define RTMI_RELIGHT_PI 3.14159265358979323846 /* M_PI */
#define RTMI_RELIGHT_LEAF 0x80000000u          /* RTMI_LIGHT_TREE_LEAF */

struct RelightBox {
    double lo[3], hi[3];
};

RTMI_RELIGHT_HD double relight_min(double a, double b) { return b < a ? b : a; }
RTMI_RELIGHT_HD double relight_max(double a, double b) { return b > a ? b : a; }
RTMI_RELIGHT_HD bool relight_finite(double v) { return v - v == 0.0; }

// plane: 0, 1, 2 for a RECT, -1 for a SPHERE (NeeLight::plane); A: plane A of the primitive
RTMI_RELIGHT_HD double relight_area(int plane, const float *A) {
    if (plane >= 0) return ((double)A[2] - (double)A[0]) * ((double)A[3] - (double)A[1]);
    return ((4.0 * RTMI_RELIGHT_PI) * (double)A[3]) * (double)A[3];
}
// what keeps a listed light from staying one (the conditions under which nee_lights_of skips an emitter), or NULL
RTMI_RELIGHT_HD const char *relight_degenerate(int plane, const float *A, double weight) {
    if (plane >= 0) {
        if (!(A[0] < A[2]) || !(A[1] < A[3])) return "a rect light with a0 >= a1 or b0 >= b1";
    } else if (!(A[3] > 0.0f) || !relight_finite((double)A[0]) || !relight_finite((double)A[1]) || !relight_finite((double)A[2])) {
        return "a sphere light with r <= 0 or a centre that is not finite";
    }
    const double area = relight_area(plane, A);
    if (!relight_finite(area * weight) || !(area > 0.0)) return "a light whose area * weight is not finite";
    return nullptr;
}
// k: the first float of plane B (a rect's coordinate on its plane's axis)
RTMI_RELIGHT_HD RelightBox relight_leaf_box(int plane, const float *A, float k) {
    RelightBox b;
    if (plane >= 0) {
        const int ka = plane == 0 ? 1 : (plane == 1 ? 2 : 0), kb = plane == 0 ? 2 : (plane == 1 ? 0 : 1);
        const int kk = plane == 0 ? 0 : (plane == 1 ? 1 : 2);
        b.lo[ka] = (double)A[0]; b.hi[ka] = (double)A[2];
        b.lo[kb] = (double)A[1]; b.hi[kb] = (double)A[3];
        b.lo[kk] = b.hi[kk] = (double)k;
    } else {
        for (int a = 0; a < 3; a++) { b.lo[a] = (double)A[a] - (double)A[3]; b.hi[a] = (double)A[a] + (double)A[3]; }
    }
    return b;
}
RTMI_RELIGHT_HD RelightBox relight_union(const RelightBox &l, const RelightBox &r) {
    RelightBox u;
    for (int a = 0; a < 3; a++) { u.lo[a] = relight_min(l.lo[a], r.lo[a]); u.hi[a] = relight_max(l.hi[a], r.hi[a]); }
    return u;
}
// the stored fields of a node over the box b with the f64 power pw: out = {c.x, c.y, c.z, r2, power}
RTMI_RELIGHT_HD void relight_node(const RelightBox &b, double pw, float *out) {
    double h[3];
    for (int a = 0; a < 3; a++) h[a] = (b.hi[a] - b.lo[a]) * 0.5;
    const double r2 = (h[0] * h[0] + h[1] * h[1]) + h[2] * h[2];
    for (int a = 0; a < 3; a++) out[a] = (float)((b.lo[a] + b.hi[a]) * 0.5);
    out[3] = (float)r2;
    out[4] = (float)pw;
}

// ---- host: a table and a tree against a description ------------------------------------------------------------------------
#include <string>
#include <vector>

#include "rtmi_light_tree.h"

// the checks that the host walks make of a caller's tree (rtmi_light_tree.hip, light_tree_check), and one slot pair per light
static inline bool relight_tree_ok(const rtmi_light_node *nodes, uint32_t n_nodes, uint32_t n_lights, std::string &err) {
    if (n_nodes < 2u || (n_nodes & 1u)) { err = "n_nodes must be even and >= 2"; return false; }
    if (n_nodes / 2u != n_lights) { err = "n_nodes is not 2 * n_lights"; return false; }
    for (uint32_t i = 1; i < n_nodes; i++) {
        const uint32_t link = nodes[i].link;
        if (link & RTMI_RELIGHT_LEAF) {
            if ((link & 0x7fffffffu) >= n_lights) { err = "a leaf names a light outside the table"; return false; }
        } else if (link <= i || (link & 1u) || link > n_nodes - 2u) {
            err = "a link leaves the array";
            return false;
        }
    }
    return true;
}

// The slots below the root by depth, deepest first, for the kernel: level k = order[lvl[k] .. lvl[k + 1]).  An interior
// link points behind its node (relight_tree_ok), so one pass in slot order knows every depth.
static inline void relight_levels(const rtmi_light_node *nodes, uint32_t n_nodes, std::vector<uint32_t> &order, std::vector<uint32_t> &lvl) {
    std::vector<int32_t> depth(n_nodes, -1);
    int32_t deepest = 0;
    depth[1] = 0;
    for (uint32_t i = 1; i < n_nodes; i++) {
        if (depth[i] < 0 || (nodes[i].link & RTMI_RELIGHT_LEAF)) continue;
        for (uint32_t c = nodes[i].link; c < nodes[i].link + 2u; c++)
            if (depth[c] < depth[i] + 1) depth[c] = depth[i] + 1;
        if (depth[i] + 1 > deepest) deepest = depth[i] + 1;
    }
    order.clear(); lvl.clear();
    for (int32_t d = deepest; d >= 0; d--) {
        lvl.push_back((uint32_t)order.size());
        for (uint32_t i = 1; i < n_nodes; i++)
            if (depth[i] == d) order.push_back(i);
    }
    lvl.push_back((uint32_t)order.size());
}

// the plane of a light as the device table stores it, or -2 for an entry that is not in the description
static inline int relight_plane_of(const rtmi_scene_desc *d, const rtmi_light &L) {
    if (L.prim < 0 || (uint32_t)L.prim >= d->n_prims || L.item < 0 || (uint32_t)L.item >= d->n_items) return -2;
    const rtmi_prim_meta &M = d->prim_meta[L.prim];
    if (L.kind == RTMI_PRIM_RECT && M.type == RTMI_PRIM_RECT) return (int)((M.flags >> RTMI_PRIMFLAG_PLANE_SHIFT) & 3u);
    if (L.kind == RTMI_PRIM_SPHERE && (M.type == RTMI_PRIM_SPHERE || M.type == RTMI_PRIM_MSPHERE)) return -1;
    return -2;
}

// rtml_relight_desc: nothing is written unless every check has passed
static inline int relight_desc(const rtmi_scene_desc *d, rtmi_light *lights, uint32_t n_lights, rtmi_light_node *nodes, uint32_t n_nodes,
                               std::string &err) {
    if (!d || (n_lights && !lights) || (n_nodes && !nodes)) { err = "NULL argument"; return RTMI_ERR_INVALID; }
    if (d->n_prims && (!d->prim_a || !d->prim_b || !d->prim_meta)) { err = "a non-empty array of the description is NULL"; return RTMI_ERR_INVALID; }
    if (n_nodes && !relight_tree_ok(nodes, n_nodes, n_lights, err)) return RTMI_ERR_INVALID;
    if (n_lights == 0u) return RTMI_OK;
    std::vector<int> plane(n_lights);
    std::vector<double> aw(n_lights);
    for (uint32_t i = 0; i < n_lights; i++) {
        plane[i] = relight_plane_of(d, lights[i]);
        if (plane[i] == -2) { err = "a table entry is outside the description or of another primitive type"; return RTMI_ERR_INVALID; }
        const float *A = d->prim_a + (size_t)lights[i].prim * 4;
        if (const char *why = relight_degenerate(plane[i], A, lights[i].weight)) { err = why; return RTMI_ERR_INVALID; }
    }
    double total = 0.0;
    for (uint32_t i = 0; i < n_lights; i++) {
        lights[i].area = relight_area(plane[i], d->prim_a + (size_t)lights[i].prim * 4);
        aw[i] = lights[i].area * lights[i].weight;
        total += aw[i];
    }
    double c = 0.0;
    for (uint32_t i = 0; i < n_lights; i++) {
        lights[i].select_p = aw[i] / total;
        c += lights[i].select_p;
        lights[i].cdf = i + 1u == n_lights ? 1.0 : c;
    }
    if (!n_nodes) return RTMI_OK;
    std::vector<RelightBox> box(n_nodes);
    std::vector<double> power(n_nodes, 0.0);
    for (uint32_t i = n_nodes - 1u; i >= 1u; i--) { // children sit behind their node: they are done when it is reached
        const uint32_t link = nodes[i].link;
        if (link & RTMI_RELIGHT_LEAF) {
            const uint32_t li = link & 0x7fffffffu;
            box[i] = relight_leaf_box(plane[li], d->prim_a + (size_t)lights[li].prim * 4, d->prim_b[(size_t)lights[li].prim * 4]);
            power[i] = aw[li];
        } else {
            box[i] = relight_union(box[link], box[link + 1u]);
            power[i] = power[link] + power[link + 1u];
        }
        float f[5];
        relight_node(box[i], power[i], f);
        nodes[i].c[0] = f[0]; nodes[i].c[1] = f[1]; nodes[i].c[2] = f[2];
        nodes[i].r2 = f[3];
        nodes[i].power = f[4];
    }
    return RTMI_OK;
}
