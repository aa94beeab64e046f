/* rtmi_light_tree.h — a light tree: position-aware light selection for next-event estimation (include/rtmi_nee.h), on the
 * MI355X (gfx950) device path.  Opt-in; see DESIGN.md §25.
 *
 * rtmi_render_nee picks the light of a vertex from one table with p_sel = area * w / sum, the same at every vertex.  With
 * RTMI_FLAG_LIGHT_TREE it picks by walking a binary tree over the lights, from the vertex's position x: at every interior
 * node a child is chosen in proportion to its importance power / max(|c - x|^2, r^2).  The probability p of the walk takes
 * p_sel's place in the estimator; nothing else of rtmi_nee.h changes: eligibility, the densities p_b and p_L, the MIS
 * ratios, visibility, the accumulation order, the draws of stream 3 (w0 is the walk's uniform) and the path signatures.
 *
 * The tree.  Built on the host in f64 over the table of rtmi_lights_from_desc, in that table's order; every stored value is
 * the f64 value rounded once to float.
 *   Per light: its box (a rect's is degenerate on its plane's axis, a sphere's is c +- r, from the description's floats
 *   widened to f64), its centroid (lo + hi) * 0.5 per axis, its power area * weight of the table.
 *   Layout: 2n slots for n lights.  Slot 0 is unused and all zero, slot 1 is the root, the two children of an interior node
 *   sit at link and link + 1 with link even (one aligned 64-B pair in a 64-B-aligned array); a leaf has
 *   link = 0x80000000 | light index.  pad is 0.
 *   Build over an index set, starting from all lights in table order at slot 1: one light makes a leaf.  Otherwise the axis
 *   is that of the largest extent max - min of the set's centroids (a later axis wins only when strictly larger); the set
 *   is sorted stably by centroid on that axis (ties keep the set's order); left = the first (count + 1) / 2, right = the
 *   rest; two slots are appended to the array, link = the first; left and all below it are filled, then right.
 *   Node fields: lo, hi = the union of the set's boxes; c = (lo + hi) * 0.5; with h = (hi - lo) * 0.5,
 *   r2 = (h.x * h.x + h.y * h.y) + h.z * h.z; power = left power + right power in f64 (a leaf: area * weight).
 *   Every light has area > 0, so every node has r2 > 0.  The depth of a leaf is at most ceil(log2 n) <= 32.
 *   Paths: bit d of paths[i].trail is set iff light i lies in the right child at depth d (the root is depth 0);
 *   paths[i].depth is the depth of its leaf.
 *   An empty table: n_nodes = 0; rtmi_render_nee with the flag is then rtmi_render bit for bit, as without it.
 *
 * Selection (fp32, each operation rounded once, no fused operations; the order below is the specification).
 *   Importance of node N from x: d = N.c - x per component, d2 = (d.x * d.x + d.y * d.y) + d.z * d.z,
 *   I = N.power / max(d2, N.r2).
 *   Pick from u = u01(w0): i = 1, p = 1.  While node i is interior with children L = link, R = link + 1:
 *   s = I_L + I_R, pl = I_L / s.  If u < pl: u = min(u / pl, 1 - 2^-24), p = p * pl, i = L.  Else: pr = I_R / s,
 *   u = min((u - pl) / pr, 1 - 2^-24), p = p * pr, i = R.  The light is the leaf's index, its probability p.
 *   Pmf of light li from x: i = 1, p = 1; for d = 0 .. paths[li].depth - 1 the same s, then p = p * (I_R / s), i = R when
 *   bit d of the trail is set, else p = p * (I_L / s), i = L.  The probability a pick returns is the pmf of the light it
 *   returns, bit for bit.
 *   Use: p replaces the light's p_sel in p_l of the light sample (vertex x) and of a BSDF hit (x = the ray's origin),
 *   operand for operand.  A one-light tree has p = 1.0f = the table's p_sel: the flag changes no bit there.
 *   Known limit.  When pl rounds to 1 (an importance ratio above 2^25) the right child is never picked while its pmf is a
 *   tiny positive number: an error of order 2^-24 in the expectation, as the 24-bit uniforms carry already.  Not branched on.
 *
 * Flag.  RTMI_FLAG_LIGHT_TREE is accepted by rtmi_render_nee only: its semantics, outputs, accepted flags and checks are
 * unchanged.  Without an attached tree (rtmi_scene_attach_light_tree) it answers RTMI_ERR_INVALID before any device work;
 * together with RTMI_FLAG_LIGHT_COOP it answers RTMI_ERR_UNSUPPORTED.  Every other entry answers the bit as an unknown flag.
 */
#ifndef RTMI_LIGHT_TREE_H
#define RTMI_LIGHT_TREE_H

#include "rtmi_nee.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTMI_FLAG_LIGHT_TREE 262144u /* bit 18 of rtmi_render_params.flags */

#define RTMI_LIGHT_TREE_LEAF 0x80000000u /* link of a leaf: this bit | the light's index in the table */

typedef struct {
    float c[3];      /* centre of the box of the lights below */
    float r2;        /* squared half-diagonal of that box */
    float power;     /* sum of area * weight below */
    uint32_t link;   /* interior: slot of the left child (even; the right one follows); leaf: RTMI_LIGHT_TREE_LEAF | light */
    uint32_t pad[2]; /* 0 */
} rtmi_light_node;   /* 32 B */

typedef struct {
    uint32_t trail; /* bit d: the light lies in the right child at depth d */
    uint32_t depth; /* depth of its leaf (the root is 0) */
} rtmi_light_path;  /* 8 B */

#define RTMI_LIGHT_TREE_PROBE_PICK 0 /* aux: n floats u in [0, 1) -> out_light, out_p */
#define RTMI_LIGHT_TREE_PROBE_PMF 1  /* aux: n uint32 light indices -> out_p (out_light is not written) */

/* The tree over the light table of a description.  Pure host code: initialises no device.  Writes at most `cap` nodes to
 * `nodes` (which may be NULL when cap is 0), the paths of the first min(cap / 2, lights) lights to `paths` (which may be
 * NULL) and the full node count, 2 * lights, to *n_nodes.  RTMI_ERR_INVALID as rtmi_lights_from_desc, and for a NULL
 * n_nodes or a cap without a buffer. */
int rtmi_light_tree_from_desc(const rtmi_scene_desc *desc, rtmi_light_node *nodes, uint32_t cap, uint32_t *n_nodes,
                              rtmi_light_path *paths);

/* The walk on the host, compiled from the inline functions the device kernels call.  points: n * 3 floats; us: n floats;
 * out_light and out_p: n entries, either may be NULL.  RTMI_ERR_INVALID for NULL nodes, points or us with n > 0, for
 * n_nodes < 2 or odd, and for a tree whose links leave the array. */
int rtmi_light_tree_pick(const rtmi_light_node *nodes, uint32_t n_nodes, const float *points, const float *us, uint32_t n,
                         uint32_t *out_light, float *out_p);
/* ... and the reverse walk: the probability of light lights[k] from points[k].  RTMI_ERR_INVALID also for NULL paths,
 * lights or out_p with n > 0 and for a light index >= n_nodes / 2. */
int rtmi_light_tree_pmf(const rtmi_light_node *nodes, uint32_t n_nodes, const rtmi_light_path *paths, const float *points,
                        const uint32_t *lights, uint32_t n, float *out_p);

/* Attaches the light table of `desc` when the handle has none yet (rtmi_scene_attach_lights), builds the tree and uploads
 * it.  Attaching a new light table detaches the tree.  RTMI_ERR_INVALID as rtmi_scene_attach_lights. */
int rtmi_scene_attach_light_tree(rtmi_scene *scene, const rtmi_scene_desc *desc);

/* The device's own walk on a batch (op = RTMI_LIGHT_TREE_PROBE_*): points n * 3 floats, aux and the outputs as the op
 * says, all host pointers.  RTMI_ERR_INVALID for NULL arguments, an unknown op, a handle without an attached tree, an
 * empty tree with n > 0 and a light index outside the table. */
int rtmi_probe_light_tree(rtmi_scene *scene, int op, const float *points, const void *aux, uint32_t n, uint32_t *out_light,
                          float *out_p);

#ifdef __cplusplus
}
#endif
#endif /* RTMI_LIGHT_TREE_H */
