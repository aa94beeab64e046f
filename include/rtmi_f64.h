/* rtmi_f64.h — opt-in f64 render mode of the MI355X (gfx950) device path.
 *
 * The reference computes in f64 throughout (Vector3<f64>; color and create_image in double).  The default device path
 * computes in fp32 under the contract of DESIGN.md.  This mode traces the same paths in double with the reference's
 * literal arithmetic: divisions where the reference divides, the reference's sphere discriminant b*b - a*c, no
 * contract substitutions.  It draws from the same Philox streams (rtmi.h), so for a given (seed, sample, pixel) it
 * follows the path of the f64 restatement of the reference in its iterative (throughput) form.  See DESIGN.md §10.
 *
 * Usage: create the handle from the fp32 description as usual (rtmi_scene_create), then attach the double planes of
 * the same scene (rtmi_scene_attach_f64) and call rtmi_render_f64.  Topology, flags, indices, images and Perlin
 * permutations come from the fp32 description already uploaded; the planes below carry every floating-point value
 * the f64 kernel reads, with the same indices and counts as the fp32 description.
 */
#ifndef RTMI_F64_H
#define RTMI_F64_H

#include "rtmi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTMI_SAMPLE_SLOT_BYTES_F64 24u /* per-sample radiance buffer of the f64 mode: three doubles per finished path */

typedef struct {
    uint32_t n_items, n_prims, n_nodes, n_xforms, n_materials, n_textures, n_perlin;
    uint32_t pad;
    const double *prim_a;    /* n_prims * 4: plane A of rtmi.h in double */
    const double *prim_b;    /* n_prims * 4: plane B of rtmi.h in double (MSPHERE: c1 - c0, time0) */
    const double *prim_dt;   /* n_prims: MSPHERE time1 - time0, the divisor of sphere.rs:115-118 (else 1) */
    const double *prim_gate; /* n_prims * 8: prim_gate of rtmi.h in double */
    const double *nodes;     /* n_nodes * 12: lmin, lmax, rmin, rmax of the reference-topology tree */
    const double *xforms;    /* n_xforms * 4: x, y, z, 0 of every rtmi_xform (also RTMI_XF_INNER_MEDIUM and the gate records) */
    const double *item_neg_inv_density; /* n_items: MEDIUM items' -(1/density) */
    const double *item_root;            /* n_items * 6: BVH items' root box min.xyz, max.xyz */
    const double *material_param;       /* n_materials: fuzz | ref_idx */
    const double *texture_f;            /* n_textures * 4: f0..f3 (SOLID r,g,b | NOISE scale) */
    const double *perlin_ranvec;        /* n_perlin * 768: the 256 unit vectors x, y, z of each table */
} rtmi_scene_f64;

/* Camera state (src/camera.rs:8-18) in double */
typedef struct {
    double origin[3], lower_left_corner[3], horizontal[3], vertical[3], u[3], v[3];
    double time0, time1, lens_radius;
} rtmi_camera_f64;

/* Checks that the counts match the handle and that every plane the handle needs is present (a plane may be NULL only
 * when its count is 0), then uploads the planes to the handle's device.  They are freed with the handle; a second
 * call replaces them.  RTMI_ERR_INVALID on a mismatch. */
int rtmi_scene_attach_f64(rtmi_scene *scene, const rtmi_scene_f64 *planes);

/* Blocking whole-image render in double (tile_world must be 1).  t_min is a double because rtmi_render_params.t_min is
 * a float (0.001f != 0.001); params->t_min is ignored.
 *   out_linear_rgb: ny*nx*3 doubles, row 0 = top row; may be NULL
 *   out_rgb8:       ny*nx*3 bytes, the quantisation of tests/test.rs:71-78; may be NULL
 *   out_path_sig:   ny*nx path signatures (rtmi.h; the fp32 bits of (float)t are mixed); optional, sets RTMI_FLAG_PATH_SIG
 * Honours SKY, FACE_FORWARD, UV_BOOK and PATH_SIG; FAST_CULL, SYNC and REF_TREE are accepted and ignored (the mode
 * always walks the reference tree exactly).  RTMI_ERR_UNSUPPORTED for PROGRESSIVE, ASYNC, BLOCK_COOP, PROFILE,
 * TEST_OVERFLOW and for scenes with DEFERRED, LISTSCAN or NESTED_MEDIUM items; RTMI_ERR_INVALID without attached planes.
 * sample_buffer_bytes budgets RTMI_SAMPLE_SLOT_BYTES_F64 per pixel sample; a smaller budget renders in passes (same
 * result). */
int rtmi_render_f64(rtmi_scene *scene, const rtmi_camera_f64 *cam, const rtmi_render_params *params, double t_min,
                    double *out_linear_rgb, uint8_t *out_rgb8, uint64_t *out_path_sig, rtmi_stats *stats);

/* The f64 kernel's arithmetic on the device, for tests: op 0 sin(x), 1 log(x), 2 atan2(x, y), 3 asin(x), 4 x / y,
 * 5 sqrt(x).  y is read by ops 2 and 4 only (may be NULL otherwise). */
int rtmi_probe_math_f64(int op, const double *x, const double *y, double *out, uint32_t n);

#ifdef __cplusplus
}
#endif
#endif /* RTMI_F64_H */
