// rtmi_f64_kernels.hpp — the f64 render mode (include/rtmi_f64.h): per-lane render kernel, resolve and math probe in
// double.  The arithmetic mirrors the non-DEVICE_ARITH branches of the f64 restatement of the reference (the oracle),
// function by function: divisions where the reference divides, the discriminant b*b - a*c, (p + n + r) - p for the
// Lambertian direction.  Compiled with -ffp-contract=off like the fp32 kernels: no fused operations.
// Topology (items, node children, primitive types and flags, transform kinds, material and texture kinds, Perlin
// permutations, images) comes from the fp32 scene's device copy; every floating-point value from the attached planes.
// Part of the translation unit rtmi_f64.hip.  The fp32 headers are included for the work queue (WaveWork, work_take) and
// the Philox draws only; nothing of them is changed.
#pragma once
#include "rtmi_f64_types.hpp"
#include "rtmi_shade.hpp"
#include "rtmi_sin_f64.hpp"

__device__ __forceinline__ D3 d3(double x, double y, double z) { return D3{x, y, z}; }
__device__ __forceinline__ D3 operator+(D3 a, D3 b) { return d3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ D3 operator-(D3 a, D3 b) { return d3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ D3 operator-(D3 a) { return d3(-a.x, -a.y, -a.z); }
__device__ __forceinline__ D3 operator*(D3 a, double s) { return d3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ D3 operator*(D3 a, D3 b) { return d3(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ D3 ddiv(D3 a, double s) { return d3(a.x / s, a.y / s, a.z / s); }
__device__ __forceinline__ double ddot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ double dnorm(D3 a) { return __builtin_sqrt(ddot(a, a)); }
__device__ __forceinline__ D3 dnormalize(D3 a) { return ddiv(a, dnorm(a)); }
__device__ __forceinline__ double dget(D3 a, int i) { return i == 0 ? a.x : (i == 1 ? a.y : a.z); }
__device__ __forceinline__ void dset(D3 &a, int i, double v) {
    if (i == 0) a.x = v; else if (i == 1) a.y = v; else a.z = v;
}

#define RTMI_DBL_MAX 1.79769313486231570814527423731704357e+308

struct RayD { // Ray (ray.rs:3-29) with the 1/d of aabb.rs:33 cached per frame
    D3 o, d, inv_d;
};
__device__ __forceinline__ void rayd_derive(RayD &r) { r.inv_d = d3(1.0 / r.d.x, 1.0 / r.d.y, 1.0 / r.d.z); }

// ---- transforms — traslate.rs:18-24, rotate.rs:85-113 ----------------------------------
__device__ __forceinline__ void plane_axes(int plane, int &k, int &a, int &b) { // rect.rs:40-44; Axis uses the same triples
    k = plane; a = plane == 0 ? 1 : (plane == 1 ? 2 : 0); b = plane == 0 ? 2 : (plane == 1 ? 0 : 1);
}
__device__ __forceinline__ bool xf_ray_one(int kind, const double *X, D3 &o, D3 &d) {
    if (kind == RTMI_XF_TRANSLATE) { o = o - d3(X[0], X[1], X[2]); return false; }
    int r, a, b;
    plane_axes(kind - RTMI_XF_ROTATE_X, r, a, b);
    const double s = X[0], c = X[1];
    const D3 oo = o, od = d;
    dset(o, a, c * dget(oo, a) + s * dget(oo, b));
    dset(o, b, -s * dget(oo, a) + c * dget(oo, b));
    dset(d, a, c * dget(od, a) + s * dget(od, b));
    dset(d, b, -s * dget(od, a) + c * dget(od, b));
    return true;
}
__device__ __forceinline__ void xf_hit_one(int kind, const double *X, D3 &p, D3 &n) {
    if (kind == RTMI_XF_TRANSLATE) { p = p + d3(X[0], X[1], X[2]); return; }
    int r, a, b;
    plane_axes(kind - RTMI_XF_ROTATE_X, r, a, b);
    const double s = X[0], c = X[1];
    const D3 op = p, on = n;
    dset(p, a, c * dget(op, a) - s * dget(op, b));
    dset(p, b, s * dget(op, a) + c * dget(op, b));
    dset(n, a, c * dget(on, a) - s * dget(on, b));
    dset(n, b, s * dget(on, a) + c * dget(on, b));
}
// world -> object through xforms[first, first + count), outermost first
__device__ __forceinline__ void xf_ray(const DevScene &sc, const DevSceneF64 &w, int first, int count, D3 &o, D3 &d) {
    for (int k = 0; k < count; k++) xf_ray_one(sc.xforms[first + k].kind, w.xforms + 4 * (size_t)(first + k), o, d);
}
// object -> world, innermost first
__device__ __forceinline__ void xf_hit(const DevScene &sc, const DevSceneF64 &w, int first, int count, D3 &p, D3 &n) {
    for (int k = count - 1; k >= 0; k--) xf_hit_one(sc.xforms[first + k].kind, w.xforms + 4 * (size_t)(first + k), p, n);
}

// ---- AABB::hit — aabb.rs:31-44, the sequential form of the oracle ---------------------
__device__ __forceinline__ bool aabb_hit_d(const double *mn, const double *mx, const RayD &r, double t_min, double t_max) {
    for (int a = 0; a < 3; a++) {
        const double inv_d = dget(r.inv_d, a);
        double t0 = (mn[a] - dget(r.o, a)) * inv_d;
        double t1 = (mx[a] - dget(r.o, a)) * inv_d;
        if (inv_d < 0.0) { const double tmp = t0; t0 = t1; t1 = tmp; }
        t_min = fmax(t_min, t0);
        t_max = fmin(t_max, t1);
        if (t_max <= t_min) return false;
    }
    return true;
}

// ---- primitives — sphere.rs:37-77, rect.rs:39-69, cube.rs:84-86 ------------------------
__device__ __forceinline__ bool sphere_test_d(const RayD &r, D3 c, double radius, double t_min, double t_max, double &t_out) {
    const D3 oc = r.o - c;
    const double a = ddot(r.d, r.d);
    const double b = ddot(oc, r.d);
    const double cc = ddot(oc, oc) - radius * radius;
    const double disc = b * b - a * cc;
    if (disc > 0.0) {
        const double sq = __builtin_sqrt(disc);
        double t = (-b - sq) / a;
        if (t < t_max && t > t_min) { t_out = t; return true; }
        t = (-b + sq) / a;
        if (t < t_max && t > t_min) { t_out = t; return true; }
    }
    return false;
}
__device__ __forceinline__ D3 moving_center_d(const double *A, const double *B, double dt, double time) {
    const double f = (time - B[3]) / dt;
    return d3(A[0], A[1], A[2]) + d3(B[0], B[1], B[2]) * f;
}
__device__ __forceinline__ bool rect_test_d(int plane, double x0, double y0, double x1, double y1, double k, const RayD &r,
                                            double t_min, double t_max, double &t_out) {
    int ka, aa, ba;
    plane_axes(plane, ka, aa, ba);
    const double t = (k - dget(r.o, ka)) / dget(r.d, ka);
    if (t < t_min || t > t_max) return false;
    const double x = dget(r.o, aa) + t * dget(r.d, aa);
    const double y = dget(r.o, ba) + t * dget(r.d, ba);
    if (x < x0 || x > x1 || y < y0 || y > y1) return false;
    t_out = t;
    return true;
}
// the six rects of a Cube in construction order (cube.rs:21-74), scanned like a HittableList
__device__ __forceinline__ void cube_face(const double *A, const double *B, int f, int &plane, double &x0, double &y0,
                                          double &x1, double &y1, double &k) {
    const double ax = A[0], ay = A[1], az = A[2], bx = A[3], by = B[0], bz = B[1];
    if (f < 2) { plane = 2; x0 = ax; y0 = ay; x1 = bx; y1 = by; k = f == 0 ? bz : az; }
    else if (f < 4) { plane = 1; x0 = az; y0 = ax; x1 = bz; y1 = bx; k = f == 2 ? by : ay; }
    else { plane = 0; x0 = ay; y0 = az; x1 = by; y1 = bz; k = f == 4 ? bx : ax; }
}
__device__ __forceinline__ bool prim_test_d(const DevScene &sc, const DevSceneF64 &w, int idx, const RayD &r0, double time,
                                            double t_min, double t_max, double &t_out, int &pf) {
    const rtmi_prim_meta M = sc.meta[idx];
    const double *A = w.prim_a + 4 * (size_t)idx, *B = w.prim_b + 4 * (size_t)idx;
    RayD r = r0;
    const int xc = (int)((M.flags >> RTMI_PRIMFLAG_XF_COUNT_SHIFT) & RTMI_PRIM_XF_MAX);
    if (xc > 0) {
        xf_ray(sc, w, (int)(M.flags >> RTMI_PRIMFLAG_XF_FIRST_SHIFT), xc, r.o, r.d);
        rayd_derive(r);
    }
    bool h = false;
    int face = 0;
    if (M.type == RTMI_PRIM_SPHERE) {
        h = sphere_test_d(r, d3(A[0], A[1], A[2]), A[3], t_min, t_max, t_out);
    } else if (M.type == RTMI_PRIM_MSPHERE) {
        h = sphere_test_d(r, moving_center_d(A, B, w.prim_dt[idx], time), A[3], t_min, t_max, t_out);
    } else if (M.type == RTMI_PRIM_RECT) {
        h = rect_test_d((int)((M.flags >> RTMI_PRIMFLAG_PLANE_SHIFT) & 3u), A[0], A[1], A[2], A[3], B[0], r, t_min, t_max, t_out);
    } else {
        double cl = t_max;
        for (int f = 0; f < 6; f++) {
            int plane;
            double x0, y0, x1, y1, k, t;
            cube_face(A, B, f, plane, x0, y0, x1, y1, k);
            if (rect_test_d(plane, x0, y0, x1, y1, k, r, t_min, cl, t)) { cl = t; face = f; h = true; }
        }
        if (h) t_out = cl;
    }
    pf = (idx << 3) | face;
    return h;
}

// ---- BVHNode::hit — bvh.rs:70-89, the exact walk of the reference tree (order of rtmi_bvh.hpp, FAST = false) -------
__device__ __forceinline__ bool bvh_query_d(const DevScene &sc, const DevSceneF64 &w, int root, const RayD &r, double time,
                                            double t_min, double t_max, uint32_t *stack, double &t_out, int &pf_out) {
    bool have = false;
    double bt = 0.0;
    int bpf = 0;
    int sp = 0;
    int cur = root;
    for (;;) {
        if (cur >= 0) {
            const float4 n3 = sc.nodes[(size_t)cur * 4 + 3];
            const int left = __float_as_int(n3.x), right = __float_as_int(n3.y);
            const double *nb = w.nodes + 12 * (size_t)cur;
            const bool vl = left < 0 || aabb_hit_d(nb, nb + 3, r, t_min, t_max);
            bool vr = right < 0 || aabb_hit_d(nb + 6, nb + 9, r, t_min, t_max);
            if (right == left) vr = false; // BVHNode over one object: the same answer twice
            if (vl) {
                if (vr) { stack[sp * 64] = (uint32_t)right; sp++; }
                cur = left;
                continue;
            }
            if (vr) { cur = right; continue; }
        } else {
            const int idx = (int)((uint32_t)cur & 0x0fffffffu);
            double t;
            int pf;
            if (prim_test_d(sc, w, idx, r, time, t_min, t_max, t, pf)) {
                if (!have || !(bt < t)) { bt = t; bpf = pf; have = true; } // ties -> the later (right) leaf
            }
        }
        if (sp == 0) break;
        sp--;
        cur = (int)stack[sp * 64];
    }
    t_out = bt;
    pf_out = bpf;
    return have;
}
__device__ __forceinline__ bool geom_query_d(const DevScene &sc, const DevSceneF64 &w, int item, const rtmi_item &I, const RayD &r,
                                             double time, double q_min, double q_max, uint32_t *stack, double &t_out, int &pf_out) {
    if (I.kind == RTMI_ITEM_BVH) {
        const double *rb = w.item_root + 6 * (size_t)item;
        if (!aabb_hit_d(rb, rb + 3, r, q_min, q_max)) return false;
        return bvh_query_d(sc, w, I.first, r, time, q_min, q_max, stack, t_out, pf_out);
    }
    double cl = q_max;
    bool any = false;
    for (int k = 0; k < I.count; k++) {
        double t;
        int pf;
        if (prim_test_d(sc, w, I.first + k, r, time, q_min, cl, t, pf)) { cl = t; any = true; pf_out = pf; }
    }
    t_out = cl;
    return any;
}

// ---- samplers — util.rs:4-24 (the 24-bit uniforms of rtmi_u01 are exact in double) ------------------------------------
__device__ __forceinline__ double u01d(uint32_t w) { return (double)rtmi_u01(w); }
__device__ __forceinline__ D3 random_in_unit_sphere_d(RngReg &g, uint32_t k0, uint32_t k1) {
    for (;;) {
        uint32_t w0, w1, w2;
        rng_take3(g, k0, k1, w0, w1, w2);
        const D3 p = d3(2.0 * u01d(w0) - 1.0, 2.0 * u01d(w1) - 1.0, 2.0 * u01d(w2) - 1.0);
        if (ddot(p, p) < 1.0) return p;
    }
}
__device__ __forceinline__ D3 random_in_unit_disk_d(RngReg &g, uint32_t k0, uint32_t k1) {
    for (;;) {
        uint32_t w0, w1;
        rng_take2(g, k0, k1, w0, w1);
        const D3 p = d3(2.0 * u01d(w0) - 1.0, 2.0 * u01d(w1) - 1.0, 2.0 * 0.0 - 0.0);
        if (ddot(p, p) < 1.0) return p;
    }
}
__device__ __forceinline__ double rng_uniform_d(RngReg &g, uint32_t k0, uint32_t k1) { return (double)rng_uniform(g, k0, k1); }

// ---- textures — texture.rs, perlin.rs -------------------------------------------------------------------------------
// f64::sin (texture.rs:41, :68): below 2^40 the double-double sine of rtmi_sin_f64.hpp, rounded once; it is what glibc's
// returns for all but about 1 argument in 1000.  The device library's beyond.  One copy, called.
__device__ __noinline__ double sin_d(double x) { return fabs(x) < rtmi_sin64::SIN_CR_LIMIT ? rtmi_sin64::sin_cr(x) : sin(x); }
__device__ __forceinline__ uint64_t as_usize_d(double x) { // Rust `f64 as usize`: saturating, NaN -> 0
    if (!(x > 0.0)) return 0ull;
    if (x >= 18446744073709551615.0) return ~0ull;
    return (uint64_t)x;
}
__device__ double perlin_noise_d(const DevScene &sc, const DevSceneF64 &w, int table, D3 p) {
    const rtmi_perlin *pn = sc.perlin + table;
    const double *rv = w.ranvec + 768 * (size_t)table;
    const double u = p.x - floor(p.x), v = p.y - floor(p.y), ww = p.z - floor(p.z);
    const uint64_t i = as_usize_d(floor(p.x)), j = as_usize_d(floor(p.y)), k = as_usize_d(floor(p.z));
    const double uu = u * u * (3.0 - 2.0 * u);
    const double vv = v * v * (3.0 - 2.0 * v);
    const double wu = ww * ww * (3.0 - 2.0 * ww);
    double accum = 0.0;
    for (int di = 0; di < 2; di++)
        for (int dj = 0; dj < 2; dj++)
            for (int dk = 0; dk < 2; dk++) {
                const int h = pn->perm[(i + di) & 255u] ^ pn->perm[256 + ((j + dj) & 255u)] ^ pn->perm[512 + ((k + dk) & 255u)];
                const D3 c = d3(rv[3 * h], rv[3 * h + 1], rv[3 * h + 2]);
                const D3 weight = d3(u - (double)di, v - (double)dj, ww - (double)dk);
                accum += ((double)di * uu + (double)(1 - di) * (1.0 - uu)) * ((double)dj * vv + (double)(1 - dj) * (1.0 - vv)) *
                         ((double)dk * wu + (double)(1 - dk) * (1.0 - wu)) * ddot(c, weight);
            }
    return accum;
}
__device__ D3 tex_value_d(const DevScene &sc, const DevSceneF64 &w, int tex, double u, double v, D3 p) {
    for (int guard = 0; guard < 16; guard++) {
        const rtmi_texture t = sc.texs[tex];
        const double *f = w.texf + 4 * (size_t)tex;
        if (t.kind == RTMI_TEX_CHECKER) { // texture.rs:39-48
            const double s = sin_d(10.0 * p.x) * sin_d(10.0 * p.y) * sin_d(10.0 * p.z);
            tex = s < 0.0 ? t.i0 : t.i1;
            continue;
        }
        if (t.kind == RTMI_TEX_NOISE) { // texture.rs:65-71, perlin.rs:99-109: turb gets the unscaled p
            double accum = 0.0, weight = 1.0;
            D3 tp = p;
            for (int o = 0; o < 7; o++) {
                accum += weight * perlin_noise_d(sc, w, t.i0, tp);
                weight *= 0.5;
                tp = tp * 2.0;
            }
            const double g = 0.5 * (1.0 + sin_d(f[0] * p.x + 5.0 * fabs(accum)));
            return d3(g, g, g);
        }
        if (t.kind == RTMI_TEX_IMAGE) { // texture.rs:86-108
            const rtmi_image im = sc.images[t.i0];
            const uint64_t nx = im.nx, ny = im.ny;
            uint64_t i = as_usize_d(u * (double)nx), j = as_usize_d((1.0 - v) * (double)ny);
            if (i > nx - 1) i = nx - 1;
            if (j > ny - 1) j = ny - 1;
            const uint8_t *px = sc.image_data + im.offset + 3 * i + 3 * nx * j;
            return d3((double)px[0] / 255.0, (double)px[1] / 255.0, (double)px[2] / 255.0);
        }
        return d3(f[0], f[1], f[2]);
    }
    return d3(1.0, 1.0, 1.0); // unreachable: rtmi_scene_create rejects deeper nests
}

// ---- materials — material.rs:9-28 --------------------------------------------------------------------------------------
__device__ __forceinline__ D3 reflect_d(D3 v, D3 n) { return v - n * (2.0 * ddot(v, n)); }
__device__ __forceinline__ bool refract_d(D3 v, D3 n, double ni_over_nt, D3 &out) {
    const D3 uv = dnormalize(v);
    const double dt = ddot(uv, n);
    const double disc = 1.0 - ni_over_nt * ni_over_nt * (1.0 - dt * dt);
    if (disc > 0.0) {
        out = (uv - n * dt) * ni_over_nt - n * __builtin_sqrt(disc);
        return true;
    }
    return false;
}
__device__ __forceinline__ double schlick_d(double cosine, double ref_idx) {
    double r0 = (1.0 - ref_idx) / (1.0 + ref_idx);
    r0 = r0 * r0;
    const double x = 1.0 - cosine;
    const double x2 = x * x;
    const double x4 = x2 * x2;
    return r0 + (1.0 - r0) * (x * x4);
}
__device__ __forceinline__ D3 sky_color_d(D3 d) { // color.rs:18-20
    const D3 unit = dnormalize(d);
    const double t = 0.5 * (unit.y + 1.0);
    const double a = 1.0 - t;
    return d3(a * 1.0 + t * 0.5, a * 1.0 + t * 0.7, a * 1.0 + t * 1.0);
}

struct PathD {
    D3 ro, rd;
    double rtime;
    D3 T, L;
    uint32_t depth;
};

// Camera::get_ray — camera.rs:53-67, after u, v of tests/test.rs:66-67
__device__ __forceinline__ void camera_sample_d(const DevCameraF64 &cam, const DevParams &P, RngReg &g, uint32_t k0, uint32_t k1,
                                                uint32_t s, uint32_t pixel, uint32_t px, uint32_t j, PathD &pa) {
    rng_init(g, s, pixel);
    uint32_t wu, wv;
    rng_take2(g, k0, k1, wu, wv);
    const double u = ((double)px + u01d(wu)) / (double)P.nx;
    const double v = ((double)j + u01d(wv)) / (double)P.ny;
    D3 origin = cam.origin;
    if (cam.lens_radius != 0.0) {
        const D3 rd = random_in_unit_disk_d(g, k0, k1) * cam.lens_radius;
        origin = cam.origin + (cam.u * rd.x + cam.v * rd.y);
    }
    pa.rtime = cam.time0 + rng_uniform_d(g, k0, k1) * (cam.time1 - cam.time0);
    pa.ro = origin;
    pa.rd = cam.llc + cam.horizontal * u + cam.vertical * v - origin;
    pa.T = d3(1, 1, 1);
    pa.L = d3(0, 0, 0);
    pa.depth = 0;
}

// ConstantMedium::hit after its two boundary queries — medium.rs:32-45
__device__ __forceinline__ bool medium_sample_d(double t1, double t2, double t_min, double t_max, double dn, double nid, RngReg &g,
                                                uint32_t k0, uint32_t k1, double &t_out) {
    if (t1 < t_min) t1 = t_min;
    if (t2 > t_max) t2 = t_max;
    if (t1 < t2) {
        const double dist_inside = (t2 - t1) * dn;
        const double hit_distance = nid * log(rng_uniform_d(g, k0, k1));
        if (hit_distance < dist_inside) {
            t_out = t1 + hit_distance / dn;
            return true;
        }
    }
    return false;
}
// the ray direction's norm as the medium sees it: inside the `outer` wrappers that hold the medium itself
__device__ __forceinline__ double medium_dir_norm_d(const DevScene &sc, const DevSceneF64 &w, uint32_t flags, int xform_first, D3 o, D3 d) {
    const int outer = (int)((flags >> RTMI_ITEMFLAG_MEDIUM_OUTER_SHIFT) & 15u);
    if (outer > 0) xf_ray(sc, w, xform_first, outer, o, d);
    return dnorm(d);
}

// hit record + Material::{emitted, scatter} of the closest hit (the oracle's color_throughput body); false: the path ends
__device__ bool shade_hit_d(const DevScene &sc, const DevSceneF64 &w, uint32_t max_depth, uint32_t ext, RngReg &g, uint32_t k0, uint32_t k1,
                            double closest, int best_item, int best_pf, bool best_medium, PathD &pa) {
    const rtmi_item I = sc.items[best_item].it;
    D3 hp, hn;
    double hu = 0.0, hv = 0.0;
    int mat;
    if (best_medium) {
        mat = I.medium_material;
        const int outer = (int)((I.flags >> RTMI_ITEMFLAG_MEDIUM_OUTER_SHIFT) & 15u);
        D3 lo = pa.ro, ld = pa.rd;
        if (outer > 0) xf_ray(sc, w, I.xform_first, outer, lo, ld);
        hp = lo + ld * closest; // medium.rs:47-48
        hn = d3(1.0, 0.0, 0.0);
        if (outer > 0) xf_hit(sc, w, I.xform_first, outer, hp, hn);
    } else {
        const int idx = best_pf >> 3, face = best_pf & 7;
        const rtmi_prim_meta M = sc.meta[idx];
        mat = M.material;
        const double *A = w.prim_a + 4 * (size_t)idx, *B = w.prim_b + 4 * (size_t)idx;
        D3 lo = pa.ro, ld = pa.rd;
        xf_ray(sc, w, I.xform_first, I.xform_count, lo, ld);
        const int pxc = (int)((M.flags >> RTMI_PRIMFLAG_XF_COUNT_SHIFT) & RTMI_PRIM_XF_MAX);
        const int pxf = (int)(M.flags >> RTMI_PRIMFLAG_XF_FIRST_SHIFT);
        if (pxc > 0) xf_ray(sc, w, pxf, pxc, lo, ld);
        hp = lo + ld * closest; // ray.pointing_at(t)
        if (M.type == RTMI_PRIM_SPHERE || M.type == RTMI_PRIM_MSPHERE) { // sphere.rs:48-52
            const D3 c = M.type == RTMI_PRIM_MSPHERE ? moving_center_d(A, B, w.prim_dt[idx], pa.rtime) : d3(A[0], A[1], A[2]);
            hn = ddiv(hp - c, A[3]);
            if (sc.mats[mat].flags & RTMI_MATFLAG_NEEDS_UV) { // sphere.rs:9-15
                const double phi = atan2(hn.z, hn.x), theta = asin(hn.y);
                const double PI = 3.14159265358979323846264338327950288;
                hu = 1.0 - (phi + PI) / (2.0 * PI);
                hv = (theta + ((ext & RTMI_EXT_UV_BOOK) ? 1.57079632679489661923132169163975144 : 0.636619772367581343075535053490057448)) / PI;
            }
        } else { // rect.rs:52-59 (a cube face is its rect)
            int plane;
            double x0, y0, x1, y1, k;
            if (M.type == RTMI_PRIM_RECT) {
                plane = (int)((M.flags >> RTMI_PRIMFLAG_PLANE_SHIFT) & 3u);
                x0 = A[0]; y0 = A[1]; x1 = A[2]; y1 = A[3];
            } else {
                cube_face(A, B, face, plane, x0, y0, x1, y1, k);
            }
            int ka, aa, ba;
            plane_axes(plane, ka, aa, ba);
            const double x = dget(lo, aa) + closest * dget(ld, aa), y = dget(lo, ba) + closest * dget(ld, ba);
            hu = (x - x0) / (x1 - x0);
            hv = (y - y0) / (y1 - y0);
            hn = d3(0, 0, 0);
            dset(hn, ka, 1.0);
        }
        if (pxc > 0) xf_hit(sc, w, pxf, pxc, hp, hn);
        xf_hit(sc, w, I.xform_first, I.xform_count, hp, hn);
        if (((M.flags ^ I.flags) & 1u) != 0u) hn = -hn; // FlipNormals — hittable.rs:78-83
    }
    const rtmi_material Mt = sc.mats[mat];
    const double param = w.mparam[mat];
    if (Mt.kind == RTMI_MAT_DIFFUSE_LIGHT) pa.L = pa.L + pa.T * tex_value_d(sc, w, Mt.tex, hu, hv, hp);
    if (pa.depth >= max_depth) return false; // color.rs:9
    const D3 rd = pa.rd;
    if ((ext & RTMI_EXT_FACE_FORWARD) && Mt.kind != RTMI_MAT_DIELECTRIC && ddot(rd, hn) > 0.0) hn = -hn;
    D3 nd, att = d3(1, 1, 1);
    if (Mt.kind == RTMI_MAT_LAMBERTIAN) { // material.rs:49-53
        const D3 rs = random_in_unit_sphere_d(g, k0, k1);
        const D3 target = (hp + hn) + rs;
        nd = target - hp;
        att = tex_value_d(sc, w, Mt.tex, hu, hv, hp);
    } else if (Mt.kind == RTMI_MAT_METAL) { // material.rs:75-87
        D3 refl = reflect_d(dnormalize(rd), hn);
        if (param > 0.0) refl = refl + random_in_unit_sphere_d(g, k0, k1) * param;
        if (!(ddot(refl, hn) > 0.0)) return false;
        nd = refl;
        att = tex_value_d(sc, w, Mt.tex, hu, hv, hp);
    } else if (Mt.kind == RTMI_MAT_DIELECTRIC) { // material.rs:106-126
        D3 outward;
        double ni_over_nt, cosine;
        const double ddn = ddot(rd, hn);
        if (ddn > 0.0) {
            cosine = param * ddn / dnorm(rd);
            outward = -hn;
            ni_over_nt = param;
        } else {
            cosine = -ddn / dnorm(rd);
            outward = hn;
            ni_over_nt = 1.0 / param;
        }
        D3 refr;
        bool took = false;
        if (refract_d(rd, outward, ni_over_nt, refr)) {
            if (rng_uniform_d(g, k0, k1) >= schlick_d(cosine, param)) { nd = refr; took = true; }
        }
        if (!took) nd = reflect_d(rd, hn);
    } else if (Mt.kind == RTMI_MAT_ISOTROPIC) { // material.rs:165-168
        nd = random_in_unit_sphere_d(g, k0, k1);
        att = tex_value_d(sc, w, Mt.tex, hu, hv, hp);
    } else {
        return false; // DiffuseLight does not scatter (material.rs:144-146)
    }
    pa.T = pa.T * att;
    pa.ro = hp;
    pa.rd = nd;
    pa.depth++;
    return true;
}

// world.hit(ray, t_min, f64::MAX): the scan of the top-level list (hittable.rs:37-47)
__device__ __forceinline__ bool world_hit_d(const DevScene &sc, const DevSceneF64 &w, const PathD &pa, double t_min, uint32_t *stack,
                                            RngReg &g, uint32_t k0, uint32_t k1, double &closest, int &best_item, int &best_pf,
                                            bool &best_medium) {
    closest = RTMI_DBL_MAX;
    best_item = -1; best_pf = 0; best_medium = false;
    for (uint32_t it = 0; it < sc.n_items; it++) {
        const rtmi_item I = sc.items[it].it;
        RayD R;
        R.o = pa.ro; R.d = pa.rd;
        xf_ray(sc, w, I.xform_first, I.xform_count, R.o, R.d);
        rayd_derive(R);
        double t;
        int pf = 0;
        if (!(I.flags & RTMI_ITEMFLAG_MEDIUM)) {
            if (geom_query_d(sc, w, (int)it, I, R, pa.rtime, t_min, closest, stack, t, pf)) {
                closest = t; best_item = (int)it; best_pf = pf; best_medium = false;
            }
        } else { // ConstantMedium::hit — medium.rs:28-56
            double t1, t2, tm;
            if (geom_query_d(sc, w, (int)it, I, R, pa.rtime, -RTMI_DBL_MAX, RTMI_DBL_MAX, stack, t1, pf) &&
                geom_query_d(sc, w, (int)it, I, R, pa.rtime, t1 + 0.0001, RTMI_DBL_MAX, stack, t2, pf)) {
                const double dn = medium_dir_norm_d(sc, w, I.flags, I.xform_first, pa.ro, pa.rd);
                if (medium_sample_d(t1, t2, t_min, closest, dn, w.item_nid[it], g, k0, k1, tm)) {
                    closest = tm; best_item = (int)it; best_medium = true;
                }
            }
        }
    }
    return best_item >= 0;
}

// Per-lane render kernel in double: the schedule of rtmi_render_kernel<false, SIG, false> (work queue, two phases: trace
// until enough lanes hold a hit, then shade them), the exact walk of the reference tree, double arithmetic throughout.
template <bool SIG>
__global__ __launch_bounds__(64) void rtmi_render_f64_kernel(DevScene sc, DevSceneF64 w, DevCameraF64 cam, DevParams P, DevParamsF64 Q) {
    __shared__ uint32_t lds_stack[RTMI_MAX_BVH_DEPTH][64];
    const int lane = threadIdx.x & 63;
    uint32_t *stack = &lds_stack[0][lane];
    unsigned long long sig = 0ull;
    WaveWork wk;
    wk.ltile = 0u; wk.ps_base = 0u; wk.obase = 0u; wk.x0 = 0u; wk.y0 = 0u; wk.cols = 0u; wk.n_valid = 0u; wk.next = 0u; wk.total = 0u;
    bool queue_empty = false;
    const uint32_t k0 = P.key0, k1 = P.key1;
    const int threshold = (int)P.shade_threshold;
    uint32_t oidx = 0u, ltile = 0u;
    bool alive = false, done = false, have_hit = false;
    RngReg g;
    rng_init(g, 0, 0);
    PathD pa;
    pa.ro = d3(0, 0, 0); pa.rd = d3(0, 0, 1); pa.rtime = 0.0; pa.T = d3(1, 1, 1); pa.L = d3(0, 0, 0); pa.depth = 0;
    double closest = RTMI_DBL_MAX;
    int best_item = -1, best_pf = 0;
    bool best_medium = false;
    const auto finish = [&]() {
        double *o = Q.samples + 3 * (size_t)oidx;
        o[0] = pa.L.x; o[1] = pa.L.y; o[2] = pa.L.z;
        if (SIG) { atomicAdd(P.path_sig + (size_t)ltile * 64 + (oidx & 63u), sig); sig = 0ull; }
        alive = false;
    };
    for (;;) {
        for (;;) { // phase A: trace
            if (__ballot(!have_hit && !done) == 0ull) break;
            {
                const bool want = !have_hit && !done && !alive;
                if (__ballot(want) != 0ull) {
                    uint32_t smp = 0u, px = 0u, j = 0u;
                    if (work_take(wk, queue_empty, want, P, oidx, ltile, smp, px, j)) {
                        camera_sample_d(cam, P, g, k0, k1, smp, j * P.nx + px, px, j, pa);
                        alive = true;
                    } else if (want) {
                        done = true;
                    }
                }
            }
            if (!have_hit && !done) {
                if (world_hit_d(sc, w, pa, Q.t_min, stack, g, k0, k1, closest, best_item, best_pf, best_medium)) {
                    have_hit = true;
                } else { // miss: black background (color.rs:21), or the sky extension
                    if (P.sky) pa.L = pa.L + pa.T * sky_color_d(pa.rd);
                    finish();
                }
            }
            if (__popcll(__ballot(have_hit)) >= threshold) break;
        }
        if (__ballot(have_hit) == 0ull) break;
        if (have_hit) { // phase B: shade
            have_hit = false;
            if (SIG) sig += (unsigned long long)sig_mix(__float_as_uint((float)closest), pa.depth);
            if (!shade_hit_d(sc, w, P.max_depth, P.ext, g, k0, k1, closest, best_item, best_pf, best_medium, pa)) finish();
        }
    }
}

// `col += color(..)` in sample order, then the mean and the quantisation of tests/test.rs:69-78, per local texel, in
// double; one thread per (local tile, pixel).  acc carries the sums between passes.  out_lin: [local tile][64][3].
__global__ __launch_bounds__(256) void rtmi_resolve_f64_kernel(const double *__restrict__ samples, double *__restrict__ acc,
                                                               double *__restrict__ out_lin, uint32_t *__restrict__ out_q,
                                                               DevParams P, int first, int last) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= P.ntiles_local * 64u) return;
    const uint32_t ltile = tid >> 6, lane = tid & 63u;
    const uint32_t tile = ltile * P.tile_world + P.tile_rank;
    const uint32_t ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
    const bool in_image = tx * RTMI_TILE + (lane & 7u) < P.nx && ty * RTMI_TILE + (lane >> 3) < P.ny;
    double sum[3] = {0.0, 0.0, 0.0};
    if (!first) { sum[0] = acc[3 * (size_t)tid]; sum[1] = acc[3 * (size_t)tid + 1]; sum[2] = acc[3 * (size_t)tid + 2]; }
    if (in_image) {
        const double *src = samples + 3 * (((size_t)ltile * P.pass_stride) * 64u + lane);
        for (uint32_t s = 0; s < P.pass_cnt; s++) {
            const double *v = src + 3 * (size_t)s * 64u;
            sum[0] += v[0]; sum[1] += v[1]; sum[2] += v[2];
        }
    }
    if (!last) {
        acc[3 * (size_t)tid] = sum[0]; acc[3 * (size_t)tid + 1] = sum[1]; acc[3 * (size_t)tid + 2] = sum[2];
        return;
    }
    uint32_t q[3];
    for (int ch = 0; ch < 3; ch++) {
        const double m = sum[ch] / (double)P.ns;
        out_lin[3 * (size_t)tid + ch] = m;
        double gm = sqrt(m);
        gm = (gm > 0.0) ? ((gm < 1.0) ? gm : 1.0) : 0.0; // nalgebra::clamp; NaN -> 0
        const double x = 255.99 * gm;
        q[ch] = (x != x) ? 0u : (uint32_t)(int32_t)x;
    }
    out_q[tid] = q[0] | (q[1] << 8) | (q[2] << 16);
}

// the functions of the f64 kernel, for tests (rtmi_probe_math_f64)
__global__ void rtmi_math_probe_f64_kernel(int op, const double *x, const double *y, double *out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double r;
    switch (op) {
    case 0: r = sin_d(x[i]); break;
    case 1: r = log(x[i]); break;
    case 2: r = atan2(x[i], y[i]); break;
    case 3: r = asin(x[i]); break;
    case 4: r = x[i] / y[i]; break;
    default: r = __builtin_sqrt(x[i]); break;
    }
    out[i] = r;
}
