/* oracle/rt_oracle.c — TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * CPU restatement of the hot path of DrStiev/raytracing_rust
 *   create_image (tests/test.rs:55-85) -> Camera::get_ray (src/camera.rs:53-67)
 *   -> color (src/color.rs:6-23) -> Hittable::hit (src/{hittable,aabb,bvh,sphere,rect,
 *   cube,traslate,rotate,medium}.rs) -> Material::scatter/emitted (src/material.rs)
 *   -> Texture::value (src/texture.rs, src/perlin.rs), samplers (src/util.rs).
 * Structure follows the reference: an object graph walked by recursive, dynamically
 * dispatched `hit` calls and a recursive `color`.  Each function cites the reference
 * lines it restates.  Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline
 * leg may load this library; the product (raytracing_rust_amd/) never does.
 *
 * Built twice from this one source (oracle/Makefile):
 *   liborc_f64.so  REAL = double : the literal restatement (the reference's arithmetic).
 *   liborc_f32.so  REAL = float  : same algorithm in the device's fp32 arithmetic
 *                                  contract (DESIGN.md "fp32 arithmetic contract"):
 *                                  selected at run time with ORC_ARITH_DEVICE.
 *
 * PINNING.  The reference is Rust and cannot be built here (no cargo/rustc); its RNG is
 * OS-seeded (rand::thread_rng), so its lit images are not reproducible.  The only golden
 * vectors its repo holds for this path are output/final_scene.ppm and
 * output/cornell_smoke.ppm (sha256 a78e19cf...b0eb5b, all-black 800x800 P3); this oracle
 * reproduces both byte-for-byte (tests/test_oracle_golden.py).  Everything that depends
 * on the random stream is "parity unpinned" against the reference and is pinned only
 * against the formulas in the cited source lines via known-answer tests.
 *
 * RNG.  rand::thread_rng()/gen::<f64>() (rand 0.8.5, not vendored) is replaced by a
 * Philox4x32-10 counter stream: counter = (block, sample, pixel, stream_id), key = seed;
 * the n-th draw of a sample is word n%4 of block n/4, mapped to [0,1) with 24 bits.
 * Draw ORDER is the reference's program order (SURVEY.md §8 "Per-sample RNG draw order").
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/rtmi_math.h"

#ifdef ORC_F32
typedef float REAL;
#define R_SQRT sqrtf
#define R_FMA fmaf
#define R_FMAX fmaxf
#define R_FMIN fminf
#define R_FLOOR floorf
#define R_FABS fabsf
#define R_MAX 3.40282346638528859811704183484516925e+38f
#define ORC_IS_F32 1
#else
typedef double REAL;
#define R_SQRT sqrt
#define R_FMA fma
#define R_FMAX fmax
#define R_FMIN fmin
#define R_FLOOR floor
#define R_FABS fabs
#define R_MAX 1.79769313486231570814527423731704357e+308
#define ORC_IS_F32 0
#endif

#define ORC_API __attribute__((visibility("default")))

/* ---- run-time switches -------------------------------------------------------- */
enum {
    ORC_ARITH_DEVICE = 1,  /* fp32 arithmetic contract substitutions      */
    ORC_THROUGHPUT_FORM = 2, /* iterative L += T*e form of color() instead of the recursion */
    ORC_SKY = 4,             /* opt-in extension: the gradient background the reference keeps
                              * commented out at color.rs:18-20 (default: black, color.rs:21)  */
    ORC_FACE_FORWARD = 8,    /* opt-in extension: Lambertian / Metal / Isotropic scatter about the normal turned
                              * against the incoming ray (the reference never turns it: sphere.rs:50, rect.rs:58-59);
                              * Dielectric keeps the geometric normal (material.rs:106-114)                      */
    ORC_UV_BOOK = 16         /* opt-in extension: get_sphere_uv adds pi/2 (the book) instead of FRAC_2_PI
                              * (sphere.rs:13)                                                                  */
};
static int g_flags = 0;
#define DEVICE_ARITH (g_flags & ORC_ARITH_DEVICE)

/* ---- instrumentation: operation counts that define the algorithmic work per sample
 *      (SURVEY.md §8(d) cost table) ------------------------------------------------ */
enum {
    C_SAMPLES, C_QUERIES, C_AABB, C_SPHERE, C_MSPHERE, C_RECT, C_XFORM, C_MEDIUM, C_MEDIUM_DRAW,
    C_MAT_FETCH, C_TEX_SOLID, C_TEX_CHECKER, C_TEX_NOISE, C_TEX_IMAGE, C_SC_LAMBERT, C_SC_METAL,
    C_SC_DIELECTRIC, C_SC_ISOTROPIC, C_EMIT, C_DRAWS, C_SPHERE_TRIALS, C_DISK_TRIALS, C_SPHERE_ACCEPT,
    C_RECT_ACCEPT,
    /* environment estimator (include/rtmi_env.h) and roulette (include/rtmi_roulette.h): which branches a render reached.
     * Appended only: the indices above keep their meaning. */
    C_ENV_SAMPLE,        /* light samples aimed at the map (us < p_env)                                      */
    C_ENV_NO_SAMPLE,     /* ... that had no sample: ct <= 0, or pdf outside (0, FLT_MAX)                     */
    C_ENV_OCCLUDED,      /* shadow rays toward the map that hit something                                    */
    C_ENV_UNOCCLUDED,    /* shadow rays toward the map that left the world                                   */
    C_ENV_MISS_MIS,      /* misses weighted by nee_mis_bsdf                                                  */
    C_ENV_MISS_ONE,      /* misses with weight 1 after a Lambertian / Isotropic vertex, under nee = 1        */
    C_ENV_AREA_SAMPLE,   /* area-light samples taken with p_env > 0                                          */
    C_ENV_EMIT_SCALED,   /* emitter hits whose weight used the (1 - p_env) scaling, p_env > 0                */
    C_RR_TEST,           /* roulette tests made (a scatter reached min_depth)                                */
    C_RR_DRAW,           /* roulette draws made (q < 1)                                                      */
    C_RR_END_PENDING,    /* draws that ended the continuation of a vertex with a pending shadow ray          */
    C_RR_END_BARE,       /* ... of a vertex without one                                                      */
    C_RR_FLOOR_SURVIVE,  /* survivals with q == q_min: the floor binds                                       */
    C_RR_ZERO,           /* continuations ended by m == 0                                                    */
    /* the light tree (include/rtmi_light_tree.h) under color_nee.  Appended only. */
    C_TREE_WALK,         /* light samples chosen by a walk                                                   */
    C_TREE_LEFT,         /* child choices of the walks: left ...                                             */
    C_TREE_RIGHT,        /* ... and right                                                                    */
    C_TREE_FLOOR,        /* node importances where r2 won the max                                            */
    C_TREE_P_ONE,        /* interior nodes of a walk where pl or pr rounded to exactly 1                     */
    C_TREE_CLAMP,        /* uniforms clamped to 1 - 2^-24                                                    */
    C_TREE_NO_SAMPLE,    /* walks whose nee_sample returned 0                                                */
    C_TREE_HIT_PMF,      /* BSDF hits of a table light weighted through the reverse walk                     */
    C_TREE_HIT_PICKED,   /* ... whose light is the one the previous vertex's walk picked                     */
    C_TREE_HIT_PICKED_MISMATCH, /* ... whose pmf differs from the probability that pick returned: stays 0    */
    C_NCOUNTERS
};
static uint64_t g_cnt[C_NCOUNTERS];
#ifdef ORC_NO_COUNT /* the timed CPU-baseline build: no instrumentation on the hot path */
#define COUNT(k) ((void)0)
#else
#define COUNT(k) (g_cnt[k]++)
#endif

/* ---- Philox4x32-10 (Salmon et al., SC'11) ------------------------------------- */
static void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
    uint32_t k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; r++) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        uint32_t n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

typedef struct {
    uint32_t key[2];
    uint32_t ctr[4]; /* ctr[0] = next block index */
    uint32_t buf[4];
    int pos; /* 4 = empty */
    const uint32_t *script; /* not NULL: the blocks come from this list instead of Philox (orc_script) */
} Stream;

/* the `rand::thread_rng()` of the render path: one stream per (pixel, sample) */
static Stream g_rng;

/* A scripted word source for the per-operation tests (tests/test_path_contract.py): while a script is set, every
 * stream_init of the render path's stream points it at the start of the list, and the stream then delivers the list's
 * words in order wherever the path draws.  A draw beyond the list delivers 0x80000000 (u = 0.5, the samplers' p = 0,
 * which they accept: no rejection loop outlives the list).  The words are handed out through the stream's 4-word
 * buffer, so a draw costs what it cost; the words consumed are counted from the blocks filled (orc_script_consumed). */
static const uint32_t *g_script = NULL;
static uint32_t g_script_len = 0;

static void stream_init(Stream *s, uint64_t seed, uint32_t sample, uint32_t pixel, uint32_t stream_id) {
    s->key[0] = (uint32_t)seed;
    s->key[1] = (uint32_t)(seed >> 32);
    s->ctr[0] = 0;
    s->ctr[1] = sample;
    s->ctr[2] = pixel;
    s->ctr[3] = stream_id;
    s->pos = 4;
    s->script = s == &g_rng ? g_script : NULL;
}
static void stream_fill(Stream *s) {
    if (s->script) {
        for (uint32_t k = 0; k < 4; k++) {
            const uint64_t at = (uint64_t)s->ctr[0] * 4 + k;
            s->buf[k] = at < g_script_len ? s->script[at] : 0x80000000u;
        }
    } else {
        philox4x32_10(s->ctr, s->key, s->buf);
    }
}
static uint32_t stream_u32(Stream *s) {
    if (s->pos == 4) {
        stream_fill(s);
        s->ctr[0]++;
        s->pos = 0;
    }
    return s->buf[s->pos++];
}

/* the `rand::thread_rng()` of scene construction (BVH axes, Perlin tables) */
static Stream g_scene_rng;

/* rng.gen::<f64>() — tests/test.rs:66-67, camera.rs:61, util.rs:8,19, material.rs:118,
 * medium.rs:40.  24-bit uniform (see rtmi_math.h rtmi_u01). */
static REAL rng_uniform(void) {
    COUNT(C_DRAWS);
    return (REAL)rtmi_u01(stream_u32(&g_rng));
}
static double scene_uniform(void) { return (double)rtmi_u01(stream_u32(&g_scene_rng)); }
/* rng.gen_range(0..n) — bvh.rs:40, perlin.rs:7 */
static uint32_t scene_range(uint32_t n) { return (uint32_t)(((uint64_t)stream_u32(&g_scene_rng) * n) >> 32); }

/* ---- Vector3 (nalgebra 0.32 semantics for the ops the path uses) ---------------- */
typedef struct { REAL x, y, z; } V3;
typedef struct { double x, y, z; } D3;
static inline V3 v3(REAL x, REAL y, REAL z) { V3 v = {x, y, z}; return v; }
static inline V3 v_add(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline V3 v_sub(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline V3 v_scale(V3 a, REAL s) { return v3(a.x * s, a.y * s, a.z * s); }
static inline V3 v_div(V3 a, REAL s) { return v3(a.x / s, a.y / s, a.z / s); }
static inline V3 v_neg(V3 a) { return v3(-a.x, -a.y, -a.z); }
static inline V3 v_mul(V3 a, V3 b) { return v3(a.x * b.x, a.y * b.y, a.z * b.z); }
static inline REAL v_dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static inline REAL v_norm(V3 a) { return R_SQRT(v_dot(a, a)); }
static inline V3 v_normalize(V3 a) { return v_div(a, v_norm(a)); }
static inline REAL v_get(V3 a, int i) { return i == 0 ? a.x : (i == 1 ? a.y : a.z); }
static inline void v_set(V3 *a, int i, REAL v) { if (i == 0) a->x = v; else if (i == 1) a->y = v; else a->z = v; }
static inline V3 d3_to_v3(D3 d) { return v3((REAL)d.x, (REAL)d.y, (REAL)d.z); }

/* ---- Ray (src/ray.rs:3-29).  inv_d / inv_a are derived values cached per ray frame:
 *      inv_d[a] is exactly the `1.0 / ray.direction()[a]` of aabb.rs:33. ------------ */
typedef struct {
    V3 o, d;
    REAL time;
    V3 inv_d;
    REAL inv_a;
} Ray;
static Ray ray_new(V3 o, V3 d, REAL time) {
    Ray r;
    r.o = o; r.d = d; r.time = time;
    r.inv_d = v3((REAL)1 / d.x, (REAL)1 / d.y, (REAL)1 / d.z);
    r.inv_a = (REAL)1 / v_dot(d, d);
    return r;
}
static inline V3 ray_at(const Ray *r, REAL t) { return v_add(r->o, v_scale(r->d, t)); } /* ray.rs:23-25 */

/* ---- transcendental dispatch --------------------------------------------------- */
static inline REAL m_sin(REAL x) {
#ifdef ORC_F32
    if (DEVICE_ARITH) return rtmi_sinf(x);
    return sinf(x);
#else
    return sin(x);
#endif
}
static inline REAL m_cos(REAL x) {
#ifdef ORC_F32
    if (DEVICE_ARITH) return rtmi_cosf(x);
    return cosf(x);
#else
    return cos(x);
#endif
}
static inline REAL m_log(REAL x) {
#ifdef ORC_F32
    if (DEVICE_ARITH) return rtmi_logf(x);
    return logf(x);
#else
    return log(x);
#endif
}
static inline REAL m_atan2(REAL y, REAL x) {
#ifdef ORC_F32
    if (DEVICE_ARITH) return rtmi_atan2f(y, x);
    return atan2f(y, x);
#else
    return atan2(y, x);
#endif
}
static inline REAL m_asin(REAL x) {
#ifdef ORC_F32
    if (DEVICE_ARITH) return rtmi_asinf(x);
    return asinf(x);
#else
    return asin(x);
#endif
}

/* ---- object graph --------------------------------------------------------------- */
typedef struct Texture Texture;
typedef struct Material Material;
typedef struct Hittable Hittable;

typedef struct {
    V3 ran_vec[256];
    int perm_x[256], perm_y[256], perm_z[256];
} Perlin;

enum { TEX_SOLID = 0, TEX_CHECKER = 1, TEX_NOISE = 2, TEX_IMAGE = 3 };
struct Texture {
    int kind;
    V3 color;
    const Texture *odd, *even;
    REAL scale;
    Perlin *noise;
    uint8_t *data;
    uint32_t nx, ny;
};

enum { MAT_LAMBERTIAN = 0, MAT_METAL = 1, MAT_DIELECTRIC = 2, MAT_DIFFUSE_LIGHT = 3, MAT_ISOTROPIC = 4 };
struct Material {
    int kind;
    const Texture *tex;
    REAL param; /* fuzz | ref_idx */
};

typedef struct {
    REAL t, u, v;
    V3 p, normal;
    const Material *mat;
    const Hittable *prim; /* the leaf primitive (sphere, moving sphere, rect, cube side) that produced the hit; NULL for
                           * a medium's scattering event.  Not in the reference: next-event estimation matches its
                           * shadow ray's hit against the sampled light by it (include/rtmi_nee.h) */
} HitRecord; /* hittable.rs:9-16 */

typedef struct { D3 min, max; } AABBd; /* scene set-up stays f64 like the reference */
typedef struct { V3 min, max; } AABB;

enum { H_SPHERE = 0, H_MOVING_SPHERE, H_RECT, H_CUBE, H_LIST, H_FLIP, H_TRANSLATE, H_ROTATE, H_MEDIUM, H_BVH,
       H_PROBE_POINT /* test only (orc_probe_point): a hit at a given t with a given normal, whatever the ray */ };
struct Hittable {
    int kind;
    /* sphere / moving sphere */
    D3 c0d, c1d; double rd, t0d, t1d;
    V3 c0, c1; REAL radius, t0, t1;
    /* rect */
    int plane; double x0d, y0d, x1d, y1d, kd;
    REAL x0, y0, x1, y1, k;
    /* cube */
    D3 pmind, pmaxd;
    Hittable *sides; /* H_LIST of 6 rects */
    /* list */
    Hittable **items; int n, cap;
    /* wrappers */
    Hittable *child;
    D3 offsetd; V3 offset;
    int axis; double sind, cosd; REAL sin_t, cos_t; int has_bbox; AABBd rot_bbox;
    /* medium */
    REAL density; Material phase;
    /* bvh */
    Hittable *left, *right; AABBd boxd; AABB box;
    const Material *mat;
};

/* ---- allocation arena ------------------------------------------------------------ */
typedef struct Blk { struct Blk *next; char pad[8]; } Blk; /* 16 bytes: payload stays 16-aligned */
static Blk *g_blocks = NULL;
static void *arena_alloc(size_t n) {
    Blk *b = (Blk *)calloc(1, sizeof(Blk) + n);
    if (!b) { fprintf(stderr, "orc: out of memory\n"); abort(); }
    b->next = g_blocks;
    g_blocks = b;
    return (char *)b + sizeof(Blk);
}
ORC_API void orc_free_all(void) {
    while (g_blocks) { Blk *n = g_blocks->next; free(g_blocks); g_blocks = n; }
}

/* ================================================================================== */
/* Textures — src/texture.rs, src/perlin.rs                                           */
/* ================================================================================== */

/* perlin.rs:38-56 */
static REAL perlin_interpolation(V3 c[2][2][2], REAL u, REAL v, REAL w) {
    REAL uu = u * u * ((REAL)3.0 - (REAL)2.0 * u);
    REAL vv = v * v * ((REAL)3.0 - (REAL)2.0 * v);
    REAL ww = w * w * ((REAL)3.0 - (REAL)2.0 * w);
    REAL accum = 0;
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 2; j++)
            for (int k = 0; k < 2; k++) {
                V3 weight = v3(u - (REAL)i, v - (REAL)j, w - (REAL)k);
                accum += ((REAL)i * uu + (REAL)(1 - i) * ((REAL)1.0 - uu)) *
                         ((REAL)j * vv + (REAL)(1 - j) * ((REAL)1.0 - vv)) *
                         ((REAL)k * ww + (REAL)(1 - k) * ((REAL)1.0 - ww)) * v_dot(c[i][j][k], weight);
            }
    return accum;
}

/* Rust `f64 as usize`: saturating, NaN -> 0 (perlin.rs:83-85, texture.rs:91-92) */
static uint64_t as_usize(REAL x) {
    if (!(x > 0)) return 0; /* negative, -0, NaN */
    if (x >= (REAL)18446744073709551615.0) return UINT64_MAX;
    return (uint64_t)x;
}

/* perlin.rs:76-97 */
static REAL perlin_noise(const Perlin *pn, V3 p) {
    REAL u = p.x - R_FLOOR(p.x);
    REAL v = p.y - R_FLOOR(p.y);
    REAL w = p.z - R_FLOOR(p.z);
    uint64_t i = as_usize(R_FLOOR(p.x));
    uint64_t j = as_usize(R_FLOOR(p.y));
    uint64_t k = as_usize(R_FLOOR(p.z));
    V3 c[2][2][2];
    for (uint64_t di = 0; di < 2; di++)
        for (uint64_t dj = 0; dj < 2; dj++)
            for (uint64_t dk = 0; dk < 2; dk++)
                c[di][dj][dk] =
                    pn->ran_vec[pn->perm_x[(i + di) & 255] ^ pn->perm_y[(j + dj) & 255] ^ pn->perm_z[(k + dk) & 255]];
    return perlin_interpolation(c, u, v, w);
}

/* perlin.rs:99-109 */
static REAL perlin_turb(const Perlin *pn, V3 p, int depth) {
    REAL accum = 0;
    V3 temp_p = p;
    REAL weight = 1.0;
    for (int i = 0; i < depth; i++) {
        accum += weight * perlin_noise(pn, temp_p);
        weight *= (REAL)0.5;
        temp_p = v_scale(temp_p, (REAL)2.0);
    }
    return R_FABS(accum);
}

/* texture.rs:4-6 and the four impls */
static V3 tex_value(const Texture *t, REAL u, REAL v, V3 p) {
    switch (t->kind) {
    case TEX_SOLID: /* texture.rs:21-25 */
        COUNT(C_TEX_SOLID);
        return t->color;
    case TEX_CHECKER: { /* texture.rs:39-48 */
        COUNT(C_TEX_CHECKER);
        REAL s = m_sin((REAL)10.0 * p.x) * m_sin((REAL)10.0 * p.y) * m_sin((REAL)10.0 * p.z);
        if (s < 0) return tex_value(t->odd, u, v, p);
        return tex_value(t->even, u, v, p);
    }
    case TEX_NOISE: { /* texture.rs:65-71 — turb gets the UNSCALED p */
        COUNT(C_TEX_NOISE);
        REAL g = (REAL)0.5 * ((REAL)1.0 + m_sin(t->scale * p.x + (REAL)5.0 * perlin_turb(t->noise, p, 7)));
        /* Vector3::new(1,1,1) * 0.5 * (1 + sin(..)): ((1*0.5) * x) per component == 0.5*x */
        return v3(g, g, g);
    }
    case TEX_IMAGE: { /* texture.rs:86-108 */
        COUNT(C_TEX_IMAGE);
        uint64_t nx = t->nx, ny = t->ny;
        uint64_t i = as_usize(u * (REAL)nx);
        uint64_t j = as_usize(((REAL)1.0 - v) * (REAL)ny);
        if (i > nx - 1) i = nx - 1;
        if (j > ny - 1) j = ny - 1;
        uint64_t idx = 3 * i + 3 * nx * j;
        return v3((REAL)t->data[idx] / (REAL)255.0, (REAL)t->data[idx + 1] / (REAL)255.0,
                  (REAL)t->data[idx + 2] / (REAL)255.0);
    }
    }
    return v3(0, 0, 0);
}

/* ================================================================================== */
/* Samplers — src/util.rs                                                             */
/* ================================================================================== */
/* util.rs:4-13 : draws x, y, z per trial */
static V3 random_in_unit_sphere(void) {
    for (;;) {
        COUNT(C_SPHERE_TRIALS);
        REAL x = rng_uniform(), y = rng_uniform(), z = rng_uniform();
        V3 p = v3((REAL)2.0 * x - (REAL)1.0, (REAL)2.0 * y - (REAL)1.0, (REAL)2.0 * z - (REAL)1.0);
        if (v_dot(p, p) < (REAL)1.0) return p;
    }
}
/* util.rs:15-24 : draws x, y per trial */
static V3 random_in_unit_disk(void) {
    for (;;) {
        COUNT(C_DISK_TRIALS);
        REAL x = rng_uniform(), y = rng_uniform();
        V3 p = v3((REAL)2.0 * x - (REAL)1.0, (REAL)2.0 * y - (REAL)1.0, (REAL)2.0 * (REAL)0.0 - (REAL)0.0);
        if (v_dot(p, p) < (REAL)1.0) return p;
    }
}

/* ================================================================================== */
/* Materials — src/material.rs                                                        */
/* ================================================================================== */
static V3 reflect(V3 v, V3 n) { /* material.rs:9-11 : v - 2.0 * v.dot(n) * n */
    REAL s = (REAL)2.0 * v_dot(v, n);
    return v_sub(v, v_scale(n, s));
}
static int refract(V3 v, V3 n, REAL ni_over_nt, V3 *out) { /* material.rs:13-23 */
    V3 uv = v_normalize(v);
    REAL dt = v_dot(uv, n);
    REAL disc = (REAL)1.0 - ni_over_nt * ni_over_nt * ((REAL)1.0 - dt * dt);
    if (disc > 0) {
        *out = v_sub(v_scale(v_sub(uv, v_scale(n, dt)), ni_over_nt), v_scale(n, R_SQRT(disc)));
        return 1;
    }
    return 0;
}
static REAL schlick(REAL cosine, REAL ref_idx) { /* material.rs:25-28 ; powi(5) = x*(x^2)^2 */
    REAL r0 = ((REAL)1.0 - ref_idx) / ((REAL)1.0 + ref_idx);
    r0 = r0 * r0;
    REAL x = (REAL)1.0 - cosine;
    REAL x2 = x * x;
    REAL x4 = x2 * x2;
    return r0 + ((REAL)1.0 - r0) * (x * x4);
}

/* Material::emitted — material.rs:32 and impls (:55-57, :89-91, :128-130, :148-150, :170-172) */
static V3 mat_emitted(const Material *m, REAL u, REAL v, V3 p) {
    if (m->kind == MAT_DIFFUSE_LIGHT) { COUNT(C_EMIT); return tex_value(m->tex, u, v, p); }
    return v3(0, 0, 0);
}

/* Material::scatter — material.rs:31 and impls */
static int mat_scatter(const Material *m, const Ray *ray, const HitRecord *hit, Ray *scattered, V3 *attenuation) {
    COUNT(C_MAT_FETCH);
    HitRecord turned;
    if ((g_flags & ORC_FACE_FORWARD) && m->kind != MAT_DIELECTRIC && v_dot(ray->d, hit->normal) > (REAL)0.0) {
        turned = *hit;
        turned.normal = v3(-hit->normal.x, -hit->normal.y, -hit->normal.z);
        hit = &turned;
    }
    switch (m->kind) {
    case MAT_LAMBERTIAN: { /* material.rs:49-53 */
        COUNT(C_SC_LAMBERT);
        V3 rs = random_in_unit_sphere();
        V3 dir;
        if (DEVICE_ARITH) {
            dir = v_add(hit->normal, rs); /* contract: (p+n+r)-p evaluated without the p round trip */
        } else {
            V3 target = v_add(v_add(hit->p, hit->normal), rs);
            dir = v_sub(target, hit->p);
        }
        *scattered = ray_new(hit->p, dir, ray->time);
        *attenuation = tex_value(m->tex, hit->u, hit->v, hit->p);
        return 1;
    }
    case MAT_METAL: { /* material.rs:75-87 (fuzz clamp is in the constructor, :70) */
        COUNT(C_SC_METAL);
        V3 reflected = reflect(v_normalize(ray->d), hit->normal);
        if (m->param > 0) reflected = v_add(reflected, v_scale(random_in_unit_sphere(), m->param));
        if (v_dot(reflected, hit->normal) > 0) {
            *scattered = ray_new(hit->p, reflected, ray->time);
            *attenuation = tex_value(m->tex, hit->u, hit->v, hit->p);
            return 1;
        }
        return 0;
    }
    case MAT_DIELECTRIC: { /* material.rs:106-126 */
        COUNT(C_SC_DIELECTRIC);
        *attenuation = v3(1.0, 1.0, 1.0);
        V3 outward_normal;
        REAL ni_over_nt, cosine;
        REAL ddn = v_dot(ray->d, hit->normal);
        if (ddn > 0) {
            cosine = m->param * ddn / v_norm(ray->d);
            outward_normal = v_neg(hit->normal);
            ni_over_nt = m->param;
        } else {
            cosine = -ddn / v_norm(ray->d);
            outward_normal = hit->normal;
            ni_over_nt = (REAL)1.0 / m->param;
        }
        V3 refracted;
        if (refract(ray->d, outward_normal, ni_over_nt, &refracted)) {
            REAL reflect_prob = schlick(cosine, m->param);
            if (rng_uniform() >= reflect_prob) {
                *scattered = ray_new(hit->p, refracted, ray->time);
                return 1;
            }
        }
        *scattered = ray_new(hit->p, reflect(ray->d, hit->normal), ray->time);
        return 1;
    }
    case MAT_DIFFUSE_LIGHT: /* material.rs:144-146 */
        return 0;
    case MAT_ISOTROPIC: { /* material.rs:165-168 */
        COUNT(C_SC_ISOTROPIC);
        V3 rs = random_in_unit_sphere();
        *scattered = ray_new(hit->p, rs, ray->time);
        *attenuation = tex_value(m->tex, hit->u, hit->v, hit->p);
        return 1;
    }
    }
    return 0;
}

/* ================================================================================== */
/* Geometry — hit()                                                                   */
/* ================================================================================== */
static int hit(const Hittable *h, const Ray *r, REAL t_min, REAL t_max, HitRecord *rec);

/* aabb.rs:31-44 */
static int aabb_hit(const AABB *b, const Ray *r, REAL t_min, REAL t_max) {
    COUNT(C_AABB);
    for (int a = 0; a < 3; a++) {
        REAL inv_d = v_get(r->inv_d, a);
        REAL t0 = (v_get(b->min, a) - v_get(r->o, a)) * inv_d;
        REAL t1 = (v_get(b->max, a) - v_get(r->o, a)) * inv_d;
        if (inv_d < 0) { REAL tmp = t0; t0 = t1; t1 = tmp; }
        t_min = R_FMAX(t_min, t0);
        t_max = R_FMIN(t_max, t1);
        if (t_max <= t_min) return 0;
    }
    return 1;
}

/* sphere.rs:9-15 */
static void get_sphere_uv(V3 p, REAL *u, REAL *v) {
    REAL phi = m_atan2(p.z, p.x);
    REAL theta = m_asin(p.y);
#ifdef ORC_F32
    const REAL PI = RTMI_PI_F, FRAC_2_PI = RTMI_2_OVER_PI_F;
#else
    const REAL PI = 3.14159265358979323846264338327950288, FRAC_2_PI = 0.636619772367581343075535053490057448;
#endif
    *u = (REAL)1.0 - (phi + PI) / ((REAL)2.0 * PI);
#ifdef ORC_F32
    const REAL FRAC_PI_2 = RTMI_PIO2_F;
#else
    const REAL FRAC_PI_2 = 1.57079632679489661923132169163975144;
#endif
    *v = (theta + ((g_flags & ORC_UV_BOOK) ? FRAC_PI_2 : FRAC_2_PI)) / PI; /* sic: FRAC_2_PI, not FRAC_PI_2 */
}

/* sphere.rs:37-77 and :122-164 (identical bodies, centre differs) */
static int sphere_hit_at(const Hittable *h, V3 center, REAL radius, const Material *mat, const Ray *r, REAL t_min,
                         REAL t_max, HitRecord *rec) {
    V3 oc = v_sub(r->o, center);
    REAL a = v_dot(r->d, r->d);
    REAL b = v_dot(oc, r->d);
    REAL c = v_dot(oc, oc) - radius * radius;
    REAL disc = b * b - a * c;
    if (DEVICE_ARITH) {
        /* contract substitution 5: the same discriminant as a (r^2 - |oc - (b/a) d|^2) — the squared
         * distance of the centre from the ray instead of a difference of two numbers of size |oc|^2 a, which in fp32
         * puts the hit point of a small far sphere up to 5e-3 off its surface (the scattered ray then meets the same
         * sphere again beyond t_min: final_scene's small spheres 10 % too dark against the f64 literal).  Explicit
         * fma (one rounding each) exactly as csrc/rtmi_geom.hpp sphere_disc(). */
        REAL q = b * r->inv_a;
        REAL lx = R_FMA(-q, r->d.x, oc.x), ly = R_FMA(-q, r->d.y, oc.y), lz = R_FMA(-q, r->d.z, oc.z);
        REAL l2 = R_FMA(lz, lz, R_FMA(ly, ly, lx * lx));
        disc = a * (radius * radius - l2);
    }
    if (disc > 0) {
        REAL sq = R_SQRT(disc);
        REAL t = DEVICE_ARITH ? (-b - sq) * r->inv_a : (-b - sq) / a;
        if (t < t_max && t > t_min) goto accept;
        t = DEVICE_ARITH ? (-b + sq) * r->inv_a : (-b + sq) / a;
        if (t < t_max && t > t_min) goto accept;
        return 0;
    accept:
        COUNT(C_SPHERE_ACCEPT);
        rec->t = t;
        rec->p = ray_at(r, t);
        rec->normal = v_div(v_sub(rec->p, center), radius); /* outward; never face-forwarded */
        get_sphere_uv(rec->normal, &rec->u, &rec->v);
        rec->mat = mat;
        rec->prim = h;
        return 1;
    }
    return 0;
}

/* sphere.rs:115-118 */
static V3 moving_center(const Hittable *h, REAL time) {
    REAL f = DEVICE_ARITH ? (time - h->t0) * ((REAL)1.0 / (h->t1 - h->t0)) : (time - h->t0) / (h->t1 - h->t0);
    return v_add(h->c0, v_scale(v_sub(h->c1, h->c0), f));
}
static D3 moving_center_d(const Hittable *h, double time) {
    double f = (time - h->t0d) / (h->t1d - h->t0d);
    D3 c = {h->c0d.x + f * (h->c1d.x - h->c0d.x), h->c0d.y + f * (h->c1d.y - h->c0d.y),
            h->c0d.z + f * (h->c1d.z - h->c0d.z)};
    return c;
}

static void plane_axes(int plane, int *k, int *a, int *b) { /* rect.rs:40-44 */
    switch (plane) {
    case 0: *k = 0; *a = 1; *b = 2; break; /* YZ */
    case 1: *k = 1; *a = 2; *b = 0; break; /* ZX */
    default: *k = 2; *a = 0; *b = 1; break; /* XY */
    }
}

/* rect.rs:39-69 */
static int rect_hit(const Hittable *h, const Ray *r, REAL t_min, REAL t_max, HitRecord *rec) {
    COUNT(C_RECT);
    int ka, aa, ba;
    plane_axes(h->plane, &ka, &aa, &ba);
    REAL t = DEVICE_ARITH ? (h->k - v_get(r->o, ka)) * v_get(r->inv_d, ka) : (h->k - v_get(r->o, ka)) / v_get(r->d, ka);
    if (t < t_min || t > t_max) return 0;
    REAL x = v_get(r->o, aa) + t * v_get(r->d, aa);
    REAL y = v_get(r->o, ba) + t * v_get(r->d, ba);
    if (x < h->x0 || x > h->x1 || y < h->y0 || y > h->y1) return 0;
    COUNT(C_RECT_ACCEPT);
    rec->u = (x - h->x0) / (h->x1 - h->x0);
    rec->v = (y - h->y0) / (h->y1 - h->y0);
    rec->t = t;
    rec->p = ray_at(r, t);
    rec->normal = v3(0, 0, 0);
    v_set(&rec->normal, ka, 1.0);
    rec->mat = h->mat;
    rec->prim = h;
    return 1;
}

/* hittable.rs:37-47 */
static int list_hit(const Hittable *h, const Ray *r, REAL t_min, REAL t_max, HitRecord *rec) {
    REAL closest = t_max;
    int hit_anything = 0;
    HitRecord tmp;
    for (int i = 0; i < h->n; i++) {
        if (hit(h->items[i], r, t_min, closest, &tmp)) {
            closest = tmp.t;
            *rec = tmp;
            hit_anything = 1;
        }
    }
    return hit_anything;
}

/* ConstantMedium::hit after both boundary queries returned t1 and t2 — medium.rs:33-53; dn = ray.direction().norm() */
static int medium_sample(REAL t1, REAL t2, REAL t_min, REAL t_max, REAL dn, REAL density, REAL *t_out) {
    if (t1 < t_min) t1 = t_min;
    if (t2 > t_max) t2 = t_max;
    if (t1 < t2) {
        REAL dist_inside = (t2 - t1) * dn;
        COUNT(C_MEDIUM_DRAW);
        REAL hit_distance = -((REAL)1.0 / density) * m_log(rng_uniform());
        if (hit_distance < dist_inside) {
            *t_out = t1 + hit_distance / dn;
            return 1;
        }
    }
    return 0;
}

static int hit(const Hittable *h, const Ray *r, REAL t_min, REAL t_max, HitRecord *rec) {
    switch (h->kind) {
    case H_SPHERE: /* sphere.rs:37-77 */
        COUNT(C_SPHERE);
        return sphere_hit_at(h, h->c0, h->radius, h->mat, r, t_min, t_max, rec);
    case H_MOVING_SPHERE: /* sphere.rs:122-164 */
        COUNT(C_MSPHERE);
        return sphere_hit_at(h, moving_center(h, r->time), h->radius, h->mat, r, t_min, t_max, rec);
    case H_RECT:
        return rect_hit(h, r, t_min, t_max, rec);
    case H_CUBE: /* cube.rs:84-86 */
        return list_hit(h->sides, r, t_min, t_max, rec);
    case H_LIST:
        return list_hit(h, r, t_min, t_max, rec);
    case H_PROBE_POINT: /* what every primitive does last: p = ray.point_at_parameter(t) in its own frame */
        rec->t = h->radius; rec->u = 0; rec->v = 0;
        rec->p = ray_at(r, h->radius);
        rec->normal = h->c0;
        rec->mat = NULL; rec->prim = NULL;
        return 1;
    case H_FLIP: /* hittable.rs:78-83 */
        if (hit(h->child, r, t_min, t_max, rec)) {
            rec->normal = v_neg(rec->normal);
            return 1;
        }
        return 0;
    case H_TRANSLATE: { /* traslate.rs:18-24 */
        COUNT(C_XFORM);
        Ray moved = ray_new(v_sub(r->o, h->offset), r->d, r->time);
        if (hit(h->child, &moved, t_min, t_max, rec)) {
            rec->p = v_add(rec->p, h->offset);
            return 1;
        }
        return 0;
    }
    case H_ROTATE: { /* rotate.rs:85-113 */
        COUNT(C_XFORM);
        int ra, aa, ba;
        plane_axes(h->axis, &ra, &aa, &ba); /* Axis::{X,Y,Z} -> same (r,a,b) triples as Plane */
        V3 o = r->o, d = r->d;
        v_set(&o, aa, h->cos_t * v_get(r->o, aa) + h->sin_t * v_get(r->o, ba));
        v_set(&o, ba, -h->sin_t * v_get(r->o, aa) + h->cos_t * v_get(r->o, ba));
        v_set(&d, aa, h->cos_t * v_get(r->d, aa) + h->sin_t * v_get(r->d, ba));
        v_set(&d, ba, -h->sin_t * v_get(r->d, aa) + h->cos_t * v_get(r->d, ba));
        Ray rot = ray_new(o, d, r->time);
        if (hit(h->child, &rot, t_min, t_max, rec)) {
            V3 p = rec->p, n = rec->normal;
            v_set(&p, aa, h->cos_t * v_get(rec->p, aa) - h->sin_t * v_get(rec->p, ba));
            v_set(&p, ba, h->sin_t * v_get(rec->p, aa) + h->cos_t * v_get(rec->p, ba));
            v_set(&n, aa, h->cos_t * v_get(rec->normal, aa) - h->sin_t * v_get(rec->normal, ba));
            v_set(&n, ba, h->sin_t * v_get(rec->normal, aa) + h->cos_t * v_get(rec->normal, ba));
            rec->p = p;
            rec->normal = n;
            return 1;
        }
        return 0;
    }
    case H_MEDIUM: { /* medium.rs:28-56 */
        COUNT(C_MEDIUM);
        HitRecord h1, h2;
        if (hit(h->child, r, -R_MAX, R_MAX, &h1)) {
            if (hit(h->child, r, h1.t + (REAL)0.0001, R_MAX, &h2)) {
                REAL t;
                if (medium_sample(h1.t, h2.t, t_min, t_max, v_norm(r->d), h->density, &t)) {
                    rec->t = t;
                    rec->u = 0; rec->v = 0;
                    rec->p = ray_at(r, t);
                    rec->normal = v3(1.0, 0.0, 0.0);
                    rec->mat = &h->phase;
                    rec->prim = NULL;
                    return 1;
                }
            }
        }
        return 0;
    }
    case H_BVH: { /* bvh.rs:70-89 */
        if (aabb_hit(&h->box, r, t_min, t_max)) {
            HitRecord l, rr;
            int hl = hit(h->left, r, t_min, t_max, &l);
            int hr = hit(h->right, r, t_min, t_max, &rr);
            if (hl && hr) { *rec = (l.t < rr.t) ? l : rr; return 1; } /* tie -> right */
            if (hl) { *rec = l; return 1; }
            if (hr) { *rec = rr; return 1; }
        }
        return 0;
    }
    }
    return 0;
}

/* ================================================================================== */
/* bounding_box (f64, scene set-up) — hittable.rs:49-64, aabb.rs:6-18, sphere.rs:79-84,  */
/* :165-174, rect.rs:71-75, cube.rs:88-93, traslate.rs:26-32, rotate.rs:115-117,         */
/* medium.rs:58-60, bvh.rs:91-93                                                         */
/* ================================================================================== */
static AABBd surrounding_box(AABBd a, AABBd b) {
    AABBd r;
    r.min.x = fmin(a.min.x, b.min.x); r.min.y = fmin(a.min.y, b.min.y); r.min.z = fmin(a.min.z, b.min.z);
    r.max.x = fmax(a.max.x, b.max.x); r.max.y = fmax(a.max.y, b.max.y); r.max.z = fmax(a.max.z, b.max.z);
    return r;
}
static int bounding_box(const Hittable *h, double t0, double t1, AABBd *out) {
    switch (h->kind) {
    case H_SPHERE:
        out->min.x = h->c0d.x - h->rd; out->min.y = h->c0d.y - h->rd; out->min.z = h->c0d.z - h->rd;
        out->max.x = h->c0d.x + h->rd; out->max.y = h->c0d.y + h->rd; out->max.z = h->c0d.z + h->rd;
        return 1;
    case H_MOVING_SPHERE: {
        D3 ca = moving_center_d(h, t0), cb = moving_center_d(h, t1);
        AABBd a = {{ca.x - h->rd, ca.y - h->rd, ca.z - h->rd}, {ca.x + h->rd, ca.y + h->rd, ca.z + h->rd}};
        AABBd b = {{cb.x - h->rd, cb.y - h->rd, cb.z - h->rd}, {cb.x + h->rd, cb.y + h->rd, cb.z + h->rd}};
        *out = surrounding_box(a, b);
        return 1;
    }
    case H_RECT: /* sic: ignores the plane (rect.rs:72-73) */
        out->min.x = h->x0d; out->min.y = h->y0d; out->min.z = h->kd - 0.0001;
        out->max.x = h->x1d; out->max.y = h->y1d; out->max.z = h->kd + 0.0001;
        return 1;
    case H_CUBE:
        out->min = h->pmind; out->max = h->pmaxd;
        return 1;
    case H_LIST: {
        if (h->n == 0) return 0;
        AABBd acc;
        if (!bounding_box(h->items[0], t0, t1, &acc)) return 0;
        for (int i = 1; i < h->n; i++) {
            AABBd b;
            if (!bounding_box(h->items[i], t0, t1, &b)) return 0;
            acc = surrounding_box(acc, b);
        }
        *out = acc;
        return 1;
    }
    case H_FLIP:
    case H_MEDIUM:
        return bounding_box(h->child, t0, t1, out);
    case H_TRANSLATE:
        if (!bounding_box(h->child, t0, t1, out)) return 0;
        out->min.x += h->offsetd.x; out->min.y += h->offsetd.y; out->min.z += h->offsetd.z;
        out->max.x += h->offsetd.x; out->max.y += h->offsetd.y; out->max.z += h->offsetd.z;
        return 1;
    case H_ROTATE:
        if (!h->has_bbox) return 0;
        *out = h->rot_bbox;
        return 1;
    case H_BVH:
        *out = h->boxd;
        return 1;
    }
    return 0;
}

/* ================================================================================== */
/* color — src/color.rs:6-23                                                           */
/* ================================================================================== */
typedef struct {
    const Hittable *world;
    int max_depth;
    REAL t_min;
    int rr_min_depth; /* Russian roulette (include/rtmi_roulette.h): the first depth tested; 0 = off */
    REAL rr_q_min;
} RenderCtx;

/* the depth at which the last colour loop wrote its path: the scatters it made (rtmi_roulette.h "Bounce count") */
static int g_bounces;

/* The test of include/rtmi_roulette.h, made after a scatter has set T = T * att and raised the depth to d; `pending`:
 * the vertex holds a light sample whose shadow ray is not traced yet (counted only).  The draw is stateless: word 0 of
 * philox(counter = (d, sample, pixel, 4), key = seed), sample and pixel being the words of the path's stream 0 (g_rng).
 * Returns 1 when the continuation ends; a survivor's T is divided by q. */
static int roulette_ends(const RenderCtx *cx, V3 *T, int d, int pending) {
    if (cx->rr_min_depth <= 0 || d < cx->rr_min_depth) return 0;
    COUNT(C_RR_TEST);
    const REAL m = R_FMAX(R_FMAX(T->x, T->y), T->z);
    if (m == (REAL)0) { COUNT(C_RR_ZERO); return 1; }
    const REAL q = R_FMIN(R_FMAX(m, cx->rr_q_min), (REAL)1);
    if (q < (REAL)1) {
        COUNT(C_RR_DRAW);
        const uint32_t ctr[4] = {(uint32_t)d, g_rng.ctr[1], g_rng.ctr[2], 4u};
        uint32_t out[4];
        philox4x32_10(ctr, g_rng.key, out);
        const REAL u = (REAL)rtmi_u01(out[0]);
        if (!(u < q)) {
            if (pending) COUNT(C_RR_END_PENDING); else COUNT(C_RR_END_BARE);
            return 1;
        }
        if (q == cx->rr_q_min) COUNT(C_RR_FLOOR_SURVIVE);
        *T = v_div(*T, q);
    }
    return 0;
}

/* Path signature (validation aid, see include/rtmi.h): every hit query that finds a hit adds
 * mix(bits of (float)t, bounce index) to the pixel's wrapping uint64 signature. */
static uint64_t g_sig;
static uint32_t sig_mix(uint32_t x, uint32_t k) {
    x ^= (k + 1u) * 0x9E3779B9u;
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}
static void sig_add(REAL t, int depth) { g_sig += (uint64_t)sig_mix(rtmi_f2u((float)t), (uint32_t)depth); }

/* color.rs:18-20 (commented out in the reference; rendered only under ORC_SKY) */
static V3 sky_color(V3 d) {
    V3 unit = v_normalize(d);
    REAL t = (REAL)0.5 * (unit.y + (REAL)1.0);
    REAL a = (REAL)1.0 - t;
    return v3(a * (REAL)1.0 + t * (REAL)0.5, a * (REAL)1.0 + t * (REAL)0.7, a * (REAL)1.0 + t * (REAL)1.0);
}

static V3 color(const RenderCtx *cx, const Ray *ray, int depth) {
    HitRecord rec;
    COUNT(C_QUERIES);
    if (hit(cx->world, ray, cx->t_min, R_MAX, &rec)) {
        sig_add(rec.t, depth);
        V3 emitted = mat_emitted(rec.mat, rec.u, rec.v, rec.p);
        if (depth < cx->max_depth) {
            Ray scattered;
            V3 att;
            if (mat_scatter(rec.mat, ray, &rec, &scattered, &att)) {
                V3 c = color(cx, &scattered, depth + 1);
                return v_add(emitted, v_mul(att, c));
            }
        }
        return emitted;
    }
    if (g_flags & ORC_SKY) return sky_color(ray->d);
    return v3(0, 0, 0); /* background is black (color.rs:21) */
}

/* Same estimator, unrolled: L = sum_k (prod_{i<k} att_i) * emitted_k.  Equal to the
 * recursion in exact arithmetic; differs by rounding order only. */
static V3 color_throughput(const RenderCtx *cx, Ray ray) {
    V3 L = v3(0, 0, 0), T = v3(1, 1, 1);
    int depth;
    for (depth = 0;; depth++) {
        HitRecord rec;
        COUNT(C_QUERIES);
        if (!hit(cx->world, &ray, cx->t_min, R_MAX, &rec)) {
            if (g_flags & ORC_SKY) L = v_add(L, v_mul(T, sky_color(ray.d)));
            break;
        }
        sig_add(rec.t, depth);
        V3 emitted = mat_emitted(rec.mat, rec.u, rec.v, rec.p);
        L = v_add(L, v_mul(T, emitted));
        if (depth >= cx->max_depth) break;
        Ray scattered;
        V3 att;
        if (!mat_scatter(rec.mat, &ray, &rec, &scattered, &att)) break;
        T = v_mul(T, att);
        if (roulette_ends(cx, &T, depth + 1, 0)) { depth++; break; }
        ray = scattered;
    }
    g_bounces = depth;
    return L;
}

/* ================================================================================== */
/* next-event estimation — include/rtmi_nee.h (not in the reference)                   */
/* ================================================================================== */
/* One entry of the light table in the device's order (rtmi_scene_attach_lights): the leaf, its geometry and the three
 * float values the device keeps.  OrcLight is the exported layout (80 B); NeeL the working copy in REAL. */
typedef struct {
    uint64_t handle; /* the leaf Hittable (orc_emitters) */
    int32_t kind;    /* 0 sphere, 2 rect (RTMI_PRIM_*) */
    int32_t plane;   /* rect: 0 YZ, 1 ZX, 2 XY; sphere: -1 */
    double geo[5];   /* rect {a0, b0, a1, b1, k}; sphere {cx, cy, cz, r, 0} */
    double area, p_sel, cdf;
} OrcLight;
typedef struct {
    const Hittable *h;
    int plane;
    REAL g0, g1, g2, g3, k;
    REAL area, p_sel, cdf;
} NeeL;

#ifdef ORC_F32
#define NEE_2_OVER_PI 0.63661977236758134f /* RTMI_NEE_2_OVER_PI */
#define NEE_INV_4PI 0.079577471545947668f  /* RTMI_NEE_INV_4PI */
#define NEE_PI RTMI_PI_F
#else
#define NEE_2_OVER_PI 0.636619772367581343075535053490057448
#define NEE_INV_4PI 0.0795774715459476678844418816862571810
#define NEE_PI 3.14159265358979323846264338327950288
#endif

/* the Lambertian's density of direction w about the scatter normal n: (2/pi) max(0, cos)^3 */
static REAL nee_pb_lambert(V3 w, V3 n) {
    REAL c = v_dot(w, n) / R_SQRT(v_dot(w, w) * v_dot(n, n));
    return c > (REAL)0 ? NEE_2_OVER_PI * (c * c * c) : (REAL)0;
}
/* power heuristic as ratios: light sample p_b p_l / (p_b^2 + p_l^2), BSDF hit p_b^2 / (p_b^2 + p_l^2) */
static REAL nee_mis_light(REAL pb, REAL pl) {
    REAL r = pb < pl ? pb / pl : pl / pb;
    return r / ((REAL)1 + r * r);
}
static REAL nee_mis_bsdf(REAL pb, REAL pl) {
    if (pb >= pl) { REAL r = pl / pb; return (REAL)1 / ((REAL)1 + r * r); }
    REAL r = pb / pl, r2 = r * r;
    return r2 / ((REAL)1 + r2);
}
static V3 nee_rect_point(const NeeL *L, REAL a, REAL b) {
    return L->plane == 0 ? v3(L->k, a, b) : (L->plane == 1 ? v3(b, L->k, a) : v3(a, b, L->k));
}
static REAL nee_axis(const NeeL *L, V3 w) { return L->plane == 0 ? w.x : (L->plane == 1 ? w.y : w.z); }
/* p_l = p_sel p_L of the light at q seen from x; a sphere's from inside is 0 */
static REAL nee_pdf(const NeeL *L, V3 x, V3 q) {
    if (L->plane >= 0) {
        V3 w = v_sub(q, x);
        REAL d2 = v_dot(w, w);
        return L->p_sel * (d2 * R_SQRT(d2)) / (R_FABS(nee_axis(L, w)) * L->area);
    }
    V3 dc = v_sub(v3(L->g0, L->g1, L->g2), x);
    REAL s = (L->g3 * L->g3) / v_dot(dc, dc);
    if (!(s < (REAL)1)) return 0;
    REAL omc = s / ((REAL)1 + R_SQRT((REAL)1 - s));
    return L->p_sel / ((REAL)2 * NEE_PI * omc);
}
/* a point on L for the vertex x: *dir = q - x (unnormalised) and *pl; 0 = no sample */
static int nee_sample(const NeeL *L, V3 x, REAL u1, REAL u2, V3 *dir, REAL *pl) {
    if (L->plane >= 0) {
        V3 q = nee_rect_point(L, L->g0 + u1 * (L->g2 - L->g0), L->g1 + u2 * (L->g3 - L->g1));
        *dir = v_sub(q, x);
        *pl = nee_pdf(L, x, q);
        return 1;
    }
    V3 dc = v_sub(v3(L->g0, L->g1, L->g2), x);
    REAL dist2 = v_dot(dc, dc), r2 = L->g3 * L->g3;
    REAL s = r2 / dist2;
    if (!(s < (REAL)1)) return 0;
    REAL omc = s / ((REAL)1 + R_SQRT((REAL)1 - s));
    REAL om = u1 * omc;
    REAL ct = (REAL)1 - om, st = R_SQRT(R_FMAX((REAL)0, om * ((REAL)2 - om)));
    REAL phi = (REAL)2 * NEE_PI * u2;
    REAL dist = R_SQRT(dist2);
    V3 w = v_div(dc, dist);
    REAL sg = w.z >= (REAL)0 ? (REAL)1 : (REAL)-1;
    REAL a = (REAL)-1 / (sg + w.z), b = w.x * w.y * a;
    V3 t1 = v3((REAL)1 + sg * w.x * w.x * a, sg * b, -sg * w.x), t2 = v3(b, sg + w.y * w.y * a, -w.y);
    V3 d = v_add(v_add(v_scale(w, ct), v_scale(t1, st * m_cos(phi))), v_scale(t2, st * m_sin(phi)));
    REAL tq = dist * ct - R_SQRT(R_FMAX((REAL)0, r2 - dist2 * (st * st)));
    *dir = v_scale(d, tq);
    *pl = L->p_sel / ((REAL)2 * NEE_PI * omc);
    return tq > (REAL)0;
}

/* ---- the light tree — include/rtmi_light_tree.h, written from its "Selection" paragraph ---------------------------- */
/* The exported layouts are rtmi_light_node (32 B) and rtmi_light_path (8 B).  The stored values are floats; every
 * operation below is in REAL: the fp32 library rounds each once as the header says, the f64 library evaluates the same
 * operations in double on the floats widened. */
typedef struct {
    float c[3];
    float r2;
    float power;
    uint32_t link; /* interior: slot of the left child, the right one follows; leaf: TREE_LEAF | light */
    uint32_t pad[2];
} OrcLightNode;
typedef struct {
    uint32_t trail, depth;
} OrcLightPath;
typedef struct {
    const OrcLightNode *nodes;
    uint32_t n_nodes;
    const OrcLightPath *paths; /* n_nodes / 2 entries; pick does not read them */
} LightTree;
#define TREE_LEAF 0x80000000u
#define TREE_ONE_MINUS ((REAL)0.99999994039535522) /* 1 - 2^-24 */

/* 0 when every walk over the tree stays inside it and ends: 2 * lights slots, the children of an interior node at an
 * even link past their parent, every leaf a light of the table, no path deeper than 32 */
static int tree_invalid(const LightTree *t) {
    if (!t->nodes || t->n_nodes < 2u || (t->n_nodes & 1u)) return 1;
    for (uint32_t i = 1; i < t->n_nodes; i++) {
        const uint32_t link = t->nodes[i].link;
        if (link & TREE_LEAF) {
            if ((link & ~TREE_LEAF) >= t->n_nodes / 2u) return 1;
        } else if (link <= i || (link & 1u) || link >= t->n_nodes - 1u) {
            return 1;
        }
    }
    if (t->paths)
        for (uint32_t i = 0; i < t->n_nodes / 2u; i++)
            if (t->paths[i].depth > 32u) return 1;
    return 0;
}
/* I = N.power / max(d2, N.r2), d = N.c - x per component, d2 = (d.x * d.x + d.y * d.y) + d.z * d.z */
static REAL tree_importance(const OrcLightNode *N, V3 x) {
    const REAL dx = (REAL)N->c[0] - x.x, dy = (REAL)N->c[1] - x.y, dz = (REAL)N->c[2] - x.z;
    const REAL d2 = (dx * dx + dy * dy) + dz * dz;
    const REAL r2 = (REAL)N->r2;
    if (!(d2 > r2)) COUNT(C_TREE_FLOOR);
    return (REAL)N->power / (d2 > r2 ? d2 : r2);
}
/* the light the walk from x with the uniform u ends at, and its probability */
static uint32_t tree_pick(const LightTree *t, V3 x, REAL u, REAL *p_out) {
    uint32_t link = t->nodes[1].link;
    REAL p = 1;
    while (!(link & TREE_LEAF)) {
        const OrcLightNode *Lc = &t->nodes[link], *Rc = &t->nodes[link + 1u];
        const REAL il = tree_importance(Lc, x), ir = tree_importance(Rc, x);
        const REAL s = il + ir;
        const REAL pl = il / s;
        REAL v;
        if (pl == (REAL)1 || ir / s == (REAL)1) COUNT(C_TREE_P_ONE); /* counted only: pr is the else branch's */
        if (u < pl) {
            COUNT(C_TREE_LEFT);
            v = u / pl;
            p = p * pl;
            link = Lc->link;
        } else {
            const REAL pr = ir / s;
            COUNT(C_TREE_RIGHT);
            v = (u - pl) / pr;
            p = p * pr;
            link = Rc->link;
        }
        u = v < TREE_ONE_MINUS ? v : TREE_ONE_MINUS;
        if (!(v <= TREE_ONE_MINUS)) COUNT(C_TREE_CLAMP);
    }
    *p_out = p;
    return link & ~TREE_LEAF;
}
/* the probability that the walk from x ends at light li: the product along paths[li] */
static REAL tree_pmf(const LightTree *t, V3 x, uint32_t li) {
    const uint32_t trail = t->paths[li].trail, depth = t->paths[li].depth;
    uint32_t link = t->nodes[1].link;
    REAL p = 1;
    for (uint32_t d = 0; d < depth && !(link & TREE_LEAF); d++) {
        const OrcLightNode *Lc = &t->nodes[link], *Rc = &t->nodes[link + 1u];
        const REAL il = tree_importance(Lc, x), ir = tree_importance(Rc, x);
        const REAL s = il + ir;
        if ((trail >> d) & 1u) { p = p * (ir / s); link = Rc->link; }
        else { p = p * (il / s); link = Lc->link; }
    }
    return p;
}

/* the light-sample stream of the current pixel sample: counter (block, sample, pixel, 3) */
static Stream g_light_rng;

/* The shadow ray of a light sample from x toward `dir` at the path's time: the path's item scan, its media drawing their
 * free flights from the light-sample stream.  Returns whether it hit anything (*srec). */
static int shadow_hit(const RenderCtx *cx, V3 x, V3 dir, REAL time, HitRecord *srec) {
    Ray sray = ray_new(x, dir, time);
    Stream keep = g_rng;
    g_rng = g_light_rng;
    int got = hit(cx->world, &sray, cx->t_min, R_MAX, srec);
    g_light_rng = g_rng;
    g_rng = keep;
    return got;
}

/* color_throughput with one light sample per scattering Lambertian / Isotropic vertex, combined with the BSDF sample by
 * the power heuristic (include/rtmi_nee.h).  With n == 0 it is color_throughput.  The vertex's light sample is fixed
 * (c, dir) before T takes the attenuation and before the roulette test; its shadow ray is traced after the test, also
 * when the test ends the continuation (include/rtmi_roulette.h).
 * With a light tree over a table of more than one light (include/rtmi_light_tree.h) the vertex's light is the walk's
 * from the vertex, and the walk's probability takes p_sel's place in a working copy of the light: the pick's at the
 * light sample, the reverse walk's from the ray's origin at a BSDF hit.  Nothing else changes. */
static V3 color_nee(const RenderCtx *cx, Ray ray, const NeeL *lights, int n, const LightTree *tree) {
    V3 L = v3(0, 0, 0), T = v3(1, 1, 1);
    REAL pb = 0; /* density of the scatter that produced `ray`; 0 = weight 1 at an emitter hit */
    const int walk = tree && n > 1;
    int picked = -1;   /* the light the previous vertex's walk picked (meaningful while pb > 0) ... */
    REAL picked_p = 0; /* ... and the probability the pick returned */
    int depth;
    for (depth = 0;; depth++) {
        HitRecord rec;
        COUNT(C_QUERIES);
        if (!hit(cx->world, &ray, cx->t_min, R_MAX, &rec)) {
            if (g_flags & ORC_SKY) L = v_add(L, v_mul(T, sky_color(ray.d)));
            break;
        }
        sig_add(rec.t, depth);
        V3 emitted = mat_emitted(rec.mat, rec.u, rec.v, rec.p);
        if (rec.mat->kind == MAT_DIFFUSE_LIGHT && rec.prim && pb > (REAL)0) {
            for (int li = 0; li < n; li++) {
                if (lights[li].h != rec.prim) continue;
                REAL pl;
                if (walk) {
                    NeeL Lt = lights[li];
                    Lt.p_sel = tree_pmf(tree, ray.o, (uint32_t)li);
                    COUNT(C_TREE_HIT_PMF);
                    if (li == picked) {
                        COUNT(C_TREE_HIT_PICKED);
                        if (memcmp(&Lt.p_sel, &picked_p, sizeof(REAL)) != 0) COUNT(C_TREE_HIT_PICKED_MISMATCH);
                    }
                    pl = nee_pdf(&Lt, ray.o, rec.p);
                } else {
                    pl = nee_pdf(&lights[li], ray.o, rec.p);
                }
                if (pl > (REAL)0) emitted = v_scale(emitted, nee_mis_bsdf(pb, pl));
                break;
            }
        }
        L = v_add(L, v_mul(T, emitted));
        if (depth >= cx->max_depth) break;
        Ray scattered;
        V3 att;
        const int kind = rec.mat->kind;
        if (!mat_scatter(rec.mat, &ray, &rec, &scattered, &att)) break;
        pb = 0;
        int pending = 0, lo = 0;
        V3 c = v3(0, 0, 0), dir = v3(0, 0, 0);
        if (n > 0 && (kind == MAT_LAMBERTIAN || kind == MAT_ISOTROPIC)) {
            const int iso = kind == MAT_ISOTROPIC;
            V3 hn = rec.normal; /* the normal the scatter saw (mat_scatter's FACE_FORWARD rule) */
            if ((g_flags & ORC_FACE_FORWARD) && v_dot(ray.d, hn) > (REAL)0) hn = v_neg(hn);
            pb = iso ? NEE_INV_4PI : nee_pb_lambert(scattered.d, hn);
            uint32_t w0 = stream_u32(&g_light_rng), w1 = stream_u32(&g_light_rng), w2 = stream_u32(&g_light_rng);
            REAL us = (REAL)rtmi_u01(w0);
            NeeL Lt;               /* the working copy under the tree */
            const NeeL *Ls;        /* the light that is sampled */
            if (walk) {
                COUNT(C_TREE_WALK);
                lo = (int)tree_pick(tree, rec.p, us, &picked_p);
                picked = lo;
                Lt = lights[lo];
                Lt.p_sel = picked_p;
                Ls = &Lt;
            } else {
                int hi = n - 1; /* the first light whose cdf exceeds us */
                while (lo < hi) {
                    int mid = (lo + hi) >> 1;
                    if (us < lights[mid].cdf) hi = mid; else lo = mid + 1;
                }
                Ls = &lights[lo];
            }
            REAL pl;
            const int sampled = nee_sample(Ls, rec.p, (REAL)rtmi_u01(w1), (REAL)rtmi_u01(w2), &dir, &pl);
            if (walk && !sampled) COUNT(C_TREE_NO_SAMPLE);
            if (sampled) {
                REAL pbl = iso ? NEE_INV_4PI : nee_pb_lambert(dir, hn);
                if (pbl > (REAL)0 && pl > (REAL)0 && pl < R_MAX) {
                    c = v_scale(v_mul(T, att), nee_mis_light(pbl, pl));
                    pending = 1;
                }
            }
        }
        T = v_mul(T, att);
        const int ends = roulette_ends(cx, &T, depth + 1, pending);
        if (pending) {
            HitRecord srec;
            if (shadow_hit(cx, rec.p, dir, ray.time, &srec) && srec.prim == lights[lo].h && srec.mat->kind == MAT_DIFFUSE_LIGHT)
                L = v_add(L, v_mul(c, mat_emitted(srec.mat, srec.u, srec.v, srec.p)));
        }
        if (ends) { depth++; break; }
        ray = scattered;
    }
    g_bounces = depth;
    return L;
}

/* ================================================================================== */
/* environment lighting — include/rtmi_env.h (not in the reference)                    */
/* ================================================================================== */
/* The map and its sampling tables (rtmi_env_tables' outputs, passed in like the light table), and the render's p_env. */
typedef struct {
    int w, h;
    const float *rgb;                               /* [h][w][3], row 0 the top row */
    const float *row_cdf, *row_p, *col_cdf, *col_p; /* [h], [h], [h][w], [h][w] */
    REAL p_env;
} EnvMap;

#ifdef ORC_F32
#define ENV_PI RTMI_PI_F
#define ENV_PIO2 RTMI_PIO2_F
#define ENV_2PI2 19.739208802178716f     /* RTMI_ENV_2PI2_F */
#define ENV_ONE_MINUS 0.99999994039535522f /* RTMI_ENV_ONE_MINUS */
#else
#define ENV_PI 3.14159265358979323846264338327950288
#define ENV_PIO2 1.57079632679489661923132169163975144
#define ENV_2PI2 19.7392088021787172376689819991737235
#define ENV_ONE_MINUS 0.99999994039535522
#endif

/* "Direction -> (u, v)": 0 for a direction that sees nothing */
static int env_uv(V3 d, REAL *u, REAL *v, REAL *theta) {
    const REAL ax = R_FABS(d.x), ay = R_FABS(d.y), az = R_FABS(d.z);
    if (!(ax <= R_MAX && ay <= R_MAX && az <= R_MAX)) return 0; /* a component that is not finite */
    const REAL m = R_FMAX(R_FMAX(ax, ay), az);
    if (!(m > (REAL)0)) return 0;
    const V3 s = v_div(d, m);
    const REAL l = R_SQRT((s.x * s.x + s.y * s.y) + s.z * s.z);
    const V3 n = v_div(s, l);
    const REAL phi = m_atan2(n.z, n.x);
    *theta = m_asin(R_FMIN(R_FMAX(n.y, (REAL)-1), (REAL)1));
    *u = (REAL)1 - (phi + ENV_PI) / ((REAL)2 * ENV_PI);
    *v = (*theta + ENV_PIO2) / ENV_PI;
    return 1;
}
static V3 env_texel(const EnvMap *E, int j, int i) {
    const float *t = E->rgb + ((size_t)j * (size_t)E->w + (size_t)i) * 3;
    return v3((REAL)t[0], (REAL)t[1], (REAL)t[2]);
}
static V3 env_lerp(V3 a, V3 b, REAL f) { /* a + f * (b - a) per channel */
    return v3(a.x + f * (b.x - a.x), a.y + f * (b.y - a.y), a.z + f * (b.z - a.z));
}
static int env_clampi(long v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }
/* "Radiance env(d)" at d's (u, v): bilinear, columns wrapped, rows clamped */
static V3 env_radiance(const EnvMap *E, REAL u, REAL v) {
    const REAL x = u * (REAL)E->w - (REAL)0.5, y = ((REAL)1 - v) * (REAL)E->h - (REAL)0.5;
    const REAL x0 = R_FLOOR(x), y0 = R_FLOOR(y);
    const REAL fx = x - x0, fy = y - y0;
    const long xi = (long)x0, yi = (long)y0;
    const int i0 = (int)(((xi % E->w) + E->w) % E->w), i1 = (i0 + 1) % E->w;
    const int j0 = env_clampi(yi, 0, E->h - 1), j1 = env_clampi(yi + 1, 0, E->h - 1);
    const V3 t0 = env_lerp(env_texel(E, j0, i0), env_texel(E, j0, i1), fx);
    const V3 t1 = env_lerp(env_texel(E, j1, i0), env_texel(E, j1, i1), fx);
    return env_lerp(t0, t1, fy);
}
/* the light sample's density in texel (i, j) at cos(theta) = ct */
static REAL env_pdf_texel(const EnvMap *E, int i, int j, REAL ct) {
    const size_t k = (size_t)j * (size_t)E->w + (size_t)i;
    return (((E->p_env * (REAL)E->row_p[j]) * (REAL)E->col_p[k]) * (REAL)(E->w * E->h)) / (ENV_2PI2 * ct);
}
/* the BSDF-side pdf of the direction with (u, v, theta) */
static REAL env_pdf(const EnvMap *E, REAL u, REAL v, REAL theta) {
    if (!(E->p_env > (REAL)0)) return 0;
    const REAL ct = m_cos(theta);
    if (!(ct > (REAL)0)) return 0;
    const int i = env_clampi((long)R_FLOOR(u * (REAL)E->w), 0, E->w - 1);
    const int j = env_clampi((long)R_FLOOR(((REAL)1 - v) * (REAL)E->h), 0, E->h - 1);
    return env_pdf_texel(E, i, j, ct);
}
/* the first index with us < cdf[index] */
static int env_search(const float *cdf, int n, REAL us) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (us < (REAL)cdf[mid]) hi = mid; else lo = mid + 1;
    }
    return lo;
}
/* "Light sample from two uniforms": a unit direction and its pdf; 0 = no sample */
static int env_sample(const EnvMap *E, REAL u1, REAL u2, V3 *dir, REAL *pdf) {
    const int j = env_search(E->row_cdf, E->h, u1);
    const float *cc = E->col_cdf + (size_t)j * (size_t)E->w;
    const int i = env_search(cc, E->w, u2);
    const REAL r0 = j > 0 ? (REAL)E->row_cdf[j - 1] : (REAL)0, c0 = i > 0 ? (REAL)cc[i - 1] : (REAL)0;
    const REAL fy = R_FMIN((u1 - r0) / ((REAL)E->row_cdf[j] - r0), ENV_ONE_MINUS);
    const REAL fx = R_FMIN((u2 - c0) / ((REAL)cc[i] - c0), ENV_ONE_MINUS);
    const REAL u = ((REAL)i + fx) / (REAL)E->w, v = (REAL)1 - ((REAL)j + fy) / (REAL)E->h;
    const REAL phi = ((REAL)1 - u) * ((REAL)2 * ENV_PI) - ENV_PI;
    const REAL theta = v * ENV_PI - ENV_PIO2;
    const REAL ct = m_cos(theta);
    if (!(ct > (REAL)0)) return 0;
    *dir = v3(ct * m_cos(phi), m_sin(theta), ct * m_sin(phi));
    *pdf = env_pdf_texel(E, i, j, ct);
    return *pdf > (REAL)0 && *pdf < R_MAX;
}

/* rtmi_render_env's estimator ("Estimator" in include/rtmi_env.h): color_nee with the map where a ray leaves the world
 * and, with nee != 0, the map as one more light.  nee == 0 is color_throughput plus the map at weight 1. */
static V3 color_env(const RenderCtx *cx, Ray ray, const NeeL *lights, int n, const EnvMap *E, int nee) {
    V3 L = v3(0, 0, 0), T = v3(1, 1, 1);
    const REAL p_env = E->p_env, p_area = (REAL)1 - E->p_env;
    REAL pb = 0;     /* density of the scatter that produced `ray`, set where the vertex read its stream-3 words */
    int diffuse = 0; /* `ray` left a Lambertian or Isotropic vertex (counters only) */
    int depth;
    for (depth = 0;; depth++) {
        HitRecord rec;
        COUNT(C_QUERIES);
        if (!hit(cx->world, &ray, cx->t_min, R_MAX, &rec)) { /* the map, with its weight */
            REAL u, v, theta;
            if (env_uv(ray.d, &u, &v, &theta)) {
                REAL w = 1;
                int weighted = 0;
                if (nee && pb > (REAL)0) {
                    const REAL pe = env_pdf(E, u, v, theta);
                    if (pe > (REAL)0) { w = nee_mis_bsdf(pb, pe); weighted = 1; }
                }
                if (weighted) COUNT(C_ENV_MISS_MIS); else if (nee && diffuse) COUNT(C_ENV_MISS_ONE);
                L = v_add(L, v_mul(T, v_scale(env_radiance(E, u, v), w)));
            }
            break;
        }
        sig_add(rec.t, depth);
        V3 emitted = mat_emitted(rec.mat, rec.u, rec.v, rec.p);
        if (nee && rec.mat->kind == MAT_DIFFUSE_LIGHT && rec.prim && pb > (REAL)0) {
            for (int li = 0; li < n; li++) {
                if (lights[li].h != rec.prim) continue;
                REAL pl = p_area * nee_pdf(&lights[li], ray.o, rec.p);
                if (pl > (REAL)0) {
                    emitted = v_scale(emitted, nee_mis_bsdf(pb, pl));
                    if (p_env > (REAL)0) COUNT(C_ENV_EMIT_SCALED);
                }
                break;
            }
        }
        L = v_add(L, v_mul(T, emitted));
        if (depth >= cx->max_depth) break;
        Ray scattered;
        V3 att;
        const int kind = rec.mat->kind;
        if (!mat_scatter(rec.mat, &ray, &rec, &scattered, &att)) break;
        pb = 0;
        diffuse = kind == MAT_LAMBERTIAN || kind == MAT_ISOTROPIC;
        int pending = 0, to_env = 0, lo = 0;
        V3 c = v3(0, 0, 0), dir = v3(0, 0, 0);
        if (nee && diffuse && (n > 0 || p_env > (REAL)0)) { /* the map or the table can be sampled */
            const int iso = kind == MAT_ISOTROPIC;
            V3 hn = rec.normal;
            if ((g_flags & ORC_FACE_FORWARD) && v_dot(ray.d, hn) > (REAL)0) hn = v_neg(hn);
            pb = iso ? NEE_INV_4PI : nee_pb_lambert(scattered.d, hn);
            uint32_t w0 = stream_u32(&g_light_rng), w1 = stream_u32(&g_light_rng), w2 = stream_u32(&g_light_rng);
            REAL us = (REAL)rtmi_u01(w0), pl = 0;
            int ok = 0;
            if (us < p_env) { /* the map */
                to_env = 1;
                COUNT(C_ENV_SAMPLE);
                ok = env_sample(E, (REAL)rtmi_u01(w1), (REAL)rtmi_u01(w2), &dir, &pl);
                if (!ok) COUNT(C_ENV_NO_SAMPLE);
            } else if (n > 0) { /* an area light, with the rest of us */
                us = (us - p_env) / p_area;
                int hi = n - 1;
                while (lo < hi) {
                    int mid = (lo + hi) >> 1;
                    if (us < lights[mid].cdf) hi = mid; else lo = mid + 1;
                }
                ok = nee_sample(&lights[lo], rec.p, (REAL)rtmi_u01(w1), (REAL)rtmi_u01(w2), &dir, &pl);
                pl = p_area * pl;
                if (p_env > (REAL)0) COUNT(C_ENV_AREA_SAMPLE);
            }
            if (ok) {
                REAL pbl = iso ? NEE_INV_4PI : nee_pb_lambert(dir, hn);
                if (pbl > (REAL)0 && pl > (REAL)0 && pl < R_MAX) {
                    c = v_scale(v_mul(T, att), nee_mis_light(pbl, pl));
                    pending = 1;
                }
            }
        }
        T = v_mul(T, att);
        const int ends = roulette_ends(cx, &T, depth + 1, pending);
        if (pending) {
            HitRecord srec;
            const int got = shadow_hit(cx, rec.p, dir, ray.time, &srec);
            if (to_env) { /* V = 1 iff the ray hits nothing; env(d) from the sampled direction */
                REAL u, v, theta;
                if (got) COUNT(C_ENV_OCCLUDED); else COUNT(C_ENV_UNOCCLUDED);
                if (!got && env_uv(dir, &u, &v, &theta)) L = v_add(L, v_mul(c, env_radiance(E, u, v)));
            } else if (got && srec.prim == lights[lo].h && srec.mat->kind == MAT_DIFFUSE_LIGHT) {
                L = v_add(L, v_mul(c, mat_emitted(srec.mat, srec.u, srec.v, srec.p)));
            }
        }
        if (ends) { depth++; break; }
        ray = scattered;
    }
    g_bounces = depth;
    return L;
}

/* ================================================================================== */
/* Camera — src/camera.rs                                                              */
/* ================================================================================== */
typedef struct {
    D3 origind, llcd, hord, verd, ud, vd;
    double time0d, time1d, lens_radiusd;
    V3 origin, llc, horizontal, vertical, u, v;
    REAL time0, time1, lens_radius;
} Camera;

/* camera.rs:53-67 */
static Ray camera_get_ray(const Camera *c, REAL s, REAL t) {
    V3 origin;
    if (c->lens_radius == 0) {
        origin = c->origin;
    } else {
        V3 rd = v_scale(random_in_unit_disk(), c->lens_radius);
        V3 offset = v_add(v_scale(c->u, rd.x), v_scale(c->v, rd.y));
        origin = v_add(c->origin, offset);
    }
    REAL time = c->time0 + rng_uniform() * (c->time1 - c->time0);
    V3 dir = v_sub(v_add(v_add(c->llc, v_scale(c->horizontal, s)), v_scale(c->vertical, t)), origin);
    return ray_new(origin, dir, time);
}
/* one sample of pixel (i, j) from the render path's stream: u then v, then get_ray's draws — tests/test.rs:66-68 */
static Ray pixel_ray(const Camera *cam, int i, int j, int nx, int ny) {
    REAL u = ((REAL)i + rng_uniform()) / (REAL)nx;
    REAL v = ((REAL)j + rng_uniform()) / (REAL)ny;
    return camera_get_ray(cam, u, v);
}

/* ================================================================================== */
/* exported builder API                                                                */
/* ================================================================================== */
ORC_API int orc_is_f32(void) { return ORC_IS_F32; }
ORC_API void orc_set_flags(int flags) { g_flags = flags; }
ORC_API void orc_seed_scene_rng(uint64_t seed) { stream_init(&g_scene_rng, seed, 0, 0, 1); }
ORC_API void orc_philox(const uint32_t *ctr, const uint32_t *key, uint32_t *out) { philox4x32_10(ctr, key, out); }
ORC_API double orc_scene_uniform(void) { return scene_uniform(); }
ORC_API uint32_t orc_scene_range(uint32_t n) { return scene_range(n); }

static Texture *new_tex(int kind) { Texture *t = (Texture *)arena_alloc(sizeof(Texture)); t->kind = kind; return t; }
ORC_API void *orc_tex_solid(double r, double g, double b) {
    Texture *t = new_tex(TEX_SOLID);
    t->color = v3((REAL)r, (REAL)g, (REAL)b);
    return t;
}
ORC_API void *orc_tex_checker(void *odd, void *even) {
    Texture *t = new_tex(TEX_CHECKER);
    t->odd = (Texture *)odd; t->even = (Texture *)even;
    return t;
}
/* Perlin::new — perlin.rs:12-36, 67-74.  Tables are drawn in f64 (scene set-up), then
 * rounded once to the working precision. */
ORC_API void *orc_tex_noise(double scale) {
    Texture *t = new_tex(TEX_NOISE);
    t->scale = (REAL)scale;
    Perlin *pn = (Perlin *)arena_alloc(sizeof(Perlin));
    for (int i = 0; i < 256; i++) { /* perlin_generate :12-26 */
        double x = -1.0 + 2.0 * scene_uniform();
        double y = -1.0 + 2.0 * scene_uniform();
        double z = -1.0 + 2.0 * scene_uniform();
        double n = sqrt(x * x + y * y + z * z);
        pn->ran_vec[i] = v3((REAL)(x / n), (REAL)(y / n), (REAL)(z / n));
    }
    int *perms[3] = {pn->perm_x, pn->perm_y, pn->perm_z};
    for (int k = 0; k < 3; k++) { /* perlin_generate_perm :28-36 + permute :4-10 */
        int *p = perms[k];
        for (int i = 0; i < 256; i++) p[i] = i;
        for (int i = 255; i >= 0; i--) {
            uint32_t target = scene_range((uint32_t)i + 1);
            int tmp = p[i]; p[i] = p[target]; p[target] = tmp;
        }
    }
    t->noise = pn;
    return t;
}
ORC_API void *orc_tex_image(const uint8_t *data, uint32_t nx, uint32_t ny) {
    Texture *t = new_tex(TEX_IMAGE);
    size_t n = (size_t)nx * ny * 3;
    t->data = (uint8_t *)arena_alloc(n);
    memcpy(t->data, data, n);
    t->nx = nx; t->ny = ny;
    return t;
}
ORC_API void orc_perlin_tables(void *tex, double *ranvec768, int *perm768) {
    Texture *t = (Texture *)tex;
    for (int i = 0; i < 256; i++) {
        ranvec768[3 * i] = t->noise->ran_vec[i].x; ranvec768[3 * i + 1] = t->noise->ran_vec[i].y;
        ranvec768[3 * i + 2] = t->noise->ran_vec[i].z;
        perm768[i] = t->noise->perm_x[i]; perm768[256 + i] = t->noise->perm_y[i]; perm768[512 + i] = t->noise->perm_z[i];
    }
}

static Material *new_mat(int kind, void *tex, double param) {
    Material *m = (Material *)arena_alloc(sizeof(Material));
    m->kind = kind; m->tex = (Texture *)tex; m->param = (REAL)param;
    return m;
}
ORC_API void *orc_mat_lambertian(void *tex) { return new_mat(MAT_LAMBERTIAN, tex, 0); }
ORC_API void *orc_mat_metal(void *tex, double fuzz) { return new_mat(MAT_METAL, tex, fuzz < 1.0 ? fuzz : 1.0); } /* :70 */
ORC_API void *orc_mat_dielectric(double ref_idx) { return new_mat(MAT_DIELECTRIC, NULL, ref_idx); }
ORC_API void *orc_mat_diffuse_light(void *tex) { return new_mat(MAT_DIFFUSE_LIGHT, tex, 0); }
ORC_API void *orc_mat_isotropic(void *tex) { return new_mat(MAT_ISOTROPIC, tex, 0); }

static Hittable *new_hit(int kind) { Hittable *h = (Hittable *)arena_alloc(sizeof(Hittable)); h->kind = kind; return h; }
ORC_API void *orc_sphere(double cx, double cy, double cz, double r, void *mat) {
    Hittable *h = new_hit(H_SPHERE);
    h->c0d = (D3){cx, cy, cz}; h->rd = r;
    h->c0 = d3_to_v3(h->c0d); h->radius = (REAL)r; h->mat = (Material *)mat;
    return h;
}
ORC_API void *orc_moving_sphere(double c0x, double c0y, double c0z, double c1x, double c1y, double c1z, double t0,
                                double t1, double r, void *mat) {
    Hittable *h = new_hit(H_MOVING_SPHERE);
    h->c0d = (D3){c0x, c0y, c0z}; h->c1d = (D3){c1x, c1y, c1z}; h->rd = r; h->t0d = t0; h->t1d = t1;
    h->c0 = d3_to_v3(h->c0d); h->c1 = d3_to_v3(h->c1d); h->radius = (REAL)r; h->t0 = (REAL)t0; h->t1 = (REAL)t1;
    h->mat = (Material *)mat;
    return h;
}
static Hittable *make_rect(int plane, double x0, double y0, double x1, double y1, double k, const Material *mat) {
    Hittable *h = new_hit(H_RECT);
    h->plane = plane;
    h->x0d = x0; h->y0d = y0; h->x1d = x1; h->y1d = y1; h->kd = k;
    h->x0 = (REAL)x0; h->y0 = (REAL)y0; h->x1 = (REAL)x1; h->y1 = (REAL)y1; h->k = (REAL)k;
    h->mat = mat;
    return h;
}
ORC_API void *orc_rect(int plane, double x0, double y0, double x1, double y1, double k, void *mat) {
    return make_rect(plane, x0, y0, x1, y1, k, (Material *)mat);
}
static void list_push(Hittable *l, Hittable *h) {
    if (l->n == l->cap) {
        int ncap = l->cap ? l->cap * 2 : 8;
        Hittable **ni = (Hittable **)arena_alloc(sizeof(Hittable *) * ncap);
        if (l->n) memcpy(ni, l->items, sizeof(Hittable *) * l->n);
        l->items = ni; l->cap = ncap;
    }
    l->items[l->n++] = h;
}
ORC_API void *orc_list_new(void) { return new_hit(H_LIST); }
ORC_API void orc_list_push(void *list, void *h) { list_push((Hittable *)list, (Hittable *)h); }
/* cube.rs:15-80 : XY@max.z, XY@min.z, ZX@max.y, ZX@min.y, YZ@max.x, YZ@min.x — none flipped */
ORC_API void *orc_cube(double ax, double ay, double az, double bx, double by, double bz, void *mat) {
    Hittable *h = new_hit(H_CUBE);
    const Material *m = (Material *)mat;
    h->pmind = (D3){ax, ay, az}; h->pmaxd = (D3){bx, by, bz};
    Hittable *s = new_hit(H_LIST);
    list_push(s, make_rect(2, ax, ay, bx, by, bz, m));
    list_push(s, make_rect(2, ax, ay, bx, by, az, m));
    list_push(s, make_rect(1, az, ax, bz, bx, by, m));
    list_push(s, make_rect(1, az, ax, bz, bx, ay, m));
    list_push(s, make_rect(0, ay, az, by, bz, bx, m));
    list_push(s, make_rect(0, ay, az, by, bz, ax, m));
    h->sides = s;
    return h;
}
/* test only: the innermost object of a transform chain's round trip (tests/test_path_contract.py) */
ORC_API void *orc_probe_point(double t, double nx, double ny, double nz) {
    Hittable *h = new_hit(H_PROBE_POINT);
    h->radius = (REAL)t; h->c0 = v3((REAL)nx, (REAL)ny, (REAL)nz);
    return h;
}
ORC_API void *orc_flip_normals(void *child) { Hittable *h = new_hit(H_FLIP); h->child = (Hittable *)child; return h; }
ORC_API void *orc_translate(void *child, double ox, double oy, double oz) {
    Hittable *h = new_hit(H_TRANSLATE);
    h->child = (Hittable *)child; h->offsetd = (D3){ox, oy, oz}; h->offset = d3_to_v3(h->offsetd);
    return h;
}
/* rotate.rs:30-81 ; the bbox loop never updates (min starts at f64::MIN, max at f64::MAX) */
ORC_API void *orc_rotate(int axis, void *child, double angle) {
    Hittable *h = new_hit(H_ROTATE);
    h->axis = axis; h->child = (Hittable *)child;
    double radians = (3.14159265358979323846264338327950288 / 180.0) * angle;
    h->sind = sin(radians); h->cosd = cos(radians);
    h->sin_t = (REAL)h->sind; h->cos_t = (REAL)h->cosd;
    AABBd b;
    h->has_bbox = bounding_box(h->child, 0.0, 1.0, &b);
    if (h->has_bbox) {
        const double MX = 1.79769313486231570814527423731704357e+308;
        h->rot_bbox.min = (D3){-MX, -MX, -MX};
        h->rot_bbox.max = (D3){MX, MX, MX};
    }
    return h;
}
ORC_API void *orc_constant_medium(void *boundary, double density, void *tex) {
    Hittable *h = new_hit(H_MEDIUM);
    h->child = (Hittable *)boundary; h->density = (REAL)density;
    h->phase.kind = MAT_ISOTROPIC; h->phase.tex = (Texture *)tex; h->phase.param = 0;
    return h;
}

/* BVHNode::new — bvh.rs:17-66.  `sort_unstable_by` with the reference's Less/Greater-only
 * comparator has no defined result on ties; this restatement sorts STABLY by
 * bbox.min[axis] (strict `a - b < 0`), which is one valid outcome. */
static int g_bvh_error = 0;
static void stable_sort(Hittable **v, double *key, int n) {
    /* insertion sort is O(n^2) but n <= a few thousand at set-up; merge for larger */
    if (n < 2) return;
    Hittable **tv = (Hittable **)malloc(sizeof(Hittable *) * n);
    double *tk = (double *)malloc(sizeof(double) * n);
    for (int w = 1; w < n; w *= 2) {
        for (int lo = 0; lo < n; lo += 2 * w) {
            int mid = lo + w < n ? lo + w : n, hi = lo + 2 * w < n ? lo + 2 * w : n;
            int i = lo, j = mid, o = lo;
            while (i < mid && j < hi) {
                if (key[j] - key[i] < 0.0) { tv[o] = v[j]; tk[o++] = key[j++]; }
                else { tv[o] = v[i]; tk[o++] = key[i++]; }
            }
            while (i < mid) { tv[o] = v[i]; tk[o++] = key[i++]; }
            while (j < hi) { tv[o] = v[j]; tk[o++] = key[j++]; }
        }
        memcpy(v, tv, sizeof(Hittable *) * n);
        memcpy(key, tk, sizeof(double) * n);
    }
    free(tv); free(tk);
}
static Hittable *bvh_new(Hittable **list, int len, double t0, double t1) {
    uint32_t axis = scene_range(3); /* bvh.rs:40 */
    double *key = (double *)malloc(sizeof(double) * len);
    for (int i = 0; i < len; i++) {
        AABBd b;
        if (!bounding_box(list[i], t0, t1, &b)) { g_bvh_error = 1; b.min = (D3){0, 0, 0}; }
        key[i] = axis == 0 ? b.min.x : (axis == 1 ? b.min.y : b.min.z);
    }
    stable_sort(list, key, len);
    free(key);
    Hittable *h = new_hit(H_BVH);
    if (len == 1) { h->left = list[0]; h->right = list[0]; }
    else if (len == 2) { h->left = list[0]; h->right = list[1]; }
    else {
        h->left = bvh_new(list, len / 2, t0, t1);
        h->right = bvh_new(list + len / 2, len - len / 2, t0, t1);
    }
    AABBd lb, rb;
    if (!bounding_box(h->left, t0, t1, &lb) || !bounding_box(h->right, t0, t1, &rb)) { g_bvh_error = 1; return h; }
    h->boxd = surrounding_box(lb, rb);
    h->box.min = d3_to_v3(h->boxd.min);
    h->box.max = d3_to_v3(h->boxd.max);
    return h;
}
/* returns NULL where the reference panics ("No bounding box in BVHNode", bvh.rs:30,58) */
ORC_API void *orc_bvh(void **items, int n, double t0, double t1) {
    if (n <= 0) return NULL;
    Hittable **tmp = (Hittable **)malloc(sizeof(Hittable *) * n);
    memcpy(tmp, items, sizeof(Hittable *) * n);
    g_bvh_error = 0;
    Hittable *h = bvh_new(tmp, n, t0, t1);
    free(tmp);
    return g_bvh_error ? NULL : h;
}

/* Camera::new — camera.rs:21-51 (f64, then rounded once to the working precision) */
ORC_API void *orc_camera(double fx, double fy, double fz, double ax, double ay, double az, double ux, double uy,
                         double uz, double vfov, double aspect, double aperture, double focus_dist, double time0,
                         double time1) {
    Camera *c = (Camera *)arena_alloc(sizeof(Camera));
    double theta = vfov * 3.14159265358979323846264338327950288 / 180.0;
    double half_height = focus_dist * tan(theta / 2.0);
    double half_width = aspect * half_height;
    double wx = fx - ax, wy = fy - ay, wz = fz - az;
    double wn = sqrt(wx * wx + wy * wy + wz * wz);
    wx /= wn; wy /= wn; wz /= wn;
    double cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx; /* view_up x w */
    double cn = sqrt(cx * cx + cy * cy + cz * cz);
    cx /= cn; cy /= cn; cz /= cn;
    double vx = wy * cz - wz * cy, vy = wz * cx - wx * cz, vz = wx * cy - wy * cx; /* w x u */
    c->origind = (D3){fx, fy, fz};
    c->llcd = (D3){fx - half_width * cx - half_height * vx - focus_dist * wx,
                   fy - half_width * cy - half_height * vy - focus_dist * wy,
                   fz - half_width * cz - half_height * vz - focus_dist * wz};
    c->hord = (D3){2.0 * half_width * cx, 2.0 * half_width * cy, 2.0 * half_width * cz};
    c->verd = (D3){2.0 * half_height * vx, 2.0 * half_height * vy, 2.0 * half_height * vz};
    c->ud = (D3){cx, cy, cz};
    c->vd = (D3){vx, vy, vz};
    c->time0d = time0; c->time1d = time1; c->lens_radiusd = aperture / 2.0;
    c->origin = d3_to_v3(c->origind); c->llc = d3_to_v3(c->llcd);
    c->horizontal = d3_to_v3(c->hord); c->vertical = d3_to_v3(c->verd);
    c->u = d3_to_v3(c->ud); c->v = d3_to_v3(c->vd);
    c->time0 = (REAL)time0; c->time1 = (REAL)time1; c->lens_radius = (REAL)c->lens_radiusd;
    return c;
}
ORC_API void orc_camera_state(void *cam, double *out21) {
    Camera *c = (Camera *)cam;
    D3 *v[6] = {&c->origind, &c->llcd, &c->hord, &c->verd, &c->ud, &c->vd};
    for (int i = 0; i < 6; i++) { out21[3 * i] = v[i]->x; out21[3 * i + 1] = v[i]->y; out21[3 * i + 2] = v[i]->z; }
    out21[18] = c->time0d; out21[19] = c->time1d; out21[20] = c->lens_radiusd;
}

/* ================================================================================== */
/* create_image — tests/test.rs:55-85                                                  */
/* ================================================================================== */
/* nalgebra::clamp(val, min, max) (tests/test.rs:74): NaN -> min */
static double na_clamp(double val, double lo, double hi) {
    if (val > lo) { if (val < hi) return val; return hi; }
    return lo;
}
/* Rust `f64 as i32` (tests/test.rs:76-78): truncation, saturating, NaN -> 0 */
static int32_t as_i32(double x) {
    if (x != x) return 0;
    if (x >= 2147483647.0) return INT32_MAX;
    if (x <= -2147483648.0) return INT32_MIN;
    return (int32_t)x;
}

/* ---- next-event estimation: emitters and the NEE render (include/rtmi_nee.h) ------------------------------------- */
/* Every DiffuseLight rect or sphere leaf the object graph reaches, with what decides whether it is a light under
 * rtmi_nee.h's rules (read here from the header, not from rtmi_lights_from_desc).  OrcEmitter is the exported layout. */
typedef struct {
    uint64_t handle;
    int32_t kind, plane; /* as OrcLight */
    double geo[5];       /* as OrcLight, the working precision's values */
    int32_t under_xform; /* under a Traslate or Rotate chain */
    int32_t in_medium;   /* part of a ConstantMedium's boundary */
    int32_t count;       /* how many times the graph reaches the leaf */
    int32_t eligible;
    double weight; /* the largest channel of a SOLID texture, else 1 */
    double area;   /* rect (x1 - x0) (y1 - y0); sphere 4 pi r^2 */
} OrcEmitter; /* 88 B */

typedef struct { OrcEmitter *v; int n, cap; } EmitterList;

static void emitters_walk(const Hittable *h, int under_xform, int in_medium, EmitterList *out) {
    switch (h->kind) {
    case H_SPHERE:
    case H_RECT: {
        if (h->mat->kind != MAT_DIFFUSE_LIGHT) return;
        for (int i = 0; i < out->n; i++) {
            if (out->v[i].handle == (uint64_t)(uintptr_t)h) {
                out->v[i].count++;
                out->v[i].under_xform |= under_xform;
                out->v[i].in_medium |= in_medium;
                return;
            }
        }
        if (out->n == out->cap) {
            out->cap = out->cap ? 2 * out->cap : 16;
            out->v = (OrcEmitter *)realloc(out->v, sizeof(OrcEmitter) * (size_t)out->cap);
            if (!out->v) { fprintf(stderr, "orc: out of memory\n"); abort(); }
        }
        OrcEmitter *e = &out->v[out->n++];
        memset(e, 0, sizeof(*e));
        e->handle = (uint64_t)(uintptr_t)h;
        e->under_xform = under_xform;
        e->in_medium = in_medium;
        e->count = 1;
        const Texture *t = h->mat->tex;
        e->weight = (t && t->kind == TEX_SOLID) ? fmax(fmax((double)t->color.x, (double)t->color.y), (double)t->color.z) : 1.0;
        if (h->kind == H_RECT) {
            e->kind = 2; e->plane = h->plane;
            e->geo[0] = h->x0; e->geo[1] = h->y0; e->geo[2] = h->x1; e->geo[3] = h->y1; e->geo[4] = h->k;
            e->area = ((double)h->x1 - (double)h->x0) * ((double)h->y1 - (double)h->y0);
        } else {
            e->kind = 0; e->plane = -1;
            e->geo[0] = h->c0.x; e->geo[1] = h->c0.y; e->geo[2] = h->c0.z; e->geo[3] = h->radius; e->geo[4] = 0.0;
            e->area = 4.0 * 3.14159265358979323846264338327950288 * (double)h->radius * (double)h->radius;
        }
        return;
    }
    case H_MOVING_SPHERE:
    case H_CUBE: /* a cube's faces are one primitive of its own kind: never a light */
        return;
    case H_LIST:
        for (int i = 0; i < h->n; i++) emitters_walk(h->items[i], under_xform, in_medium, out);
        return;
    case H_FLIP:
        emitters_walk(h->child, under_xform, in_medium, out);
        return;
    case H_TRANSLATE:
    case H_ROTATE:
        emitters_walk(h->child, 1, in_medium, out);
        return;
    case H_MEDIUM:
        emitters_walk(h->child, under_xform, 1, out);
        return;
    case H_BVH: /* a node of one object holds it twice (bvh.rs:46-48): one occurrence */
        emitters_walk(h->left, under_xform, in_medium, out);
        if (h->right != h->left) emitters_walk(h->right, under_xform, in_medium, out);
        return;
    }
}

/* Writes at most `cap` emitters to `out` in the order the graph first reaches them; returns how many there are. */
ORC_API int orc_emitters(void *world, OrcEmitter *out, int cap) {
    EmitterList l = {NULL, 0, 0};
    emitters_walk((const Hittable *)world, 0, 0, &l);
    for (int i = 0; i < l.n; i++) {
        OrcEmitter *e = &l.v[i];
        int geometry = e->kind == 2 ? (e->geo[0] < e->geo[2] && e->geo[1] < e->geo[3])
                                    : (e->geo[3] > 0.0 && isfinite(e->geo[0]) && isfinite(e->geo[1]) && isfinite(e->geo[2]));
        e->eligible = geometry && !e->under_xform && !e->in_medium && e->count == 1 && e->weight > 0.0 &&
                      e->area > 0.0 && isfinite(e->area * e->weight);
        if (i < cap) out[i] = *e;
    }
    free(l.v);
    return l.n;
}

/* What render_rows takes beyond orc_render's arguments; NULL = the plain path. */
typedef struct {
    int nee;                /* color_nee with the light table */
    const OrcLight *lights; /* n_lights entries, the device's order */
    int n_lights;
    const EnvMap *env;      /* not NULL: color_env (with `nee` as its nee) */
    int rr_min_depth;       /* roulette: 0 = off */
    double rr_q_min;
    float *out_samples;     /* [ny, nx, ns, 3] or NULL */
    uint32_t *out_bounces;  /* [ny, nx] or NULL */
    const LightTree *tree;  /* not NULL: color_nee selects by the light tree (read by the NEE path only) */
} RowsExt;

/* The pixel loop of orc_render for the estimators the tests compare: the plain path, NEE (always the throughput form),
 * the environment estimator, each with or without roulette, every sample's fp32 radiance in out_samples and the
 * per-pixel sum of the depths at which the paths were written in out_bounces. */
static int render_rows(void *cam_, void *world_, const RowsExt *x, int nx, int ny, int ns, uint64_t seed, int flags,
                       int max_depth, double t_min, int row_begin, int row_end, float *out_linear, int32_t *out_rgb,
                       double *out_mean, uint64_t *out_sig) {
    static const RowsExt plain = {0, NULL, 0, NULL, 0, 1.0, NULL, NULL, NULL};
    if (!x) x = &plain;
    const Camera *cam = (Camera *)cam_;
    const int nee = x->nee, n_lights = x->n_lights;
    float *out_samples = x->out_samples;
    RenderCtx cx;
    cx.world = (Hittable *)world_;
    cx.max_depth = max_depth;
    cx.t_min = (REAL)t_min;
    cx.rr_min_depth = x->rr_min_depth;
    cx.rr_q_min = (REAL)(float)x->rr_q_min;
    g_flags = flags;
    NeeL *lights = NULL;
    if (x->lights && n_lights > 0) {
        lights = (NeeL *)malloc(sizeof(NeeL) * (size_t)n_lights);
        if (!lights) return 1;
        for (int i = 0; i < n_lights; i++) {
            const OrcLight *s = &x->lights[i];
            NeeL *d = &lights[i];
            d->h = (const Hittable *)(uintptr_t)s->handle;
            d->plane = s->kind == 2 ? s->plane : -1;
            d->g0 = (REAL)s->geo[0]; d->g1 = (REAL)s->geo[1]; d->g2 = (REAL)s->geo[2]; d->g3 = (REAL)s->geo[3];
            d->k = (REAL)s->geo[4];
            d->area = (REAL)s->area; d->p_sel = (REAL)s->p_sel; d->cdf = (REAL)s->cdf;
        }
    }
    const int throughput = (flags & ORC_THROUGHPUT_FORM) || x->rr_min_depth > 0;
    if (row_begin < 0) row_begin = 0;
    if (row_end > ny) row_end = ny;
    for (int row = row_begin; row < row_end; row++) {
        int j = ny - 1 - row;
        for (int i = 0; i < nx; i++) {
            double col[3] = {0.0, 0.0, 0.0};
            uint32_t bounces = 0;
            g_sig = 0;
            for (int s = 0; s < ns; s++) {
                stream_init(&g_rng, seed, (uint32_t)s, (uint32_t)(j * nx + i), 0);
                COUNT(C_SAMPLES);
                Ray ray = pixel_ray(cam, i, j, nx, ny);
                V3 c;
                g_bounces = 0;
                if (x->env || nee) stream_init(&g_light_rng, seed, (uint32_t)s, (uint32_t)(j * nx + i), 3);
                if (x->env) {
                    c = color_env(&cx, ray, lights, lights ? n_lights : 0, x->env, nee);
                } else if (nee) {
                    c = color_nee(&cx, ray, lights, lights ? n_lights : 0, x->tree);
                } else {
                    c = throughput ? color_throughput(&cx, ray) : color(&cx, &ray, 0);
                }
                bounces += (uint32_t)g_bounces;
                if (out_samples) {
                    float *o = out_samples + (((size_t)row * nx + i) * ns + s) * 3;
                    o[0] = (float)c.x; o[1] = (float)c.y; o[2] = (float)c.z;
                }
                col[0] += (double)c.x; col[1] += (double)c.y; col[2] += (double)c.z;
            }
            size_t o = ((size_t)row * nx + i) * 3;
            if (out_sig) out_sig[(size_t)row * nx + i] = g_sig;
            if (x->out_bounces) x->out_bounces[(size_t)row * nx + i] = bounces;
            for (int ch = 0; ch < 3; ch++) {
                double m = col[ch] / (double)ns;
                if (out_mean) out_mean[o + ch] = m;
                if (out_linear) out_linear[o + ch] = (float)m;
                if (out_rgb) out_rgb[o + ch] = as_i32(255.99 * na_clamp(sqrt(m), 0.0, 1.0));
            }
        }
    }
    free(lights);
    return 0;
}

/* Renders output rows [row_begin,row_end) (row 0 = top = reference j = ny-1) and, inside
 * them, samples [0,ns).  out_linear: ny*nx*3 float (mean radiance before gamma);
 * out_rgb: ny*nx*3 int32 (the ir/ig/ib the reference prints); out_mean: ny*nx*3 double.
 * out_sig: ny*nx uint64 path signatures.  Any output pointer may be NULL. */
ORC_API int orc_render(void *cam_, void *world_, int nx, int ny, int ns, uint64_t seed, int flags, int max_depth,
                       double t_min, int row_begin, int row_end, float *out_linear, int32_t *out_rgb,
                       double *out_mean, uint64_t *out_sig) {
    return render_rows(cam_, world_, NULL, nx, ny, ns, seed, flags, max_depth, t_min, row_begin, row_end, out_linear,
                       out_rgb, out_mean, out_sig);
}
/* orc_render plus every sample's fp32 radiance: out_samples [ny, nx, ns, 3] (rows outside [row_begin, row_end) are
 * not written) */
ORC_API int orc_render_samples(void *cam_, void *world_, int nx, int ny, int ns, uint64_t seed, int flags, int max_depth,
                               double t_min, int row_begin, int row_end, float *out_linear, int32_t *out_rgb,
                               double *out_mean, uint64_t *out_sig, float *out_samples) {
    RowsExt x = {0, NULL, 0, NULL, 0, 1.0, out_samples, NULL, NULL};
    return render_rows(cam_, world_, &x, nx, ny, ns, seed, flags, max_depth, t_min, row_begin, row_end, out_linear,
                       out_rgb, out_mean, out_sig);
}
/* rtmi_render_nee's estimator (include/rtmi_nee.h) with the light table `lights` (n_lights entries, the device's
 * order; area, p_sel and cdf already the floats rtmi_scene_attach_lights makes of them).  Paths, signatures and
 * outputs as orc_render in the throughput form; the light samples come from stream 3. */
ORC_API int orc_render_nee(void *cam_, void *world_, const OrcLight *lights, int n_lights, int nx, int ny, int ns,
                           uint64_t seed, int flags, int max_depth, double t_min, int row_begin, int row_end,
                           float *out_linear, int32_t *out_rgb, double *out_mean, uint64_t *out_sig, float *out_samples) {
    if (n_lights < 0 || (n_lights > 0 && !lights)) return 1;
    RowsExt x = {1, lights, n_lights, NULL, 0, 1.0, out_samples, NULL, NULL};
    return render_rows(cam_, world_, &x, nx, ny, ns, seed, flags | ORC_THROUGHPUT_FORM, max_depth, t_min, row_begin,
                       row_end, out_linear, out_rgb, out_mean, out_sig);
}
/* orc_render_nee under RTMI_FLAG_LIGHT_TREE (include/rtmi_light_tree.h): the tree over that table first (nodes: n_nodes
 * = 2 * n_lights entries, paths: n_lights entries, as rtmi_light_tree_from_desc writes them), then orc_render_nee's
 * arguments.  An empty table with n_nodes = 0, and a table of one light, render as orc_render_nee does. */
ORC_API int orc_render_nee_tree(void *cam_, void *world_, const OrcLight *lights, int n_lights, const OrcLightNode *nodes,
                                int n_nodes, const OrcLightPath *paths, int nx, int ny, int ns, uint64_t seed, int flags,
                                int max_depth, double t_min, int row_begin, int row_end, float *out_linear, int32_t *out_rgb,
                                double *out_mean, uint64_t *out_sig, float *out_samples) {
    if (n_lights < 0 || (n_lights > 0 && !lights) || n_nodes != 2 * n_lights) return 1;
    LightTree t = {nodes, (uint32_t)n_nodes, paths};
    if (n_lights > 0 && (!paths || tree_invalid(&t))) return 1;
    RowsExt x = {1, lights, n_lights, NULL, 0, 1.0, out_samples, NULL, n_lights > 0 ? &t : NULL};
    return render_rows(cam_, world_, &x, nx, ny, ns, seed, flags | ORC_THROUGHPUT_FORM, max_depth, t_min, row_begin,
                       row_end, out_linear, out_rgb, out_mean, out_sig);
}
/* The walks alone, as rtmi_light_tree_pick and rtmi_light_tree_pmf: points n * 3 floats, us n floats, lights n indices;
 * out_light and out_p n entries (pick: either may be NULL).  1 for a NULL argument that is read, a tree that
 * tree_invalid refuses and a light index outside the table. */
ORC_API int orc_light_tree_pick(const OrcLightNode *nodes, uint32_t n_nodes, const float *points, const float *us, uint32_t n,
                                uint32_t *out_light, float *out_p) {
    LightTree t = {nodes, n_nodes, NULL};
    if (tree_invalid(&t) || (n > 0 && (!points || !us))) return 1;
    for (uint32_t k = 0; k < n; k++) {
        REAL p;
        const uint32_t li = tree_pick(&t, v3((REAL)points[3 * k], (REAL)points[3 * k + 1], (REAL)points[3 * k + 2]), (REAL)us[k], &p);
        if (out_light) out_light[k] = li;
        if (out_p) out_p[k] = (float)p;
    }
    return 0;
}
ORC_API int orc_light_tree_pmf(const OrcLightNode *nodes, uint32_t n_nodes, const OrcLightPath *paths, const float *points,
                               const uint32_t *lights, uint32_t n, float *out_p) {
    LightTree t = {nodes, n_nodes, paths};
    if (!paths || tree_invalid(&t) || (n > 0 && (!points || !lights || !out_p))) return 1;
    for (uint32_t k = 0; k < n; k++) {
        if (lights[k] >= n_nodes / 2u) return 1;
        out_p[k] = (float)tree_pmf(&t, v3((REAL)points[3 * k], (REAL)points[3 * k + 1], (REAL)points[3 * k + 2]), lights[k]);
    }
    return 0;
}

/* The exported map: the texels and the tables of rtmi_env_tables (the tests pass tests/env_ref.py's), 56 B. */
typedef struct {
    int32_t w, h;
    const float *rgb, *row_cdf, *row_p, *col_cdf, *col_p;
    double total; /* the f64 total weight: the map can be sampled iff total > 0 */
} OrcEnv;
/* p_env by include/rtmi_env.h's rule: env_select_p with a light table that is not empty, 1 with an empty one, 0 when
 * the map cannot be sampled */
static int env_map_of(const OrcEnv *e, int n_lights, double env_select_p, EnvMap *E) {
    if (!e || e->w < 1 || e->h < 1 || !e->rgb || !e->row_cdf || !e->row_p || !e->col_cdf || !e->col_p) return 1;
    E->w = e->w; E->h = e->h;
    E->rgb = e->rgb; E->row_cdf = e->row_cdf; E->row_p = e->row_p; E->col_cdf = e->col_cdf; E->col_p = e->col_p;
    E->p_env = !(e->total > 0.0) ? (REAL)0 : (n_lights > 0 ? (REAL)(float)env_select_p : (REAL)1);
    return 0;
}
/* rtmi_render_env's estimator (include/rtmi_env.h): orc_render_nee's arguments plus the map, nee (0 or 1) and
 * env_select_p.  With nee = 0 the light table is not read. */
ORC_API int orc_render_env(void *cam_, void *world_, const OrcLight *lights, int n_lights, const OrcEnv *env, int nee,
                           double env_select_p, int nx, int ny, int ns, uint64_t seed, int flags, int max_depth,
                           double t_min, int row_begin, int row_end, float *out_linear, int32_t *out_rgb,
                           double *out_mean, uint64_t *out_sig, float *out_samples) {
    EnvMap E;
    if (n_lights < 0 || (n_lights > 0 && !lights) || (nee != 0 && nee != 1)) return 1;
    if (env_map_of(env, n_lights, env_select_p, &E)) return 1;
    RowsExt x = {nee, lights, n_lights, &E, 0, 1.0, out_samples, NULL, NULL};
    return render_rows(cam_, world_, &x, nx, ny, ns, seed, flags | ORC_THROUGHPUT_FORM, max_depth, t_min, row_begin,
                       row_end, out_linear, out_rgb, out_mean, out_sig);
}
/* rtmi_render_roulette's estimator (include/rtmi_roulette.h): estimator 0 plain, 1 NEE, 2 the map with nee = 0, 3 the
 * map with nee = 1 and env_select_p (RTMI_ROULETTE_*); min_depth >= 1 and q_min in (0, 1].  out_bounces [ny, nx]: the
 * sum over the pixel's samples of the depth at which the path was written. */
ORC_API int orc_render_roulette(void *cam_, void *world_, const OrcLight *lights, int n_lights, const OrcEnv *env,
                                int estimator, int min_depth, double q_min, double env_select_p, int nx, int ny, int ns,
                                uint64_t seed, int flags, int max_depth, double t_min, int row_begin, int row_end,
                                float *out_linear, int32_t *out_rgb, double *out_mean, uint64_t *out_sig,
                                float *out_samples, uint32_t *out_bounces) {
    EnvMap E;
    if (estimator < 0 || estimator > 3 || min_depth < 1 || !(q_min > 0.0 && q_min <= 1.0)) return 1;
    const int nee = estimator == 1 || estimator == 3, with_env = estimator >= 2;
    if (n_lights < 0 || (n_lights > 0 && !lights)) return 1;
    if (!nee) n_lights = 0;
    if (with_env && env_map_of(env, n_lights, env_select_p, &E)) return 1;
    RowsExt x = {nee, nee ? lights : NULL, n_lights, with_env ? &E : NULL, min_depth, q_min, out_samples, out_bounces, NULL};
    return render_rows(cam_, world_, &x, nx, ny, ns, seed, flags | ORC_THROUGHPUT_FORM, max_depth, t_min, row_begin,
                       row_end, out_linear, out_rgb, out_mean, out_sig);
}
/* The map functions alone: env(d) and the BSDF-side pdf of n directions (out: n x (r, g, b, pdf)) ... */
ORC_API int orc_env_lookup(const OrcEnv *env, double p_env, int flags, const float *dirs, float *out, long n) {
    EnvMap E;
    if (env_map_of(env, 0, 1.0, &E)) return 1;
    E.p_env = (REAL)(float)p_env;
    g_flags = flags;
    for (long k = 0; k < n; k++) {
        REAL u, v, theta;
        float *o = out + 4 * k;
        o[0] = o[1] = o[2] = o[3] = 0.0f;
        if (!env_uv(v3((REAL)dirs[3 * k], (REAL)dirs[3 * k + 1], (REAL)dirs[3 * k + 2]), &u, &v, &theta)) continue;
        const V3 c = env_radiance(&E, u, v);
        o[0] = (float)c.x; o[1] = (float)c.y; o[2] = (float)c.z;
        o[3] = (float)env_pdf(&E, u, v, theta);
    }
    return 0;
}
/* ... and the light sample of n pairs of uniforms (out: n x (dx, dy, dz, pdf), all 0 where there is no sample) */
ORC_API int orc_env_sample(const OrcEnv *env, double p_env, int flags, const float *u12, float *out, long n) {
    EnvMap E;
    if (env_map_of(env, 0, 1.0, &E)) return 1;
    E.p_env = (REAL)(float)p_env;
    g_flags = flags;
    for (long k = 0; k < n; k++) {
        V3 d;
        REAL pdf;
        float *o = out + 4 * k;
        o[0] = o[1] = o[2] = o[3] = 0.0f;
        if (!env_sample(&E, (REAL)u12[2 * k], (REAL)u12[2 * k + 1], &d, &pdf)) continue;
        o[0] = (float)d.x; o[1] = (float)d.y; o[2] = (float)d.z; o[3] = (float)pdf;
    }
    return 0;
}

/* P3 text exactly as tests/test.rs:59,79 : "P3\n{nx} {ny}\n255\n" then "{ir} {ig} {ib}\n" per pixel.
 * Returns bytes written (excluding the NUL), or the size needed if cap is too small. */
ORC_API size_t orc_ppm_text(int nx, int ny, const int32_t *rgb, char *buf, size_t cap) {
    size_t need = 32 + (size_t)nx * ny * 36;
    if (!buf || cap < need) return need;
    size_t n = (size_t)sprintf(buf, "P3\n%d %d\n255\n", nx, ny);
    for (size_t p = 0; p < (size_t)nx * ny; p++)
        n += (size_t)sprintf(buf + n, "%d %d %d\n", rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]);
    return n;
}

/* ---- probes for known-answer tests ------------------------------------------------ */
ORC_API int orc_hit(void *h, const double *o, const double *d, double time, double t_min, double t_max, int flags,
                    uint64_t seed, double *out9, int *out_mat_kind) {
    g_flags = flags;
    stream_init(&g_rng, seed, 0, 0, 0);
    Ray r = ray_new(v3((REAL)o[0], (REAL)o[1], (REAL)o[2]), v3((REAL)d[0], (REAL)d[1], (REAL)d[2]), (REAL)time);
    HitRecord rec;
    REAL tmn = t_min <= -1.7e308 ? -R_MAX : (REAL)t_min;
    REAL tmx = t_max >= 1.7e308 ? R_MAX : (REAL)t_max;
    if (!hit((Hittable *)h, &r, tmn, tmx, &rec)) return 0;
    out9[0] = rec.t; out9[1] = rec.u; out9[2] = rec.v;
    out9[3] = rec.p.x; out9[4] = rec.p.y; out9[5] = rec.p.z;
    out9[6] = rec.normal.x; out9[7] = rec.normal.y; out9[8] = rec.normal.z;
    if (out_mat_kind) *out_mat_kind = rec.mat ? rec.mat->kind : -1;
    return 1;
}
ORC_API int orc_bounding_box(void *h, double t0, double t1, double *out6) {
    AABBd b;
    if (!bounding_box((Hittable *)h, t0, t1, &b)) return 0;
    out6[0] = b.min.x; out6[1] = b.min.y; out6[2] = b.min.z; out6[3] = b.max.x; out6[4] = b.max.y; out6[5] = b.max.z;
    return 1;
}
ORC_API void orc_tex_value(void *tex, double u, double v, const double *p, int flags, double *out3) {
    g_flags = flags;
    V3 c = tex_value((Texture *)tex, (REAL)u, (REAL)v, v3((REAL)p[0], (REAL)p[1], (REAL)p[2]));
    out3[0] = c.x; out3[1] = c.y; out3[2] = c.z;
}
/* scatter probe: returns 0 if absorbed; out = scattered o(3) d(3) time, attenuation(3) */
ORC_API int orc_scatter(void *mat, const double *ro, const double *rd, double time, const double *rec9, int flags,
                        uint64_t seed, double *out10) {
    g_flags = flags;
    stream_init(&g_rng, seed, 0, 0, 0);
    Ray r = ray_new(v3((REAL)ro[0], (REAL)ro[1], (REAL)ro[2]), v3((REAL)rd[0], (REAL)rd[1], (REAL)rd[2]), (REAL)time);
    HitRecord rec;
    rec.t = (REAL)rec9[0]; rec.u = (REAL)rec9[1]; rec.v = (REAL)rec9[2];
    rec.p = v3((REAL)rec9[3], (REAL)rec9[4], (REAL)rec9[5]);
    rec.normal = v3((REAL)rec9[6], (REAL)rec9[7], (REAL)rec9[8]);
    rec.mat = (Material *)mat;
    Ray sc; V3 att;
    if (!mat_scatter(rec.mat, &r, &rec, &sc, &att)) return 0;
    out10[0] = sc.o.x; out10[1] = sc.o.y; out10[2] = sc.o.z; out10[3] = sc.d.x; out10[4] = sc.d.y; out10[5] = sc.d.z;
    out10[6] = sc.time; out10[7] = att.x; out10[8] = att.y; out10[9] = att.z;
    return 1;
}
ORC_API void orc_emitted(void *mat, double u, double v, const double *p, double *out3) {
    V3 c = mat_emitted((Material *)mat, (REAL)u, (REAL)v, v3((REAL)p[0], (REAL)p[1], (REAL)p[2]));
    out3[0] = c.x; out3[1] = c.y; out3[2] = c.z;
}
ORC_API void orc_get_ray(void *cam, double s, double t, uint64_t seed, double *out7) {
    stream_init(&g_rng, seed, 0, 0, 0);
    Ray r = camera_get_ray((Camera *)cam, (REAL)s, (REAL)t);
    out7[0] = r.o.x; out7[1] = r.o.y; out7[2] = r.o.z; out7[3] = r.d.x; out7[4] = r.d.y; out7[5] = r.d.z; out7[6] = r.time;
}
/* ---- the scripted word source and the pieces of the path that draw from it (tests/test_path_contract.py); each only
 *      calls the functions above ---- */
/* words != NULL: the render path's stream reads this list from its next stream_init on (the caller keeps it alive);
 * NULL: Philox again */
ORC_API void orc_script(const uint32_t *words, uint32_t n) { g_script = words; g_script_len = words ? n : 0; }
/* words the render path's stream has delivered since its last stream_init */
ORC_API uint32_t orc_script_consumed(void) { return g_rng.ctr[0] * 4u - (uint32_t)(4 - g_rng.pos); }
/* util.rs:4-24: kind 0 = random_in_unit_sphere, 1 = random_in_unit_disk */
ORC_API void orc_sample_unit(int kind, double *out3) {
    stream_init(&g_rng, 0, 0, 0, 0);
    V3 p = kind == 0 ? random_in_unit_sphere() : random_in_unit_disk();
    out3[0] = p.x; out3[1] = p.y; out3[2] = p.z;
}
/* the same samplers with `<= limit` for `< 1`: the negative controls of the acceptance band, never part of a render */
ORC_API void orc_sample_unit_wrong(int kind, double limit, double *out3) {
    stream_init(&g_rng, 0, 0, 0, 0);
    for (;;) {
        REAL x = rng_uniform(), y = rng_uniform(), z = kind == 0 ? rng_uniform() : (REAL)0.5;
        V3 p = v3((REAL)2.0 * x - (REAL)1.0, (REAL)2.0 * y - (REAL)1.0, (REAL)2.0 * z - (REAL)1.0);
        if (v_dot(p, p) <= (REAL)limit) { out3[0] = p.x; out3[1] = p.y; out3[2] = p.z; return; }
    }
}
/* medium.rs:33-53 after the two boundary queries; returns 1 and the t of the scatter, or 0 */
ORC_API int orc_medium_sample(double t1, double t2, double t_min, double t_max, double dn, double density, int flags, double *t_out) {
    g_flags = flags;
    stream_init(&g_rng, 0, 0, 0, 0);
    REAL tmn = t_min <= -1.7e308 ? -R_MAX : (REAL)t_min;
    REAL tmx = t_max >= 1.7e308 ? R_MAX : (REAL)t_max;
    REAL t = 0;
    int taken = medium_sample((REAL)t1, (REAL)t2, tmn, tmx, (REAL)dn, (REAL)density, &t);
    *t_out = taken ? t : 0.0;
    return taken;
}
/* sample 0 of pixel (i, j) of an nx x ny image as render_rows takes it */
ORC_API void orc_pixel_ray(void *cam, int i, int j, int nx, int ny, double *out7) {
    stream_init(&g_rng, 0, 0, (uint32_t)j * (uint32_t)nx + (uint32_t)i, 0);
    Ray r = pixel_ray((Camera *)cam, i, j, nx, ny);
    out7[0] = r.o.x; out7[1] = r.o.y; out7[2] = r.o.z; out7[3] = r.d.x; out7[4] = r.d.y; out7[5] = r.d.z; out7[6] = r.time;
}
/* One turn of color_throughput's loop for a path with T = 1, L = 0 at `depth`: world.hit under the ray's own interval, the
 * emission, and the scatter unless depth >= max_depth.  Draws come from the render path's stream (a script, when set).
 * out22 = {hit, t, hit point (3), normal (3), material kind, scattered, scattered origin (3), direction (3), T (3),
 * L (3)}; without a hit only out[0] = 0 is written. */
ORC_API void orc_bounce(void *world, const double *o, const double *d, double time, double t_min, double t_max, int depth,
                        int max_depth, int flags, double *out22) {
    g_flags = flags;
    stream_init(&g_rng, 0, 0, 0, 0);
    Ray r = ray_new(v3((REAL)o[0], (REAL)o[1], (REAL)o[2]), v3((REAL)d[0], (REAL)d[1], (REAL)d[2]), (REAL)time);
    REAL tmn = t_min <= -1.7e308 ? -R_MAX : (REAL)t_min;
    REAL tmx = t_max >= 1.7e308 ? R_MAX : (REAL)t_max;
    HitRecord rec;
    for (int k = 0; k < 22; k++) out22[k] = 0.0;
    if (!hit((Hittable *)world, &r, tmn, tmx, &rec)) return;
    out22[0] = 1.0; out22[1] = rec.t;
    out22[2] = rec.p.x; out22[3] = rec.p.y; out22[4] = rec.p.z;
    out22[5] = rec.normal.x; out22[6] = rec.normal.y; out22[7] = rec.normal.z;
    out22[8] = rec.mat->kind;
    V3 T = v3(1, 1, 1), L = v_mul(T, mat_emitted(rec.mat, rec.u, rec.v, rec.p));
    Ray sc = r; V3 att;
    if (depth < max_depth && mat_scatter(rec.mat, &r, &rec, &sc, &att)) {
        out22[9] = 1.0;
        T = v_mul(T, att);
    }
    out22[10] = sc.o.x; out22[11] = sc.o.y; out22[12] = sc.o.z; out22[13] = sc.d.x; out22[14] = sc.d.y; out22[15] = sc.d.z;
    out22[16] = T.x; out22[17] = T.y; out22[18] = T.z; out22[19] = L.x; out22[20] = L.y; out22[21] = L.z;
}
/* a camera from its derived state (rtmi_camera's 21 values) instead of Camera::new's arguments: the working-precision
 * fields are the given values rounded once */
ORC_API void *orc_camera_from_state(const double *s21) {
    Camera *c = (Camera *)arena_alloc(sizeof(Camera));
    D3 *v[6] = {&c->origind, &c->llcd, &c->hord, &c->verd, &c->ud, &c->vd};
    for (int i = 0; i < 6; i++) { v[i]->x = s21[3 * i]; v[i]->y = s21[3 * i + 1]; v[i]->z = s21[3 * i + 2]; }
    c->time0d = s21[18]; c->time1d = s21[19]; c->lens_radiusd = s21[20];
    c->origin = d3_to_v3(c->origind); c->llc = d3_to_v3(c->llcd);
    c->horizontal = d3_to_v3(c->hord); c->vertical = d3_to_v3(c->verd);
    c->u = d3_to_v3(c->ud); c->v = d3_to_v3(c->vd);
    c->time0 = (REAL)c->time0d; c->time1 = (REAL)c->time1d; c->lens_radius = (REAL)c->lens_radiusd;
    return c;
}
ORC_API void orc_reset_counters(void) { memset(g_cnt, 0, sizeof(g_cnt)); }
ORC_API int orc_get_counters(uint64_t *out, int n) {
    for (int i = 0; i < n && i < C_NCOUNTERS; i++) out[i] = g_cnt[i];
    return C_NCOUNTERS;
}
/* host evaluation of the fp32 transcendental contract, for tests */
ORC_API float orc_rtmi_sinf(float x) { return rtmi_sinf(x); }
ORC_API float orc_rtmi_cosf(float x) { return rtmi_cosf(x); }
ORC_API float orc_rtmi_logf(float x) { return rtmi_logf(x); }
ORC_API float orc_rtmi_atan2f(float y, float x) { return rtmi_atan2f(y, x); }
ORC_API float orc_rtmi_asinf(float x) { return rtmi_asinf(x); }
/* pieces of the hot path that have no hittable of their own, for the per-operation tests (tests/test_geom_contract.py);
 * each only calls the functions above */
ORC_API int orc_probe_aabb(const double *o, const double *d, const double *box6, double t_min, double t_max, int flags) {
    g_flags = flags;
    Ray r = ray_new(v3((REAL)o[0], (REAL)o[1], (REAL)o[2]), v3((REAL)d[0], (REAL)d[1], (REAL)d[2]), (REAL)0);
    AABB b = {v3((REAL)box6[0], (REAL)box6[1], (REAL)box6[2]), v3((REAL)box6[3], (REAL)box6[4], (REAL)box6[5])};
    REAL tmn = t_min <= -1.7e308 ? -R_MAX : (REAL)t_min;
    REAL tmx = t_max >= 1.7e308 ? R_MAX : (REAL)t_max;
    return aabb_hit(&b, &r, tmn, tmx);
}
/* ConstantMedium's two boundary queries (medium.rs:29-30) as H_MEDIUM makes them; out4 = {h1, t1, h2, t2} */
ORC_API void orc_probe_medium(void *boundary, const double *o, const double *d, double time, int flags, double *out4) {
    g_flags = flags;
    Ray r = ray_new(v3((REAL)o[0], (REAL)o[1], (REAL)o[2]), v3((REAL)d[0], (REAL)d[1], (REAL)d[2]), (REAL)time);
    HitRecord h1, h2;
    out4[0] = out4[1] = out4[2] = out4[3] = 0.0;
    if (hit((Hittable *)boundary, &r, -R_MAX, R_MAX, &h1)) {
        out4[0] = 1.0; out4[1] = h1.t;
        if (hit((Hittable *)boundary, &r, h1.t + (REAL)0.0001, R_MAX, &h2)) { out4[2] = 1.0; out4[3] = h2.t; }
    }
}
/* material.rs:9-28: out8 = {reflect(v, n) (3), refract ok, its vector (3), schlick(cosine, ref_idx)} */
ORC_API void orc_probe_shade(const double *v, const double *n, double ni_over_nt, double cosine, double ref_idx, double *out8) {
    V3 vv = v3((REAL)v[0], (REAL)v[1], (REAL)v[2]), nn = v3((REAL)n[0], (REAL)n[1], (REAL)n[2]);
    V3 rf = reflect(vv, nn), rr = v3(0, 0, 0);
    int ok = refract(vv, nn, (REAL)ni_over_nt, &rr);
    out8[0] = rf.x; out8[1] = rf.y; out8[2] = rf.z;
    out8[3] = ok; out8[4] = rr.x; out8[5] = rr.y; out8[6] = rr.z;
    out8[7] = schlick((REAL)cosine, (REAL)ref_idx);
}
/* sphere.rs:9-15 (flags: ORC_UV_BOOK) */
ORC_API void orc_probe_uv(const double *n, int flags, double *out2) {
    g_flags = flags;
    REAL u, v;
    get_sphere_uv(v3((REAL)n[0], (REAL)n[1], (REAL)n[2]), &u, &v);
    out2[0] = u; out2[1] = v;
}
