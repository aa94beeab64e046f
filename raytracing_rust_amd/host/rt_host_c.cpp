// rt_host_c.cpp — C bindings of the C++ host mirror (rt_host.hpp) for ctypes/FFI users.
// Handles are opaque pointers owned by this library until rth_free_all().  No exception
// crosses the boundary: constructors return NULL and functions return a non-zero code,
// with the message in rth_last_error().  Where the reference panics the code is RTH_PANIC.
#include <cstring>
#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "rt_host.hpp"
#include "rtmi_env.h"
#include "rtmi_light_tree.h"
#include "rtmi_adaptive_nee.h"
#include "rtmi_roulette.h"
#include "rtmi_session.h"
#include "rtmi_query.h"
#include "rtmi_radiance.h"
#include "rtmi_sparse.h"
#include "rtmi_pixelwise.h"
#include "rtmi_window.h"
#include "rtmi_gather.h"
#include "rtmi_frame.h"
#include "rtmi_upscale.h"
#include "rtmi_update.h"
#include "rtmi_relight.h"

using namespace rt;

#define RTH_API extern "C" __attribute__((visibility("default")))
enum { RTH_OK = 0, RTH_ERROR = 1, RTH_PANIC = 2, RTH_UNSUPPORTED = 3 };

namespace {
thread_local std::string g_err;
thread_local int g_code = 0;

struct Obj {
    enum Kind { TEX, MAT, HIT, LIST, CAM, LOWERED } kind;
    TexturePtr tex;
    MaterialPtr mat;
    HittablePtr hit;
    std::shared_ptr<HittableList> list;
    std::shared_ptr<Camera> cam;
    std::shared_ptr<LoweredScene> lowered;
    rtmi_scene *dev = nullptr;
    rtmi_multi *multi = nullptr; // the lowered scene resident on a device list (rth_upload_multi)
    bool edited = false; // a scene update has edited the fp32 description (or the resident handle alone): the double planes
                         // of the f64 render mode still hold the lowering's positions and are no longer attached
};
std::mutex g_mu;
std::vector<Obj *> g_objs;
std::vector<rtmi_session *> g_sessions; // the live render sessions (rth_session_*): freed before their scenes
std::vector<rtmi_frame *> g_frames;     // the live frame handles (rth_frame_*): freed before their scenes
std::vector<rtmi_upscaler *> g_upscalers; // the live upscalers (rth_upscaler_*): freed before their scenes

Obj *reg(Obj *o) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_objs.push_back(o);
    return o;
}
int set_err(const std::exception &e) {
    g_err = e.what();
    g_code = RTH_ERROR;
    if (dynamic_cast<const Panic *>(&e)) g_code = RTH_PANIC;
    if (dynamic_cast<const Unsupported *>(&e)) g_code = RTH_UNSUPPORTED;
    return g_code;
}
template <typename F>
void *guard_new(F f) {
    try {
        return f();
    } catch (const std::exception &e) {
        set_err(e);
        return nullptr;
    }
}
template <typename F>
int guard(F f) {
    try {
        return f();
    } catch (const std::exception &e) {
        return set_err(e);
    }
}
Obj *O(void *h) { return static_cast<Obj *>(h); }
void *new_tex(TexturePtr t) { Obj *o = new Obj{Obj::TEX}; o->tex = std::move(t); return reg(o); }
void *new_mat(MaterialPtr m) { Obj *o = new Obj{Obj::MAT}; o->mat = std::move(m); return reg(o); }
void *new_hit(HittablePtr h) { Obj *o = new Obj{Obj::HIT}; o->hit = std::move(h); return reg(o); }
HittablePtr H(void *h) {
    Obj *o = O(h);
    if (!o || (o->kind != Obj::HIT && o->kind != Obj::LIST)) throw std::runtime_error("handle is not a Hittable");
    return o->kind == Obj::LIST ? std::static_pointer_cast<const Hittable>(o->list) : o->hit;
}
TexturePtr T(void *h) {
    if (!h || O(h)->kind != Obj::TEX) throw std::runtime_error("handle is not a Texture");
    return O(h)->tex;
}
MaterialPtr M(void *h) {
    if (!h || O(h)->kind != Obj::MAT) throw std::runtime_error("handle is not a Material");
    return O(h)->mat;
}
} // namespace

RTH_API const char *rth_last_error(void) { return g_err.c_str(); }
RTH_API int rth_last_error_code(void) { return g_code; }
RTH_API void rth_free_all(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    for (rtmi_session *ss : g_sessions) rtmi_session_destroy(ss);
    g_sessions.clear();
    for (rtmi_frame *f : g_frames) rtmi_frame_destroy(f);
    g_frames.clear();
    for (rtmi_upscaler *u : g_upscalers) rtmi_upscaler_destroy(u);
    g_upscalers.clear();
    for (Obj *o : g_objs) {
        if (o->dev) rtmi_scene_destroy(o->dev);
        if (o->multi) rtmi_multi_destroy(o->multi);
        delete o;
    }
    g_objs.clear();
}
RTH_API void rth_seed_scene_rng(uint64_t seed) { scene_rng().seed(seed, 0, 0, 1); }
RTH_API double rth_scene_uniform(void) { return scene_rng().gen(); }
RTH_API void rth_philox(const uint32_t *ctr, const uint32_t *key, uint32_t *out) { philox4x32_10(ctr, key, out); }

// ---- textures -------------------------------------------------------------------------
RTH_API void *rth_tex_solid(double r, double g, double b) {
    return guard_new([&] { return new_tex(std::make_shared<SolidTexture>(r, g, b)); });
}
RTH_API void *rth_tex_checker(void *odd, void *even) {
    return guard_new([&] { return new_tex(std::make_shared<CheckerTexture>(T(odd), T(even))); });
}
RTH_API void *rth_tex_noise(double scale) {
    return guard_new([&] { return new_tex(std::make_shared<NoiseTexture>(scale)); });
}
RTH_API void *rth_tex_image(const uint8_t *data, uint32_t nx, uint32_t ny) {
    return guard_new([&] {
        std::vector<uint8_t> v(data, data + (size_t)nx * ny * 3);
        return new_tex(std::make_shared<ImageTexture>(std::move(v), nx, ny));
    });
}
RTH_API int rth_perlin_tables(void *tex, double *ranvec768, int *perm768) {
    return guard([&] {
        auto n = std::dynamic_pointer_cast<const NoiseTexture>(T(tex));
        if (!n) throw std::runtime_error("not a NoiseTexture");
        for (size_t i = 0; i < 256; i++) {
            ranvec768[3 * i] = n->noise_.ran_vec_[i].x; ranvec768[3 * i + 1] = n->noise_.ran_vec_[i].y;
            ranvec768[3 * i + 2] = n->noise_.ran_vec_[i].z;
            perm768[i] = (int)n->noise_.perm_x_[i]; perm768[256 + i] = (int)n->noise_.perm_y_[i];
            perm768[512 + i] = (int)n->noise_.perm_z_[i];
        }
        return RTH_OK;
    });
}
// ---- materials ------------------------------------------------------------------------
RTH_API void *rth_mat_lambertian(void *tex) { return guard_new([&] { return new_mat(std::make_shared<Lambertian>(T(tex))); }); }
RTH_API void *rth_mat_metal(void *tex, double fuzz) { return guard_new([&] { return new_mat(std::make_shared<Metal>(T(tex), fuzz)); }); }
RTH_API void *rth_mat_dielectric(double ri) { return guard_new([&] { return new_mat(std::make_shared<Dielectric>(ri)); }); }
RTH_API void *rth_mat_diffuse_light(void *tex) { return guard_new([&] { return new_mat(std::make_shared<DiffuseLight>(T(tex))); }); }
RTH_API void *rth_mat_isotropic(void *tex) { return guard_new([&] { return new_mat(std::make_shared<Isotropic>(T(tex))); }); }
// ---- hittables ------------------------------------------------------------------------
RTH_API void *rth_sphere(double cx, double cy, double cz, double r, void *mat) {
    return guard_new([&] { return new_hit(std::make_shared<Sphere>(Vec3(cx, cy, cz), r, M(mat))); });
}
RTH_API void *rth_moving_sphere(double ax, double ay, double az, double bx, double by, double bz, double t0, double t1,
                                double r, void *mat) {
    return guard_new([&] {
        return new_hit(std::make_shared<MovingSphere>(Vec3(ax, ay, az), Vec3(bx, by, bz), t0, t1, r, M(mat)));
    });
}
RTH_API void *rth_rect(int plane, double x0, double y0, double x1, double y1, double k, void *mat) {
    return guard_new([&] {
        if (plane < 0 || plane > 2) throw std::runtime_error("bad Plane");
        return new_hit(std::make_shared<Rect>((Plane)plane, x0, y0, x1, y1, k, M(mat)));
    });
}
RTH_API void *rth_cube(double ax, double ay, double az, double bx, double by, double bz, void *mat) {
    return guard_new([&] { return new_hit(std::make_shared<Cube>(Vec3(ax, ay, az), Vec3(bx, by, bz), M(mat))); });
}
RTH_API void *rth_flip_normals(void *h) { return guard_new([&] { return new_hit(std::make_shared<FlipNormals>(H(h))); }); }
RTH_API void *rth_translate(void *h, double ox, double oy, double oz) {
    return guard_new([&] { return new_hit(std::make_shared<Traslate>(H(h), Vec3(ox, oy, oz))); });
}
RTH_API void *rth_rotate(int axis, void *h, double angle) {
    return guard_new([&] {
        if (axis < 0 || axis > 2) throw std::runtime_error("bad Axis");
        return new_hit(std::make_shared<Rotate>((Axis)axis, H(h), angle));
    });
}
RTH_API void *rth_constant_medium(void *boundary, double density, void *tex) {
    return guard_new([&] { return new_hit(std::make_shared<ConstantMedium>(H(boundary), density, T(tex))); });
}
RTH_API void *rth_list_new(void) {
    return guard_new([&] {
        Obj *o = new Obj{Obj::LIST};
        o->list = std::make_shared<HittableList>();
        return (void *)reg(o);
    });
}
RTH_API int rth_list_push(void *list, void *h) {
    return guard([&] {
        if (!list || O(list)->kind != Obj::LIST) throw std::runtime_error("handle is not a HittableList");
        O(list)->list->push(H(h));
        return RTH_OK;
    });
}
RTH_API void *rth_bvh(void **items, int n, double t0, double t1) {
    return guard_new([&] {
        std::vector<HittablePtr> v;
        for (int i = 0; i < n; i++) v.push_back(H(items[i]));
        return new_hit(std::make_shared<BVHNode>(v, t0, t1));
    });
}
RTH_API void *rth_camera(double fx, double fy, double fz, double ax, double ay, double az, double ux, double uy,
                         double uz, double vfov, double aspect, double aperture, double focus_dist, double t0, double t1) {
    return guard_new([&] {
        Obj *o = new Obj{Obj::CAM};
        o->cam = std::make_shared<Camera>(Vec3(fx, fy, fz), Vec3(ax, ay, az), Vec3(ux, uy, uz), vfov, aspect, aperture,
                                          focus_dist, t0, t1);
        return (void *)reg(o);
    });
}
static Camera &CAM(void *h) {
    if (!h || O(h)->kind != Obj::CAM) throw std::runtime_error("handle is not a Camera");
    return *O(h)->cam;
}
RTH_API int rth_camera_lower(void *cam, rtmi_camera *out) { return guard([&] { *out = CAM(cam).lower(); return RTH_OK; }); }
RTH_API int rth_camera_state(void *cam, double *out21) {
    return guard([&] {
        Camera &c = CAM(cam);
        const Vec3 *v[6] = {&c.origin_, &c.lower_left_corner_, &c.horizontal_, &c.vertical_, &c.u_, &c.v_};
        for (int i = 0; i < 6; i++) { out21[3 * i] = v[i]->x; out21[3 * i + 1] = v[i]->y; out21[3 * i + 2] = v[i]->z; }
        out21[18] = c.time0_; out21[19] = c.time1_; out21[20] = c.lens_radius_;
        return RTH_OK;
    });
}

// ---- lowering + device ------------------------------------------------------------------
static Obj *LOW(void *h) {
    if (!h || O(h)->kind != Obj::LOWERED) throw std::runtime_error("handle is not a lowered scene");
    return O(h);
}
RTH_API void *rth_lower(void *world) {
    return guard_new([&] {
        auto ls = std::make_shared<LoweredScene>(lower_scene(*H(world)));
        Obj *o = new Obj{Obj::LOWERED};
        o->lowered = std::move(ls);
        return (void *)reg(o);
    });
}
RTH_API int rth_lowered_desc(void *lowered, rtmi_scene_desc *out) {
    return guard([&] { *out = LOW(lowered)->lowered->desc(); return RTH_OK; });
}
// The uploaded device handle of a lowered scene.  `name` and `no_multi`: the rtmi entry and the kind of entry a scene
// resident on a device list (rth_upload_multi) lacks, in the wrappers that refuse such a scene as Unsupported.
static rtmi_scene *DEV(void *lowered, const char *name = nullptr, const char *no_multi = nullptr) {
    Obj *o = LOW(lowered);
    if (!o->dev && o->multi && no_multi)
        throw Unsupported(std::string(name) + ": multi-GPU handles have no " + no_multi + " entry (RTMI_ERR_UNSUPPORTED)");
    if (!o->dev) throw std::runtime_error("scene not uploaded: call rth_upload first");
    return o->dev;
}
// A non-zero return of the rtmi entry `name` as the wrapper's exception.  The older wrappers (PLAIN) throw "name: message";
// the newer ones add the code, and the render modes among them map RTMI_ERR_UNSUPPORTED to Unsupported.
enum ErrStyle { PLAIN, CODED, CODED_UNSUPPORTED };
static int done(const char *name, int rc, ErrStyle style) {
    if (!rc) return RTH_OK;
    const std::string msg = std::string(name) + ": " + rtmi_last_error();
    if (style == PLAIN) throw std::runtime_error(msg);
    if (style == CODED_UNSUPPORTED && rc == RTMI_ERR_UNSUPPORTED) throw Unsupported(msg);
    throw std::runtime_error(msg + " (code " + std::to_string(rc) + ")");
}
RTH_API int rth_upload(void *lowered, int device) {
    return guard([&] {
        Obj *o = LOW(lowered);
        if (o->dev) { rtmi_scene_destroy(o->dev); o->dev = nullptr; }
        const rtmi_scene_desc d = o->lowered->desc();
        if (int rc = done("rtmi_scene_create", rtmi_scene_create(&d, device, &o->dev), CODED)) return rc;
        // the places of the FlipNormals in the wrapper chains, for the normals of the ray queries (include/rtmi_query.h)
        const LoweredScene &ls = *o->lowered;
        return done("rtmi_scene_attach_flips", rtmi_scene_attach_flips(o->dev, ls.prim_flip_gaps.data(), (uint32_t)ls.prim_flip_gaps.size(),
                                                                        ls.item_flip_gaps.data(), (uint32_t)ls.item_flip_gaps.size()), CODED);
    });
}
RTH_API int rth_render(void *lowered, void *cam, const rtmi_render_params *p, float *out_linear, uint8_t *out_rgb8,
                       uint64_t *out_path_sig, rtmi_stats *stats) {
    return guard([&] {
        rtmi_scene *dev = DEV(lowered);
        const rtmi_camera c = CAM(cam).lower();
        return done("rtmi_render", rtmi_render(dev, &c, p, out_linear, out_rgb8, out_path_sig, stats), PLAIN);
    });
}
// adaptive sampling (include/rtmi_adaptive.h): RTH_UNSUPPORTED for what rtmi_render_adaptive does not support
RTH_API int rth_render_adaptive(void *lowered, void *cam, const rtmi_render_params *p, const rtmi_adaptive *a, float *out_linear,
                                uint8_t *out_rgb8, float *out_stderr, uint32_t *out_spp, rtmi_stats *stats) {
    return guard([&] {
        rtmi_scene *dev = DEV(lowered);
        const rtmi_camera c = CAM(cam).lower();
        return done("rtmi_render_adaptive", rtmi_render_adaptive(dev, &c, p, a, out_linear, out_rgb8, out_stderr, out_spp, stats),
                    CODED_UNSUPPORTED);
    });
}
// first-hit features (include/rtmi_features.h): RTH_UNSUPPORTED for what rtmi_render_features does not support, a
// multi-GPU handle (rth_upload_multi) among it
RTH_API int rth_render_features(void *lowered, void *cam, const rtmi_render_params *p, float *out_albedo, float *out_normal,
                                float *out_depth, uint32_t *out_hits, uint64_t *out_path_sig, rtmi_stats *stats) {
    return guard([&] {
        const char *name = "rtmi_render_features";
        rtmi_scene *dev = DEV(lowered, name, "features");
        const rtmi_camera c = CAM(cam).lower();
        return done(name, rtmi_render_features(dev, &c, p, out_albedo, out_normal, out_depth, out_hits, out_path_sig, stats),
                    CODED_UNSUPPORTED);
    });
}
// ray queries (include/rtmi_query.h) on the uploaded handle: host pointers and blocking, or device pointers enqueued on
// `stream`; RTH_UNSUPPORTED for the flags the queries do not carry and for a multi-GPU handle
RTH_API int rth_trace(void *lowered, const rtmi_query_params *p, const rtmi_ray *rays, const float *time, rtmi_hit *hits_out,
                      double *kernel_ms) {
    return guard([&] {
        const char *name = "rtmi_trace";
        return done(name, rtmi_trace(DEV(lowered, name, "ray-query"), p, rays, time, hits_out, kernel_ms), CODED_UNSUPPORTED);
    });
}
RTH_API int rth_occluded(void *lowered, const rtmi_query_params *p, const rtmi_ray *rays, const float *time, uint8_t *occluded_out,
                         double *kernel_ms) {
    return guard([&] {
        const char *name = "rtmi_occluded";
        return done(name, rtmi_occluded(DEV(lowered, name, "ray-query"), p, rays, time, occluded_out, kernel_ms), CODED_UNSUPPORTED);
    });
}
RTH_API int rth_trace_device(void *lowered, const rtmi_query_params *p, const void *d_rays, const void *d_time, void *d_hits,
                             void *stream) {
    return guard([&] {
        const char *name = "rtmi_trace_device";
        return done(name, rtmi_trace_device(DEV(lowered, name, "ray-query"), p, d_rays, d_time, d_hits, stream), CODED_UNSUPPORTED);
    });
}
RTH_API int rth_occluded_device(void *lowered, const rtmi_query_params *p, const void *d_rays, const void *d_time, void *d_occluded,
                                void *stream) {
    return guard([&] {
        const char *name = "rtmi_occluded_device";
        return done(name, rtmi_occluded_device(DEV(lowered, name, "ray-query"), p, d_rays, d_time, d_occluded, stream),
                    CODED_UNSUPPORTED);
    });
}
// radiance queries (include/rtmi_radiance.h) on the uploaded handle, as the ray queries: host pointers and blocking, or
// device pointers enqueued on `stream`; RTH_UNSUPPORTED for unknown flags and for a multi-GPU handle
RTH_API int rth_radiance(void *lowered, const rtmi_radiance_params *p, const rtmi_ray *rays, const float *time, float *out_mean,
                         float *out_stderr, float *out_samples, double *kernel_ms) {
    return guard([&] {
        const char *name = "rtmi_radiance";
        return done(name, rtmi_radiance(DEV(lowered, name, "radiance-query"), p, rays, time, out_mean, out_stderr, out_samples, kernel_ms),
                    CODED_UNSUPPORTED);
    });
}
RTH_API int rth_radiance_device(void *lowered, const rtmi_radiance_params *p, const void *d_rays, const void *d_time, void *d_mean,
                                void *d_stderr, void *d_samples, void *stream) {
    return guard([&] {
        const char *name = "rtmi_radiance_device";
        return done(name, rtmi_radiance_device(DEV(lowered, name, "radiance-query"), p, d_rays, d_time, d_mean, d_stderr, d_samples, stream),
                    CODED_UNSUPPORTED);
    });
}
// sparse renders (include/rtmi_sparse.h) on the uploaded handle, as the radiance queries: chosen pixels of the image of `p`
// under `cam`; host pointers and blocking, or device pointers enqueued on `stream`
RTH_API int rth_sparse_render(void *lowered, void *cam, const rtmi_render_params *p, const rtmi_sparse_params *sp, const uint32_t *pixels,
                              float *out_mean, float *out_stderr, float *out_samples, double *kernel_ms) {
    return guard([&] {
        const char *name = "rtmi_sparse_render";
        rtmi_scene *dev = DEV(lowered, name, "sparse-render");
        const rtmi_camera c = CAM(cam).lower();
        return done(name, rtmi_sparse_render(dev, p, &c, sp, pixels, out_mean, out_stderr, out_samples, kernel_ms), CODED_UNSUPPORTED);
    });
}
RTH_API int rth_sparse_render_device(void *lowered, void *cam, const rtmi_render_params *p, const rtmi_sparse_params *sp,
                                     const void *d_pixels, const void *d_count, void *d_mean, void *d_stderr, void *d_samples,
                                     void *d_scratch, void *stream) {
    return guard([&] {
        const char *name = "rtmi_sparse_render_device";
        rtmi_scene *dev = DEV(lowered, name, "sparse-render");
        const rtmi_camera c = CAM(cam).lower();
        return done(name, rtmi_sparse_render_device(dev, p, &c, sp, d_pixels, d_count, d_mean, d_stderr, d_samples, d_scratch, stream),
                    CODED_UNSUPPORTED);
    });
}
// select -> sparse render -> patch of the planes; device = 1: device planes, enqueued on `stream` (counts: 2 device words
// or NULL); device = 0: host planes, blocking (counts: 2 host words or NULL; scratch and stream are not read)
RTH_API int rth_sparse_refine(void *lowered, void *cam, const rtmi_render_params *p, const rtmi_sparse_params *sp, uint32_t accept_mask,
                              uint32_t mark, void *bytes, void *linear, void *rgb8, void *stderr_rgb, void *d_scratch,
                              uint64_t scratch_bytes, void *counts, int device, void *stream) {
    return guard([&] {
        const char *name = device ? "rtmi_sparse_refine_device" : "rtmi_sparse_refine";
        rtmi_scene *dev = DEV(lowered, name, "sparse-render");
        const rtmi_camera c = CAM(cam).lower();
        const int rc = device ? rtmi_sparse_refine_device(dev, p, &c, sp, accept_mask, mark, bytes, linear, rgb8, stderr_rgb, d_scratch,
                                                          scratch_bytes, counts, stream)
                              : rtmi_sparse_refine(dev, p, &c, sp, accept_mask, mark, static_cast<uint8_t *>(bytes),
                                                   static_cast<float *>(linear), static_cast<uint8_t *>(rgb8),
                                                   static_cast<float *>(stderr_rgb), static_cast<uint32_t *>(counts));
        return done(name, rc, CODED_UNSUPPORTED);
    });
}
// per-pixel adaptive sampling (include/rtmi_pixelwise.h) on the uploaded handle: host planes and blocking, or device planes
// enqueued on `stream`
RTH_API int rth_render_pixelwise(void *lowered, void *cam, const rtmi_render_params *p, const rtmi_pixelwise_opts *o, float *out_linear,
                                 uint8_t *out_rgb8, float *out_stderr, uint32_t *out_spp, uint32_t *out_counts, rtmi_stats *stats) {
    return guard([&] {
        const char *name = "rtmi_render_pixelwise";
        rtmi_scene *dev = DEV(lowered, name, "pixelwise");
        const rtmi_camera c = CAM(cam).lower();
        return done(name, rtmi_render_pixelwise(dev, &c, p, o, out_linear, out_rgb8, out_stderr, out_spp, out_counts, stats),
                    CODED_UNSUPPORTED);
    });
}
RTH_API int rth_render_pixelwise_device(void *lowered, void *cam, const rtmi_render_params *p, const rtmi_pixelwise_opts *o,
                                        void *d_linear, void *d_rgb8, void *d_stderr, void *d_spp, void *d_counts, void *d_scratch,
                                        uint64_t scratch_bytes, void *stream) {
    return guard([&] {
        const char *name = "rtmi_render_pixelwise_device";
        rtmi_scene *dev = DEV(lowered, name, "pixelwise");
        const rtmi_camera c = CAM(cam).lower();
        return done(name, rtmi_render_pixelwise_device(dev, p, &c, o, d_linear, d_rgb8, d_stderr, d_spp, d_counts, d_scratch, scratch_bytes,
                                                       stream),
                    CODED_UNSUPPORTED);
    });
}
// windowed adaptive sampling (include/rtmi_window.h) on the uploaded handle, as the per-pixel entries above
RTH_API int rth_render_window(void *lowered, void *cam, const rtmi_render_params *p, const rtmi_window_opts *o, float *out_linear,
                              uint8_t *out_rgb8, float *out_stderr, uint32_t *out_spp, uint32_t *out_counts, rtmi_stats *stats) {
    return guard([&] {
        const char *name = "rtmi_render_window";
        rtmi_scene *dev = DEV(lowered, name, "windowed");
        const rtmi_camera c = CAM(cam).lower();
        return done(name, rtmi_render_window(dev, &c, p, o, out_linear, out_rgb8, out_stderr, out_spp, out_counts, stats), CODED_UNSUPPORTED);
    });
}
RTH_API int rth_render_window_device(void *lowered, void *cam, const rtmi_render_params *p, const rtmi_window_opts *o, void *d_linear,
                                     void *d_rgb8, void *d_stderr, void *d_spp, void *d_counts, void *d_scratch, uint64_t scratch_bytes,
                                     void *stream) {
    return guard([&] {
        const char *name = "rtmi_render_window_device";
        rtmi_scene *dev = DEV(lowered, name, "windowed");
        const rtmi_camera c = CAM(cam).lower();
        return done(name, rtmi_render_window_device(dev, p, &c, o, d_linear, d_rgb8, d_stderr, d_spp, d_counts, d_scratch, scratch_bytes, stream),
                    CODED_UNSUPPORTED);
    });
}
// hemisphere gathers (include/rtmi_gather.h) on the uploaded handle, as the radiance queries
RTH_API int rth_gather(void *lowered, const rtmi_gather_params *p, const float *points, const float *normals, const float *time,
                       float *out_value, float *out_stderr, float *out_sh, double *kernel_ms) {
    return guard([&] {
        const char *name = "rtmi_gather";
        return done(name, rtmi_gather(DEV(lowered, name, "gather"), p, points, normals, time, out_value, out_stderr, out_sh, kernel_ms),
                    CODED_UNSUPPORTED);
    });
}
RTH_API int rth_gather_device(void *lowered, const rtmi_gather_params *p, const void *d_points, const void *d_normals,
                              const void *d_time, void *d_value, void *d_stderr, void *d_sh, void *d_scratch, uint64_t scratch_bytes,
                              void *stream) {
    return guard([&] {
        const char *name = "rtmi_gather_device";
        return done(name, rtmi_gather_device(DEV(lowered, name, "gather"), p, d_points, d_normals, d_time, d_value, d_stderr, d_sh,
                                             d_scratch, scratch_bytes, stream),
                    CODED_UNSUPPORTED);
    });
}
// next-event estimation (include/rtmi_nee.h): attaches the light table of the lowered scene to its uploaded handle, then
// renders; RTH_UNSUPPORTED for what rtmi_render_nee does not support, a multi-GPU handle among it
RTH_API int rth_attach_lights(void *lowered) {
    return guard([&] {
        const char *name = "rtmi_scene_attach_lights";
        rtmi_scene *dev = DEV(lowered, name, "NEE");
        const rtmi_scene_desc d = LOW(lowered)->lowered->desc();
        return done(name, rtmi_scene_attach_lights(dev, &d), CODED);
    });
}
// ---- light tree (include/rtmi_light_tree.h) ---------------------------------------------------------
RTH_API int rth_attach_light_tree(void *lowered) {
    return guard([&] {
        const char *name = "rtmi_scene_attach_light_tree";
        rtmi_scene *dev = DEV(lowered, name, "light-tree");
        const rtmi_scene_desc d = LOW(lowered)->lowered->desc();
        return done(name, rtmi_scene_attach_light_tree(dev, &d), CODED);
    });
}
RTH_API int rth_probe_light_tree(void *lowered, int op, const float *points, const void *aux, uint32_t n, uint32_t *out_light,
                                 float *out_p) {
    return guard([&] {
        const char *name = "rtmi_probe_light_tree";
        return done(name, rtmi_probe_light_tree(DEV(lowered, name, "light-tree"), op, points, aux, n, out_light, out_p), CODED);
    });
}
RTH_API int rth_render_nee(void *lowered, void *cam, const rtmi_render_params *p, float *out_linear, uint8_t *out_rgb8,
                           float *out_stderr, uint64_t *out_path_sig, rtmi_stats *stats) {
    return guard([&] {
        const char *name = "rtmi_render_nee";
        rtmi_scene *dev = DEV(lowered, name, "NEE");
        const rtmi_camera c = CAM(cam).lower();
        return done(name, rtmi_render_nee(dev, &c, p, out_linear, out_rgb8, out_stderr, out_path_sig, stats), CODED_UNSUPPORTED);
    });
}

// environment lighting (include/rtmi_env.h): attaches a map (rgb = NULL detaches) to the uploaded handle, then renders;
// RTH_UNSUPPORTED for what rtmi_render_env does not support, a multi-GPU handle among it
RTH_API int rth_attach_env(void *lowered, uint32_t width, uint32_t height, const float *rgb) {
    return guard([&] {
        const char *name = "rtmi_scene_attach_env";
        rtmi_scene *dev = DEV(lowered, name, "environment");
        const rtmi_env_map m{width, height, rgb};
        return done(name, rtmi_scene_attach_env(dev, rgb ? &m : nullptr), CODED);
    });
}
RTH_API int rth_render_env(void *lowered, void *cam, const rtmi_render_params *p, const rtmi_env_render *opts, float *out_linear,
                           uint8_t *out_rgb8, float *out_stderr, uint64_t *out_path_sig, rtmi_stats *stats) {
    return guard([&] {
        const char *name = "rtmi_render_env";
        rtmi_scene *dev = DEV(lowered, name, "environment");
        const rtmi_camera c = CAM(cam).lower();
        return done(name, rtmi_render_env(dev, &c, p, opts, out_linear, out_rgb8, out_stderr, out_path_sig, stats),
                    CODED_UNSUPPORTED);
    });
}
// adaptive sampling with NEE or environment lighting (include/rtmi_adaptive_nee.h); RTH_UNSUPPORTED for what the two
// entries do not support, a multi-GPU handle among it
RTH_API int rth_render_adaptive_nee(void *lowered, void *cam, const rtmi_render_params *p, const rtmi_adaptive *a,
                                    float *out_linear, uint8_t *out_rgb8, float *out_stderr, uint32_t *out_spp, rtmi_stats *stats) {
    return guard([&] {
        const char *name = "rtmi_render_adaptive_nee";
        rtmi_scene *dev = DEV(lowered, name, "adaptive");
        const rtmi_camera c = CAM(cam).lower();
        return done(name, rtmi_render_adaptive_nee(dev, &c, p, a, out_linear, out_rgb8, out_stderr, out_spp, stats),
                    CODED_UNSUPPORTED);
    });
}
RTH_API int rth_render_adaptive_env(void *lowered, void *cam, const rtmi_render_params *p, const rtmi_env_render *opts,
                                    const rtmi_adaptive *a, float *out_linear, uint8_t *out_rgb8, float *out_stderr,
                                    uint32_t *out_spp, rtmi_stats *stats) {
    return guard([&] {
        const char *name = "rtmi_render_adaptive_env";
        rtmi_scene *dev = DEV(lowered, name, "adaptive");
        const rtmi_camera c = CAM(cam).lower();
        return done(name, rtmi_render_adaptive_env(dev, &c, p, opts, a, out_linear, out_rgb8, out_stderr, out_spp, stats),
                    CODED_UNSUPPORTED);
    });
}
// Russian-roulette path termination (include/rtmi_roulette.h); RTH_UNSUPPORTED for what the two entries do not support, a
// multi-GPU handle among it
RTH_API int rth_render_roulette(void *lowered, void *cam, const rtmi_render_params *p, const rtmi_roulette *opts, float *out_linear,
                                uint8_t *out_rgb8, float *out_stderr, uint32_t *out_bounces, rtmi_stats *stats) {
    return guard([&] {
        const char *name = "rtmi_render_roulette";
        rtmi_scene *dev = DEV(lowered, name, "roulette");
        const rtmi_camera c = CAM(cam).lower();
        return done(name, rtmi_render_roulette(dev, &c, p, opts, out_linear, out_rgb8, out_stderr, out_bounces, stats),
                    CODED_UNSUPPORTED);
    });
}
RTH_API int rth_render_adaptive_roulette(void *lowered, void *cam, const rtmi_render_params *p, const rtmi_roulette *opts,
                                         const rtmi_adaptive *a, float *out_linear, uint8_t *out_rgb8, float *out_stderr,
                                         uint32_t *out_spp, uint32_t *out_bounces, rtmi_stats *stats) {
    return guard([&] {
        const char *name = "rtmi_render_adaptive_roulette";
        rtmi_scene *dev = DEV(lowered, name, "roulette");
        const rtmi_camera c = CAM(cam).lower();
        return done(name,
                    rtmi_render_adaptive_roulette(dev, &c, p, opts, a, out_linear, out_rgb8, out_stderr, out_spp, out_bounces, stats),
                    CODED_UNSUPPORTED);
    });
}
// render sessions (include/rtmi_session.h): the entries one to one on the uploaded handle; RTH_UNSUPPORTED for what they do
// not support, a multi-GPU handle among it.  A session is freed by rth_session_close or, at the latest, by rth_free_all
// (before the scenes); re-uploading its scene (rth_upload) while it lives is the caller's error.
static rtmi_session *SES(void *h) {
    std::lock_guard<std::mutex> lk(g_mu);
    for (rtmi_session *ss : g_sessions)
        if (ss == h) return ss;
    throw std::runtime_error("handle is not a live render session");
}
RTH_API void *rth_session_create(void *lowered, void *cam, const rtmi_render_params *p, const rtmi_session_opts *opts) {
    return guard_new([&] {
        const char *name = "rtmi_session_create";
        rtmi_scene *dev = DEV(lowered, name, "session");
        const rtmi_camera c = CAM(cam).lower();
        rtmi_session *ss = nullptr;
        done(name, rtmi_session_create(dev, &c, p, opts, &ss), CODED_UNSUPPORTED);
        std::lock_guard<std::mutex> lk(g_mu);
        g_sessions.push_back(ss);
        return (void *)ss;
    });
}
RTH_API int rth_session_close(void *session) {
    return guard([&] {
        rtmi_session *ss = SES(session);
        {
            std::lock_guard<std::mutex> lk(g_mu);
            g_sessions.erase(std::find(g_sessions.begin(), g_sessions.end(), ss));
        }
        rtmi_session_destroy(ss);
        return RTH_OK;
    });
}
RTH_API int rth_session_render(void *session, uint32_t add_spp, rtmi_stats *stats) {
    return guard([&] { return done("rtmi_session_render", rtmi_session_render(SES(session), add_spp, stats), CODED_UNSUPPORTED); });
}
RTH_API int rth_session_refine(void *session, double abs_tol, double rel_tol, uint32_t cap, rtmi_stats *stats) {
    return guard([&] {
        return done("rtmi_session_refine", rtmi_session_refine(SES(session), abs_tol, rel_tol, cap, stats), CODED_UNSUPPORTED);
    });
}
RTH_API int rth_session_image(void *session, float *out_linear, uint8_t *out_rgb8, float *out_stderr, uint32_t *out_spp,
                              uint32_t *out_bounces) {
    return guard([&] {
        return done("rtmi_session_image", rtmi_session_image(SES(session), out_linear, out_rgb8, out_stderr, out_spp, out_bounces),
                    CODED);
    });
}
RTH_API int rth_session_export(void *session, void *buf, size_t cap, size_t *need) {
    return guard([&] { return done("rtmi_session_export", rtmi_session_export(SES(session), buf, cap, need), CODED); });
}
RTH_API int rth_session_import(void *session, const void *buf, size_t len) {
    return guard([&] { return done("rtmi_session_import", rtmi_session_import(SES(session), buf, len), CODED); });
}
RTH_API int rth_session_merge(void *dst, void *src) {
    return guard([&] { return done("rtmi_session_merge", rtmi_session_merge(SES(dst), SES(src)), CODED_UNSUPPORTED); });
}
RTH_API int rth_session_spp(void *session, uint32_t *min_spp, uint32_t *max_spp) {
    return guard([&] { return done("rtmi_session_spp", rtmi_session_spp(SES(session), min_spp, max_spp), CODED); });
}
// the frame pipeline (include/rtmi_frame.h): the entries one to one on the uploaded handle; RTH_UNSUPPORTED for what they do
// not support, a multi-GPU handle among it.  A frame is freed by rth_frame_close or, at the latest, by rth_free_all (before
// the scenes); re-uploading its scene (rth_upload) while it lives is the caller's error.
static rtmi_frame *FRM(void *h) {
    std::lock_guard<std::mutex> lk(g_mu);
    for (rtmi_frame *f : g_frames)
        if (f == h) return f;
    throw std::runtime_error("handle is not a live frame");
}
RTH_API void *rth_frame_create(void *lowered, const rtmi_render_params *p, const rtmi_frame_opts *opts) {
    return guard_new([&] {
        const char *name = "rtmi_frame_create";
        rtmi_scene *dev = DEV(lowered, name, "frame");
        rtmi_frame *f = nullptr;
        done(name, rtmi_frame_create(dev, p, opts, &f), CODED_UNSUPPORTED);
        std::lock_guard<std::mutex> lk(g_mu);
        g_frames.push_back(f);
        return (void *)f;
    });
}
RTH_API int rth_frame_close(void *frame) {
    return guard([&] {
        rtmi_frame *f = FRM(frame);
        {
            std::lock_guard<std::mutex> lk(g_mu);
            g_frames.erase(std::find(g_frames.begin(), g_frames.end(), f));
        }
        rtmi_frame_destroy(f);
        return RTH_OK;
    });
}
RTH_API int rth_frame_render(void *frame, void *cam, uint32_t ns, uint64_t seed, const rtmi_frame_out *out, int on_device,
                             rtmi_stats *stats) {
    return guard([&] {
        const rtmi_camera c = CAM(cam).lower();
        if (on_device)
            return done("rtmi_frame_render_device", rtmi_frame_render_device(FRM(frame), &c, ns, seed, out, stats), CODED_UNSUPPORTED);
        return done("rtmi_frame_render", rtmi_frame_render(FRM(frame), &c, ns, seed, out, stats), CODED_UNSUPPORTED);
    });
}
RTH_API int rth_frame_reset(void *frame) {
    return guard([&] { return done("rtmi_frame_reset", rtmi_frame_reset(FRM(frame)), CODED); });
}
// guided upscaling (include/rtmi_upscale.h): the handle's entries one to one on the uploaded scene, as the frame wrappers; an
// upscaler is freed by rth_upscaler_close or, at the latest, by rth_free_all (before the scenes).
static rtmi_upscaler *UPS(void *h) {
    std::lock_guard<std::mutex> lk(g_mu);
    for (rtmi_upscaler *u : g_upscalers)
        if (u == h) return u;
    throw std::runtime_error("handle is not a live upscaler");
}
RTH_API void *rth_upscaler_create(void *lowered, const rtmi_render_params *p, const rtmi_upscaler_opts *opts) {
    return guard_new([&] {
        const char *name = "rtmi_upscaler_create";
        rtmi_scene *dev = DEV(lowered, name, "upscaler");
        rtmi_upscaler *u = nullptr;
        done(name, rtmi_upscaler_create(dev, p, opts, &u), CODED_UNSUPPORTED);
        std::lock_guard<std::mutex> lk(g_mu);
        g_upscalers.push_back(u);
        return (void *)u;
    });
}
RTH_API int rth_upscaler_close(void *upscaler) {
    return guard([&] {
        rtmi_upscaler *u = UPS(upscaler);
        {
            std::lock_guard<std::mutex> lk(g_mu);
            g_upscalers.erase(std::find(g_upscalers.begin(), g_upscalers.end(), u));
        }
        rtmi_upscaler_destroy(u);
        return RTH_OK;
    });
}
RTH_API int rth_upscaler_render(void *upscaler, void *cam, uint32_t ns, uint64_t seed, const rtmi_upscaler_out *out, int on_device,
                                rtmi_stats *stats) {
    return guard([&] {
        const rtmi_camera c = CAM(cam).lower();
        if (on_device)
            return done("rtmi_upscaler_render_device", rtmi_upscaler_render_device(UPS(upscaler), &c, ns, seed, out, stats),
                        CODED_UNSUPPORTED);
        return done("rtmi_upscaler_render", rtmi_upscaler_render(UPS(upscaler), &c, ns, seed, out, stats), CODED_UNSUPPORTED);
    });
}
RTH_API int rth_upscaler_reset(void *upscaler) {
    return guard([&] { return done("rtmi_upscaler_reset", rtmi_upscaler_reset(UPS(upscaler)), CODED); });
}
RTH_API int rth_probe_env(void *lowered, int op, const float *in, float *out, uint32_t n) {
    return guard([&] { return done("rtmi_probe_env", rtmi_probe_env(DEV(lowered), op, in, out, n), CODED); });
}
// ---- f64 render mode (include/rtmi_f64.h) ------------------------------------------------------------
RTH_API int rth_lowered_desc_f64(void *lowered, rtmi_scene_f64 *out) {
    return guard([&] { *out = LOW(lowered)->lowered->desc_f64(); return RTH_OK; });
}
RTH_API int rth_camera_lower_f64(void *cam, rtmi_camera_f64 *out) { return guard([&] { *out = CAM(cam).lower_f64(); return RTH_OK; }); }
// attaches the lowered scene's double planes to its uploaded handle (rtmi_scene_attach_f64)
RTH_API int rth_attach_f64(void *lowered) {
    return guard([&] {
        rtmi_scene *dev = DEV(lowered);
        if (LOW(lowered)->edited)
            throw Unsupported("rtmi_scene_attach_f64: the scene was edited by a scene update; its double planes hold the positions it was lowered with");
        const rtmi_scene_f64 w = LOW(lowered)->lowered->desc_f64();
        return done("rtmi_scene_attach_f64", rtmi_scene_attach_f64(dev, &w), CODED);
    });
}
RTH_API int rth_render_f64(void *lowered, void *cam, const rtmi_render_params *p, double t_min, double *out_linear, uint8_t *out_rgb8,
                           uint64_t *out_path_sig, rtmi_stats *stats) {
    return guard([&] {
        rtmi_scene *dev = DEV(lowered);
        const rtmi_camera_f64 c = CAM(cam).lower_f64();
        return done("rtmi_render_f64", rtmi_render_f64(dev, &c, p, t_min, out_linear, out_rgb8, out_path_sig, stats), PLAIN);
    });
}
// ---- scene updates (include/rtmi_update.h): edits of the FLAT scene; the object graph it was lowered from keeps the old
// positions, and so do the double planes of the f64 render mode --------------------------------------------------------------
RTH_API int rthu_refittable(void *lowered, uint8_t *mask) {
    return guard([&] {
        const rtmi_scene_desc d = LOW(lowered)->lowered->desc();
        return done("rtmu_refittable", rtmu_refittable(&d, mask), CODED);
    });
}
// New planes for [first, first + count) from host memory (b may be NULL): the resident handle first, when there is one —
// it refuses what cannot be updated before anything changes —, then the lowered arrays and their refit, so that the
// description stays the description of what is resident.
RTH_API int rthu_update_prims(void *lowered, uint32_t first, uint32_t count, const float *a, const float *b) {
    return guard([&] {
        const char *name = "rtmu_scene_update_prims";
        Obj *o = LOW(lowered);
        LoweredScene &ls = *o->lowered;
        if ((uint64_t)first + count > ls.prim_meta.size()) throw std::runtime_error(std::string(name) + ": the range leaves the primitives");
        if (count == 0) return (int)RTH_OK;
        if (!a) throw std::runtime_error(std::string(name) + ": a is NULL");
        if (o->multi && !o->dev) DEV(lowered, name, "update");
        if (o->dev)
            if (int rc = done(name, rtmu_scene_update_prims(o->dev, first, count, a, b), CODED_UNSUPPORTED)) return rc;
        const bool was_edited = o->edited;
        o->edited = true;
        const std::vector<float> old_a(ls.prim_a.begin() + (size_t)first * 4, ls.prim_a.begin() + (size_t)(first + count) * 4);
        const std::vector<float> old_b(ls.prim_b.begin() + (size_t)first * 4, ls.prim_b.begin() + (size_t)(first + count) * 4);
        std::copy(a, a + (size_t)count * 4, ls.prim_a.begin() + (size_t)first * 4);
        if (b) std::copy(b, b + (size_t)count * 4, ls.prim_b.begin() + (size_t)first * 4);
        const rtmi_scene_desc d = ls.desc();
        const int rc = rtmu_refit_desc(&d, first, count, ls.items.data(), ls.nodes.data(), ls.alt_nodes.data(), d.prim_gate ? ls.prim_gate.data() : nullptr);
        if (rc) { // (only without a resident handle: it refuses the same ranges)
            o->edited = was_edited;
            std::copy(old_a.begin(), old_a.end(), ls.prim_a.begin() + (size_t)first * 4);
            std::copy(old_b.begin(), old_b.end(), ls.prim_b.begin() + (size_t)first * 4);
        }
        return done("rtmu_refit_desc", rc, CODED_UNSUPPORTED);
    });
}
// ... from device memory, asynchronous on `stream`: the lowered arrays are NOT edited and go stale
RTH_API int rthu_update_prepare(void *lowered) {
    return guard([&] {
        const char *name = "rtmu_scene_update_prepare";
        return done(name, rtmu_scene_update_prepare(DEV(lowered, name, "update")), CODED);
    });
}
RTH_API int rthu_update_prims_device(void *lowered, uint32_t first, uint32_t count, const void *d_a, const void *d_b, void *stream) {
    return guard([&] {
        const char *name = "rtmu_scene_update_prims_device";
        const int rc = done(name, rtmu_scene_update_prims_device(DEV(lowered, name, "update"), first, count, d_a, d_b, stream), CODED_UNSUPPORTED);
        if (count) LOW(lowered)->edited = true;
        return rc;
    });
}
// New transform records [first, first + count): the resident handle first, when there is one (it refuses what cannot be
// replaced), then the lowered array.  Without a handle the kinds alone are checked here.
RTH_API int rthu_update_xforms(void *lowered, uint32_t first, uint32_t count, const rtmi_xform *recs) {
    return guard([&] {
        const char *name = "rtmu_scene_update_xforms";
        Obj *o = LOW(lowered);
        LoweredScene &ls = *o->lowered;
        if ((uint64_t)first + count > ls.xforms.size()) throw std::runtime_error(std::string(name) + ": the range leaves the transform records");
        if (count == 0) return (int)RTH_OK;
        if (!recs) throw std::runtime_error(std::string(name) + ": recs is NULL");
        if (o->multi && !o->dev) DEV(lowered, name, "update");
        if (o->dev)
            if (int rc = done(name, rtmu_scene_update_xforms(o->dev, first, count, recs), CODED_UNSUPPORTED)) return rc;
        for (uint32_t k = 0; k < count; k++)
            if (recs[k].kind != ls.xforms[first + k].kind) throw std::runtime_error(std::string(name) + ": a record must keep its kind");
        std::copy(recs, recs + count, ls.xforms.begin() + first);
        o->edited = true;
        return (int)RTH_OK;
    });
}
// The primitives lowered from a host object (rt::prims_of): *n receives their number, out (when not NULL) the first
// min(*n, cap) indices, ascending.
RTH_API int rthu_prims_of(void *lowered, void *hittable, uint32_t *out, uint32_t cap, uint32_t *n) {
    return guard([&] {
        const std::vector<uint32_t> found = prims_of(*LOW(lowered)->lowered, *H(hittable));
        if (n) *n = (uint32_t)found.size();
        if (out) std::copy(found.begin(), found.begin() + std::min<size_t>(found.size(), cap), out);
        return (int)RTH_OK;
    });
}
RTH_API int rthu_probe_scene_words(void *lowered, int which, void *out, size_t cap, size_t *need) {
    return guard([&] {
        const char *name = "rtmu_probe_scene_words";
        return done(name, rtmu_probe_scene_words(DEV(lowered, name, "update"), which, out, cap, need), CODED);
    });
}
// ---- the lights that follow an update (include/rtmi_relight.h), on the uploaded handle -------------------------------------
RTH_API int rthl_follow_lights(void *lowered, int on) {
    return guard([&] {
        const char *name = "rtml_scene_follow_lights";
        return done(name, rtml_scene_follow_lights(DEV(lowered, name, "update"), on), CODED_UNSUPPORTED);
    });
}
RTH_API int rthl_probe_light_words(void *lowered, int which, void *out, size_t cap, size_t *need) {
    return guard([&] {
        const char *name = "rtml_probe_light_words";
        return done(name, rtml_probe_light_words(DEV(lowered, name, "update"), which, out, cap, need), CODED);
    });
}
RTH_API int rth_render_device(void *lowered, void *cam, const rtmi_render_params *p, void *d_texels, void *stream,
                              rtmi_stats *stats) {
    return guard([&] {
        rtmi_scene *dev = DEV(lowered);
        const rtmi_camera c = CAM(cam).lower();
        return done("rtmi_render_device", rtmi_render_device(dev, &c, p, d_texels, stream, stats), PLAIN);
    });
}
// overflow report of the asynchronous render calls since the last report (rtmi_scene_status)
RTH_API int rth_scene_status(void *lowered) {
    return guard([&] { return done("rtmi_scene_status", rtmi_scene_status(DEV(lowered), nullptr), PLAIN); });
}
// whole image on several GPUs of this process (rtmi_render_multi): uploads the lowered scene to every listed device
RTH_API int rth_render_multi(void *lowered, void *cam, const rtmi_render_params *p, const int *devices, uint32_t n,
                             float *out_linear, uint8_t *out_rgb8, rtmi_stats *stats) {
    return guard([&] {
        const rtmi_scene_desc d = LOW(lowered)->lowered->desc();
        const rtmi_camera c = CAM(cam).lower();
        return done("rtmi_render_multi", rtmi_render_multi(&d, devices, n, &c, p, out_linear, out_rgb8, stats), PLAIN);
    });
}
// RTMI_FLAG_PROGRESSIVE: the image of the passes finished so far (only from inside the progress callback of rth_render)
RTH_API int rth_partial_image(void *lowered, const rtmi_render_params *p, float *out_linear, uint8_t *out_rgb8, uint32_t *spp_done) {
    return guard([&] {
        return done("rtmi_partial_image", rtmi_partial_image(DEV(lowered), p, out_linear, out_rgb8, spp_done), PLAIN);
    });
}
// the lowered scene resident on a list of GPUs of this process (rtmi_multi_create); replaces an earlier list
RTH_API int rth_upload_multi(void *lowered, const int *devices, uint32_t n) {
    return guard([&] {
        Obj *o = LOW(lowered);
        if (o->multi) { rtmi_multi_destroy(o->multi); o->multi = nullptr; }
        const rtmi_scene_desc d = o->lowered->desc();
        return done("rtmi_multi_create", rtmi_multi_create(&d, devices, n, &o->multi), CODED);
    });
}
RTH_API int rth_multi_free(void *lowered) {
    return guard([&] {
        Obj *o = LOW(lowered);
        if (o->multi) { rtmi_multi_destroy(o->multi); o->multi = nullptr; }
        return RTH_OK;
    });
}
// which exchange the resident handle's renders perform (RTMI_COLLECTIVE_*), -1 without a handle
RTH_API int rth_multi_collective(void *lowered) {
    Obj *o = LOW(lowered);
    return o && o->multi ? rtmi_multi_collective(o->multi) : -1;
}
// the handle of a lowered scene resident on a device list
static rtmi_multi *MULTI(void *lowered) {
    Obj *o = LOW(lowered);
    if (!o->multi) throw std::runtime_error("scene not resident on a device list: call rth_upload_multi first");
    return o->multi;
}
RTH_API int rth_multi_prepare(void *lowered, const rtmi_render_params *p) {
    return guard([&] { return done("rtmi_multi_prepare", rtmi_multi_prepare(MULTI(lowered), p), PLAIN); });
}
RTH_API int rth_multi_render(void *lowered, void *cam, const rtmi_render_params *p, float *out_linear, uint8_t *out_rgb8,
                             rtmi_stats *stats) {
    return guard([&] {
        rtmi_multi *multi = MULTI(lowered);
        const rtmi_camera c = CAM(cam).lower();
        return done("rtmi_multi_render", rtmi_multi_render(multi, &c, p, out_linear, out_rgb8, stats), PLAIN);
    });
}
// allocate the render buffers for `p` ahead of the first render call (optional)
RTH_API int rth_render_prepare(void *lowered, const rtmi_render_params *p) {
    return guard([&] { return done("rtmi_render_prepare", rtmi_render_prepare(DEV(lowered), p), PLAIN); });
}
// Camera::render / create_image in one call (lower + upload + render + free)
RTH_API int rth_camera_render(void *cam, void *world, uint32_t nx, uint32_t ny, uint32_t ns, uint64_t seed, uint32_t flags,
                              int device, float *out_linear, uint8_t *out_rgb8, rtmi_stats *stats) {
    return guard([&] {
        RenderOptions opt;
        opt.seed = seed; opt.flags = flags; opt.device = device;
        Image img = CAM(cam).render(*H(world), nx, ny, ns, opt);
        if (out_linear) memcpy(out_linear, img.linear.data(), img.linear.size() * sizeof(float));
        if (out_rgb8) memcpy(out_rgb8, img.rgb8.data(), img.rgb8.size());
        if (stats) *stats = img.stats;
        return RTH_OK;
    });
}

// the f64 render mode in one call, like rth_camera_render: lower + create + attach + render + destroy (nothing stays resident)
RTH_API int rth_camera_render_f64(void *cam, void *world, uint32_t nx, uint32_t ny, uint32_t ns, uint64_t seed, uint32_t flags,
                                  int device, double *out_linear, uint8_t *out_rgb8, rtmi_stats *stats) {
    return guard([&] {
        const LoweredScene ls = lower_scene(*H(world));
        const rtmi_scene_desc d = ls.desc();
        const rtmi_scene_f64 w = ls.desc_f64();
        rtmi_render_params p{};
        p.nx = nx; p.ny = ny; p.ns = ns; p.max_depth = 50; p.t_min = 0.001f; p.flags = flags; p.seed = seed;
        p.tile_rank = 0; p.tile_world = 1;
        const rtmi_camera_f64 c = CAM(cam).lower_f64();
        rtmi_scene *scene = nullptr;
        done("rtmi_scene_create", rtmi_scene_create(&d, device, &scene), CODED);
        int rc = rtmi_scene_attach_f64(scene, &w);
        if (!rc) rc = rtmi_render_f64(scene, &c, &p, 0.001, out_linear, out_rgb8, nullptr, stats); // t_min: color.rs:7
        const std::string err = rc ? rtmi_last_error() : "";
        rtmi_scene_destroy(scene);
        if (rc) throw std::runtime_error("rtmi_render_f64: " + err);
        return RTH_OK;
    });
}

// ---- CPU evaluation of the mirror (f64, the reference's arithmetic) ------------------------
RTH_API int rth_hit(void *h, const double *o, const double *d, double time, double t_min, double t_max, uint64_t seed,
                    double *out9, int *found) {
    return guard([&] {
        render_rng().seed(seed, 0, 0, 0);
        const double mx = 1.79769313486231570814527423731704357e+308;
        auto r = H(h)->hit(Ray(Vec3(o[0], o[1], o[2]), Vec3(d[0], d[1], d[2]), time), t_min <= -1.7e308 ? -mx : t_min,
                           t_max >= 1.7e308 ? mx : t_max);
        *found = r ? 1 : 0;
        if (r) {
            out9[0] = r->t; out9[1] = r->u; out9[2] = r->v;
            out9[3] = r->p.x; out9[4] = r->p.y; out9[5] = r->p.z;
            out9[6] = r->normal.x; out9[7] = r->normal.y; out9[8] = r->normal.z;
        }
        return RTH_OK;
    });
}
RTH_API int rth_bounding_box(void *h, double t0, double t1, double *out6, int *found) {
    return guard([&] {
        auto b = H(h)->bounding_box(t0, t1);
        *found = b ? 1 : 0;
        if (b) { out6[0] = b->min.x; out6[1] = b->min.y; out6[2] = b->min.z; out6[3] = b->max.x; out6[4] = b->max.y; out6[5] = b->max.z; }
        return RTH_OK;
    });
}
RTH_API int rth_tex_value(void *tex, double u, double v, const double *p, double *out3) {
    return guard([&] {
        const Vec3 c = T(tex)->value(u, v, Vec3(p[0], p[1], p[2]));
        out3[0] = c.x; out3[1] = c.y; out3[2] = c.z;
        return RTH_OK;
    });
}
RTH_API int rth_scatter(void *mat, const double *ro, const double *rd, double time, const double *rec9, uint64_t seed,
                        double *out10, int *scattered) {
    return guard([&] {
        render_rng().seed(seed, 0, 0, 0);
        HitRecord rec;
        rec.t = rec9[0]; rec.u = rec9[1]; rec.v = rec9[2];
        rec.p = Vec3(rec9[3], rec9[4], rec9[5]); rec.normal = Vec3(rec9[6], rec9[7], rec9[8]);
        rec.material = M(mat).get();
        auto s = M(mat)->scatter(Ray(Vec3(ro[0], ro[1], ro[2]), Vec3(rd[0], rd[1], rd[2]), time), rec);
        *scattered = s ? 1 : 0;
        if (s) {
            const Vec3 o = s->first.origin(), d = s->first.direction();
            out10[0] = o.x; out10[1] = o.y; out10[2] = o.z; out10[3] = d.x; out10[4] = d.y; out10[5] = d.z;
            out10[6] = s->first.time(); out10[7] = s->second.x; out10[8] = s->second.y; out10[9] = s->second.z;
        }
        return RTH_OK;
    });
}
RTH_API int rth_emitted(void *mat, double u, double v, const double *p, double *out3) {
    return guard([&] {
        const Vec3 c = M(mat)->emitted(u, v, Vec3(p[0], p[1], p[2]));
        out3[0] = c.x; out3[1] = c.y; out3[2] = c.z;
        return RTH_OK;
    });
}
RTH_API int rth_get_ray(void *cam, double s, double t, uint64_t seed, double *out7) {
    return guard([&] {
        render_rng().seed(seed, 0, 0, 0);
        const Ray r = CAM(cam).get_ray(s, t);
        const Vec3 o = r.origin(), d = r.direction();
        out7[0] = o.x; out7[1] = o.y; out7[2] = o.z; out7[3] = d.x; out7[4] = d.y; out7[5] = d.z; out7[6] = r.time();
        return RTH_OK;
    });
}
RTH_API void rth_set_sky_background(int on) { set_sky_background(on != 0); }
RTH_API void rth_set_face_forward(int on) { set_face_forward(on != 0); }
RTH_API void rth_set_uv_book(int on) { set_uv_book(on != 0); }
// color() of one camera sample on the CPU (f64), same stream layout as the device
RTH_API int rth_color_sample(void *cam, void *world, uint32_t nx, uint32_t ny, uint32_t i, uint32_t j, uint32_t s,
                             uint64_t seed, double *out3) {
    return guard([&] {
        Rng &rng = render_rng();
        rng.seed(seed, s, j * nx + i, 0);
        const double u = ((double)i + rng.gen()) / (double)nx;
        const double v = ((double)j + rng.gen()) / (double)ny;
        const Ray ray = CAM(cam).get_ray(u, v);
        const Vec3 c = color(ray, *H(world), 0);
        out3[0] = c.x; out3[1] = c.y; out3[2] = c.z;
        return RTH_OK;
    });
}
