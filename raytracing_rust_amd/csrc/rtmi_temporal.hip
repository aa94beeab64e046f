// rtmi_temporal.hip — translation unit of the temporal accumulation (include/rtmi_temporal.h): one fused kernel per push
// and the host entry points.  Compiled with the flags of rtmi_denoise.hip (-ffp-contract=off, no fast-math, IEEE / and
// sqrt, denormals kept), so tests/temporal_ref.py restates every output bit for bit.  See DESIGN.md §27.
//
// Device layout, per pixel (row-major, row 0 = top), two copies that the pushes ping-pong between:
//   col   float4 {x_r, x_g, x_b, N}: the demodulated colour and the history length; N == 0 = never a source
//   geo   float4 {n_x, n_y, n_z, z}
//   var   float4 {var_r, var_g, var_b, 0}: only touched when standard errors are supplied
// so every record is one 16-byte access, and the four taps of a pixel are neighbouring records.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>

#include "rtmi.h"
#include "rtmi_temporal.h"
#include "rtmi_frame_launch.hpp"
#include "rtmi_hostkit.hpp"
#include "rtmi_image_dev.hpp"

namespace {

constexpr int kBlock = 16; // 16x16 workgroups, as the denoiser: a wavefront is 16 columns x 4 rows, so taps share L1 lines

struct TemporalPush {
    uint32_t nx, ny;
    int has_prev;     // a previous frame is stored
    int same_cam;     // ... and its camera has the bytes of the current one
    int demodulate;
    float max_history, alpha_min, depth_tol, normal_min, albedo_min;
    float org[3], llc[3], hor[3], ver[3]; // the current camera
    float porg[3], m[9];                  // the previous camera's origin and inverse matrix, row-major
};

// Steps 1-7 of the header for one pixel per lane.  VAR: standard errors are supplied.
template <bool VAR>
__global__ __launch_bounds__(256) void rtmi_temporal_push_kernel(
    const float *__restrict__ linear, const float *__restrict__ albedo, const float *__restrict__ normal,
    const float *__restrict__ depth, const float *__restrict__ se, const float4 *__restrict__ pcol,
    const float4 *__restrict__ pgeo, const float4 *__restrict__ pvar, float4 *__restrict__ ncol, float4 *__restrict__ ngeo,
    float4 *__restrict__ nvar, float *__restrict__ out_linear, float *__restrict__ out_se, float *__restrict__ out_hist,
    float2 *__restrict__ out_motion, TemporalPush P) {
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x), r = (int)(blockIdx.y * kBlock + threadIdx.y);
    const int nx = (int)P.nx, ny = (int)P.ny;
    if (i >= nx || r >= ny) return;
    const size_t p = (size_t)r * nx + i;
    const float z = depth[p];
    const float n0 = normal[p * 3], n1 = normal[p * 3 + 1], n2 = normal[p * 3 + 2];
    const float l0 = linear[p * 3], l1 = linear[p * 3 + 1], l2 = linear[p * 3 + 2];
    float e0 = 0.0f, e1 = 0.0f, e2 = 0.0f;
    if (VAR) {
        e0 = se[p * 3];
        e1 = se[p * 3 + 1];
        e2 = se[p * 3 + 2];
    }
    ngeo[p] = make_float4(n0, n1, n2, z);
    if (!surface(z)) {
        ncol[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (VAR) nvar[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        out_linear[p * 3] = l0;
        out_linear[p * 3 + 1] = l1;
        out_linear[p * 3 + 2] = l2;
        if (VAR) {
            out_se[p * 3] = e0;
            out_se[p * 3 + 1] = e1;
            out_se[p * 3 + 2] = e2;
        }
        out_hist[p] = 0.0f;
        out_motion[p] = make_float2(0.0f, 0.0f);
        return;
    }
    // 2. demodulate
    float a0 = 1.0f, a1 = 1.0f, a2 = 1.0f;
    if (P.demodulate) {
        a0 = fmaxf(albedo[p * 3], P.albedo_min);
        a1 = fmaxf(albedo[p * 3 + 1], P.albedo_min);
        a2 = fmaxf(albedo[p * 3 + 2], P.albedo_min);
    }
    const float x0 = l0 / a0, x1 = l1 / a1, x2 = l2 / a2;
    float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
    if (VAR) {
        e0 = e0 / a0;
        e1 = e1 / a1;
        e2 = e2 / a2;
        v0 = e0 * e0;
        v1 = e1 * e1;
        v2 = e2 * e2;
    }
    // 3, 4. where the pixel's point was in the previous frame
    bool valid = P.has_prev != 0;
    float fx = (float)i, fr = (float)r, z_exp = z, mx = 0.0f, my = 0.0f;
    if (valid && !P.same_cam) {
        const float u = ((float)i + 0.5f) / (float)nx, v = ((float)(ny - 1 - r) + 0.5f) / (float)ny;
        const float dx = ((P.llc[0] + P.hor[0] * u) + P.ver[0] * v) - P.org[0];
        const float dy = ((P.llc[1] + P.hor[1] * u) + P.ver[1] * v) - P.org[1];
        const float dz = ((P.llc[2] + P.hor[2] * u) + P.ver[2] * v) - P.org[2];
        const float len = sqrtf((dx * dx + dy * dy) + dz * dz);
        const float s = z / len;
        const float qx = (P.org[0] + dx * s) - P.porg[0], qy = (P.org[1] + dy * s) - P.porg[1],
                    qz = (P.org[2] + dz * s) - P.porg[2];
        const float a = (P.m[0] * qx + P.m[1] * qy) + P.m[2] * qz;
        const float b = (P.m[3] * qx + P.m[4] * qy) + P.m[5] * qz;
        const float c = (P.m[6] * qx + P.m[7] * qy) + P.m[8] * qz;
        z_exp = sqrtf((qx * qx + qy * qy) + qz * qz);
        valid = c > 0.0f;
        if (valid) {
            fx = (a / c) * (float)nx - 0.5f;
            fr = (float)(ny - 1) - ((b / c) * (float)ny - 0.5f);
            mx = fx - (float)i;
            my = fr - (float)r;
        }
    }
    // 5. the four bilinear taps of the history
    float W = 0.0f, X0 = 0.0f, X1 = 0.0f, X2 = 0.0f, V0 = 0.0f, V1 = 0.0f, V2 = 0.0f, L = 0.0f;
    if (valid && __builtin_isfinite(fx) && __builtin_isfinite(fr) && fx >= -1.0f && fx < (float)nx && fr >= -1.0f &&
        fr < (float)ny) {
        const float bx = floorf(fx), by = floorf(fr);
        const float wx1 = fx - bx, wy1 = fr - by;
        const float wx[2] = {1.0f - wx1, wx1}, wy[2] = {1.0f - wy1, wy1};
        const int tx = (int)bx, ty = (int)by;
        const float lc = (n0 * n0 + n1 * n1) + n2 * n2;
        const float tol = P.depth_tol * z_exp;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int qx = tx + (k & 1), qy = ty + (k >> 1);
            const float w = wy[k >> 1] * wx[k & 1];
            if (!(w > 0.0f) || qx < 0 || qx >= nx || qy < 0 || qy >= ny) continue;
            const size_t q = (size_t)qy * nx + qx;
            const float4 hc = pcol[q];
            if (!(hc.w > 0.0f)) continue;
            const float4 hg = pgeo[q];
            if (!(fabsf(hg.w - z_exp) <= tol)) continue;
            const float lt = (hg.x * hg.x + hg.y * hg.y) + hg.z * hg.z;
            if (lc != 0.0f && lt != 0.0f) {
                const float d = (n0 * hg.x + n1 * hg.y) + n2 * hg.z;
                if (!(d >= P.normal_min * sqrtf(lc * lt))) continue;
            }
            W = W + w;
            X0 = X0 + w * hc.x;
            X1 = X1 + w * hc.y;
            X2 = X2 + w * hc.z;
            L = L + w * hc.w;
            if (VAR) {
                const float4 hv = pvar[q];
                const float ww = w * w;
                V0 = V0 + ww * hv.x;
                V1 = V1 + ww * hv.y;
                V2 = V2 + ww * hv.z;
            }
        }
    }
    // 6. blend
    float N = 1.0f, y0 = x0, y1 = x1, y2 = x2, u0 = v0, u1 = v1, u2 = v2;
    if (W > 0.0f) {
        N = fminf(L / W + 1.0f, P.max_history);
        const float al = fmaxf(1.0f / N, P.alpha_min), be = 1.0f - al;
        y0 = be * (X0 / W) + al * x0;
        y1 = be * (X1 / W) + al * x1;
        y2 = be * (X2 / W) + al * x2;
        if (VAR) {
            const float WW = W * W, bb = be * be, aa = al * al;
            u0 = bb * (V0 / WW) + aa * v0;
            u1 = bb * (V1 / WW) + aa * v1;
            u2 = bb * (V2 / WW) + aa * v2;
        }
    }
    // 7. store and output
    ncol[p] = make_float4(y0, y1, y2, N);
    out_linear[p * 3] = y0 * a0;
    out_linear[p * 3 + 1] = y1 * a1;
    out_linear[p * 3 + 2] = y2 * a2;
    if (VAR) {
        nvar[p] = make_float4(u0, u1, u2, 0.0f);
        out_se[p * 3] = sqrtf(u0) * a0;
        out_se[p * 3 + 1] = sqrtf(u1) * a1;
        out_se[p * 3 + 2] = sqrtf(u2) * a2;
    }
    out_hist[p] = N;
    out_motion[p] = make_float2(mx, my);
}

// the RTMI_ERR_INVALID checks in `name`'s words (rtmi_temporal_create, or the frame handle's entry)
int check_ranges(const std::string &name, uint32_t nx, uint32_t ny, const rtmi_temporal_params *p) {
    const auto bad = [&](const char *msg) { return fail(RTMI_ERR_INVALID, name, msg); };
    if (nx == 0 || ny == 0 || nx > 32768u || ny > 32768u) return bad("nx and ny must be in [1, 32768]");
    if (p->max_history < 1u || p->max_history > 65535u) return bad("max_history must be in [1, 65535]");
    if (!(p->alpha_min >= 0.0f && p->alpha_min <= 1.0f)) return bad("alpha_min must be in [0, 1]");
    if (!finite_f(p->depth_tol) || !(p->depth_tol >= 0.0f)) return bad("depth_tol must be finite and >= 0");
    if (!(p->normal_min >= -1.0f && p->normal_min <= 1.0f)) return bad("normal_min must be in [-1, 1]");
    if (!finite_f(p->albedo_min) || !(p->albedo_min > 0.0f)) return bad("albedo_min must be finite and > 0");
    if (p->reserved[0] || p->reserved[1]) return bad("reserved must be 0");
    return RTMI_OK;
}

int check_params(uint32_t nx, uint32_t ny, const rtmi_temporal_params *p) {
    if (int rc = check_ranges("rtmi_temporal_create", nx, ny, p)) return rc;
    if (p->flags & ~RTMI_TEMPORAL_NO_DEMODULATE) return rtmi_fail(RTMI_ERR_UNSUPPORTED, "rtmi_temporal_create: unknown flags bit");
    return RTMI_OK;
}

// The inverse of the matrix with columns (horizontal, vertical, llc - origin), in double, each entry rounded once to
// float (step 4 of the header).  false: singular or not finite.
bool camera_inverse(const rtmi_camera *cam, float m[9]) {
    double h[3], w[3], g[3];
    for (int k = 0; k < 3; k++) {
        h[k] = (double)cam->horizontal[k];
        w[k] = (double)cam->vertical[k];
        g[k] = (double)cam->lower_left_corner[k] - (double)cam->origin[k];
    }
    const auto cross = [](const double *a, const double *b, double *o) {
        o[0] = a[1] * b[2] - a[2] * b[1];
        o[1] = a[2] * b[0] - a[0] * b[2];
        o[2] = a[0] * b[1] - a[1] * b[0];
    };
    double r[3][3];
    cross(w, g, r[0]);
    cross(g, h, r[1]);
    cross(h, w, r[2]);
    const double det = (h[0] * r[0][0] + h[1] * r[0][1]) + h[2] * r[0][2];
    if (!(det == det) || det - det != 0.0 || det == 0.0) return false;
    for (int j = 0; j < 3; j++)
        for (int k = 0; k < 3; k++) m[3 * j + k] = (float)(r[j][k] / det);
    return true;
}

} // namespace

struct RTMI_HIDDEN rtmi_temporal {
    int device = 0;
    uint32_t nx = 0, ny = 0;
    rtmi_temporal_params params{};
    DeviceArena mem; // one allocation, carved in 256-B aligned pieces
    RtmiTemporalHistory hist;
    float *d_lin = nullptr, *d_alb = nullptr, *d_nrm = nullptr, *d_dep = nullptr, *d_se = nullptr;
    float *o_lin = nullptr, *o_se = nullptr, *o_hist = nullptr;
    float2 *o_motion = nullptr;
    hipStream_t stream = nullptr;
    bool with_se = false;
};

#define TP_TRY(fn, expr) RTMI_HIP_TRY(fn ": ", false, expr, #expr)

static int temporal_alloc(rtmi_temporal *h) {
    TP_TRY("rtmi_temporal_create", hipSetDevice(h->device));
    const size_t n = (size_t)h->nx * h->ny;
    const auto layout = [&](Carve256 &c) {
        rtmi_temporal_history_layout(h->hist, c, h->nx, h->ny);
        h->d_lin = c.take<float>(n * 3);
        h->d_alb = c.take<float>(n * 3);
        h->d_nrm = c.take<float>(n * 3);
        h->d_se = c.take<float>(n * 3);
        h->o_lin = c.take<float>(n * 3);
        h->o_se = c.take<float>(n * 3);
        h->d_dep = c.take<float>(n);
        h->o_hist = c.take<float>(n);
        h->o_motion = c.take<float2>(n);
    };
    TP_TRY("rtmi_temporal_create", h->mem.alloc(layout));
    TP_TRY("rtmi_temporal_create", hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    return RTMI_OK;
}

extern "C" void rtmi_temporal_destroy(rtmi_temporal *h) {
    if (!h) return;
    if (h->mem.base || h->stream) (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    h->mem.release();
    delete h;
}

extern "C" int rtmi_temporal_create(int device, uint32_t nx, uint32_t ny, const rtmi_temporal_params *p, rtmi_temporal **out) {
    // every argument check comes before the first HIP call
    if (out) *out = nullptr;
    if (!p || !out) return rtmi_fail(RTMI_ERR_INVALID, "rtmi_temporal_create: NULL argument");
    int rc = check_params(nx, ny, p);
    if (rc) return rc;
    rc = device_ok("rtmi_temporal_create: ", device);
    if (rc) return rc;
    rtmi_temporal *h = new (std::nothrow) rtmi_temporal;
    if (!h) return rtmi_fail(RTMI_ERR_NOMEM, "rtmi_temporal_create: out of host memory");
    h->device = device;
    h->nx = nx;
    h->ny = ny;
    h->params = *p;
    rc = temporal_alloc(h);
    if (rc) {
        rtmi_temporal_destroy(h);
        return rc;
    }
    *out = h;
    return RTMI_OK;
}

extern "C" int rtmi_temporal_reset(rtmi_temporal *h) {
    if (!h) return rtmi_fail(RTMI_ERR_INVALID, "rtmi_temporal_reset: NULL handle");
    h->hist.has_prev = false;
    return RTMI_OK;
}

// ---- the device half, shared with the frame handle (rtmi_frame_launch.hpp) --------------------------------------------
void rtmi_temporal_history_layout(RtmiTemporalHistory &H, Carve256 &c, uint32_t nx, uint32_t ny) {
    const size_t n = (size_t)nx * ny;
    for (int k = 0; k < 2; k++) {
        H.col[k] = c.take<float4>(n);
        H.geo[k] = c.take<float4>(n);
        H.var[k] = c.take<float4>(n);
    }
}

int rtmi_temporal_check_ranges(const char *name, uint32_t nx, uint32_t ny, const rtmi_temporal_params *p) {
    return check_ranges(name, nx, ny, p);
}

int rtmi_temporal_camera_matrix(const char *name, const rtmi_camera *cam, float m[9]) {
    float fields[sizeof(rtmi_camera) / sizeof(float)];
    static_assert(sizeof(rtmi_camera) == 84, "rtmi_camera is 21 floats");
    memcpy(fields, cam, sizeof(rtmi_camera));
    for (float f : fields)
        if (!finite_f(f)) return fail(RTMI_ERR_INVALID, name, "non-finite camera field");
    if (!camera_inverse(cam, m)) return fail(RTMI_ERR_INVALID, name, "singular camera (horizontal, vertical and the corner are coplanar)");
    return RTMI_OK;
}

hipError_t rtmi_temporal_push_launch(hipStream_t stream, uint32_t nx, uint32_t ny, const rtmi_temporal_params &params,
                                     const RtmiTemporalHistory &H, const rtmi_camera *cam, const float *linear, const float *albedo,
                                     const float *normal, const float *depth, const float *se, float *out_linear, float *out_se,
                                     float *out_hist, float2 *out_motion) {
    TemporalPush P{};
    P.nx = nx;
    P.ny = ny;
    P.has_prev = H.has_prev;
    P.same_cam = H.has_prev && memcmp(&H.prev_cam, cam, sizeof(rtmi_camera)) == 0;
    P.demodulate = !(params.flags & RTMI_TEMPORAL_NO_DEMODULATE);
    P.max_history = (float)params.max_history;
    P.alpha_min = params.alpha_min;
    P.depth_tol = params.depth_tol;
    P.normal_min = params.normal_min;
    P.albedo_min = params.albedo_min;
    for (int k = 0; k < 3; k++) {
        P.org[k] = cam->origin[k];
        P.llc[k] = cam->lower_left_corner[k];
        P.hor[k] = cam->horizontal[k];
        P.ver[k] = cam->vertical[k];
        P.porg[k] = H.prev_cam.origin[k];
    }
    memcpy(P.m, H.prev_m, sizeof(P.m));
    const int src = H.cur, dst = H.cur ^ 1;
    const dim3 block(kBlock, kBlock), grid((nx + kBlock - 1) / kBlock, (ny + kBlock - 1) / kBlock);
    if (se)
        hipLaunchKernelGGL(rtmi_temporal_push_kernel<true>, grid, block, 0, stream, linear, albedo, normal, depth, se, H.col[src],
                           H.geo[src], H.var[src], H.col[dst], H.geo[dst], H.var[dst], out_linear, out_se, out_hist, out_motion, P);
    else
        hipLaunchKernelGGL(rtmi_temporal_push_kernel<false>, grid, block, 0, stream, linear, albedo, normal, depth, se, H.col[src],
                           H.geo[src], H.var[src], H.col[dst], H.geo[dst], H.var[dst], out_linear, out_se, out_hist, out_motion, P);
    return hipGetLastError();
}

void rtmi_temporal_history_advance(RtmiTemporalHistory &H, const rtmi_camera *cam, const float m[9]) {
    H.cur ^= 1;
    H.has_prev = true;
    H.prev_cam = *cam;
    memcpy(H.prev_m, m, 9 * sizeof(float));
}

// the staging copies around one push
static int temporal_run(rtmi_temporal *h, const rtmi_camera *cam, const float *linear, const float *albedo, const float *normal,
                        const float *depth, const float *se, float *out_linear, float *out_stderr, float *out_history,
                        float *out_motion) {
    const size_t n = (size_t)h->nx * h->ny;
    hipStream_t s = h->stream;
    TP_TRY("rtmi_temporal_push", hipSetDevice(h->device));
    TP_TRY("rtmi_temporal_push", hipMemcpyAsync(h->d_lin, linear, n * 12, hipMemcpyHostToDevice, s));
    if (!(h->params.flags & RTMI_TEMPORAL_NO_DEMODULATE))
        TP_TRY("rtmi_temporal_push", hipMemcpyAsync(h->d_alb, albedo, n * 12, hipMemcpyHostToDevice, s));
    TP_TRY("rtmi_temporal_push", hipMemcpyAsync(h->d_nrm, normal, n * 12, hipMemcpyHostToDevice, s));
    TP_TRY("rtmi_temporal_push", hipMemcpyAsync(h->d_dep, depth, n * 4, hipMemcpyHostToDevice, s));
    if (se) TP_TRY("rtmi_temporal_push", hipMemcpyAsync(h->d_se, se, n * 12, hipMemcpyHostToDevice, s));
    TP_TRY("rtmi_temporal_push", rtmi_temporal_push_launch(s, h->nx, h->ny, h->params, h->hist, cam, h->d_lin, h->d_alb, h->d_nrm,
                                                           h->d_dep, se ? h->d_se : nullptr, h->o_lin, h->o_se, h->o_hist,
                                                           h->o_motion));
    if (out_linear) TP_TRY("rtmi_temporal_push", hipMemcpyAsync(out_linear, h->o_lin, n * 12, hipMemcpyDeviceToHost, s));
    if (out_stderr) TP_TRY("rtmi_temporal_push", hipMemcpyAsync(out_stderr, h->o_se, n * 12, hipMemcpyDeviceToHost, s));
    if (out_history) TP_TRY("rtmi_temporal_push", hipMemcpyAsync(out_history, h->o_hist, n * 4, hipMemcpyDeviceToHost, s));
    if (out_motion) TP_TRY("rtmi_temporal_push", hipMemcpyAsync(out_motion, h->o_motion, n * 8, hipMemcpyDeviceToHost, s));
    TP_TRY("rtmi_temporal_push", hipStreamSynchronize(s));
    return RTMI_OK;
}

extern "C" int rtmi_temporal_push(rtmi_temporal *h, const rtmi_camera *cam, const float *linear, const float *albedo,
                                  const float *normal, const float *depth, const float *stderr_rgb, float *out_linear,
                                  float *out_stderr, float *out_history, float *out_motion) {
    // every argument check comes before the first HIP call; the handle comes last, so that a machine without a device
    // (where no handle can exist) still answers for every other argument
    if (!cam || !linear || !albedo || !normal || !depth) return rtmi_fail(RTMI_ERR_INVALID, "rtmi_temporal_push: NULL argument");
    float m[9];
    if (int rc = rtmi_temporal_camera_matrix("rtmi_temporal_push", cam, m)) return rc;
    if (out_stderr && !stderr_rgb) return rtmi_fail(RTMI_ERR_INVALID, "rtmi_temporal_push: out_stderr needs stderr_rgb");
    if (!h) return rtmi_fail(RTMI_ERR_INVALID, "rtmi_temporal_push: NULL handle");
    const bool with_se = stderr_rgb != nullptr;
    if (h->hist.has_prev && with_se != h->with_se)
        return rtmi_fail(RTMI_ERR_INVALID, "rtmi_temporal_push: stderr_rgb must be supplied on every push since the reset or on none");
    const int rc = temporal_run(h, cam, linear, albedo, normal, depth, stderr_rgb, out_linear, out_stderr, out_history, out_motion);
    if (rc) {
        h->hist.has_prev = false;
        return rc;
    }
    rtmi_temporal_history_advance(h->hist, cam, m);
    h->with_se = with_se;
    return RTMI_OK;
}
