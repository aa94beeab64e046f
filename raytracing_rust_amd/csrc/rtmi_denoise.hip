// rtmi_denoise.hip — translation unit of the a-trous denoiser (include/rtmi_denoise.h): three kernels and the blocking
// host entry point.  Compiled with the flags of rtmi_device.hip (-ffp-contract=off, no fast-math, IEEE / and sqrt,
// denormals kept), so tests/denoise_ref.py restates every output bit for bit.  See DESIGN.md §13.
//
// Device layout, per pixel (row-major, row 0 = top):
//   state  float4 {x_r, x_g, x_b, var}, two buffers that the iterations ping-pong between
//   guide  float4 {n_x, n_y, n_z, z}: constant; z non-finite = not a surface pixel
//   grad   float2 {gx, gy}: constant
// A non-surface pixel's state is never written nor read: taps skip it and the finish copies its linear input.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "rtmi.h"
#include "rtmi_math.h"
#include "rtmi_denoise.h"
#include "rtmi_frame_launch.hpp"
#include "rtmi_hostkit.hpp"
#include "rtmi_image_dev.hpp"

namespace {

constexpr int kBlock = 16; // 16x16 workgroups: a wavefront is 16 columns x 4 rows, so neighbouring taps share L1 lines

struct DenoiseIter {
    uint32_t nx, ny;
    int step;          // s = 2^i
    int squarings;     // log2(normal_power)
    int normal_on;     // normal_power != 0
    float sigma_l, sigma_z, eps_l, eps_z;
};

__device__ __forceinline__ float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// one lane per pixel: demodulated colour and variance, the guide and the depth gradient
__global__ __launch_bounds__(256) void rtmi_denoise_prepass_kernel(const float *__restrict__ linear,
                                                                   const float *__restrict__ albedo,
                                                                   const float *__restrict__ normal,
                                                                   const float *__restrict__ depth,
                                                                   const float *__restrict__ se, float4 *__restrict__ state,
                                                                   float4 *__restrict__ guide, float2 *__restrict__ grad,
                                                                   uint32_t nx, uint32_t ny, float albedo_min) {
    const uint32_t x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y * kBlock + threadIdx.y;
    if (x >= nx || y >= ny) return;
    const size_t p = (size_t)y * nx + x;
    const float z = depth[p];
    guide[p] = make_float4(normal[p * 3], normal[p * 3 + 1], normal[p * 3 + 2], z);
    if (!surface(z)) return;
    float a[3], xc[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        a[c] = fmaxf(albedo[p * 3 + c], albedo_min);
        xc[c] = linear[p * 3 + c] / a[c];
    }
    float var = 0.0f;
    if (se) {
        const float sr = 0.2126f * (se[p * 3] / a[0]), sg = 0.7152f * (se[p * 3 + 1] / a[1]),
                    sb = 0.0722f * (se[p * 3 + 2] / a[2]);
        var = (sr * sr + sg * sg) + sb * sb;
    }
    state[p] = make_float4(xc[0], xc[1], xc[2], var);
    // central difference when both neighbours are surface pixels, else the one-sided one that exists, else 0
    const auto diff = [&](bool has_m, size_t qm, bool has_p, size_t qp) {
        const bool m = has_m && surface(depth[qm]), pl = has_p && surface(depth[qp]);
        if (m && pl) return 0.5f * (depth[qp] - depth[qm]);
        if (pl) return depth[qp] - z;
        if (m) return z - depth[qm];
        return 0.0f;
    };
    const float gx = diff(x > 0, p - (x > 0), x + 1 < nx, p + (x + 1 < nx));
    const float gy = diff(y > 0, p - (y > 0 ? nx : 0), y + 1 < ny, p + (y + 1 < ny ? nx : 0));
    grad[p] = make_float2(gx, gy);
}

// One a-trous iteration at step s: the 3x3 variance prefilter, then the 25 weighted taps.  Sums in tap order, skipped
// taps left out (not added with a zero weight).
template <bool LUM>
__global__ __launch_bounds__(256) void rtmi_denoise_iter_kernel(const float4 *__restrict__ src, float4 *__restrict__ dst,
                                                                const float4 *__restrict__ guide,
                                                                const float2 *__restrict__ grad, DenoiseIter P) {
    const int x = (int)(blockIdx.x * kBlock + threadIdx.x), y = (int)(blockIdx.y * kBlock + threadIdx.y);
    const int nx = (int)P.nx, ny = (int)P.ny;
    if (x >= nx || y >= ny) return;
    const size_t p = (size_t)y * nx + x;
    const float4 gp = guide[p];
    if (!surface(gp.w)) return;
    const float4 sp = src[p];
    const float2 g = grad[p];
    const float lenp = (gp.x * gp.x + gp.y * gp.y) + gp.z * gp.z;
    float inv_l = 0.0f, lp = 0.0f;
    if (LUM) {
        constexpr float k3[3] = {0.25f, 0.5f, 0.25f};
        float kv = 0.0f, ks = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const int qx = x + dx, qy = y + dy;
                if (qx < 0 || qx >= nx || qy < 0 || qy >= ny) continue;
                const size_t q = (size_t)qy * nx + qx;
                if (!surface(guide[q].w)) continue;
                const float k = k3[dy + 1] * k3[dx + 1];
                kv = kv + k * src[q].w;
                ks = ks + k;
            }
        }
        const float gv = kv / ks;
        inv_l = 1.0f / (P.sigma_l * sqrtf(gv) + P.eps_l);
        lp = lum(sp.x, sp.y, sp.z);
    }
    constexpr float k5[5] = {1.0f / 16.0f, 0.25f, 0.375f, 0.25f, 1.0f / 16.0f};
    const int s = P.step;
    float W = 0.0f, Cr = 0.0f, Cg = 0.0f, Cb = 0.0f, V = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + s * dx, qy = y + s * dy;
            if (qx < 0 || qx >= nx || qy < 0 || qy >= ny) continue;
            const size_t q = (size_t)qy * nx + qx;
            const float4 gq = guide[q];
            if (!surface(gq.w)) continue;
            const float4 sq = src[q];
            const float h = k5[dy + 2] * k5[dx + 2];
            float w = h;
            if (dx != 0 || dy != 0) {
                float wn = 1.0f;
                if (P.normal_on) {
                    const float lenq = (gq.x * gq.x + gq.y * gq.y) + gq.z * gq.z;
                    if (lenp != 0.0f && lenq != 0.0f) {
                        wn = fmaxf((gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z, 0.0f);
                        for (int k = 0; k < P.squarings; k++) wn = wn * wn;
                    }
                }
                const float dz = fabsf(gp.w - gq.w) /
                                 (P.sigma_z * (fabsf(g.x * (float)(s * dx)) + fabsf(g.y * (float)(s * dy))) + P.eps_z);
                const float dl = LUM ? fabsf(lp - lum(sq.x, sq.y, sq.z)) * inv_l : 0.0f;
                w = (h * wn) * rtmi_expf(-(dl + dz));
            }
            W = W + w;
            Cr = Cr + w * sq.x;
            Cg = Cg + w * sq.y;
            Cb = Cb + w * sq.z;
            V = V + (w * w) * sq.w;
        }
    }
    dst[p] = make_float4(Cr / W, Cg / W, Cb / W, V / (W * W));
}

// remodulation (surface pixels) or the copy of linear (the others, and every pixel when copy_all), then the quantiser
// of rtmi_resolve_kernel
__global__ __launch_bounds__(256) void rtmi_denoise_finish_kernel(const float4 *__restrict__ state,
                                                                  const float *__restrict__ linear,
                                                                  const float *__restrict__ albedo,
                                                                  const float *__restrict__ depth, float *__restrict__ out,
                                                                  uint8_t *__restrict__ rgb8, uint32_t n, float albedo_min,
                                                                  int copy_all) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    float o[3] = {linear[(size_t)p * 3], linear[(size_t)p * 3 + 1], linear[(size_t)p * 3 + 2]};
    if (!copy_all && surface(depth[p])) {
        const float4 st = state[p];
        o[0] = st.x * fmaxf(albedo[(size_t)p * 3], albedo_min);
        o[1] = st.y * fmaxf(albedo[(size_t)p * 3 + 1], albedo_min);
        o[2] = st.z * fmaxf(albedo[(size_t)p * 3 + 2], albedo_min);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        out[(size_t)p * 3 + c] = o[c];
        double g = sqrt((double)o[c]);
        g = (g > 0.0) ? ((g < 1.0) ? g : 1.0) : 0.0; // NaN -> 0
        const double v = 255.99 * g;
        rgb8[(size_t)p * 3 + c] = (uint8_t)(int32_t)v;
    }
}

__global__ void rtmi_expf_probe_kernel(const float *x, float *out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = rtmi_expf(x[i]);
}

// the RTMI_ERR_INVALID checks, each message after `pre` (empty for rtmi_denoise, the entry's name for the frame handle)
int check_ranges(const std::string &pre, uint32_t nx, uint32_t ny, const rtmi_denoise_params *p) {
    const auto bad = [&](const char *msg) { return rtmi_fail(RTMI_ERR_INVALID, (pre + msg).c_str()); };
    if (nx == 0 || ny == 0 || nx > 32768u || ny > 32768u) return bad("nx and ny must be in [1, 32768]");
    if (p->iterations > 10u) return bad("iterations must be in [0, 10]");
    if (p->normal_power > 1024u || (p->normal_power & (p->normal_power - 1u)))
        return bad("normal_power must be 0 or a power of two <= 1024");
    if (!finite_f(p->sigma_l) || !(p->sigma_l >= 0.0f) || !finite_f(p->sigma_z) || !(p->sigma_z >= 0.0f))
        return bad("sigma_l and sigma_z must be finite and >= 0");
    if (!finite_f(p->eps_l) || !(p->eps_l > 0.0f) || !finite_f(p->eps_z) || !(p->eps_z > 0.0f) ||
        !finite_f(p->albedo_min) || !(p->albedo_min > 0.0f))
        return bad("eps_l, eps_z and albedo_min must be finite and > 0");
    return RTMI_OK;
}

int check_params(uint32_t nx, uint32_t ny, const rtmi_denoise_params *p) {
    if (int rc = check_ranges("", nx, ny, p)) return rc;
    if (p->flags) return rtmi_fail(RTMI_ERR_UNSUPPORTED, "flags must be 0 (reserved)");
    return RTMI_OK;
}

#define DN_TRY(expr) RTMI_HIP_TRY("", false, expr, #expr)

} // namespace

// ---- the device half, shared with the frame handle (rtmi_frame_launch.hpp) --------------------------------------------
int rtmi_denoise_check_ranges(const char *prefix, uint32_t nx, uint32_t ny, const rtmi_denoise_params *p) {
    return check_ranges(prefix, nx, ny, p);
}

void rtmi_denoise_layout(RtmiDenoisePlanes &W, Carve256 &c, uint32_t nx, uint32_t ny, uint32_t iterations) {
    if (iterations == 0) return;
    const size_t n = (size_t)nx * ny;
    W.state[0] = c.take<float4>(n);
    W.state[1] = c.take<float4>(n);
    W.guide = c.take<float4>(n);
    W.grad = c.take<float2>(n);
}

hipError_t rtmi_denoise_launch(hipStream_t stream, uint32_t nx, uint32_t ny, const rtmi_denoise_params &p, const float *linear,
                               const float *albedo, const float *normal, const float *depth, const float *se,
                               const RtmiDenoisePlanes &W, float *out, uint8_t *rgb8) {
    const size_t n = (size_t)nx * ny;
    const bool lum = se != nullptr, filter = p.iterations > 0;
    hipError_t e;
    int cur = 0;
    if (filter) {
        const dim3 block(kBlock, kBlock), grid((nx + kBlock - 1) / kBlock, (ny + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(rtmi_denoise_prepass_kernel, grid, block, 0, stream, linear, albedo, normal, depth, se, W.state[0],
                           W.guide, W.grad, nx, ny, p.albedo_min);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        DenoiseIter P{nx, ny, 1, normal_squarings(p.normal_power), p.normal_power != 0u, p.sigma_l, p.sigma_z, p.eps_l, p.eps_z};
        for (uint32_t i = 0; i < p.iterations; i++, cur ^= 1) {
            P.step = 1 << i;
            if (lum)
                hipLaunchKernelGGL(rtmi_denoise_iter_kernel<true>, grid, block, 0, stream, W.state[cur], W.state[cur ^ 1], W.guide, W.grad, P);
            else
                hipLaunchKernelGGL(rtmi_denoise_iter_kernel<false>, grid, block, 0, stream, W.state[cur], W.state[cur ^ 1], W.guide, W.grad, P);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
    }
    hipLaunchKernelGGL(rtmi_denoise_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, W.state[cur], linear,
                       albedo, depth, out, rgb8, (uint32_t)n, p.albedo_min, filter ? 0 : 1);
    return hipGetLastError();
}

extern "C" int rtmi_denoise(int device, uint32_t nx, uint32_t ny, const rtmi_denoise_params *p, const float *linear,
                            const float *albedo, const float *normal, const float *depth, const float *stderr_rgb,
                            float *out_linear, uint8_t *out_rgb8) {
    // every argument check comes before the first HIP call
    if (!p || !linear || !albedo || !normal || !depth) return rtmi_fail(RTMI_ERR_INVALID, "NULL argument");
    int rc = check_params(nx, ny, p);
    if (rc) return rc;
    rc = device_ok("", device);
    if (rc) return rc;
    if (!out_linear && !out_rgb8) return RTMI_OK;
    DN_TRY(hipSetDevice(device));
    const size_t n = (size_t)nx * ny;
    const bool lum = stderr_rgb != nullptr, filter = p->iterations > 0;
    float *d_lin, *d_alb, *d_nrm, *d_dep, *d_se = nullptr, *d_out;
    uint8_t *d_rgb;
    RtmiDenoisePlanes W;
    const auto layout = [&](Carve256 &c) {
        d_lin = c.take<float>(n * 3);
        d_alb = c.take<float>(n * 3);
        d_nrm = c.take<float>(n * 3);
        d_dep = c.take<float>(n);
        if (lum) d_se = c.take<float>(n * 3);
        rtmi_denoise_layout(W, c, nx, ny, p->iterations);
        d_out = c.take<float>(n * 3);
        d_rgb = c.take<uint8_t>(n * 3);
    };
    DeviceArena mem;
    DN_TRY(mem.alloc(layout));
    DeviceStream S;
    DN_TRY(S.create());
    DN_TRY(hipMemcpyAsync(d_lin, linear, n * 12, hipMemcpyHostToDevice, S.s));
    DN_TRY(hipMemcpyAsync(d_alb, albedo, n * 12, hipMemcpyHostToDevice, S.s));
    DN_TRY(hipMemcpyAsync(d_dep, depth, n * 4, hipMemcpyHostToDevice, S.s));
    if (filter) {
        DN_TRY(hipMemcpyAsync(d_nrm, normal, n * 12, hipMemcpyHostToDevice, S.s));
        if (lum) DN_TRY(hipMemcpyAsync(d_se, stderr_rgb, n * 12, hipMemcpyHostToDevice, S.s));
    }
    DN_TRY(rtmi_denoise_launch(S.s, nx, ny, *p, d_lin, d_alb, d_nrm, d_dep, d_se, W, d_out, d_rgb));
    if (out_linear) DN_TRY(hipMemcpyAsync(out_linear, d_out, n * 12, hipMemcpyDeviceToHost, S.s));
    if (out_rgb8) DN_TRY(hipMemcpyAsync(out_rgb8, d_rgb, n * 3, hipMemcpyDeviceToHost, S.s));
    DN_TRY(hipStreamSynchronize(S.s));
    return RTMI_OK;
}

extern "C" int rtmi_probe_expf(int device, const float *x, float *out, uint32_t n) {
    if (n > 0 && (!x || !out)) return rtmi_fail(RTMI_ERR_INVALID, "NULL argument");
    int rc = device_ok("", device);
    if (rc) return rc;
    if (n == 0) return RTMI_OK;
    DN_TRY(hipSetDevice(device));
    float *dx, *dout;
    const auto layout = [&](Carve256 &c) {
        dx = c.take<float>(n);
        dout = c.take<float>(n);
    };
    DeviceArena mem;
    DN_TRY(mem.alloc(layout));
    DN_TRY(hipMemcpy(dx, x, (size_t)n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(rtmi_expf_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, dx, dout, n);
    DN_TRY(hipGetLastError());
    DN_TRY(hipMemcpy(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RTMI_OK;
}
