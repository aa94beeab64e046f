// rtmi_upscale.hip — translation unit of guided upscaling (include/rtmi_upscale.h): the reconstruction kernel, the two
// stateless entries and the handle that renders a low-resolution frame and the full-resolution features and reconstructs.
// The low frame is a public rtmi_frame; the full-resolution features and the hold on the scene are reached through the
// seams of rtmi_frame_launch.hpp, as they are.  Compiled with the flags of rtmi_tonemap.hip (-ffp-contract=off, no
// fast-math, IEEE / and sqrt, denormals kept), so tests/upscale_ref.py restates every output bit for bit.  See DESIGN.md §30.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>

#include "rtmi.h"
#include "rtmi_upscale.h"
#include "rtmi_light_coop.h"
#include "rtmi_frame_launch.hpp"
#include "rtmi_hostkit.hpp"
#include "rtmi_image_dev.hpp"

namespace {

constexpr int kBlock = 256; // 256 lanes, four pixels per lane

// what one reconstruction reads beside the guide, and its constants
struct UpscaleArgs {
    const float *lin_lo, *alb_lo, *nrm_lo, *z_lo;
    uint32_t lx, ly, nx, n; // n = nx*ny
    float sx, sy;
    float sigma_z, eps_z, albedo_min, w_min;
    int squarings; // log2(normal_power)
    int normal_on; // normal_power != 0
};

__device__ __forceinline__ uint32_t quantise(float v) {
    double g = sqrt((double)v);
    g = (g > 0.0) ? ((g < 1.0) ? g : 1.0) : 0.0; // NaN -> 0
    return (uint32_t)(uint8_t)(int32_t)(255.99 * g);
}

// Where the taps come from.  `at` is a tap's index, then one read per value.
struct GlobalTaps { // the low-resolution planes, dword gathers through the cache
    const float *lin_lo, *alb_lo, *nrm_lo, *z_lo;
    uint32_t lx;
    __device__ __forceinline__ size_t at(int qx, int qy) const { return (size_t)qy * lx + (size_t)qx; }
    __device__ __forceinline__ float z(size_t q) const { return z_lo[q]; }
    __device__ __forceinline__ float lin(size_t q, int c) const { return lin_lo[q * 3 + c]; }
    __device__ __forceinline__ float alb(size_t q, int c) const { return alb_lo[q * 3 + c]; }
    __device__ __forceinline__ float nrm(size_t q, int c) const { return nrm_lo[q * 3 + c]; }
};
struct LdsTaps { // a workgroup's footprint [r0, r0+h) x [c0, c0+w) of the low image, ten planes of `cap` floats each in LDS
    const float *s;
    int c0, r0, w, cap;
    __device__ __forceinline__ size_t at(int qx, int qy) const { return (size_t)((qy - r0) * w + (qx - c0)); }
    __device__ __forceinline__ float z(size_t q) const { return s[9 * cap + q]; }
    __device__ __forceinline__ float lin(size_t q, int c) const { return s[c * cap + q]; }
    __device__ __forceinline__ float alb(size_t q, int c) const { return s[(3 + c) * cap + q]; }
    __device__ __forceinline__ float nrm(size_t q, int c) const { return s[(6 + c) * cap + q]; }
};

// Steps 1 to 4 of the header for the pixel (x, y) with the guide values a (albedo), nr (normal) and zp (depth): o = out,
// the return value its class.  The taps' loads are dword gathers through the cache: the lanes of a wavefront cover 256
// consecutive pixels of a row, so at a ratio of 2 they share 130 low-resolution pixels of each of two rows.
template <class Taps>
__device__ __forceinline__ uint32_t upscale_pixel(const UpscaleArgs &A, const Taps &T, uint32_t x, uint32_t y, const float a[3], const float nr[3],
                                                  float zp, float o[3]) {
    const float fx = ((float)x + 0.5f) * A.sx - 0.5f, fy = ((float)y + 0.5f) * A.sy - 0.5f;
    const int x0 = (int)floorf(fx), y0 = (int)floorf(fy);
    const float tx = fx - (float)x0, ty = fy - (float)y0;
    const float wx[2] = {1.0f - tx, tx}, wy[2] = {1.0f - ty, ty};
    const bool surf = __builtin_isfinite(zp);
    const float lenp = (nr[0] * nr[0] + nr[1] * nr[1]) + nr[2] * nr[2];
    const float zden = A.sigma_z * zp + A.eps_z;
    float B = 0.0f, R[3] = {0.0f, 0.0f, 0.0f};  // every tap: the plain bilinear mean (class 3)
    float W = 0.0f, C[3] = {0.0f, 0.0f, 0.0f};  // the taps of p's kind: (w, w*x) of a surface p, (b, b*linear) of a background p
    float best_e = 0.0f, best[3] = {0.0f, 0.0f, 0.0f};
    bool have = false; // a tap of p's kind exists
#pragma unroll
    for (int j = 0; j < 2; j++) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int qx = x0 + i, qy = y0 + j;
            if (qx < 0 || qx >= (int)A.lx || qy < 0 || qy >= (int)A.ly) continue;
            const float b = wy[j] * wx[i];
            if (b == 0.0f) continue;
            const size_t q = T.at(qx, qy);
            const float zq = T.z(q);
            const float l[3] = {T.lin(q, 0), T.lin(q, 1), T.lin(q, 2)};
            B = B + b;
            R[0] = R[0] + b * l[0];
            R[1] = R[1] + b * l[1];
            R[2] = R[2] + b * l[2];
            const bool sq = __builtin_isfinite(zq);
            if (surf && sq) {
                const float xq[3] = {l[0] / fmaxf(T.alb(q, 0), A.albedo_min), l[1] / fmaxf(T.alb(q, 1), A.albedo_min),
                                     l[2] / fmaxf(T.alb(q, 2), A.albedo_min)};
                float wn = 1.0f;
                if (A.normal_on) {
                    const float n0 = T.nrm(q, 0), n1 = T.nrm(q, 1), n2 = T.nrm(q, 2);
                    const float lenq = (n0 * n0 + n1 * n1) + n2 * n2;
                    if (lenp != 0.0f && lenq != 0.0f) {
                        wn = fmaxf((nr[0] * n0 + nr[1] * n1) + nr[2] * n2, 0.0f);
                        for (int k = 0; k < A.squarings; k++) wn = wn * wn;
                    }
                }
                const float dz = fabsf(zp - zq) / zden;
                const float e = wn * rtmi_expf(-dz);
                const float w = b * e;
                W = W + w;
                C[0] = C[0] + w * xq[0];
                C[1] = C[1] + w * xq[1];
                C[2] = C[2] + w * xq[2];
                if (!have || e > best_e) {
                    best_e = e;
                    best[0] = xq[0];
                    best[1] = xq[1];
                    best[2] = xq[2];
                }
                have = true;
            } else if (!surf && !sq) {
                W = W + b;
                C[0] = C[0] + b * l[0];
                C[1] = C[1] + b * l[1];
                C[2] = C[2] + b * l[2];
                have = true;
            }
        }
    }
    if (!have) {
        o[0] = R[0] / B;
        o[1] = R[1] / B;
        o[2] = R[2] / B;
        return RTMI_UPSCALE_MISMATCH;
    }
    if (!surf) {
        o[0] = C[0] / W;
        o[1] = C[1] / W;
        o[2] = C[2] / W;
        return RTMI_UPSCALE_BACKGROUND;
    }
    const float ap[3] = {fmaxf(a[0], A.albedo_min), fmaxf(a[1], A.albedo_min), fmaxf(a[2], A.albedo_min)};
    if (W > A.w_min) {
        o[0] = (C[0] / W) * ap[0];
        o[1] = (C[1] / W) * ap[1];
        o[2] = (C[2] / W) * ap[2];
        return RTMI_UPSCALE_GUIDED;
    }
    o[0] = best[0] * ap[0];
    o[1] = best[1] * ap[1];
    o[2] = best[2] * ap[2];
    return RTMI_UPSCALE_NEAREST;
}

// The four pixels of group g (pixels 4g .. 4g+3 of the packed image, the first at (x, y)): with WIDE seven 16-byte loads of
// the guide, else dword loads; three 16-byte stores of linear, one 12-byte store of rgb8 and one 4-byte store of cls.
// Whether an output is written is a uniform branch on its pointer.
template <bool WIDE, class Taps>
__device__ __forceinline__ void upscale_group(const UpscaleArgs &A, const Taps &T, uint32_t g, uint32_t x, uint32_t y,
                                              const float *__restrict__ albedo, const float *__restrict__ normal,
                                              const float *__restrict__ depth, float *__restrict__ out_linear,
                                              uint8_t *__restrict__ out_rgb8, uint8_t *__restrict__ out_cls) {
    float al[12], nr[12], z[4];
    if (WIDE) {
        const float4 *pa = reinterpret_cast<const float4 *>(albedo) + (size_t)g * 3;
        const float4 *pn = reinterpret_cast<const float4 *>(normal) + (size_t)g * 3;
        const float4 a0 = pa[0], a1 = pa[1], a2 = pa[2], n0 = pn[0], n1 = pn[1], n2 = pn[2];
        const float4 z4 = reinterpret_cast<const float4 *>(depth)[g];
        const float ta[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
        const float tn[12] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w, n2.x, n2.y, n2.z, n2.w};
#pragma unroll
        for (int k = 0; k < 12; k++) {
            al[k] = ta[k];
            nr[k] = tn[k];
        }
        z[0] = z4.x;
        z[1] = z4.y;
        z[2] = z4.z;
        z[3] = z4.w;
    } else {
#pragma unroll
        for (int k = 0; k < 12; k++) {
            al[k] = albedo[(size_t)g * 12 + k];
            nr[k] = normal[(size_t)g * 12 + k];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) z[k] = depth[(size_t)g * 4 + k];
    }
    float o[12];
    Bytes12 q = {{0u, 0u, 0u}};
    uint32_t cls = 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t c = upscale_pixel(A, T, x, y, al + 3 * k, nr + 3 * k, z[k], o + 3 * k);
        cls |= c << (8 * k);
        if (++x == A.nx) {
            x = 0u;
            y++;
        }
    }
    if (out_linear) {
        float4 *po = reinterpret_cast<float4 *>(out_linear) + (size_t)g * 3;
        po[0] = make_float4(o[0], o[1], o[2], o[3]);
        po[1] = make_float4(o[4], o[5], o[6], o[7]);
        po[2] = make_float4(o[8], o[9], o[10], o[11]);
    }
    if (out_rgb8) {
#pragma unroll
        for (int k = 0; k < 12; k++) q.w[k >> 2] |= quantise(o[k]) << (8 * (k & 3));
        *reinterpret_cast<Bytes12 *>(out_rgb8 + (size_t)g * 12) = q;
    }
    if (out_cls) reinterpret_cast<uint32_t *>(out_cls)[g] = cls;
}

// one pixel p = (x, y) with dword and byte accesses
template <class Taps>
__device__ __forceinline__ void upscale_single(const UpscaleArgs &A, const Taps &T, uint32_t p, uint32_t x, uint32_t y,
                                               const float *__restrict__ albedo, const float *__restrict__ normal,
                                               const float *__restrict__ depth, float *__restrict__ out_linear,
                                               uint8_t *__restrict__ out_rgb8, uint8_t *__restrict__ out_cls) {
    const float a[3] = {albedo[(size_t)p * 3], albedo[(size_t)p * 3 + 1], albedo[(size_t)p * 3 + 2]};
    const float nr[3] = {normal[(size_t)p * 3], normal[(size_t)p * 3 + 1], normal[(size_t)p * 3 + 2]};
    float o[3];
    const uint32_t c = upscale_pixel(A, T, x, y, a, nr, depth[p], o);
    for (int k = 0; k < 3; k++) {
        if (out_linear) out_linear[(size_t)p * 3 + k] = o[k];
        if (out_rgb8) out_rgb8[(size_t)p * 3 + k] = (uint8_t)quantise(o[k]);
    }
    if (out_cls) out_cls[p] = (uint8_t)c;
}

// The direct variant.  A lane takes four consecutive pixels of the packed image (of one row, except where a row ends inside
// the four), so a wavefront reads 7168 contiguous bytes of the guide and writes runs of 3072, 768 and 256.  Counting the
// four in the packed order keeps every access aligned at any nx.  Without WIDE (a guide that is not 16-byte aligned: the
// scene's feature planes when nx*ny is not a multiple of four) the guide is read dword by dword; the outputs are the
// handle's own and stay wide.  The lane after the last whole group takes the n % 4 pixels of the tail one by one.  The taps
// are gathered from global memory through the cache.
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void rtmi_upscale_kernel(UpscaleArgs A, const float *__restrict__ albedo,
                                                             const float *__restrict__ normal, const float *__restrict__ depth,
                                                             float *__restrict__ out_linear, uint8_t *__restrict__ out_rgb8,
                                                             uint8_t *__restrict__ out_cls) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x, groups = A.n >> 2;
    const GlobalTaps T{A.lin_lo, A.alb_lo, A.nrm_lo, A.z_lo, A.lx};
    if (g < groups) {
        const uint32_t y = (g * 4u) / A.nx, x = g * 4u - y * A.nx;
        upscale_group<WIDE>(A, T, g, x, y, albedo, normal, depth, out_linear, out_rgb8, out_cls);
    } else if (g == groups) {
        for (uint32_t p = groups * 4u; p < A.n; p++) {
            const uint32_t y = p / A.nx;
            upscale_single(A, T, p, p - y * A.nx, y, albedo, normal, depth, out_linear, out_rgb8, out_cls);
        }
    }
}

constexpr int kTileLanes = 64, kTileRows = 4; // the staged variant: a workgroup is 256 x 4 pixels, a lane four of a row

__device__ __forceinline__ int tap_floor(uint32_t x, float s) { return (int)floorf(((float)x + 0.5f) * s - 0.5f); }

// The staged variant.  A workgroup takes a tile of 256 x 4 full-resolution pixels, a lane four consecutive pixels of a row.
// The tile's taps lie in columns tap_floor(first x) .. tap_floor(last x) + 1 and the rows alike (the tap position is
// monotone in x), clipped to the low image: that footprint is copied to LDS first, ten planes (linear, albedo, normal,
// depth) of `cap` floats, each lane copying whole low pixels with coalesced dword loads, and the taps are then read from
// LDS.  The arithmetic is upscale_pixel's, so the bits are the direct variant's.  WIDE needs aligned planes and nx a multiple
// of four (a row's groups are then groups of the packed image); otherwise, and in a row's last partial group, a lane
// goes pixel by pixel.  A footprint larger than the host allowed for (cols x rows; it cannot be, see upscale_launch) would
// be read from global memory instead: the branch is uniform.
template <bool WIDE>
__global__ __launch_bounds__(kTileLanes * kTileRows) void rtmi_upscale_staged_kernel(UpscaleArgs A, const float *__restrict__ albedo,
                                                                                   const float *__restrict__ normal,
                                                                                   const float *__restrict__ depth,
                                                                                   float *__restrict__ out_linear,
                                                                                   uint8_t *__restrict__ out_rgb8,
                                                                                   uint8_t *__restrict__ out_cls, int cols, int rows) {
    extern __shared__ float stage[];
    const uint32_t ny = A.n / A.nx;
    const uint32_t xb = blockIdx.x * (kTileLanes * 4), yb = blockIdx.y * kTileRows;
    const uint32_t xe = min(xb + kTileLanes * 4 - 1u, A.nx - 1u), ye = min(yb + kTileRows - 1u, ny - 1u);
    const int c0 = max(tap_floor(xb, A.sx), 0), c1 = min(tap_floor(xe, A.sx) + 1, (int)A.lx - 1);
    const int r0 = max(tap_floor(yb, A.sy), 0), r1 = min(tap_floor(ye, A.sy) + 1, (int)A.ly - 1);
    const int w = c1 - c0 + 1, h = r1 - r0 + 1, cap = cols * rows;
    const bool fits = w <= cols && h <= rows;
    if (fits) {
        for (int i = (int)(threadIdx.y * kTileLanes + threadIdx.x); i < w * h; i += kTileLanes * kTileRows) {
            const int qy = r0 + i / w, qx = c0 + i % w;
            const size_t q = (size_t)qy * A.lx + (size_t)qx;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                stage[c * cap + i] = A.lin_lo[q * 3 + c];
                stage[(3 + c) * cap + i] = A.alb_lo[q * 3 + c];
                stage[(6 + c) * cap + i] = A.nrm_lo[q * 3 + c];
            }
            stage[9 * cap + i] = A.z_lo[q];
        }
    }
    __syncthreads();
    const uint32_t y = yb + threadIdx.y, x = xb + threadIdx.x * 4u;
    if (y >= ny || x >= A.nx) return;
    const uint32_t p = y * A.nx + x;
    const LdsTaps L{stage, c0, r0, w, cap};
    const GlobalTaps G{A.lin_lo, A.alb_lo, A.nrm_lo, A.z_lo, A.lx};
    if (WIDE && x + 3u < A.nx) {
        if (fits)
            upscale_group<true>(A, L, p >> 2, x, y, albedo, normal, depth, out_linear, out_rgb8, out_cls);
        else
            upscale_group<true>(A, G, p >> 2, x, y, albedo, normal, depth, out_linear, out_rgb8, out_cls);
    } else {
        for (uint32_t k = 0; k < 4u && x + k < A.nx; k++) {
            if (fits)
                upscale_single(A, L, p + k, x + k, y, albedo, normal, depth, out_linear, out_rgb8, out_cls);
            else
                upscale_single(A, G, p + k, x + k, y, albedo, normal, depth, out_linear, out_rgb8, out_cls);
        }
    }
}

// the RTMI_ERR_INVALID checks of the two sizes and a parameter block, in `name`'s words; the flags are the caller's
int check_sizes(const char *name, uint32_t lx, uint32_t ly, uint32_t nx, uint32_t ny) {
    if (lx == 0 || ly == 0 || nx > 32768u || ny > 32768u || lx > nx || ly > ny)
        return fail(RTMI_ERR_INVALID, name, "the sizes must satisfy 1 <= lx <= nx <= 32768 and 1 <= ly <= ny <= 32768");
    return RTMI_OK;
}
int check_ranges(const char *name, const rtmi_upscale_params *p) {
    if (p->normal_power > 1024u || (p->normal_power & (p->normal_power - 1u)))
        return fail(RTMI_ERR_INVALID, name, "normal_power must be 0 or a power of two <= 1024");
    if (!finite_f(p->sigma_z) || !(p->sigma_z >= 0.0f)) return fail(RTMI_ERR_INVALID, name, "sigma_z must be finite and >= 0");
    if (!finite_f(p->eps_z) || !(p->eps_z > 0.0f)) return fail(RTMI_ERR_INVALID, name, "eps_z must be finite and > 0");
    if (!finite_f(p->albedo_min) || !(p->albedo_min > 0.0f)) return fail(RTMI_ERR_INVALID, name, "albedo_min must be finite and > 0");
    if (!finite_f(p->w_min) || !(p->w_min >= 0.0f)) return fail(RTMI_ERR_INVALID, name, "w_min must be finite and >= 0");
    if (p->reserved[0] || p->reserved[1]) return fail(RTMI_ERR_INVALID, name, "reserved must be 0");
    return RTMI_OK;
}

// the checks the two stateless forms share, up to the device
int check_call(const char *name, uint32_t lx, uint32_t ly, uint32_t nx, uint32_t ny, const rtmi_upscale_params *p,
               const rtmi_upscale_in *in, const rtmi_upscale_out *out, bool device_form) {
    if (!p || !in || !out) return fail(RTMI_ERR_INVALID, name, "NULL argument");
    if (!in->linear_lo || !in->albedo_lo || !in->normal_lo || !in->depth_lo || !in->albedo || !in->normal || !in->depth)
        return fail(RTMI_ERR_INVALID, name, "NULL input plane");
    int rc;
    if ((rc = check_sizes(name, lx, ly, nx, ny)) || (rc = check_ranges(name, p))) return rc;
    if (in->reserved || out->reserved) return fail(RTMI_ERR_INVALID, name, "reserved pointer must be NULL");
    if (!out->linear && !out->rgb8 && !out->cls) return fail(RTMI_ERR_INVALID, name, "every output is NULL");
    if (device_form) {
        const uintptr_t f = (uintptr_t)in->linear_lo | (uintptr_t)in->albedo_lo | (uintptr_t)in->normal_lo | (uintptr_t)in->depth_lo |
                            (uintptr_t)in->albedo | (uintptr_t)in->normal | (uintptr_t)in->depth | (uintptr_t)out->linear;
        if ((f & 15u) || (((uintptr_t)out->rgb8 | (uintptr_t)out->cls) & 3u))
            return fail(RTMI_ERR_INVALID, name, "misaligned pointer (the float planes need 16 bytes, rgb8 and cls 4)");
    }
    if (p->flags) return fail(RTMI_ERR_UNSUPPORTED, name, "flags must be 0 (reserved)");
    return RTMI_OK;
}

constexpr size_t kStageLimit = 64 * 1024; // the LDS a workgroup of the staged variant may take

// RTMI_UPSCALE_VARIANT = "direct" or "staged" picks the kernel for the measurements and the tests; unset: the default.
int variant_from_env() {
    const char *v = std::getenv("RTMI_UPSCALE_VARIANT");
    if (v && !std::strcmp(v, "direct")) return 1;
    if (v && !std::strcmp(v, "staged")) return 2;
    return 0;
}

// The one launch of a reconstruction on `s`; nothing here allocates, waits or copies.  The low-resolution planes need 4-byte
// alignment only; the guide is read wide when all three of its planes are 16-byte aligned; linear needs 16 bytes, rgb8 and
// cls 4.  The staged variant is the default wherever its footprint fits kStageLimit (it is the faster one, DESIGN.md §30:
// 55 against 82 us at 1920x1080 from 960x540); a ratio below about 1.13 does not fit and takes the direct one.
hipError_t upscale_launch(hipStream_t s, uint32_t lx, uint32_t ly, uint32_t nx, uint32_t ny, const rtmi_upscale_params &p,
                          const float *lin_lo, const float *alb_lo, const float *nrm_lo, const float *z_lo, const float *albedo,
                          const float *normal, const float *depth, float *out_linear, uint8_t *out_rgb8, uint8_t *out_cls) {
    UpscaleArgs A{lin_lo, alb_lo, nrm_lo, z_lo, lx, ly, nx, nx * ny, (float)lx / (float)nx, (float)ly / (float)ny,
                  p.sigma_z, p.eps_z, p.albedo_min, p.w_min, normal_squarings(p.normal_power), p.normal_power != 0u};
    const bool wide = !(((uintptr_t)albedo | (uintptr_t)normal | (uintptr_t)depth) & 15u);
    // the staged variant's footprint: over 256 columns the tap position advances by 255*sx, its floor by less than that
    // plus 1, and the taps reach one column further: at most (int)(255*sx) + 3 columns, and one more for the fp32 roundings
    const int cols = (int)(255.0f * A.sx) + 4, rows = (int)((float)(kTileRows - 1) * A.sy) + 4;
    const size_t lds = (size_t)cols * rows * 10 * sizeof(float);
    const int variant = variant_from_env();
    const bool staged = lds <= kStageLimit && variant != 1;
    if (staged) {
        const dim3 block(kTileLanes, kTileRows), grid((nx + kTileLanes * 4 - 1) / (kTileLanes * 4), (ny + kTileRows - 1) / kTileRows);
        if (wide && nx % 4u == 0u)
            hipLaunchKernelGGL(rtmi_upscale_staged_kernel<true>, grid, block, lds, s, A, albedo, normal, depth, out_linear, out_rgb8,
                               out_cls, cols, rows);
        else
            hipLaunchKernelGGL(rtmi_upscale_staged_kernel<false>, grid, block, lds, s, A, albedo, normal, depth, out_linear, out_rgb8,
                               out_cls, cols, rows);
        return hipGetLastError();
    }
    const uint32_t lanes = (A.n >> 2) + ((A.n & 3u) ? 1u : 0u);
    const dim3 grid((lanes + kBlock - 1) / kBlock);
    if (wide)
        hipLaunchKernelGGL(rtmi_upscale_kernel<true>, grid, dim3(kBlock), 0, s, A, albedo, normal, depth, out_linear, out_rgb8, out_cls);
    else
        hipLaunchKernelGGL(rtmi_upscale_kernel<false>, grid, dim3(kBlock), 0, s, A, albedo, normal, depth, out_linear, out_rgb8, out_cls);
    return hipGetLastError();
}

#define UP_TRY(name, expr) RTMI_HIP_TRY(std::string(name) + ": ", true, expr, #expr)

// The flags that go to the lit render only and that the features render does not take: RTMI_FLAG_LIGHT_COOP and bit 11, the
// cooperative render's unnamed small-pool test knob (rtmi_device.hip reads it as 1u << 11; rtmi_frame.hip strips the same two).
const uint32_t kCoopFlags = RTMI_FLAG_LIGHT_COOP | (1u << 11);

// a refusal of the low frame's entry `theirs`, said again in `name`'s words with its code
int renamed(int rc, const char *name, const char *theirs) {
    const char *m = rtmi_last_error();
    std::string msg = m ? m : "";
    const std::string prefix = std::string(theirs) + ": ";
    if (msg.compare(0, prefix.size(), prefix) == 0) msg.erase(0, prefix.size());
    return rtmi_fail(rc, (std::string(name) + ": " + msg).c_str());
}

} // namespace

extern "C" int rtmi_upscale_device(int device, uint32_t lx, uint32_t ly, uint32_t nx, uint32_t ny, const rtmi_upscale_params *p,
                                   const rtmi_upscale_in *in, const rtmi_upscale_out *out, void *stream) {
    // every argument check comes before the first HIP call
    const char *name = "rtmi_upscale_device";
    int rc;
    if ((rc = check_call(name, lx, ly, nx, ny, p, in, out, true)) || (rc = device_ok(std::string(name) + ": ", device))) return rc;
    UP_TRY(name, hipSetDevice(device));
    UP_TRY(name, upscale_launch(static_cast<hipStream_t>(stream), lx, ly, nx, ny, *p, in->linear_lo, in->albedo_lo, in->normal_lo,
                                in->depth_lo, in->albedo, in->normal, in->depth, out->linear, out->rgb8, out->cls));
    return RTMI_OK;
}

extern "C" int rtmi_upscale(int device, uint32_t lx, uint32_t ly, uint32_t nx, uint32_t ny, const rtmi_upscale_params *p,
                            const rtmi_upscale_in *in, const rtmi_upscale_out *out) {
    const char *name = "rtmi_upscale";
    int rc;
    if ((rc = check_call(name, lx, ly, nx, ny, p, in, out, false)) || (rc = device_ok(std::string(name) + ": ", device))) return rc;
    UP_TRY(name, hipSetDevice(device));
    const size_t nl = (size_t)lx * ly, n = (size_t)nx * ny;
    float *d_lin_lo, *d_alb_lo, *d_nrm_lo, *d_z_lo, *d_alb, *d_nrm, *d_z, *d_lin;
    uint8_t *d_rgb, *d_cls;
    const auto layout = [&](Carve256 &c) {
        d_lin_lo = c.take<float>(nl * 3);
        d_alb_lo = c.take<float>(nl * 3);
        d_nrm_lo = c.take<float>(nl * 3);
        d_z_lo = c.take<float>(nl);
        d_alb = c.take<float>(n * 3);
        d_nrm = c.take<float>(n * 3);
        d_z = c.take<float>(n);
        d_lin = c.take<float>(n * 3);
        d_rgb = c.take<uint8_t>(n * 3);
        d_cls = c.take<uint8_t>(n);
    };
    DeviceArena mem;
    UP_TRY(name, mem.alloc(layout));
    UP_TRY(name, hipMemcpy(d_lin_lo, in->linear_lo, nl * 12, hipMemcpyHostToDevice));
    UP_TRY(name, hipMemcpy(d_alb_lo, in->albedo_lo, nl * 12, hipMemcpyHostToDevice));
    UP_TRY(name, hipMemcpy(d_nrm_lo, in->normal_lo, nl * 12, hipMemcpyHostToDevice));
    UP_TRY(name, hipMemcpy(d_z_lo, in->depth_lo, nl * 4, hipMemcpyHostToDevice));
    UP_TRY(name, hipMemcpy(d_alb, in->albedo, n * 12, hipMemcpyHostToDevice));
    UP_TRY(name, hipMemcpy(d_nrm, in->normal, n * 12, hipMemcpyHostToDevice));
    UP_TRY(name, hipMemcpy(d_z, in->depth, n * 4, hipMemcpyHostToDevice));
    UP_TRY(name, upscale_launch(nullptr, lx, ly, nx, ny, *p, d_lin_lo, d_alb_lo, d_nrm_lo, d_z_lo, d_alb, d_nrm, d_z,
                                out->linear ? d_lin : nullptr, out->rgb8 ? d_rgb : nullptr, out->cls ? d_cls : nullptr));
    if (out->linear) UP_TRY(name, hipMemcpy(out->linear, d_lin, n * 12, hipMemcpyDeviceToHost));
    if (out->rgb8) UP_TRY(name, hipMemcpy(out->rgb8, d_rgb, n * 3, hipMemcpyDeviceToHost));
    if (out->cls) UP_TRY(name, hipMemcpy(out->cls, d_cls, n, hipMemcpyDeviceToHost));
    return RTMI_OK;
}

// ---- the handle -----------------------------------------------------------------------------------------------------
struct RTMI_HIDDEN rtmi_upscaler {
    std::mutex mu; // one render or reset at a time: the two steps of a render take the scene's hold one after the other
    rtmi_scene *s = nullptr;
    rtmi_frame *low = nullptr;
    rtmi_render_params p{}; // the full size; ns and seed are set per call
    rtmi_upscaler_opts o{};
    DeviceArena mem; // one allocation, carved in 256-B aligned pieces
    float *lo_lin = nullptr, *lo_alb = nullptr, *lo_nrm = nullptr, *lo_z = nullptr;
    float *out_lin = nullptr;
    uint8_t *out_rgb = nullptr, *out_cls = nullptr;
};

extern "C" void rtmi_upscaler_destroy(rtmi_upscaler *h) {
    if (!h) return;
    if (h->low) rtmi_frame_destroy(h->low); // under the scene's lock, after its running work
    if (h->mem.base) {
        RtmiFrameHold *hold = nullptr;
        const RtmiFrameLit plain{"rtmi_upscaler_destroy", false, false, 1.0f};
        (void)rtmi_frame_hold_begin(h->s, plain, &hold);
        h->mem.release();
        rtmi_frame_hold_end(hold);
    }
    delete h;
}

extern "C" int rtmi_upscaler_create(rtmi_scene *s, const rtmi_render_params *p_in, const rtmi_upscaler_opts *o, rtmi_upscaler **out) {
    // every argument check comes before the first use of the scene (and of the device)
    const char *name = "rtmi_upscaler_create";
    if (out) *out = nullptr;
    if (!p_in || !o || !out) return fail(RTMI_ERR_INVALID, name, "NULL argument");
    int rc;
    if ((rc = check_sizes(name, o->lx, o->ly, p_in->nx, p_in->ny)) || (rc = check_ranges(name, &o->up))) return rc;
    if (o->guide_ns == 0u) return fail(RTMI_ERR_INVALID, name, "guide_ns must be at least 1");
    for (uint32_t r : o->reserved)
        if (r) return fail(RTMI_ERR_INVALID, name, "reserved must be 0");
    if (o->up.flags) return fail(RTMI_ERR_UNSUPPORTED, name, "up.flags must be 0 (reserved)");
    if (o->guide_ns >= (1u << 26)) return fail(RTMI_ERR_UNSUPPORTED, name, "guide_ns must be below 2^26");

    rtmi_upscaler *h = new (std::nothrow) rtmi_upscaler;
    if (!h) return fail(RTMI_ERR_NOMEM, name, "out of host memory");
    h->p = *p_in;
    h->p.ns = o->guide_ns;
    h->p.seed = 0u;
    h->p.flags &= ~kCoopFlags; // the features render takes no cooperative flag
    h->o = *o;
    rtmi_render_params pl = *p_in;
    pl.nx = o->lx;
    pl.ny = o->ly;
    if ((rc = rtmi_frame_create(s, &pl, &o->low, &h->low))) {
        rc = renamed(rc, name, "rtmi_frame_create");
        delete h;
        return rc;
    }
    h->s = s;
    const auto alloc = [&]() -> int {
        const size_t nl = (size_t)o->lx * o->ly, n = (size_t)h->p.nx * h->p.ny;
        const auto layout = [&](Carve256 &c) {
            h->lo_lin = c.take<float>(nl * 3);
            h->lo_alb = c.take<float>(nl * 3);
            h->lo_nrm = c.take<float>(nl * 3);
            h->lo_z = c.take<float>(nl);
            h->out_lin = c.take<float>(n * 3);
            h->out_rgb = c.take<uint8_t>(n * 3);
            h->out_cls = c.take<uint8_t>(n);
        };
        RtmiFrameHold *hold = nullptr; // the scene's device, under its lock
        const RtmiFrameLit plain{name, false, false, 1.0f};
        if (int r = rtmi_frame_hold_begin(s, plain, &hold)) return r;
        const hipError_t e = h->mem.alloc(layout);
        rtmi_frame_hold_end(hold);
        UP_TRY(name, e);
        return RTMI_OK;
    };
    if ((rc = alloc())) {
        rtmi_upscaler_destroy(h);
        return rc;
    }
    *out = h;
    return RTMI_OK;
}

extern "C" int rtmi_upscaler_reset(rtmi_upscaler *h) {
    if (!h) return rtmi_fail(RTMI_ERR_INVALID, "rtmi_upscaler_reset: NULL handle");
    std::lock_guard<std::mutex> lock(h->mu);
    return rtmi_frame_reset(h->low);
}

// step 2 of a render call, under the hold: the full-resolution features, the reconstruction on the scene's stream, the
// copies of the planes asked for and the final synchronise
static int upscaler_rebuild(rtmi_upscaler *h, const char *name, RtmiFrameHold *hold, const rtmi_camera *cam,
                            const rtmi_render_params &pf, const rtmi_upscaler_out &out, hipMemcpyKind kind) {
    if (int rc = rtmi_frame_enqueue_first_hits(hold, cam, pf)) return renamed(rc, name, name);
    const RtmiFramePlanes R = rtmi_frame_planes(hold, pf);
    hipStream_t st = R.stream;
    const size_t nl = (size_t)h->o.lx * h->o.ly, n = (size_t)pf.nx * pf.ny;
    UP_TRY(name, upscale_launch(st, h->o.lx, h->o.ly, pf.nx, pf.ny, h->o.up, h->lo_lin, h->lo_alb, h->lo_nrm, h->lo_z, R.albedo,
                                R.normal, R.depth, h->out_lin, h->out_rgb, h->out_cls));
    const auto copy = [&](void *dst, const void *src, size_t bytes) {
        return dst ? hipMemcpyAsync(dst, src, bytes, kind, st) : hipSuccess;
    };
    UP_TRY(name, copy(out.linear, h->out_lin, n * 12));
    UP_TRY(name, copy(out.rgb8, h->out_rgb, n * 3));
    UP_TRY(name, copy(out.cls, h->out_cls, n));
    UP_TRY(name, copy(out.albedo, R.albedo, n * 12));
    UP_TRY(name, copy(out.normal, R.normal, n * 12));
    UP_TRY(name, copy(out.depth, R.depth, n * 4));
    UP_TRY(name, copy(out.low.linear, h->lo_lin, nl * 12));
    UP_TRY(name, copy(out.low.albedo, h->lo_alb, nl * 12));
    UP_TRY(name, copy(out.low.normal, h->lo_nrm, nl * 12));
    UP_TRY(name, copy(out.low.depth, h->lo_z, nl * 4));
    UP_TRY(name, hipStreamSynchronize(st));
    return RTMI_OK;
}

static int upscaler_render(const char *name, rtmi_upscaler *h, const rtmi_camera *cam, uint32_t ns, uint64_t seed,
                           const rtmi_upscaler_out *out, rtmi_stats *stats, bool device_form) {
    if (!cam || !out) return fail(RTMI_ERR_INVALID, name, "NULL argument");
    const rtmi_frame_out &lo = out->low;
    if (!device_form && (lo.rgb8 || lo.noisy_linear || lo.noisy_stderr || lo.hits || lo.accum_linear || lo.accum_stderr || lo.history ||
                         lo.motion))
        return fail(RTMI_ERR_INVALID, name, "the host form copies linear, albedo, normal and depth of the low frame only");
    // Step 1.  The low frame into the handle's planes; the other planes of the low frame straight to the caller's device
    // pointers.  Its entry makes the remaining argument checks, the NULL handle last.
    std::unique_lock<std::mutex> lock;
    if (h) lock = std::unique_lock<std::mutex>(h->mu);
    rtmi_frame_out fo{};
    if (device_form) fo = lo;
    fo.linear = h ? h->lo_lin : nullptr;
    fo.albedo = h ? h->lo_alb : nullptr;
    fo.normal = h ? h->lo_nrm : nullptr;
    fo.depth = h ? h->lo_z : nullptr;
    int rc;
    if ((rc = rtmi_frame_render_device(h ? h->low : nullptr, cam, ns, seed, &fo, stats)))
        return renamed(rc, name, "rtmi_frame_render_device");
    // Step 2, under one hold on the scene.
    rtmi_render_params pf = h->p;
    pf.seed = seed;
    const RtmiFrameLit plain{name, false, false, 1.0f};
    RtmiFrameHold *hold = nullptr;
    if (!(rc = rtmi_frame_hold_begin(h->s, plain, &hold)))
        rc = upscaler_rebuild(h, name, hold, cam, pf, *out, device_form ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost);
    rtmi_frame_hold_end(hold);
    if (rc) (void)rtmi_frame_reset(h->low); // the frame just rendered went into a history whose image was not delivered
    return rc;
}

extern "C" int rtmi_upscaler_render(rtmi_upscaler *h, const rtmi_camera *cam, uint32_t ns, uint64_t seed, const rtmi_upscaler_out *out,
                                    rtmi_stats *stats) {
    return upscaler_render("rtmi_upscaler_render", h, cam, ns, seed, out, stats, false);
}

extern "C" int rtmi_upscaler_render_device(rtmi_upscaler *h, const rtmi_camera *cam, uint32_t ns, uint64_t seed,
                                           const rtmi_upscaler_out *out, rtmi_stats *stats) {
    return upscaler_render("rtmi_upscaler_render_device", h, cam, ns, seed, out, stats, true);
}
