// rtmi_tonemap.hip — translation unit of the tone mapper (include/rtmi_tonemap.h): the metering, solve and apply kernels
// and the host entry points.  Compiled with the flags of rtmi_temporal.hip (-ffp-contract=off, no fast-math, IEEE / and
// sqrt, denormals kept), so tests/tonemap_ref.py restates every output bit for bit.  See DESIGN.md §29.
//
// Device memory of a handle: 256 uint32 bins and one 64-byte record (the rtmi_tonemap_state of the last apply and whether
// an adapted value exists).  The bins are zero between applies: create zeroes them and every solve zeroes them again.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <new>
#include <string>

#include "rtmi.h"
#include "rtmi_tonemap.h"
#include "rtmi_hostkit.hpp"
#include "rtmi_image_dev.hpp"

namespace {

constexpr int kBins = 256;
constexpr int kBlock = 256;         // apply: 256 lanes, four pixels per lane
constexpr int kMeterBlock = 1024;   // meter: 1024 lanes, four pixels per lane and trip
constexpr uint32_t kMeterCap = 256; // the meter grid's cap: one workgroup per CU; one trip covers 2^20 pixels

// the device record: the state reported by the last apply, then what the next solve needs beside it
struct TonemapDev {
    rtmi_tonemap_state st;
    uint32_t has_adapted; // st.adapted_log2 is an adapted value (a metered frame has been seen since create or reset)
    uint32_t pad[7];
};
static_assert(sizeof(rtmi_tonemap_state) == 32 && sizeof(rtmi_tonemap_params) == 64 && sizeof(TonemapDev) == 64, "layout");

struct TonemapSolve {
    float log2_min, log2_max, p_low, p_high, speed_up, speed_down, adapt_min, adapt_max, key, ev;
    float dt;
    float e_manual; // MANUAL: E, computed on the host
    int autoexp;    // RTMI_TONEMAP_AUTO
    int fresh;      // the first apply after create or reset
};

__device__ __forceinline__ int bin_of(float r, float g, float b, float log2_min, float scale) {
    const float l = (0.2126f * r + 0.7152f * g) + 0.0722f * b;
    if (!(__builtin_isfinite(l) && l > 0.0f)) return -1;
    const float e = rtmi_logf(l) * 1.44269504f;
    const float t = (e - log2_min) * scale;
    return t < 0.0f ? 0 : (t >= 256.0f ? 255 : (int)t);
}

// Step 1.  One histogram per workgroup in LDS, not one per wavefront: what costs in an LDS atomic is lanes of one
// instruction meeting in a bin, which a copy per wavefront does not thin, and a copy each would multiply the flush.  The
// flush is what bounds the kernel: every workgroup adds its 256 totals to the same 256 words, so the workgroups are few
// and large (sixteen wavefronts, one workgroup per CU at the cap).
// A lane reads four pixels as three 16-byte loads; the n % 4 pixels of the tail go to the first lanes of workgroup 0.
__global__ __launch_bounds__(kMeterBlock) void rtmi_tonemap_meter_kernel(const float *__restrict__ linear,
                                                                        uint32_t *__restrict__ bins, uint32_t n, float log2_min,
                                                                        float scale) {
    __shared__ uint32_t hist[kBins];
    if (threadIdx.x < kBins) hist[threadIdx.x] = 0u;
    __syncthreads();
    const auto count = [&](float r, float g, float b) {
        const int k = bin_of(r, g, b, log2_min, scale);
        if (k >= 0) atomicAdd(&hist[k], 1u);
    };
    const uint32_t groups = n >> 2, stride = gridDim.x * kMeterBlock;
    for (uint32_t g = blockIdx.x * kMeterBlock + threadIdx.x; g < groups; g += stride) {
        const float4 *p = reinterpret_cast<const float4 *>(linear) + (size_t)g * 3;
        const float4 a = p[0], b = p[1], c = p[2];
        count(a.x, a.y, a.z);
        count(a.w, b.x, b.y);
        count(b.z, b.w, c.x);
        count(c.y, c.z, c.w);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3u)) {
        const float *p = linear + ((size_t)groups * 4 + threadIdx.x) * 3;
        count(p[0], p[1], p[2]);
    }
    __syncthreads();
    if (threadIdx.x < kBins) {
        const uint32_t v = hist[threadIdx.x];
        if (v) atomicAdd(&bins[threadIdx.x], v); // device scope; integer, so the order of arrival does not show
    }
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

// Step 2, one wavefront: a lane owns four consecutive bins, the counts below them come from a wave scan, lane 0 does the
// scalar rest and writes the record (and the caller's copy).  The counts fit 32 bits (nx*ny <= 2^30); lo, hi, K and S are
// 64-bit as the header writes them.  MANUAL runs the same kernel for the record alone.
__global__ __launch_bounds__(64) void rtmi_tonemap_solve_kernel(uint32_t *__restrict__ bins, TonemapDev *__restrict__ dev,
                                                               rtmi_tonemap_state *__restrict__ out_state, TonemapSolve A) {
    const int lane = (int)threadIdx.x;
    uint64_t n = 0, K = 0, S = 0;
    if (A.autoexp) {
        uint4 *mine = reinterpret_cast<uint4 *>(bins) + lane;
        const uint4 c4 = *mine;
        *mine = make_uint4(0u, 0u, 0u, 0u);
        const uint32_t c[4] = {c4.x, c4.y, c4.z, c4.w};
        const uint32_t own = (c[0] + c[1]) + (c[2] + c[3]);
        uint32_t incl = own;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
            if (lane >= d) incl += up;
        }
        n = (uint64_t)(uint32_t)__shfl((int)incl, 63, 64);
        if (n) {
            uint64_t lo = (uint64_t)((double)n * (double)A.p_low), hi = (uint64_t)((double)n * (double)A.p_high);
            if (hi == lo) {
                if (lo == n) lo = n - 1;
                hi = lo + 1;
            }
            K = hi - lo;
            uint64_t below = incl - own, s = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint64_t top = below + c[j];
                const int64_t k = (int64_t)(top < hi ? top : hi) - (int64_t)(below > lo ? below : lo);
                if (k > 0) s += (uint64_t)k * (uint64_t)(4 * lane + j);
                below = top;
            }
            S = wave_sum_u64(s);
        }
    }
    if (lane != 0) return;
    const bool has = dev->has_adapted != 0u && !A.fresh;
    const float a = dev->st.adapted_log2;
    rtmi_tonemap_state st;
    st.applies = (A.fresh ? 0u : dev->st.applies) + 1u;
    st.reserved[0] = st.reserved[1] = 0u;
    uint32_t has_next = 0u;
    if (!A.autoexp) {
        st.exposure = A.e_manual;
        st.adapted_log2 = st.metered_log2 = 0.0f;
        st.counted = st.kept = 0u;
    } else {
        float a2, m;
        if (n == 0) {
            a2 = has ? a : 0.0f;
            m = a2;
            has_next = has ? 1u : 0u;
        } else {
            m = (float)((double)A.log2_min +
                        ((double)S / (double)K + 0.5) * (((double)A.log2_max - (double)A.log2_min) / 256.0));
            if (!has) {
                a2 = m;
            } else {
                const float s = (m > a) ? A.speed_up : A.speed_down;
                const float al = 1.0f - rtmi_expf(-(A.dt * s));
                a2 = a + (m - a) * al;
            }
            a2 = fminf(fmaxf(a2, A.adapt_min), A.adapt_max);
            has_next = 1u;
        }
        st.exposure = A.key * rtmi_expf((A.ev - a2) * 0.69314718f);
        st.adapted_log2 = a2;
        st.metered_log2 = m;
        st.counted = (uint32_t)n;
        st.kept = (uint32_t)K;
    }
    dev->st = st;
    dev->has_adapted = has_next;
    if (out_state) *out_state = st;
}

// the curve and the transfer function of one channel: q = the byte, d = the display value
template <uint32_t OP, uint32_t OETF>
__device__ __forceinline__ void tone(float x, float w2, uint32_t &q, float &d) {
    float y = x;
    if (OP != RTMI_TONEMAP_CLAMP) {
        x = fmaxf(x, 0.0f);
        if (OP == RTMI_TONEMAP_REINHARD)
            y = (x * (1.0f + x / w2)) / (1.0f + x);
        else
            y = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
    }
    if (OETF == RTMI_TONEMAP_GAMMA2) {
        double g = sqrt((double)y);
        g = (g > 0.0) ? ((g < 1.0) ? g : 1.0) : 0.0; // NaN -> 0
        q = (uint32_t)(uint8_t)(int32_t)(255.99 * g);
        d = (float)g;
    } else {
        const float v = (y > 0.0f) ? ((y < 1.0f) ? y : 1.0f) : 0.0f; // NaN -> 0
        const float s = (v <= 0.0031308f) ? 12.92f * v : fminf(1.055f * rtmi_expf(rtmi_logf(v) * 0.41666667f) - 0.055f, 1.0f);
        q = (uint32_t)(uint8_t)(int32_t)(s * 255.0f + 0.5f);
        d = s;
    }
}

// Step 3.  A lane takes four consecutive pixels: three 16-byte loads, one 12-byte store of rgb8 and three 16-byte stores of
// display, so a wavefront reads 3072 contiguous bytes and writes runs of 768 and 3072.  The operator and the transfer function
// are template parameters: the six bodies differ by an f64 sqrt against a log and an exp per channel, and a kernel that held
// both would carry the registers of the larger for every setting; the host picks the instantiation once per apply.  E is
// one scalar load for the wavefront.  The lane after the last whole group takes the n % 4 pixels of the tail one by one.
template <uint32_t OP, uint32_t OETF>
__global__ __launch_bounds__(kBlock) void rtmi_tonemap_apply_kernel(const float *__restrict__ linear,
                                                                   const TonemapDev *__restrict__ dev,
                                                                   uint8_t *__restrict__ rgb8, float *__restrict__ display,
                                                                   uint32_t n, float w2) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x, groups = n >> 2;
    const float E = dev->st.exposure;
    if (g < groups) {
        const float4 *p = reinterpret_cast<const float4 *>(linear) + (size_t)g * 3;
        const float4 a = p[0], b = p[1], c = p[2];
        const float x[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
        float d[12];
        Bytes12 out = {{0u, 0u, 0u}};
#pragma unroll
        for (int k = 0; k < 12; k++) {
            uint32_t q;
            tone<OP, OETF>(x[k] * E, w2, q, d[k]);
            out.w[k >> 2] |= q << (8 * (k & 3));
        }
        if (rgb8) *reinterpret_cast<Bytes12 *>(rgb8 + (size_t)g * 12) = out;
        if (display) {
            float4 *o = reinterpret_cast<float4 *>(display) + (size_t)g * 3;
            o[0] = make_float4(d[0], d[1], d[2], d[3]);
            o[1] = make_float4(d[4], d[5], d[6], d[7]);
            o[2] = make_float4(d[8], d[9], d[10], d[11]);
        }
    } else if (g == groups) {
        for (size_t k = (size_t)groups * 12; k < (size_t)n * 3; k++) {
            uint32_t q;
            float d;
            tone<OP, OETF>(linear[k] * E, w2, q, d);
            if (rgb8) rgb8[k] = (uint8_t)q;
            if (display) display[k] = d;
        }
    }
}

// the RTMI_ERR_INVALID and RTMI_ERR_UNSUPPORTED checks of a size and a parameter block, in `name`'s words
int check_params(const char *name, uint32_t nx, uint32_t ny, const rtmi_tonemap_params *p) {
    const auto bad = [&](const char *msg) { return fail(RTMI_ERR_INVALID, name, msg); };
    if (nx == 0 || ny == 0 || nx > 32768u || ny > 32768u) return bad("nx and ny must be in [1, 32768]");
    if (p->op > RTMI_TONEMAP_ACES) return bad("op must be RTMI_TONEMAP_CLAMP, _REINHARD or _ACES");
    if (p->oetf > RTMI_TONEMAP_SRGB) return bad("oetf must be RTMI_TONEMAP_GAMMA2 or _SRGB");
    if (p->exposure > RTMI_TONEMAP_AUTO) return bad("exposure must be RTMI_TONEMAP_MANUAL or _AUTO");
    if (!finite_f(p->ev) || !(p->ev >= -64.0f && p->ev <= 64.0f)) return bad("ev must be finite and in [-64, 64]");
    if (!(p->white > 0.0f)) return bad("white must be > 0 (+inf allowed)");
    if (!finite_f(p->key) || !(p->key > 0.0f)) return bad("key must be finite and > 0");
    if (!finite_f(p->log2_min)) return bad("log2_min must be finite");
    if (!finite_f(p->log2_max) || !(p->log2_max - p->log2_min >= 1.0f)) return bad("log2_max must be finite and >= log2_min + 1");
    if (!(p->p_low >= 0.0f && p->p_low < 1.0f)) return bad("p_low must be in [0, 1)");
    if (!(p->p_high > p->p_low && p->p_high <= 1.0f)) return bad("p_high must be in (p_low, 1]");
    if (!finite_f(p->speed_up) || !(p->speed_up >= 0.0f)) return bad("speed_up must be finite and >= 0");
    if (!finite_f(p->speed_down) || !(p->speed_down >= 0.0f)) return bad("speed_down must be finite and >= 0");
    if (!finite_f(p->adapt_min)) return bad("adapt_min must be finite");
    if (!finite_f(p->adapt_max) || !(p->adapt_max >= p->adapt_min)) return bad("adapt_max must be finite and >= adapt_min");
    if (p->reserved) return bad("reserved must be 0");
    if (p->flags) return fail(RTMI_ERR_UNSUPPORTED, name, "flags must be 0 (reserved)");
    return RTMI_OK;
}

hipError_t meter_launch(hipStream_t s, const float *d_linear, uint32_t *d_bins, uint32_t n, const rtmi_tonemap_params &p) {
    const float scale = 256.0f / (p.log2_max - p.log2_min);
    const uint32_t groups = n >> 2, want = (groups + kMeterBlock - 1) / kMeterBlock;
    const uint32_t grid = want < 1u ? 1u : (want > kMeterCap ? kMeterCap : want);
    hipLaunchKernelGGL(rtmi_tonemap_meter_kernel, dim3(grid), dim3(kMeterBlock), 0, s, d_linear, d_bins, n, p.log2_min, scale);
    return hipGetLastError();
}

template <uint32_t OP>
void apply_launch_oetf(uint32_t oetf, dim3 grid, hipStream_t s, const float *lin, const TonemapDev *dev, uint8_t *rgb8, float *disp,
                       uint32_t n, float w2) {
    if (oetf == RTMI_TONEMAP_GAMMA2)
        hipLaunchKernelGGL((rtmi_tonemap_apply_kernel<OP, RTMI_TONEMAP_GAMMA2>), grid, dim3(kBlock), 0, s, lin, dev, rgb8, disp, n, w2);
    else
        hipLaunchKernelGGL((rtmi_tonemap_apply_kernel<OP, RTMI_TONEMAP_SRGB>), grid, dim3(kBlock), 0, s, lin, dev, rgb8, disp, n, w2);
}

} // namespace

struct RTMI_HIDDEN rtmi_tonemap {
    int device = 0;
    uint32_t nx = 0, ny = 0;
    rtmi_tonemap_params params{};
    DeviceArena mem; // the bins, then the record
    uint32_t *d_bins = nullptr;
    TonemapDev *d_dev = nullptr;
    bool fresh = true;  // the next apply is a first apply
    bool dirty = false; // an apply failed after its meter may have run: the next one zeroes the bins first
    // the host form's staging, allocated by its first call
    DeviceArena stage;
    float *s_lin = nullptr, *s_disp = nullptr;
    uint8_t *s_rgb = nullptr;
    rtmi_tonemap_state *s_state = nullptr;
    hipStream_t stream = nullptr;
};

#define TM_TRY(fn, expr) RTMI_HIP_TRY(fn ": ", false, expr, #expr)

// the two or three kernels of one apply on `s`; nothing here allocates, waits or copies
static hipError_t tonemap_kernels(rtmi_tonemap *h, hipStream_t s, const float *d_linear, float dt, uint8_t *d_rgb8,
                                  float *d_display, rtmi_tonemap_state *d_state) {
    const rtmi_tonemap_params &p = h->params;
    const uint32_t n = h->nx * h->ny;
    const bool autoexp = p.exposure == RTMI_TONEMAP_AUTO;
    hipError_t e;
    if (h->dirty && (e = hipMemsetAsync(h->d_bins, 0, kBins * sizeof(uint32_t), s)) != hipSuccess) return e;
    h->dirty = false;
    if (autoexp && (e = meter_launch(s, d_linear, h->d_bins, n, p)) != hipSuccess) return e;
    TonemapSolve A{p.log2_min, p.log2_max, p.p_low, p.p_high, p.speed_up, p.speed_down, p.adapt_min, p.adapt_max, p.key, p.ev,
                   dt, autoexp ? 0.0f : rtmi_expf(p.ev * 0.69314718f), autoexp ? 1 : 0, h->fresh ? 1 : 0};
    hipLaunchKernelGGL(rtmi_tonemap_solve_kernel, dim3(1), dim3(64), 0, s, h->d_bins, h->d_dev, d_state, A);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (d_rgb8 || d_display) {
        const uint32_t lanes = (n >> 2) + ((n & 3u) ? 1u : 0u);
        const dim3 grid((lanes + kBlock - 1) / kBlock);
        const float w2 = p.white * p.white;
        if (p.op == RTMI_TONEMAP_CLAMP)
            apply_launch_oetf<RTMI_TONEMAP_CLAMP>(p.oetf, grid, s, d_linear, h->d_dev, d_rgb8, d_display, n, w2);
        else if (p.op == RTMI_TONEMAP_REINHARD)
            apply_launch_oetf<RTMI_TONEMAP_REINHARD>(p.oetf, grid, s, d_linear, h->d_dev, d_rgb8, d_display, n, w2);
        else
            apply_launch_oetf<RTMI_TONEMAP_ACES>(p.oetf, grid, s, d_linear, h->d_dev, d_rgb8, d_display, n, w2);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    h->fresh = false;
    return hipSuccess;
}

// After a failure the handle is as after a reset: the next apply is a first apply and, since the meter may have run
// without its solve, zeroes the bins on its stream before it meters.
static void tonemap_failed(rtmi_tonemap *h) {
    h->fresh = true;
    h->dirty = true;
}

static hipError_t tonemap_enqueue(rtmi_tonemap *h, hipStream_t s, const float *d_linear, float dt, uint8_t *d_rgb8,
                                  float *d_display, rtmi_tonemap_state *d_state) {
    const hipError_t e = tonemap_kernels(h, s, d_linear, dt, d_rgb8, d_display, d_state);
    if (e != hipSuccess) tonemap_failed(h);
    return e;
}

extern "C" void rtmi_tonemap_destroy(rtmi_tonemap *h) {
    if (!h) return;
    if (h->mem.base || h->stage.base || h->stream) {
        (void)hipSetDevice(h->device);
        (void)hipDeviceSynchronize(); // work enqueued on the caller's streams still reads the record
    }
    if (h->stream) (void)hipStreamDestroy(h->stream);
    h->stage.release();
    h->mem.release();
    delete h;
}

extern "C" int rtmi_tonemap_create(int device, uint32_t nx, uint32_t ny, const rtmi_tonemap_params *p, rtmi_tonemap **out) {
    // every argument check comes before the first HIP call
    if (out) *out = nullptr;
    if (!p || !out) return rtmi_fail(RTMI_ERR_INVALID, "rtmi_tonemap_create: NULL argument");
    int rc = check_params("rtmi_tonemap_create", nx, ny, p);
    if (rc) return rc;
    rc = device_ok("rtmi_tonemap_create: ", device);
    if (rc) return rc;
    rtmi_tonemap *h = new (std::nothrow) rtmi_tonemap;
    if (!h) return rtmi_fail(RTMI_ERR_NOMEM, "rtmi_tonemap_create: out of host memory");
    h->device = device;
    h->nx = nx;
    h->ny = ny;
    h->params = *p;
    const auto setup = [&]() -> int {
        TM_TRY("rtmi_tonemap_create", hipSetDevice(device));
        const auto layout = [&](Carve256 &c) {
            h->d_bins = c.take<uint32_t>(kBins);
            h->d_dev = c.take<TonemapDev>(1);
        };
        TM_TRY("rtmi_tonemap_create", h->mem.alloc(layout));
        TM_TRY("rtmi_tonemap_create", hipMemset(h->mem.base, 0, h->mem.bytes));
        TM_TRY("rtmi_tonemap_create", hipDeviceSynchronize());
        return RTMI_OK;
    };
    rc = setup();
    if (rc) {
        rtmi_tonemap_destroy(h);
        return rc;
    }
    *out = h;
    return RTMI_OK;
}

extern "C" int rtmi_tonemap_reset(rtmi_tonemap *h) {
    if (!h) return rtmi_fail(RTMI_ERR_INVALID, "rtmi_tonemap_reset: NULL handle");
    h->fresh = true;
    return RTMI_OK;
}

// the argument checks the two forms share, the handle left to the caller
static int check_apply(const char *name, const void *linear, float dt, const void *rgb8, const void *display, const void *state) {
    const auto bad = [&](const char *msg) { return fail(RTMI_ERR_INVALID, name, msg); };
    if (!linear) return bad("NULL linear");
    if (!finite_f(dt) || !(dt >= 0.0f)) return bad("dt must be finite and >= 0");
    if (!rgb8 && !display && !state) return bad("every output is NULL");
    return RTMI_OK;
}

extern "C" int rtmi_tonemap_apply_device(rtmi_tonemap *h, const void *d_linear, float dt, void *d_rgb8, void *d_display,
                                         void *d_state, void *stream) {
    if (int rc = check_apply("rtmi_tonemap_apply_device", d_linear, dt, d_rgb8, d_display, d_state)) return rc;
    if (misaligned(d_linear, 16) || misaligned(d_display, 16) || misaligned(d_rgb8, 4) || misaligned(d_state, 4))
        return rtmi_fail(RTMI_ERR_INVALID, "rtmi_tonemap_apply_device: misaligned pointer (d_linear and d_display need 16 bytes, "
                                           "d_rgb8 and d_state 4)");
    if (!h) return rtmi_fail(RTMI_ERR_INVALID, "rtmi_tonemap_apply_device: NULL handle");
    TM_TRY("rtmi_tonemap_apply_device", hipSetDevice(h->device));
    TM_TRY("rtmi_tonemap_apply_device",
           tonemap_enqueue(h, static_cast<hipStream_t>(stream), static_cast<const float *>(d_linear), dt,
                           static_cast<uint8_t *>(d_rgb8), static_cast<float *>(d_display), static_cast<rtmi_tonemap_state *>(d_state)));
    return RTMI_OK;
}

static int tonemap_run(rtmi_tonemap *h, const float *linear, float dt, uint8_t *out_rgb8, float *out_display,
                       rtmi_tonemap_state *out_state) {
    const size_t n = (size_t)h->nx * h->ny;
    TM_TRY("rtmi_tonemap_apply", hipSetDevice(h->device));
    if (!h->stage.base) {
        const auto layout = [&](Carve256 &c) {
            h->s_lin = c.take<float>(n * 3);
            h->s_disp = c.take<float>(n * 3);
            h->s_rgb = c.take<uint8_t>(n * 3);
            h->s_state = c.take<rtmi_tonemap_state>(1);
        };
        TM_TRY("rtmi_tonemap_apply", h->stage.alloc(layout));
    }
    if (!h->stream) TM_TRY("rtmi_tonemap_apply", hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    hipStream_t s = h->stream;
    TM_TRY("rtmi_tonemap_apply", hipMemcpyAsync(h->s_lin, linear, n * 12, hipMemcpyHostToDevice, s));
    TM_TRY("rtmi_tonemap_apply", tonemap_enqueue(h, s, h->s_lin, dt, out_rgb8 ? h->s_rgb : nullptr, out_display ? h->s_disp : nullptr,
                                                 out_state ? h->s_state : nullptr));
    if (out_rgb8) TM_TRY("rtmi_tonemap_apply", hipMemcpyAsync(out_rgb8, h->s_rgb, n * 3, hipMemcpyDeviceToHost, s));
    if (out_display) TM_TRY("rtmi_tonemap_apply", hipMemcpyAsync(out_display, h->s_disp, n * 12, hipMemcpyDeviceToHost, s));
    if (out_state) TM_TRY("rtmi_tonemap_apply", hipMemcpyAsync(out_state, h->s_state, sizeof(rtmi_tonemap_state), hipMemcpyDeviceToHost, s));
    TM_TRY("rtmi_tonemap_apply", hipStreamSynchronize(s));
    return RTMI_OK;
}

extern "C" int rtmi_tonemap_apply(rtmi_tonemap *h, const float *linear, float dt, uint8_t *out_rgb8, float *out_display,
                                  rtmi_tonemap_state *out_state) {
    // every argument check comes before the first HIP call; the handle comes last, so that a machine without a device
    // (where no handle can exist) still answers for every other argument
    if (int rc = check_apply("rtmi_tonemap_apply", linear, dt, out_rgb8, out_display, out_state)) return rc;
    if (!h) return rtmi_fail(RTMI_ERR_INVALID, "rtmi_tonemap_apply: NULL handle");
    const int rc = tonemap_run(h, linear, dt, out_rgb8, out_display, out_state);
    if (rc) tonemap_failed(h); // a copy or the wait may have failed after the kernels were enqueued
    return rc;
}

extern "C" int rtmi_probe_tonemap_histogram(int device, uint32_t nx, uint32_t ny, const rtmi_tonemap_params *p, const float *linear,
                                            uint32_t *out_bins) {
    if (!p || !linear || !out_bins) return rtmi_fail(RTMI_ERR_INVALID, "rtmi_probe_tonemap_histogram: NULL argument");
    int rc = check_params("rtmi_probe_tonemap_histogram", nx, ny, p);
    if (rc) return rc;
    rc = device_ok("rtmi_probe_tonemap_histogram: ", device);
    if (rc) return rc;
    TM_TRY("rtmi_probe_tonemap_histogram", hipSetDevice(device));
    const size_t n = (size_t)nx * ny;
    float *d_lin;
    uint32_t *d_bins;
    const auto layout = [&](Carve256 &c) {
        d_lin = c.take<float>(n * 3);
        d_bins = c.take<uint32_t>(kBins);
    };
    DeviceArena mem;
    TM_TRY("rtmi_probe_tonemap_histogram", mem.alloc(layout));
    TM_TRY("rtmi_probe_tonemap_histogram", hipMemcpy(d_lin, linear, n * 12, hipMemcpyHostToDevice));
    TM_TRY("rtmi_probe_tonemap_histogram", hipMemset(d_bins, 0, kBins * sizeof(uint32_t)));
    TM_TRY("rtmi_probe_tonemap_histogram", meter_launch(nullptr, d_lin, d_bins, (uint32_t)n, *p));
    TM_TRY("rtmi_probe_tonemap_histogram", hipMemcpy(out_bins, d_bins, kBins * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RTMI_OK;
}
