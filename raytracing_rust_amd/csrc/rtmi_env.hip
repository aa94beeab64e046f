// rtmi_env.hip — translation unit of environment lighting (include/rtmi_env.h): the environment kernels, the probe
// kernel, their launchers and the host code of the sampling tables.  Compiled with the flags of rtmi_device.hip
// (-ffp-contract=off: no fused operations, so numpy restates the lookup and the sampler bit for bit).
//
// The environment kernel is the body of rtmi_render_kernel (rtmi_kernel_perlane.inc) with ENV = true: same work queue,
// camera_sample, item scan and two-phase schedule.  A ray that leaves the world adds the map's radiance (env_radiance,
// rtmi_shade.hpp).  With NEE = true it is rtmi_nee_kernel with the map as one more light: shade_hit<.., NEE, ENV> picks
// the map with probability p_env and samples a direction from its tables (env_sample); the shadow ray toward it counts
// when phase A finds that it leaves the world, and a BSDF ray that leaves the world is weighted by nee_mis_bsdf.
// Instantiated for FAST x SIG x NEE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "rtmi.h"
#include "rtmi_math.h"
#include "rtmi_env.h"

#define RTMI_LEAN_TU 1 /* the plain kernels are defined in rtmi_device.hip */
#include "rtmi_kernels.hpp"
#include "rtmi_light_launch.hpp"
#include "rtmi_hostkit.hpp"

template <bool FAST, bool SIG, bool NEE>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void rtmi_env_kernel(DevScene sc, DevCamera cam, DevParams P, DevLights nl,
                                                                        DevEnv ev) {
    constexpr bool PROF = false, TILE_LIST = false, FEATURES = false, ENV = true;
    const uint32_t *const tiles = nullptr;
#include "rtmi_kernel_perlane.inc"
}

hipError_t rtmi_env_launch_render(bool fast, bool sig, bool nee, uint32_t blocks, hipStream_t stream, const DevScene &sc,
                                  const DevCamera &cam, const DevParams &P, const DevLights &L, const DevEnv &E) {
    const dim3 grid(blocks), block(64 * WAVES_PER_BLOCK);
    return rtmi_with_bools([&](auto NEE, auto FAST, auto SIG) {
        hipLaunchKernelGGL((rtmi_env_kernel<FAST(), SIG(), NEE()>), grid, block, 0, stream, sc, cam, P, L, E);
        return hipGetLastError();
    }, nee, fast, sig);
}

// one item per thread: RTMI_ENV_PROBE_LOOKUP (env and the BSDF-side pdf of a direction) or RTMI_ENV_PROBE_SAMPLE (the
// direction and pdf of a light sample; zeros when there is none)
__global__ __launch_bounds__(256) void rtmi_env_probe_kernel(int op, DevEnv E, const float *__restrict__ in,
                                                            float *__restrict__ out, uint32_t n) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (op == RTMI_ENV_PROBE_LOOKUP) {
        float u, v, th;
        if (env_uv(f3(in[3 * (size_t)k], in[3 * (size_t)k + 1], in[3 * (size_t)k + 2]), u, v, th)) {
            const F3 e = env_radiance(E, u, v);
            r = make_float4(e.x, e.y, e.z, env_pdf(E, u, v, th));
        }
    } else {
        F3 d;
        float pdf;
        if (E.p_env > 0.0f && env_sample(E, in[2 * (size_t)k], in[2 * (size_t)k + 1], d, pdf)) r = make_float4(d.x, d.y, d.z, pdf);
    }
    reinterpret_cast<float4 *>(out)[k] = r;
}

hipError_t rtmi_env_launch_probe(int op, const DevEnv &E, const float *in, float *out, uint32_t n, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(rtmi_env_probe_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, op, E, in, out, n);
    return hipGetLastError();
}

// ---- host: the sampling tables (include/rtmi_env.h), f64, each output rounded once to float ----------------------------
int rtmi_env_build_tables(const rtmi_env_map *m, EnvTables &t) {
    if (!m || !m->rgb) return rtmi_fail(RTMI_ERR_INVALID, "rtmi_env: the map or its texels are NULL");
    const uint32_t W = m->width, H = m->height;
    if (W < 1u || H < 1u || W > RTMI_ENV_MAX_SIDE || H > RTMI_ENV_MAX_SIDE || (uint64_t)W * H > RTMI_ENV_MAX_TEXELS)
        return rtmi_fail(RTMI_ERR_INVALID, "rtmi_env: width and height must be in [1, 16384] with width * height <= 2^25");
    const size_t n = (size_t)W * H;
    for (size_t k = 0; k < 3 * n; k++)
        if (!(m->rgb[k] >= 0.0f && m->rgb[k] <= 3.40282347e38f)) return rtmi_fail(RTMI_ERR_INVALID, "rtmi_env: texels must be finite and >= 0");
    // the largest channel of every texel, its maximum over the row neighbours (wrapped), then over the rows (clamped)
    std::vector<float> mc(n), mr(n);
    for (size_t k = 0; k < n; k++) mc[k] = std::max(std::max(m->rgb[3 * k], m->rgb[3 * k + 1]), m->rgb[3 * k + 2]);
    for (uint32_t j = 0; j < H; j++) {
        const float *row = mc.data() + (size_t)j * W;
        for (uint32_t i = 0; i < W; i++)
            mr[(size_t)j * W + i] = std::max(std::max(row[(i + W - 1u) % W], row[i]), row[(i + 1u) % W]);
    }
    t.row_cdf.assign(H, 1.0f); t.row_p.assign(H, 0.0f);
    t.col_cdf.assign(n, 1.0f); t.col_p.assign(n, 0.0f);
    std::vector<double> R(H), w(W);
    for (uint32_t j = 0; j < H; j++) {
        const float *up = mr.data() + (size_t)(j > 0u ? j - 1u : 0u) * W, *mid = mr.data() + (size_t)j * W;
        const float *dn = mr.data() + (size_t)(j + 1u < H ? j + 1u : H - 1u) * W;
        const double c = std::sin(((double)j + 0.5) * M_PI / (double)H); // cos of the row centre's latitude
        double r = 0.0;
        for (uint32_t i = 0; i < W; i++) {
            w[i] = (double)std::max(std::max(up[i], mid[i]), dn[i]) * c;
            r += w[i];
        }
        R[j] = r;
        if (r > 0.0) {
            double s = 0.0;
            for (uint32_t i = 0; i < W; i++) {
                const double p = w[i] / r;
                s += p;
                t.col_p[(size_t)j * W + i] = (float)p;
                t.col_cdf[(size_t)j * W + i] = i + 1u == W ? 1.0f : (float)s;
            }
        }
    }
    double total = 0.0;
    for (uint32_t j = 0; j < H; j++) total += R[j];
    t.total = total;
    if (total > 0.0) {
        double s = 0.0;
        for (uint32_t j = 0; j < H; j++) {
            const double p = R[j] / total;
            s += p;
            t.row_p[j] = (float)p;
            t.row_cdf[j] = j + 1u == H ? 1.0f : (float)s;
        }
    }
    return RTMI_OK;
}

extern "C" int rtmi_env_tables(const rtmi_env_map *map, float *row_cdf, float *row_p, float *col_cdf, float *col_p, double *total) {
    EnvTables t;
    if (int rc = rtmi_env_build_tables(map, t)) return rc;
    if (row_cdf) std::memcpy(row_cdf, t.row_cdf.data(), t.row_cdf.size() * sizeof(float));
    if (row_p) std::memcpy(row_p, t.row_p.data(), t.row_p.size() * sizeof(float));
    if (col_cdf) std::memcpy(col_cdf, t.col_cdf.data(), t.col_cdf.size() * sizeof(float));
    if (col_p) std::memcpy(col_p, t.col_p.data(), t.col_p.size() * sizeof(float));
    if (total) *total = t.total;
    return RTMI_OK;
}
