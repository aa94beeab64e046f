// rtmi_sparse.hip — translation unit of the sparse renders (include/rtmi_sparse.h): the select of a byte plane into an
// ascending pixel list, the path kernel over a list of pixels, the resolve of its samples, the patch of the results into
// the image's planes, and the launchers.  Compiled with the flags of rtmi_radiance.hip (-ffp-contract=off: the samples are
// the render's, bit for bit).
//
// The path kernel is the per-lane two-phase kernel (rtmi_kernel_perlane.inc) as rtmi_radiance.hip builds it: the fragments
// rtmi_path_lane.inc, rtmi_path_scan.inc, rtmi_path_traced.inc and rtmi_path_shade.inc are included as they are, so a path
// is traced, shaded and ended by the text the render kernels run.  The take step is this unit's own: item k * ns + s reads
// the pixel p = list[k] (an index into the image's planes, row 0 the top row) and draws the render's camera sample of that
// pixel and of sample first_sample + s, what rtmi_path_take.inc does for an item of a tile.  Instantiated for FAST x NEE x
// ENV; no profiling, signature, features, roulette or cooperative variant.
//
// Items.  Item k * ns + s (sample fastest) is sample s of entry k and slot k * ns + s of the per-sample buffer, written by
// path_end; the resolve reads an entry's samples as one contiguous run (rtmi_batch_welford.inc).  Work distribution is the
// batch modes' (batch_take, rtmi_batch.hpp); the chunk counter is a word of the caller's scratch, zeroed on the call's
// stream, and the number of items and of chunks is derived here from the device-side count.
// Count.  The number of entries is min(count[0], n), read here: the grid is sized for n, the host never learns the count,
// and a wavefront that finds the counter past the last chunk leaves at once.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "rtmi.h"
#include "rtmi_math.h"

#define RTMI_LEAN_TU 1 /* the plain kernels are defined in rtmi_device.hip */
#include "rtmi_kernels.hpp"
#include "rtmi_light_launch.hpp"
#include "rtmi_batch.hpp"
#include "rtmi_sparse_launch.hpp"

// ---- select ----------------------------------------------------------------------------------------------------------------
// Lane t of workgroup b owns the 16 pixels from b * RTMI_SPARSE_SPAN + 16 * t on, so ascending (workgroup, lane, bit) is
// ascending pixel order.  Bit j of the result: pixel base + j is selected.  A run that lies inside the plane is read as one
// 16-byte word, as four dwords or byte by byte, as the plane's alignment allows; the plane's tail is read byte by byte.
__device__ __forceinline__ uint32_t sparse_select_bits(const uint8_t *__restrict__ bytes, uint32_t n, uint32_t base, uint32_t mask) {
    if (base >= n) return 0u;
    uint32_t w[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}; // 255: never selected
    const uint8_t *p = bytes + base;
    if (n - base >= 16u) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        if ((a & 15u) == 0u) {
            const uint4 v = *reinterpret_cast<const uint4 *>(p);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else if ((a & 3u) == 0u) {
#pragma unroll
            for (int k = 0; k < 4; k++) w[k] = reinterpret_cast<const uint32_t *>(p)[k];
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                w[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) | ((uint32_t)p[4 * k + 3] << 24);
        }
    } else {
        const uint32_t left = n - base; // 1..15
        for (uint32_t j = 0; j < left; j++) w[j >> 2] = (w[j >> 2] & ~(0xffu << (8u * (j & 3u)))) | ((uint32_t)p[j] << (8u * (j & 3u)));
    }
    uint32_t bits = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 16u; j++) {
        const uint32_t b = (w[j >> 2] >> (8u * (j & 3u))) & 0xffu;
        bits |= ((b < 32u ? (mask >> (b & 31u)) & 1u : 0u)) << j;
    }
    return bits;
}
// the selected pixels of the wavefront's lower lanes and of the whole wavefront: a ballot per bit, the lane's rank by mbcnt
__device__ __forceinline__ void sparse_wave_rank(uint32_t bits, uint32_t &below, uint32_t &total) {
    below = 0u; total = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 16u; j++) {
        const unsigned long long m = __ballot((bits >> j) & 1u);
        below += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        total += (uint32_t)__popcll(m);
    }
}
// SCATTER = false: the workgroup's count.  SCATTER = true: its pixels written from its exclusive prefix on, below capacity.
template <bool SCATTER>
__global__ __launch_bounds__(256) void rtmi_sparse_select_kernel(const uint8_t *__restrict__ bytes, uint32_t n, uint32_t mask,
                                                                 uint32_t capacity, uint32_t *__restrict__ list,
                                                                 uint32_t *__restrict__ block_counts) {
    __shared__ uint32_t wave_total[4];
    const uint32_t base = blockIdx.x * RTMI_SPARSE_SPAN + threadIdx.x * 16u; // < 2^30 + 4096
    const uint32_t bits = sparse_select_bits(bytes, n, base, mask);
    uint32_t below, total;
    sparse_wave_rank(bits, below, total);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) wave_total[wave] = total;
    __syncthreads();
    if constexpr (!SCATTER) {
        if (threadIdx.x == 0u) block_counts[blockIdx.x] = wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
    } else {
        uint32_t pos = block_counts[blockIdx.x] + below; // the scan's exclusive prefix
        for (uint32_t k = 0; k < wave; k++) pos += wave_total[k];
        for (uint32_t b = bits; b != 0u && pos < capacity; b &= b - 1u) list[pos++] = base + (uint32_t)__builtin_ctz(b);
    }
}
// One workgroup: the per-workgroup counts become their exclusive prefix in place; count = {written, selected}.
__global__ __launch_bounds__(256) void rtmi_sparse_scan_kernel(uint32_t *__restrict__ block_counts, uint32_t nblocks, uint32_t capacity,
                                                               uint32_t *__restrict__ count) {
    __shared__ uint32_t part[256];
    const uint32_t per = (nblocks + 255u) / 256u;
    const uint32_t lo = threadIdx.x * per < nblocks ? threadIdx.x * per : nblocks;
    const uint32_t hi = lo + per < nblocks ? lo + per : nblocks;
    uint32_t sum = 0u;
    for (uint32_t k = lo; k < hi; k++) sum += block_counts[k];
    part[threadIdx.x] = sum;
    __syncthreads();
    uint32_t run = 0u;
    for (uint32_t k = 0; k < threadIdx.x; k++) run += part[k];
    for (uint32_t k = lo; k < hi; k++) {
        const uint32_t c = block_counts[k];
        block_counts[k] = run;
        run += c;
    }
    if (threadIdx.x == 255u) { // run: all selected pixels, at most n <= 2^30
        count[0] = run < capacity ? run : capacity;
        count[1] = run;
    }
}

// ---- the path kernel -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t sparse_entries(const SparseBatch &B) { // wave-uniform
    uint32_t e = B.n;
    if (B.count) {
        const uint32_t c = B.count[0];
        e = c < B.n ? c : B.n;
    }
    return e;
}

template <bool FAST, bool NEE, bool ENV>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void rtmi_sparse_kernel(DevScene sc, DevCamera cam, DevParams P, SparseBatch B,
                                                                           DevLights nl, DevEnv ev) {
    constexpr bool PROF = false, SIG = false, FEATURES = false;
    unsigned long long *prof = nullptr;
    // per wave: [0] node refs, [1] entry distances (FAST only); entry-major so lanes never bank-conflict
    __shared__ uint32_t lds_stack[WAVES_PER_BLOCK][FAST ? 2 : 1][RTMI_MAX_BVH_DEPTH][64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    uint32_t *stack = &lds_stack[wave][0][0][lane];
    unsigned long long sig = 0ull; // SIG = false: named by the fragments, never live
    BatchWork w;
    w.next = 0u; w.end = 0u;
    bool queue_empty = false;
    const uint32_t k0 = P.key0, k1 = P.key1;
    const int threshold = (int)P.shade_threshold;
    const uint32_t total = rfl(sparse_entries(B) * B.ns);        // < 2^31
    const uint32_t nchunks = (total + B.chunk - 1u) / B.chunk;   // 0: the list is empty, every wavefront leaves at once

    uint32_t oidx = 0u, ltile = 0u; // slot of this lane's path in the per-sample buffer (= its item)
    bool alive = false, done = false, have_hit = false;
    typename std::conditional<NEE, RngNee, RngReg>::type g;
#include "rtmi_path_lane.inc"

    for (;;) {
        // ================= phase A: trace until enough lanes hold a hit =================
        for (;;) {
            if (__ballot(!have_hit && !done) == 0ull) break;
            { // lanes whose path ended take the next (entry, sample) item, or are done when there is none
                const bool want = !have_hit && !done && !alive;
                if (__ballot(want) != 0ull) {
                    if (batch_take(w, queue_empty, want, B.queue, B.chunk, total, nchunks, oidx)) {
                        const uint32_t k = oidx / B.ns, s = oidx - k * B.ns;
                        // the list indexes the image's planes, row 0 the top row; the render counts its rows from the
                        // bottom (work_take: j = ny - 1 - row) and keys its streams by j * nx + px
                        const uint32_t p = B.list[k];
                        const uint32_t row = p / P.nx, px = p - row * P.nx;
                        const uint32_t j = P.ny - 1u - row, pixel = j * P.nx + px; // a row outside the image wraps: some path
                        camera_sample(cam, P, g, k0, k1, B.first_sample + s, pixel, px, j, pa);
                        if constexpr (NEE) { rng_init(gn, B.first_sample + s, pixel); ne.pb = 0.0f; }
                        alive = true;
                    } else if (want) {
                        done = true;
                    }
                }
            }
            const bool need = !have_hit && !done;
            if (need) {
#define RTMI_SCAN_T_MIN P.t_min
#define RTMI_SCAN_T_MAX RTMI_FLT_MAX
#include "rtmi_path_scan.inc"
#undef RTMI_SCAN_T_MIN
#undef RTMI_SCAN_T_MAX
#include "rtmi_path_traced.inc"
            }
            if (__popcll(__ballot(have_hit)) >= threshold) break;
        }
        // ================= phase B: shade every lane that holds a hit =================
#define RTMI_PATH_SCRATCH &lds_stack[wave][0][0][0]
#define RTMI_PATH_INST true
#include "rtmi_path_shade.inc"
#undef RTMI_PATH_SCRATCH
#undef RTMI_PATH_INST
    }
}

// One lane per entry: the f64 sum of its ns samples in sample order and Welford's recurrence (rtmi_batch_welford.inc);
// ns == 1: no estimate, +inf.
__global__ __launch_bounds__(256) void rtmi_sparse_resolve_kernel(const Rad3 *__restrict__ samples, SparseBatch B) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= sparse_entries(B)) return;
    const Rad3 *src = samples + (size_t)i * B.ns;
    double sum[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0}, M2[3] = {0.0, 0.0, 0.0};
    const uint32_t ns = B.ns;
#include "rtmi_batch_welford.inc"
    const double n = (double)B.ns;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        if (B.mean) B.mean[3 * (size_t)i + ch] = (float)(sum[ch] / n);
        if (B.stderr_out) B.stderr_out[3 * (size_t)i + ch] = B.ns > 1u ? (float)sqrt(M2[ch] / (n * (n - 1.0))) : __builtin_inff();
    }
}

// ---- patch -----------------------------------------------------------------------------------------------------------------
// One lane per entry; an entry whose pixel lies outside the planes is skipped.  The quantiser is rtmi_resolve_kernel's on
// (double)mean, as rtmi_denoise_finish_kernel applies it.
__global__ __launch_bounds__(256) void rtmi_sparse_patch_kernel(uint32_t n_pixels, const uint32_t *__restrict__ list,
                                                                const uint32_t *__restrict__ count, uint32_t capacity,
                                                                const float *__restrict__ mean, const float *__restrict__ se,
                                                                float *__restrict__ linear, uint8_t *__restrict__ rgb8,
                                                                float *__restrict__ stderr_plane, uint8_t *__restrict__ bytes,
                                                                uint32_t mark) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t entries = capacity;
    if (count) {
        const uint32_t c = count[0];
        entries = c < capacity ? c : capacity;
    }
    if (k >= entries) return;
    const uint32_t p = list[k];
    if (p >= n_pixels) return;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (linear || rgb8) {
            const float o = mean[3 * (size_t)k + c];
            if (linear) linear[3 * (size_t)p + c] = o;
            if (rgb8) {
                double g = sqrt((double)o);
                g = (g > 0.0) ? ((g < 1.0) ? g : 1.0) : 0.0; // NaN -> 0
                const double v = 255.99 * g;
                rgb8[3 * (size_t)p + c] = (uint8_t)(int32_t)v;
            }
        }
        if (stderr_plane) stderr_plane[3 * (size_t)p + c] = se[3 * (size_t)k + c];
    }
    if (bytes) bytes[p] = (uint8_t)mark;
}

// ---- launchers -------------------------------------------------------------------------------------------------------------
hipError_t rtmi_sparse_launch_select(hipStream_t stream, const uint8_t *bytes, uint32_t n, uint32_t accept_mask, uint32_t capacity,
                                     uint32_t *list, uint32_t *count, uint32_t *block_counts) {
    const uint32_t nblocks = (n + RTMI_SPARSE_SPAN - 1u) / RTMI_SPARSE_SPAN;
    hipLaunchKernelGGL(rtmi_sparse_select_kernel<false>, dim3(nblocks), dim3(256), 0, stream, bytes, n, accept_mask, capacity, list,
                       block_counts);
    hipLaunchKernelGGL(rtmi_sparse_scan_kernel, dim3(1), dim3(256), 0, stream, block_counts, nblocks, capacity, count);
    hipLaunchKernelGGL(rtmi_sparse_select_kernel<true>, dim3(nblocks), dim3(256), 0, stream, bytes, n, accept_mask, capacity, list,
                       block_counts);
    return hipGetLastError();
}

hipError_t rtmi_sparse_launch(bool fast, bool nee, bool env, uint32_t blocks, hipStream_t stream, const DevScene &sc,
                              const DevCamera &cam, const DevParams &P, const SparseBatch &B, const DevLights &L, const DevEnv &E) {
    const dim3 grid(blocks), block(64 * WAVES_PER_BLOCK);
    return rtmi_with_bools([&](auto FAST, auto NEE, auto ENV) {
        hipLaunchKernelGGL((rtmi_sparse_kernel<FAST(), NEE(), ENV()>), grid, block, 0, stream, sc, cam, P, B, L, E);
        return hipGetLastError();
    }, fast, nee, env);
}

hipError_t rtmi_sparse_launch_resolve(hipStream_t stream, const Rad3 *samples, const SparseBatch &B) {
    hipLaunchKernelGGL(rtmi_sparse_resolve_kernel, dim3((B.n + 255u) / 256u), dim3(256), 0, stream, samples, B);
    return hipGetLastError();
}

hipError_t rtmi_sparse_launch_patch(hipStream_t stream, uint32_t n_pixels, const uint32_t *list, const uint32_t *count, uint32_t capacity,
                                    const float *mean, const float *se, float *linear, uint8_t *rgb8, float *stderr_plane,
                                    uint8_t *bytes, uint32_t mark) {
    hipLaunchKernelGGL(rtmi_sparse_patch_kernel, dim3((capacity + 255u) / 256u), dim3(256), 0, stream, n_pixels, list, count, capacity,
                       mean, se, linear, rgb8, stderr_plane, bytes, mark);
    return hipGetLastError();
}
