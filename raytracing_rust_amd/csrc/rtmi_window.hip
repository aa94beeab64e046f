// rtmi_window.hip — translation unit of windowed adaptive sampling (include/rtmi_window.h): the spread kernel and its
// launcher.  Compiled with the flags of rtmi_pixelwise.hip.  The select, the path kernel and the step kernel of a step are
// those of rtmi_sparse.hip and rtmi_pixelwise.hip, launched as they are by the entries in rtmi_batch.hip.
//
// active[p] = active[p] != 0 && some fail byte != 0 in the (2r + 1)^2 window of p clipped to the image.  The planes are
// bytes and the window holds up to 33^2 taps, so no lane reads taps.  A wavefront owns 64 consecutive pixels of a row and
// turns that segment's fail bytes into one 64-bit mask with a ballot: one coalesced byte load per lane.  A workgroup of four
// wavefronts owns a tile of 64 x 16 pixels and stages, in LDS, the masks of its 16 rows and of r halo rows above and below,
// each with the segment to its left and to its right.  A segment beyond the image is zero, a row beyond it is zero, and a
// row that ends inside a segment has zero bits behind its end: a window never wraps into the next row.  Then
//   horizontal: one lane per staged row ORs the shifts -r .. r of the three-segment concatenation into the middle 64 bits;
//   vertical:   one lane per tile row ORs the 2r + 1 staged rows around it;
//   store:      each lane takes its own bit of its row's mask and writes it over a non-zero active byte.
// One workgroup size and one LDS size (1664 bytes) serve every radius up to the maximum; nx needs no alignment.
//
// The direct form, each lane looping over its clipped window through the cache, was built and measured against this one
// (profiles/window/spread_kernel_direct.patch).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rtmi_window_launch.hpp"

#define RTMI_WINDOW_TILE_ROWS 16u
#define RTMI_WINDOW_STAGED_ROWS (RTMI_WINDOW_TILE_ROWS + 2u * RTMI_WINDOW_RADIUS_MAX)

__global__ __launch_bounds__(256) void rtmi_window_spread_kernel(uint8_t *active, const uint8_t *fail, uint32_t nx, uint32_t ny,
                                                                  uint32_t r, uint32_t tiles_x) {
    __shared__ unsigned long long seg[RTMI_WINDOW_STAGED_ROWS][3]; // left | middle | right segment of each staged row
    __shared__ unsigned long long hor[RTMI_WINDOW_STAGED_ROWS];    // the middle segment after the horizontal pass
    __shared__ unsigned long long ver[RTMI_WINDOW_TILE_ROWS];      // the tile's rows after the vertical pass
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int64_t x0 = (int64_t)(blockIdx.x % tiles_x) * 64, y0 = (int64_t)(blockIdx.x / tiles_x) * RTMI_WINDOW_TILE_ROWS;
    const uint32_t staged = RTMI_WINDOW_TILE_ROWS + 2u * r;
    // Staged row i is image row y0 - r + i; a wavefront takes the rows wave, wave + 4, ..., four at a time.  Every lane loads
    // from an address clamped into the image, so the twelve loads of a round are unconditional and in flight together;
    // what lies outside the image is masked out of the ballot instead.
    const int64_t xs[3] = {x0 - 64 + lane, x0 + lane, x0 + 64 + lane};
    bool in_x[3];
    size_t cx[3];
#pragma unroll
    for (int s = 0; s < 3; s++) {
        in_x[s] = xs[s] >= 0 && xs[s] < (int64_t)nx;
        cx[s] = (size_t)(xs[s] < 0 ? 0 : (xs[s] < (int64_t)nx ? xs[s] : (int64_t)nx - 1));
    }
    for (uint32_t i0 = wave; i0 < staged; i0 += 16u) {
        uint8_t b[4][3];
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) {
            const int64_t y = y0 - (int64_t)r + (i0 + 4u * u);
            const uint8_t *row = fail + (size_t)(y < 0 ? 0 : (y < (int64_t)ny ? y : (int64_t)ny - 1)) * nx;
#pragma unroll
            for (int s = 0; s < 3; s++) b[u][s] = row[cx[s]];
        }
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) {
            const uint32_t i = i0 + 4u * u;
            const int64_t y = y0 - (int64_t)r + i;
            const bool in_y = y >= 0 && y < (int64_t)ny; // uniform over the wavefront
            const unsigned long long m0 = __ballot(in_y && in_x[0] && b[u][0] != 0u);
            const unsigned long long m1 = __ballot(in_y && in_x[1] && b[u][1] != 0u);
            const unsigned long long m2 = __ballot(in_y && in_x[2] && b[u][2] != 0u);
            if (i < staged && lane < 3u) seg[i][lane] = lane == 0u ? m0 : (lane == 1u ? m1 : m2);
        }
    }
    __syncthreads();
    if (threadIdx.x < staged) {
        const unsigned long long l = seg[threadIdx.x][0], m = seg[threadIdx.x][1], rr = seg[threadIdx.x][2];
        unsigned long long h = m;
        for (uint32_t d = 1u; d <= r; d++) // bit b of a mask is pixel x0 + b: pixel x - d reaches x by a shift up
            h |= (m << d) | (l >> (64u - d)) | (m >> d) | (rr << (64u - d));
        hor[threadIdx.x] = h;
    }
    __syncthreads();
    if (threadIdx.x < RTMI_WINDOW_TILE_ROWS) {
        unsigned long long v = 0ull;
        for (uint32_t k = 0u; k <= 2u * r; k++) v |= hor[threadIdx.x + k]; // tile row j is staged row j + r
        ver[threadIdx.x] = v;
    }
    __syncthreads();
    if (!in_x[1]) return;
    // tile rows wave, wave + 4, wave + 8, wave + 12: the four loads first, then the stores
    uint8_t a[RTMI_WINDOW_TILE_ROWS / 4u];
#pragma unroll
    for (uint32_t u = 0; u < RTMI_WINDOW_TILE_ROWS / 4u; u++) {
        const int64_t y = y0 + wave + 4u * u;
        a[u] = y < (int64_t)ny ? active[(size_t)y * nx + cx[1]] : (uint8_t)0u;
    }
#pragma unroll
    for (uint32_t u = 0; u < RTMI_WINDOW_TILE_ROWS / 4u; u++) {
        const uint32_t j = wave + 4u * u;
        const int64_t y = y0 + j;
        if (y < (int64_t)ny && a[u] != 0u) active[(size_t)y * nx + cx[1]] = (uint8_t)((ver[j] >> lane) & 1ull);
    }
}

hipError_t rtmi_window_launch_spread(hipStream_t stream, uint8_t *active, const uint8_t *fail, uint32_t nx, uint32_t ny, uint32_t radius) {
    const uint32_t tiles_x = (uint32_t)(((uint64_t)nx + 63ull) / 64ull);
    const uint32_t tiles_y = (uint32_t)(((uint64_t)ny + RTMI_WINDOW_TILE_ROWS - 1ull) / RTMI_WINDOW_TILE_ROWS);
    // at most 2^30 pixels: 2^26 tiles for an image one pixel wide
    hipLaunchKernelGGL(rtmi_window_spread_kernel, dim3(tiles_x * tiles_y), dim3(256), 0, stream, active, fail, nx, ny, radius, tiles_x);
    return hipGetLastError();
}
