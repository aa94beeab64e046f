// rtmi_image_dev.hpp — the few definitions the image-filter units (denoise, temporal, tonemap, upscale) share on the
// device side.  See DESIGN.md §34.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

// a first-hit depth is a surface's exactly when it is finite
__device__ __forceinline__ bool surface(float z) { return __builtin_isfinite(z); }

// four pixels of rgb8, stored as one 12-byte access
struct alignas(4) Bytes12 {
    uint32_t w[3];
};

// log2 of a normal_power that the checks found to be 0 or a power of two: the kernels square the cosine that many times
static inline int normal_squarings(uint32_t normal_power) {
    int k = 0;
    for (uint32_t pw = normal_power; pw > 1u; pw >>= 1) k++;
    return k;
}
