// rtmi_features_launch.hpp — launchers of the first-hit features kernels (include/rtmi_features.h), defined in
// rtmi_features.hip and called by rtmi_render_features in rtmi_device.hip.
#pragma once

// what the features resolve of one pass needs besides DevParams (tile_world = 1: local tile = tile)
struct FeaturesResolve {
    const FeatSlot *slots; // the per-sample buffer: [tile][P.pass_stride][64] FeatSlots
    double *state;         // [tile][8][64]: sums of albedo r,g,b | normal x,y,z | distance | hits, carried between passes
    float *albedo;         // [ny][nx][3], row 0 = top row
    float *normal;         // [ny][nx][3]
    float *depth;          // [ny][nx]
    uint32_t *hits;        // [ny][nx]
    int first;             // first pass: the sums start at zero
    int last;              // last pass: write the planes
};

hipError_t rtmi_features_launch_render(bool fast, bool sig, uint32_t blocks, hipStream_t stream, const DevScene &sc,
                                       const DevCamera &cam, const DevParams &P);
hipError_t rtmi_features_launch_resolve(hipStream_t stream, const DevParams &P, const FeaturesResolve &R);
