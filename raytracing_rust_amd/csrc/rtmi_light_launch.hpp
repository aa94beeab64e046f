// rtmi_light_launch.hpp — launchers of the lighting kernels, each defined in the translation unit of its kernels and called
// by the lighting entry points in rtmi_device.hip: next-event estimation (include/rtmi_nee.h, rtmi_nee.hip), environment
// lighting and its host tables (include/rtmi_env.h, rtmi_env.hip), adaptive sampling with either
// (include/rtmi_adaptive_nee.h, rtmi_adaptive_nee.hip) and Russian roulette (include/rtmi_roulette.h, rtmi_roulette.hip).
// The resolve of all four is adaptive sampling's (rtmi_adaptive_launch.hpp); the fixed renders run it over the list of
// all tiles: the render's sums plus Welford's standard errors.
#pragma once
#include <type_traits>
#include <vector>

#include "rtmi_env.h"
#include "rtmi_light_tree.h"

// Run-time bools to template arguments: rtmi_with_bools(f, a, b, ...) returns f(std::bool_constant<a>{},
// std::bool_constant<b>{}, ...), so a generic lambda names the kernel instantiation as kernel<A(), B()>.
template <typename F>
hipError_t rtmi_with_bools(F &&f) { return f(); }
template <typename F, typename... Bools>
hipError_t rtmi_with_bools(F &&f, bool b, Bools... rest) {
    return b ? rtmi_with_bools([&](auto... c) { return f(std::true_type{}, c...); }, rest...)
             : rtmi_with_bools([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}

hipError_t rtmi_nee_launch_render(bool fast, bool sig, uint32_t blocks, hipStream_t stream, const DevScene &sc,
                                  const DevCamera &cam, const DevParams &P, const DevLights &L);

// RTMI_FLAG_LIGHT_TREE (include/rtmi_light_tree.h, rtmi_light_tree.hip): rtmi_nee_launch_render with the light of a vertex
// taken from the tree T
hipError_t rtmi_light_tree_launch_render(bool fast, bool sig, uint32_t blocks, hipStream_t stream, const DevScene &sc,
                                         const DevCamera &cam, const DevParams &P, const DevLights &L, const DevLightTree &T);
// n walks of the device (RTMI_LIGHT_TREE_PROBE_*): points 3 floats per item, aux a uniform's bits or a light index
hipError_t rtmi_light_tree_launch_probe(int op, const DevLightTree &T, const float *points, const uint32_t *aux, uint32_t n,
                                        uint32_t *out_light, float *out_p, hipStream_t stream);
// the tree over the light table of a description (host code): 2 * lights nodes, one path per light; an RTMI code
int rtmi_light_tree_build(const rtmi_scene_desc *d, std::vector<rtmi_light_node> &nodes, std::vector<rtmi_light_path> &paths);

// the tables of rtmi_env_tables for one map, rounded to float
struct EnvTables {
    std::vector<float> row_cdf, row_p, col_cdf, col_p;
    double total = 0.0;
};
// RTMI_OK, or RTMI_ERR_INVALID (with the message of rtmi_last_error) for a NULL or bad map
int rtmi_env_build_tables(const rtmi_env_map *map, EnvTables &t);

hipError_t rtmi_env_launch_render(bool fast, bool sig, bool nee, uint32_t blocks, hipStream_t stream, const DevScene &sc,
                                  const DevCamera &cam, const DevParams &P, const DevLights &L, const DevEnv &E);
// n probe evaluations (RTMI_ENV_PROBE_*): `in` 3 (lookup) or 2 (sample) floats per item, `out` 4 floats per item
hipError_t rtmi_env_launch_probe(int op, const DevEnv &E, const float *in, float *out, uint32_t n, hipStream_t stream);

// one pass over the P.ntiles_local active tiles of `tiles`; nee / env select the estimator (not both false)
hipError_t rtmi_adaptive_nee_launch_render(bool fast, bool nee, bool env, uint32_t blocks, hipStream_t stream, const DevScene &sc,
                                           const DevCamera &cam, const DevParams &P, const uint32_t *tiles, const DevLights &L,
                                           const DevEnv &E);

// RTMI_FLAG_LIGHT_COOP (include/rtmi_light_coop.h, rtmi_light_coop.hip): the estimators above on the wave-cooperative
// kernel.  tile_list: one pass over the P.ntiles_local active tiles of `tiles` (no signatures), otherwise the fixed render's
// pass; ext: the pool form of plan_traversal; lds: the dynamic LDS of a block (the formula of rtmi_render_coop's launch);
// nee / env not both false.  The kernels are compiled for RTMI_LIGHT_COOP_WPS waves per SIMD: the persistent grid is
// CUs x 4 SIMDs x that many wavefronts.
#ifndef RTMI_LIGHT_COOP_WPS
#define RTMI_LIGHT_COOP_WPS 3
#endif
hipError_t rtmi_light_coop_launch_render(bool tile_list, bool sig, bool ext, bool nee, bool env, uint32_t blocks, size_t lds,
                                         hipStream_t stream, const DevScene &sc, const DevCamera &cam, const DevParams &P,
                                         const uint32_t *tiles, const DevLights &L, const DevEnv &E);

// the roulette parameters and the bounce plane: a kernel argument of their own, as DevLights and DevEnv are (DevParams
// goes to every kernel)
struct DevRoulette {
    uint32_t *bounces;  // [local tile][64]: scatters of the pixel's written paths, summed with integer atomics
    uint32_t min_depth; // the test is made when depth >= min_depth
    float q_min;        // floor of the survival probability
};

// one pass over the P.ntiles_local active tiles of `tiles`; nee / env select the estimator (both false: the plain one)
hipError_t rtmi_roulette_launch_render(bool fast, bool nee, bool env, uint32_t blocks, hipStream_t stream, const DevScene &sc,
                                       const DevCamera &cam, const DevParams &P, const uint32_t *tiles, const DevLights &L,
                                       const DevEnv &E, const DevRoulette &R);

// RTMI_FLAG_ROULETTE_COOP (include/rtmi_roulette_coop.h, rtmi_roulette_coop.hip): the same pass on the wave-cooperative
// kernel.  ext / lds as in rtmi_light_coop_launch_render.  The NEE / ENV kernels are compiled for RTMI_LIGHT_COOP_WPS waves
// per SIMD, the two plain ones for RTMI_ROULETTE_COOP_PLAIN_WPS (4 as rtmi_adaptive_coop: they keep no NeeLane, no second
// stream and no map, and fit without scratch): the host sizes the persistent grid per kernel.
#ifndef RTMI_ROULETTE_COOP_PLAIN_WPS
#define RTMI_ROULETTE_COOP_PLAIN_WPS 4
#endif
constexpr uint32_t rtmi_roulette_coop_wps(bool nee, bool env) {
    return nee || env ? (uint32_t)RTMI_LIGHT_COOP_WPS : (uint32_t)RTMI_ROULETTE_COOP_PLAIN_WPS;
}
hipError_t rtmi_roulette_coop_launch_render(bool ext, bool nee, bool env, uint32_t blocks, size_t lds, hipStream_t stream,
                                            const DevScene &sc, const DevCamera &cam, const DevParams &P, const uint32_t *tiles,
                                            const DevLights &L, const DevEnv &E, const DevRoulette &R);
