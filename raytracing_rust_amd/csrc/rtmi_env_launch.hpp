// rtmi_env_launch.hpp — launchers of the environment-lighting kernels (include/rtmi_env.h), defined in rtmi_env.hip and
// called by rtmi_render_env and rtmi_probe_env in rtmi_device.hip, and the host tables both sides share.  The resolve is
// adaptive sampling's (rtmi_adaptive_launch.hpp) over the list of all tiles, as rtmi_render_nee's.
#pragma once
#include <vector>

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
