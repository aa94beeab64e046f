// rtmi_f64_plan.hpp — pass plan of the f64 render mode (rtmi_render_f64): samples per pass and per work unit.
// Plain C++ (no HIP), so that tests can compile it on the host.  The per-sample buffer holds RTMI_SAMPLE_SLOT_BYTES_F64 per
// (local pixel, sample of the pass).  The work queue the f64 kernel shares with the fp32 kernels (wave_work / work_take,
// rtmi_shade.hpp) computes slot indices in 32 bits, so a pass may hold at most 2^32 - 1 slots; the buffer is also capped
// at 45 GiB, the cap of the fp32 planner.  Larger renders run in passes — the same additions in the same order.
#pragma once
#include <cstdint>

#define RTMI_F64_MAX_BUFFER_BYTES (45ull << 30)
#define RTMI_F64_MAX_PASS_SLOTS 0xffffffffull

// ntiles: local 8x8 tiles; budget: sample_buffer_bytes (0 = default: half of free_bytes); units_want: work units that keep
// every wavefront slot busy (0 = no minimum); spp_chunks: rtmi_render_params.spp_chunks.  Returns false when not even one
// sample of every pixel fits a pass (an image of more than 2^32 - 1 padded pixels).
inline bool rtmi_f64_plan(uint64_t ntiles, uint32_t ns, uint64_t budget, uint64_t free_bytes, uint64_t units_want, uint32_t spp_chunks,
                          uint32_t &chunk_spp, uint32_t &pass_ns) {
    chunk_spp = 1u;
    pass_ns = 0u;
    const uint64_t slots_per_sample = ntiles * 64u;
    if (ntiles == 0 || ns == 0 || slots_per_sample > RTMI_F64_MAX_PASS_SLOTS) return false;
    const uint64_t per_sample = slots_per_sample * 24u; // RTMI_SAMPLE_SLOT_BYTES_F64
    uint64_t want = budget ? budget : free_bytes / 2;
    if (want > RTMI_F64_MAX_BUFFER_BYTES) want = RTMI_F64_MAX_BUFFER_BYTES;
    uint64_t max_pass = want / per_sample;
    if (max_pass > RTMI_F64_MAX_PASS_SLOTS / slots_per_sample) max_pass = RTMI_F64_MAX_PASS_SLOTS / slots_per_sample;
    if (max_pass < 1) max_pass = 1;
    if (max_pass > ns) max_pass = ns;
    uint64_t chunk = spp_chunks ? (ns + spp_chunks - 1) / spp_chunks : 16u;
    if (!spp_chunks && units_want && ntiles * ((ns + chunk - 1) / chunk) < units_want) { // a few units per wavefront slot
        const uint64_t per_tile = (units_want + ntiles - 1) / ntiles;
        chunk = (ns + per_tile - 1) / per_tile;
    }
    if (chunk > max_pass) chunk = max_pass;
    if (chunk < 1) chunk = 1;
    chunk_spp = (uint32_t)chunk;
    pass_ns = max_pass >= ns ? ns : (uint32_t)((max_pass / chunk) * chunk); // whole chunks per pass
    return true;
}
