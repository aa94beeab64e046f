// rtmi_prof.hpp — lane-activity and phase-time profiling hooks (PROF instantiations only).
// Header-only device code, included by every unit that instantiates a kernel (header-only so that every
// kernel instantiation inlines the whole path); arithmetic contract as stated in rtmi_device.hip.
#pragma once
#include "rtmi_types.hpp"

// ---- lane-activity profiling (PROF instantiation only; diagnostics, never on the timed path) -----
// slot s: prof[2s] += active lanes, prof[2s+1] += 64 (one wave-iteration).  Accumulated in LDS,
// flushed to global once per block.
#define RTMI_PROF_SLOTS 32
// Cooperative kernels: the ten words of slots 20..24 (the per-lane state machine's, which no cooperative kernel ticks) count
// the traversal's pop rounds by the number of busy workers, buckets <= 4, <= 8, <= 16, <= 32, <= 64: five words for world
// item 0, then five for every other BVH item together (the split of the TIME slots 27 / 28).
#define RTMI_PROF_ROUND_HIST (2 * 20)
#define RTMI_PROF_ROUND_BUCKETS 5
// ... and two free words: the number of quad rounds (rtmi_bvh_coop.hpp) and, a maximum like slot 18, the most pending
// entries a quad round met
#define RTMI_PROF_QUAD_ROUNDS (2 * 17)
#define RTMI_PROF_QUAD_MAX_ENTRIES (2 * 19)
// 0 compiles the round counters out of the profiling build (-DRTMI_PROF_ROUND_COUNTERS=0): its TIME slots then measure the
// traversal without the counters' LDS atomics
#ifndef RTMI_PROF_ROUND_COUNTERS
#define RTMI_PROF_ROUND_COUNTERS 1
#endif
template <bool PROF>
__device__ __forceinline__ void prof_tick(unsigned long long *prof_lds, int slot, bool active) {
    if (PROF) {
        const unsigned long long m = __ballot(active);
        if (m != 0ull && (int)(__ffsll((long long)m) - 1) == (int)(threadIdx.x & 63)) {
            atomicAdd(&prof_lds[2 * slot], (unsigned long long)__popcll(m));
            atomicAdd(&prof_lds[2 * slot + 1], 64ull);
        }
    }
}

// section timing (PROF only): elapsed shader cycles of this wave since the previous stamp are added
// to slot `slot` (word 0 = cycles, word 1 = number of stamps)
template <bool PROF>
__device__ __forceinline__ void prof_time(unsigned long long *prof_lds, int slot, unsigned long long &t_prev) {
    if (PROF) {
        const unsigned long long t = __builtin_readcyclecounter();
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&prof_lds[2 * slot], t - t_prev);
            atomicAdd(&prof_lds[2 * slot + 1], 1ull);
        }
        t_prev = __builtin_readcyclecounter();
    }
}
