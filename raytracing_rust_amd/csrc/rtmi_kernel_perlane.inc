// rtmi_kernel_perlane.inc — body of the per-lane two-phase render kernel (rtmi_kernels.hpp), included INSIDE the kernels
// that run it: rtmi_render_kernel (TILE_LIST = false) and the adaptive-sampling kernel rtmi_adaptive_kernel (rtmi_adaptive.hip,
// TILE_LIST = true: the queue runs over a list of tiles, see wave_work).  The including function provides sc, cam, P, FAST, SIG,
// PROF, TILE_LIST, FEATURES, NEE, `nl` and `tiles`.  FEATURES (rtmi_features_kernel, rtmi_features.hip): every path ends at
// its first interaction, which writes a FeatSlot (rtmi_shade.hpp) to the per-sample buffer instead of a radiance.  NEE
// (rtmi_nee_kernel, rtmi_nee.hip; include/rtmi_nee.h): a lane holds either its path ray or a pending shadow ray toward a
// light sample (NeeLane); both are traced by the same item scan, the shadow ray with the light-sample stream swapped in
// for the path's, and never touch the signature.  `nl`: the light table (DevLights).  ENV (rtmi_env_kernel, rtmi_env.hip;
// include/rtmi_env.h): a ray that leaves the world sees the map `ev` (DevEnv) instead of black or the sky; with NEE the
// map is one more light, and a shadow ray toward it counts when it leaves the world.  A textual body
// and not a force-inlined function: inlining one changed the instruction stream of every existing instantiation (same
// instructions in another order and register assignment), and those must stay bit-for-bit what they were.
// RR (rtmi_roulette_kernel, rtmi_roulette.hip; include/rtmi_roulette.h) is a preprocessor switch for that reason: without
// RTMI_PATH_RR this text is what it was.  With it the including function also provides `rr` (DevRoulette) and
// roulette_survives, RTMI_RR_COUNT() (adds the written path's depth to rr.bounces) and RTMI_RR_END_PATH() (writes the
// path, counts it and frees the lane): the test follows every scatter in phase B, and a lane whose continuation ends with a
// shadow ray pending sets rr_end and is written where that shadow ray is handed back.
// The lane-level path logic is the rtmi_path_*.inc fragments', shared with rtmi_kernel_coop.inc; this body provides them
// the per-lane traversal stacks (phase B's scratch), the register Philox state `g` and the item scan each lane runs alone.
    __shared__ unsigned long long prof_lds[PROF ? 2 * RTMI_PROF_SLOTS : 1];
    unsigned long long *prof = prof_lds;
    if (PROF) {
        if (threadIdx.x < 2 * RTMI_PROF_SLOTS) prof_lds[threadIdx.x] = 0ull;
        __syncthreads();
    }
    // per wave: [0] node refs, [1] entry distances (FAST only); entry-major so lanes never bank-conflict
    __shared__ uint32_t lds_stack[WAVES_PER_BLOCK][FAST ? 2 : 1][RTMI_MAX_BVH_DEPTH][64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    uint32_t *stack = &lds_stack[wave][0][0][lane];
    unsigned long long sig = 0ull;
    WaveWork w;
    w.ltile = 0u; w.ps_base = 0u; w.obase = 0u; w.x0 = 0u; w.y0 = 0u; w.cols = 0u; w.n_valid = 0u; w.next = 0u; w.total = 0u;
    bool queue_empty = false;
    const uint32_t k0 = P.key0, k1 = P.key1;
    const int threshold = (int)P.shade_threshold;

    uint32_t oidx = 0u, ltile = 0u; // slot of this lane's path in the per-sample buffer; its local tile (SIG only)
    bool alive = false, done = false, have_hit = false;
    typename std::conditional<NEE, RngNee, RngReg>::type g;
#include "rtmi_path_lane.inc"

    for (;;) {
        // ================= phase A: trace until enough lanes hold a hit =================
        for (;;) {
            if (__ballot(!have_hit && !done) == 0ull) break;
#include "rtmi_path_take.inc"
            const bool need = !have_hit && !done;
            prof_tick<PROF>(prof, 0, need);
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

    if (PROF) {
        __syncthreads();
        if (threadIdx.x < 2 * RTMI_PROF_SLOTS && prof_lds[threadIdx.x] != 0ull) atomicAdd(P.prof + threadIdx.x, prof_lds[threadIdx.x]);
    }
