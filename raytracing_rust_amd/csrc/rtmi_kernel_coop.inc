// rtmi_kernel_coop.inc — body of the wave-cooperative render kernel (rtmi_kernels.hpp), included INSIDE the kernels that
// run it: rtmi_render_coop (TILE_LIST = false), the adaptive-sampling kernel rtmi_adaptive_coop (rtmi_adaptive.hip,
// TILE_LIST = true) and the lighting kernels of rtmi_light_coop.hip (NEE / ENV, include/rtmi_light_coop.h).  The including
// function provides sc, cam, P, SIG, PROF, EXT, INSTL, ONE_TREE, TILE_LIST, NEE, ENV, `tiles`, `nl` and `ev`; see
// rtmi_kernel_perlane.inc for why this is a textual body, for what NEE and ENV mean and for the RR switch (RTMI_PATH_RR;
// rtmi_roulette_coop_kernel, rtmi_roulette_coop.hip; include/rtmi_roulette_coop.h).  The lane-level path logic is the
// rtmi_path_*.inc fragments', shared with that body; this one provides them the wave's LDS (CoopLds; its pool is phase B's
// scratch), the Philox state `g` in the form the pool allows, and the item scan that all 64 lanes execute together.
// Two seams, as rtmi_path_scan.inc has them, for the batch kernels of rtmi_batch_coop.hip (include/rtmi_batch_coop.h):
// RTMI_COOP_TAKE names the file of the take step (default: rtmi_path_take.inc; with another one `cam`, `tiles` and TILE_LIST
// are not read), and RTMI_COOP_T_MIN / RTMI_COOP_T_MAX are the scan's interval (default: the pinned scalar t_min and
// RTMI_FLT_MAX; a batch kernel's may differ from lane to lane: it travels in the ray context of geom_query_coop).
#ifndef RTMI_COOP_TAKE
#define RTMI_COOP_TAKE "rtmi_path_take.inc"
#define RTMI_COOP_TAKE_DEFAULTED
#endif
#ifndef RTMI_COOP_T_MIN
#define RTMI_COOP_T_MIN t_min
#define RTMI_COOP_T_MAX RTMI_FLT_MAX
#define RTMI_COOP_T_DEFAULTED
#endif
#ifdef RTMI_COOP_T_DEFAULTED
    constexpr bool T_MIN_UNIFORM = true; // a render body: the ray context carries 1/(d.d) in q_min's word (coop_bvh_query's QU),
                                         // 1/(d.d) is pinned before the item loop, the media draw with block-local Philox keys
#else
    constexpr bool T_MIN_UNIFORM = false;
#endif
    constexpr bool INST = INSTL >= 1; // instanced primitives, media inside transforms
    constexpr bool INSD = INSTL >= 2; // DEFERRED items, list scans, nested media
    constexpr bool FEATURES = false; // no feature kernel runs this body
    __shared__ unsigned long long prof_lds[PROF ? 2 * RTMI_PROF_SLOTS : 1];
    unsigned long long *prof = prof_lds;
    if (PROF) {
        if (threadIdx.x < 2 * RTMI_PROF_SLOTS) prof_lds[threadIdx.x] = 0ull;
        __syncthreads();
    }
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_dyn[]; // per wave: CoopLds (rtmi_bvh_coop.hpp)
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    CoopWork cw;
    cw.cap = (int)P.coop_cap;
    const CoopLds lds{(uint32_t)cw.cap, EXT, INSD};
    cw.wlds = lds_dyn + (size_t)wave * lds.words();
    // INSD: the state of a group of DEFERRED items lives in LDS, not in registers that would stay live through every
    // traversal of every scene (parked: 20 VGPRs spilled -> see DESIGN.md §8d): per lane t0 | scan cl | scan holder | scan pf
    uint32_t *park = cw.wlds + lds.park() + lane;
    cw.spill_cap = (int)P.spill_cap;
    cw.spill = P.spill + (size_t)(blockIdx.x * WAVES_PER_BLOCK + wave) * P.spill_cap;
    unsigned long long sig = 0ull;
    WaveWork w;
    w.ltile = 0u; w.ps_base = 0u; w.obase = 0u; w.x0 = 0u; w.y0 = 0u; w.cols = 0u; w.n_valid = 0u; w.next = 0u; w.total = 0u;
    bool queue_empty = false;
    const uint32_t k0 = P.key0, k1 = P.key1;
    const int threshold = (int)P.shade_threshold;
    // Three scalars of the trace loop in registers of their OWN: as members of the kernel-argument block they sit in
    // eight-register tuples, and when the allocator spills such a tuple (this kernel keeps ~100 scalars in VGPR lanes) it
    // restores all eight registers wherever one member is read — found as 48 v_readlane per list scan for the sake of t_min.
    // The copy through an asm statement is a live range the coalescer cannot fold back into the tuple (r04: final_scene
    // +1.5 %, cornell_box +4 % together with the one-pointer primitive records; giving every scene POINTER its own pair
    // the same way lost 2 % / 7 % — profiles/r04_experiments/own_sgprs_ab.log: the allocator is not to be out-guessed twice)
    // ONE_TREE (rtmi_onetree.hip): the host has checked that the call walks alternative trees, that every BVH item has
    // one and that every medium's boundary is a static sphere — use_alt is a constant, and neither the walk of the
    // reference-topology tree nor the boundary queries of a general medium are compiled (DESIGN.md §37)
    float t_min;
    uint32_t n_items, use_alt_w = 1u;
    if constexpr (ONE_TREE) asm volatile("s_mov_b32 %0, %2\n s_mov_b32 %1, %3" : "=&s"(t_min), "=&s"(n_items) : "s"(P.t_min), "s"(sc.n_items));
    else asm volatile("s_mov_b32 %0, %3\n s_mov_b32 %1, %4\n s_mov_b32 %2, %5" : "=&s"(t_min), "=&s"(n_items), "=&s"(use_alt_w) : "s"(P.t_min), "s"(sc.n_items), "s"(P.use_alt));
    const bool use_alt = use_alt_w != 0u;

    uint32_t oidx = 0u, ltile = 0u; // slot of this lane's path in the per-sample buffer; its local tile (SIG only)
    bool alive = false, done = false, have_hit = false, overflow = false;
    // lean instantiation (scenes without alternative trees): word ring in LDS behind pool | ctx | best | dummy
    // (NEE: the register RNG with the stream id in both pool forms; the ring's words stay unused)
    typename std::conditional<NEE, RngNee, typename std::conditional<EXT, RngReg, RngRing>::type>::type g;
    rng_attach(g, cw.wlds + lds.ring());
#include "rtmi_path_lane.inc"
    unsigned long long tstamp = PROF ? __builtin_readcyclecounter() : 0ull;

    for (;;) {
        // ================= phase A =================
        for (;;) {
            if (__ballot(!have_hit && !done) == 0ull) break;
            prof_time<PROF>(prof, 31, tstamp); // loop overhead / phase switching
#include RTMI_COOP_TAKE
            const bool need = !have_hit && !done;
            prof_tick<PROF>(prof, 0, need);
            prof_time<PROF>(prof, 25, tstamp); // camera samples
            RayF W;
            W.o = pa.ro; W.d = pa.rd;
            ray_derive(W);
            if (need) { closest = RTMI_COOP_T_MAX; best_item = -1; best_pf = 0; best_medium = false; }
            // INSD, parked in LDS: [0] the closest hit before a BVH item whose media / instanced-subtree children follow as DEFERRED
            // items (T0); [64] / [128] / [192] the scan of a list with media that was a child of a BVHNode (rtmi.h, LISTSCAN): its
            // closest hit so far, who holds it (item, bit 31: a medium; RTMI_PARK_NONE: nobody) and the primitive
            int grp_first = 0x7fffffff;    // the index of the SAVE_T0 item (or of the first deferred one), and whether it is the enclosing tree
            bool grp_tree = false;
            if (INSD) park[0] = __float_as_uint(RTMI_FLT_MAX);
            // 1/(d.d) of the world ray is a result of THIS statement: without the empty asm the compiler folds the join of
            // W.inv_a with the transformed R.inv_a below into one division of the joined d.d, once per item, although only an
            // item under a rotation changes the value.  Here, not behind ray_derive: there it costs a spilled mask pair
            // (DESIGN.md §39)
            if constexpr (T_MIN_UNIFORM) asm volatile("" : "+v"(W.inv_a)); // (the batch kernels keep the code they had)
            for (uint32_t it = 0; it < n_items; it++) { // executed by all 64 lanes
                const rtmi_item I = RTMI_UNIFORM_LOAD(rtmi_item, &sc.items[it].it);
                if (INSD && (I.flags & RTMI_ITEMFLAG_SAVE_T0)) {
                    park[0] = __float_as_uint(closest); grp_first = (int)it; grp_tree = I.kind == RTMI_ITEM_BVH && !(I.flags & RTMI_ITEMFLAG_DEFERRED);
                }
                if (INSD && (I.flags & RTMI_ITEMFLAG_LISTSCAN_END)) { // wave-uniform: the terminator of a list scan
                    const uint32_t holder = park[128];
                    if (need && holder != RTMI_PARK_NONE) {
                        ListScan ls;
                        ls.cl = __uint_as_float(park[64]); ls.item = (int)(holder & 0x7fffffffu); ls.pf = (int)park[192]; ls.medium = (holder >> 31) != 0u; ls.has = true;
                        listscan_fold(ls, I.first, closest, best_item, best_pf, best_medium, grp_first, grp_tree);
                    }
                    continue;
                }
                if (INSD && (I.flags & RTMI_ITEMFLAG_LISTSCAN_BEGIN)) { park[64] = park[0]; park[128] = RTMI_PARK_NONE; }
                const bool scan = INSD && (I.flags & RTMI_ITEMFLAG_LISTSCAN_MEMBER) != 0u; // wave-uniform
                RayF R = W;
                if (I.xform_count > 0) { // both transforms of a chain of two in ONE scalar fetch (they follow the item record)
                    struct XPair { rtmi_xform x0, x1; };
                    const XPair XP = RTMI_UNIFORM_LOAD(XPair, reinterpret_cast<const XPair *>(&sc.items[it].x0));
                    if (xform_ray_item<true>(sc.xforms, I.xform_first, I.xform_count, XP.x0, XP.x1, R.o, R.d)) ray_derive(R);
                }
                const int slot = 1 + (it < 11u ? (int)it : 11);
                if (!(I.flags & RTMI_ITEMFLAG_MEDIUM)) {
                    float t;
                    int pf;
                    // ONE query site (three inlined copies of the traversal made the INSD instantiations twice the code of the
                    // others): a DEFERRED item — an instanced subtree that was a child of a BVHNode, or a primitive member of a
                    // list scan (rtmi.h) — is reached through its gate and queried up to the t_max its group was entered with
                    // (the scan's closest hit so far); what its hit means is decided afterwards
                    bool reach = need;
                    float qmax = closest;
                    const bool dfi = INSD && (I.flags & RTMI_ITEMFLAG_DEFERRED) != 0u; // wave-uniform
                    if (dfi) {
                        const float t0_saved = __uint_as_float(park[0]);
                        reach = need && deferred_gate(sc, I, W, RTMI_COOP_T_MIN, t0_saved);
                        qmax = scan ? __uint_as_float(park[64]) : t0_saved;
                    }
                    if (geom_query_coop<PROF, EXT, EXT, INST, ONE_TREE, T_MIN_UNIFORM>(sc, I, use_alt, reach, R, pa.rtime, RTMI_COOP_T_MIN, qmax, cw, t, pf, overflow, prof, slot)) {
                        if (scan) {
                            park[64] = __float_as_uint(t); park[128] = it; park[192] = (uint32_t)pf;
                        } else if (!dfi || deferred_bvh_wins(I.count, t, closest, best_item, best_pf, grp_first, grp_tree)) {
                            closest = t; best_item = (int)it; best_pf = pf; best_medium = false;
                        }
                    }
                    prof_time<PROF>(prof, I.kind == RTMI_ITEM_BVH ? (it == 0 ? 27 : 28) : 26, tstamp);
                } else {
                    // ConstantMedium::hit — medium.rs:28-56
                    float t1 = 0.0f, t2 = 0.0f, tm;
                    int pf;
                    bool h1, h2;
                    if (ONE_TREE || (I.flags & RTMI_ITEMFLAG_DEV_MEDIUM_SPHERE)) {
                        // boundary = one static sphere (wave-uniform test; the sphere travels in the item record): both
                        // boundary queries are roots of the same quadratic, evaluated once (same expressions as two
                        // Sphere::hit calls: same bits)
                        h1 = false; h2 = false;
                        if (need) sphere_two_queries(R, make_float4(I.root_min[0], I.root_min[1], I.root_min[2], I.root_max[0]), h1, t1, h2, t2);
                    } else if constexpr (!ONE_TREE) {
                        // INSD: a medium that was a child of a BVHNode (rtmi.h, DEFERRED) is reached through its parent's box
                        const bool dfr = INSD && (I.flags & RTMI_ITEMFLAG_DEFERRED) != 0u; // wave-uniform
                        bool reach = need;
                        float t0_saved = RTMI_FLT_MAX;
                        if (dfr) {
                            t0_saved = scan ? __uint_as_float(park[64]) : __uint_as_float(park[0]); // the interval's end: the scan's closest hit, or T0
                            reach = need && deferred_gate(sc, I, W, RTMI_COOP_T_MIN, __uint_as_float(park[0]));
                        }
                        h1 = geom_query_coop<PROF, EXT, false, INST>(sc, I, use_alt, reach, R, pa.rtime, -RTMI_FLT_MAX, RTMI_FLT_MAX, cw, t1, pf, overflow, prof, slot);
                        h2 = geom_query_coop<PROF, EXT, false, INST>(sc, I, use_alt, reach && h1, R, pa.rtime, t1 + 0.0001f, RTMI_FLT_MAX, cw, t2, pf, overflow, prof, slot);
                        if (INSD && (I.flags & RTMI_ITEMFLAG_NESTED_MEDIUM)) { // wave-uniform: the boundary is itself a medium (rtmi.h)
                            if (reach && h1 && h2) h1 = nested_medium_interval(sc, I, medium_dir_norm<INST>(sc, I.flags, I.xform_first, W), g, k0, k1, t1, t2);
                        }
                        if (dfr) { // its interval ends at the t_max the BVH was entered with; its hit must beat what the tree found
                            if (reach && h1 && h2 && medium_sample<T_MIN_UNIFORM>(t1, t2, RTMI_COOP_T_MIN, t0_saved, medium_dir_norm<INST>(sc, I.flags, I.xform_first, W), I.neg_inv_density, g, k0, k1, tm)) {
                                if (scan) { park[64] = __float_as_uint(tm); park[128] = it | 0x80000000u; }
                                else if (tm < closest) { closest = tm; best_item = (int)it; best_medium = true; }
                            }
                            h1 = false; // done
                        }
                    }
                    if (need && h1 && h2) {
                        // (one square root per medium: sharing it between the media of a query measured -1.1 %,
                        // profiles/r03_experiments/wdn_shared_norm_ab.log)
                        if (medium_sample<T_MIN_UNIFORM>(t1, t2, RTMI_COOP_T_MIN, closest, medium_dir_norm<INST>(sc, I.flags, I.xform_first, W), I.neg_inv_density, g, k0, k1, tm)) {
                            closest = tm; best_item = (int)it; best_medium = true;
                        }
                    }
                    prof_time<PROF>(prof, 29, tstamp); // media
                }
            }
            if (need) {
#include "rtmi_path_traced.inc"
            }
            if (__popcll(__ballot(have_hit)) >= threshold) break;
        }
        // ================= phase B =================
#define RTMI_PATH_SCRATCH cw.wlds
#define RTMI_PATH_INST INST
#include "rtmi_path_shade.inc"
#undef RTMI_PATH_SCRATCH
#undef RTMI_PATH_INST
        prof_time<PROF>(prof, 30, tstamp); // shading
    }
    if (P.ext & RTMI_EXT_TEST_OVERFLOW) overflow = true; // test knob: exercise the error path
    if (__ballot(overflow) != 0ull && lane == 0) atomicAdd(P.status, 1u); // reported loudly by the host

    if (PROF) {
        __syncthreads();
        if (threadIdx.x < 2 * RTMI_PROF_SLOTS && prof_lds[threadIdx.x] != 0ull) {
            if (threadIdx.x == 2 * 18 || threadIdx.x == RTMI_PROF_QUAD_MAX_ENTRIES) atomicMax(P.prof + threadIdx.x, prof_lds[threadIdx.x]); // maxima
            else atomicAdd(P.prof + threadIdx.x, prof_lds[threadIdx.x]);
        }
    }
#ifdef RTMI_COOP_TAKE_DEFAULTED
#undef RTMI_COOP_TAKE
#undef RTMI_COOP_TAKE_DEFAULTED
#endif
#ifdef RTMI_COOP_T_DEFAULTED
#undef RTMI_COOP_T_MIN
#undef RTMI_COOP_T_MAX
#undef RTMI_COOP_T_DEFAULTED
#endif
