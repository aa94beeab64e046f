// rtmi_path_shade.inc — phase B of both kernel bodies: every lane that holds a hit shades it; the path scatters, hands
// over to a pending shadow ray (the two Philox streams swap), is cut by roulette, or ends: written and counted here.
// The including body defines RTMI_PATH_SCRATCH (the wave's LDS, idle during shading) and RTMI_PATH_INST (shade_hit's INST:
// whether primitives can carry transforms) before the include and undefines them after it.  RTMI_PATH_TREE
// (rtmi_light_tree.hip; include/rtmi_light_tree.h) is a preprocessor switch as RTMI_PATH_RR is: with it the including
// function also provides `lt` (DevLightTree) and NEE's light comes from the tree; without it this text is what it was.
if (__ballot(have_hit) == 0ull) break; // nobody holds a hit and nobody can trace: all done
prof_tick<PROF>(prof, 16, have_hit);
{
    const bool shading = have_hit;
    have_hit = false;
    if (SIG && shading && !(NEE && ne.shadow)) sig += (unsigned long long)sig_mix(__float_as_uint(closest), pa.depth);
    // all lanes call (wavefront texture lookup); the traversal's LDS is idle now: scratch
    if constexpr (FEATURES) { // the first interaction ends every path: its record goes to the feature slot
        ShadeFeat feat;
        shade_hit<decltype(g), RTMI_PATH_INST, true>(sc, P.max_depth, P.ext, g, k0, k1, shading, closest, best_item, best_pf, best_medium,
                                      pa, reinterpret_cast<float *>(RTMI_PATH_SCRATCH), &feat);
        if (shading) {
            feat_hit(P, oidx, pa, closest, feat);
            if (SIG) { atomicAdd(P.path_sig + (size_t)ltile * 64 + (oidx & 63u), sig); sig = 0ull; }
            alive = false;
        }
    } else if constexpr (NEE) {
        const bool was_shadow = ne.shadow;
#ifdef RTMI_PATH_TREE
        const bool goes_on = shade_hit<decltype(g), RTMI_PATH_INST, false, true, ENV, true>(
            sc, P.max_depth, P.ext, g, k0, k1, shading, closest, best_item, best_pf, best_medium, pa,
            reinterpret_cast<float *>(RTMI_PATH_SCRATCH), nullptr, &nl, &ne, &gn, &ev, &lt);
#else
        const bool goes_on = shade_hit<decltype(g), RTMI_PATH_INST, false, true, ENV>(
            sc, P.max_depth, P.ext, g, k0, k1, shading, closest, best_item, best_pf, best_medium, pa,
            reinterpret_cast<float *>(RTMI_PATH_SCRATCH), nullptr, &nl, &ne, &gn, &ev);
#endif
        if (shading) {
            if (was_shadow) { // the light sample is counted: the path's continuation is traced next
                pa.rd = ne.cont_rd; ne.shadow = false;
                const auto t = g; g = gn; gn = t;
#ifdef RTMI_PATH_RR
                if (rr_end) { rr_end = false; RTMI_RR_END_PATH(); } // roulette ended the continuation at this shadow ray's vertex
#endif
            } else if (!goes_on) {
                path_end(P, oidx, pa);
#ifdef RTMI_PATH_RR
                RTMI_RR_COUNT();
#endif
                if (SIG) { atomicAdd(P.path_sig + (size_t)ltile * 64 + (oidx & 63u), sig); sig = 0ull; }
                alive = false;
#ifdef RTMI_PATH_RR
            } else if (!roulette_survives(rr, g, k0, k1, pa)) { // g is still the path's stream here
                if (ne.shadow) { // the vertex's light sample is still traced and counted
                    rr_end = true;
                    const auto t = g; g = gn; gn = t;
                } else {
                    RTMI_RR_END_PATH();
                }
#endif
            } else if (ne.shadow) { // a shadow ray was sampled: trace it with the light-sample stream
                const auto t = g; g = gn; gn = t;
            }
        }
    } else {
    const bool goes_on = shade_hit<decltype(g), RTMI_PATH_INST>(sc, P.max_depth, P.ext, g, k0, k1, shading, closest, best_item, best_pf, best_medium, pa,
                                   reinterpret_cast<float *>(RTMI_PATH_SCRATCH));
    if (shading && !goes_on) {
        // absorbed, emitter or depth limit: the path ends
        path_end(P, oidx, pa);
#ifdef RTMI_PATH_RR
        RTMI_RR_COUNT();
#endif
        if (SIG) { atomicAdd(P.path_sig + (size_t)ltile * 64 + (oidx & 63u), sig); sig = 0ull; }
        alive = false;
    }
#ifdef RTMI_PATH_RR
    else if (shading && !roulette_survives(rr, g, k0, k1, pa)) {
        RTMI_RR_END_PATH();
    }
#endif
    }
}
