// rtmi_path_traced.inc — what both kernel bodies do with a lane whose ray has been traced through the item scan (included
// under `need`): a hit is kept for phase B, a shadow ray that left the world is handed back to its path, a miss ends
// the path.  The including body provides FEATURES (the cooperative one: false).
if (best_item >= 0) {
    have_hit = true;
} else if (NEE && ne.shadow) { // the shadow ray left the world: V = 0; the path goes on
    if constexpr (NEE) {
        if constexpr (ENV) { // ... unless it aims at the map: V = 1
            float eu, evv, eth;
            if (ne.env && env_uv(pa.rd, eu, evv, eth)) pa.L = pa.L + ne.c * env_radiance(ev, eu, evv);
        }
        pa.rd = ne.cont_rd; ne.shadow = false; const auto t = g; g = gn; gn = t;
#ifdef RTMI_PATH_RR
        if (rr_end) { rr_end = false; RTMI_RR_END_PATH(); } // roulette ended the continuation at this shadow ray's vertex
#endif
    }
} else { // miss: black background (color.rs:21); the path ends
    if constexpr (FEATURES) {
        feat_miss(P, oidx, pa);
    } else {
    if constexpr (ENV) { // the map, weighted by MIS after a diffuse scatter that took a light sample
        float eu, evv, eth;
        if (env_uv(pa.rd, eu, evv, eth)) {
            float w = 1.0f;
            if constexpr (NEE) {
                if (ne.pb > 0.0f) {
                    const float pe = env_pdf(ev, eu, evv, eth);
                    if (pe > 0.0f) w = nee_mis_bsdf(ne.pb, pe);
                }
            }
            pa.L = pa.L + pa.T * (env_radiance(ev, eu, evv) * w);
        }
    } else
    if (P.sky) pa.L = pa.L + pa.T * sky_color(pa.rd);
    path_end(P, oidx, pa);
#ifdef RTMI_PATH_RR
    RTMI_RR_COUNT();
#endif
    }
    if (SIG) { atomicAdd(P.path_sig + (size_t)ltile * 64 + (oidx & 63u), sig); sig = 0ull; }
    alive = false;
}
