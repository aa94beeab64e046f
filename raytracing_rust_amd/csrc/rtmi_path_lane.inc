// rtmi_path_lane.inc — what a lane of the two-phase render kernels carries from one ray to the next, included by both
// kernel bodies (rtmi_kernel_perlane.inc, rtmi_kernel_coop.inc) right after they have declared the lane's Philox state `g`
// (and attached it to its LDS ring where it has one).
    rng_init(g, 0, 0);
    NeeLane ne;
#ifdef RTMI_PATH_RR
    bool rr_end = false; // the path ends after its pending shadow ray
#endif
    decltype(g) gn; // NEE: the light-sample stream (swapped with g for a shadow ray)
    if constexpr (NEE) {
        rng_set_stream(g, 0u);
        rng_init(gn, 0, 0);
        rng_set_stream(gn, 3u);
        ne.cont_rd = f3(0, 0, 1); ne.c = f3(0, 0, 0); ne.pb = 0.0f; ne.light = 0; ne.shadow = false;
        if constexpr (ENV) ne.env = false;
    }
    Path pa;
    pa.ro = f3(0, 0, 0); pa.rd = f3(0, 0, 1); pa.rtime = 0.0f; pa.T = f3(1, 1, 1); pa.L = f3(0, 0, 0); pa.depth = 0;
    float closest = RTMI_FLT_MAX;
    int best_item = -1, best_pf = 0;
    bool best_medium = false;
