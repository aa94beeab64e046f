// rtmi_path_take.inc — start of a round of phase A in both kernel bodies: lanes whose path ended take the next
// (sample, pixel) item of the chunk (work_take: the queue of rtmi_path_lane.inc), or are done when there is none.
{
    const bool want = !have_hit && !done && !alive;
    if (__ballot(want) != 0ull) {
        uint32_t smp = 0u, px = 0u, j = 0u;
        if (work_take<TILE_LIST>(w, queue_empty, want, P, oidx, ltile, smp, px, j, tiles)) {
            camera_sample(cam, P, g, k0, k1, smp, j * P.nx + px, px, j, pa);
            if constexpr (NEE) { rng_init(gn, smp, j * P.nx + px); ne.pb = 0.0f; }
            alive = true;
        } else if (want) {
            done = true;
        }
    }
}
