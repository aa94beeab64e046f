// rtmi_batch_coop_take.inc — the take step of the cooperative batch kernels (rtmi_batch_coop.hip), included by
// rtmi_kernel_coop.inc through its RTMI_COOP_TAKE seam in place of rtmi_path_take.inc: lanes whose path ended take the next
// item of the batch (batch_take, rtmi_batch.hpp) and start its path as the per-lane kernel of the same mode starts it
// (rtmi_radiance.hip, rtmi_gather.hip, rtmi_sparse.hip: the same statements in the same order).  RTMI_BATCH_COOP_MODE
// selects the mode; the including kernel provides the batch `B`, the wavefront's chunk `bw` and, per mode: the lane's
// `first`, `ray_t_min`, `ray_t_max` (radiance), `cam`, `total` and `nchunks` (sparse).
#if RTMI_BATCH_COOP_MODE == RTMI_BATCH_COOP_RADIANCE
// A lane scans in the very round it takes (it is alive and holds no hit), so "cleared after the lane's first scan" is
// "cleared at the start of the next round": before phase B, hence before any shadow ray can be pending.
first = false;
#endif
{
    const bool want = !have_hit && !done && !alive;
    if (__ballot(want) != 0ull) {
#if RTMI_BATCH_COOP_MODE == RTMI_BATCH_COOP_SPARSE
        if (batch_take(bw, queue_empty, want, B.queue, B.chunk, total, nchunks, oidx)) {
            const uint32_t k = oidx / B.ns, s = oidx - k * B.ns;
            // the list indexes the image's planes, row 0 the top row; the render counts its rows from the bottom
            const uint32_t p = B.list[k];
            const uint32_t row = p / P.nx, px = p - row * P.nx;
            const uint32_t j = P.ny - 1u - row, pixel = j * P.nx + px; // a row outside the image wraps: some path
            camera_sample(cam, P, g, k0, k1, B.first_sample + s, pixel, px, j, pa);
            if constexpr (NEE) { rng_init(gn, B.first_sample + s, pixel); ne.pb = 0.0f; }
#elif RTMI_BATCH_COOP_MODE == RTMI_BATCH_COOP_GATHER
        if (batch_take(bw, queue_empty, want, B.queue, B.chunk, B.total, B.nchunks, oidx)) {
            const uint32_t i = oidx / B.spp, s = oidx - i * B.spp;
            const float *pt = B.points + 3 * (size_t)i;
            pa.ro = f3(pt[0], pt[1], pt[2]);
            float nrm[3] = {0.0f, 0.0f, 1.0f}, d[3];
            if constexpr (!SPHERE) {
                const float *pn = B.normals + 3 * (size_t)i;
                nrm[0] = pn[0]; nrm[1] = pn[1]; nrm[2] = pn[2];
            }
            batch_gather_direction<SPHERE>(k0, k1, B.first_sample + s, B.first_point + i, nrm, d);
            pa.rd = f3(d[0], d[1], d[2]);
            pa.rtime = B.time ? B.time[i] : 0.0f;
            pa.T = f3(1, 1, 1);
            pa.L = f3(0, 0, 0);
            pa.depth = 0;
            rng_init(g, B.first_sample + s, B.first_point + i);
            if constexpr (NEE) { rng_init(gn, B.first_sample + s, B.first_point + i); ne.pb = 0.0f; }
#else
        if (batch_take(bw, queue_empty, want, B.queue, B.chunk, B.total, B.nchunks, oidx)) {
            const uint32_t i = oidx / B.spp, s = oidx - i * B.spp;
            const float4 r0 = B.rays[2 * (size_t)i], r1 = B.rays[2 * (size_t)i + 1];
            pa.ro = f3(r0.x, r0.y, r0.z);
            pa.rd = f3(r1.x, r1.y, r1.z);
            pa.rtime = B.time ? B.time[i] : 0.0f;
            pa.T = f3(1, 1, 1);
            pa.L = f3(0, 0, 0);
            pa.depth = 0;
            ray_t_min = r0.w;
            ray_t_max = r1.w < RTMI_FLT_MAX ? r1.w : RTMI_FLT_MAX; // +inf, >= FLT_MAX: the render's
            first = true;
            rng_init(g, B.first_sample + s, B.first_ray + i);
            batch_rng_seek(g, k0, k1, B.skip_block, B.skip_pos);
            if constexpr (NEE) { rng_init(gn, B.first_sample + s, B.first_ray + i); ne.pb = 0.0f; }
#endif
            alive = true;
        } else if (want) {
            done = true;
        }
    }
}
#if RTMI_BATCH_COOP_MODE == RTMI_BATCH_COOP_RADIANCE
// the interval of this round's scan (RTMI_COOP_T_MIN / RTMI_COOP_T_MAX of the including kernel): the caller's own on a
// ray's first segment, the render's afterwards
const float scan_t_min = first ? ray_t_min : t_min;
const float scan_t_max = first ? ray_t_max : RTMI_FLT_MAX;
#endif
