// rtmi_batch.hpp — the take of the batch modes: the radiance queries (rtmi_radiance.hip), the hemisphere gathers
// (rtmi_gather.hip) and the sparse renders (rtmi_sparse.hip, which per-pixel adaptive sampling drives).  Included after
// rtmi_kernels.hpp (rfl).
//
// Items.  A batch is `total` items, item e * ns + s (sample fastest) being sample s of entry e and slot e * ns + s of the
// per-sample buffer, written by path_end: the lanes of a wavefront start on the same or neighbouring entries and walk the
// same subtrees on the first segment, and the resolve (rtmi_batch_welford.inc) reads an entry's samples as one contiguous run.
// Refill.  Two levels, as work_take: a wavefront owns a chunk of consecutive items and deals them to the lanes whose path
// has ended with a ballot and mbcnt, no memory traffic; when the chunk is exhausted it takes the next one from a device
// counter while its other lanes finish paths of the previous chunk, so a wavefront drains once, at the end of the launch.
// The counter is a word of the handle or of the caller's scratch, zeroed on the call's stream before the launch; calls on one
// handle serialise (the busy event), so no two launches ever share it (DESIGN.md §24 has the reason for the counter over a
// grid stride, and the host's rule for the size of a chunk).
#pragma once

struct BatchWork { // wave-uniform: the wavefront's chunk, items [next, end)
    uint32_t next, end;
};
// Persistent wavefront; all 64 lanes call this together.  Every lane with want = true receives the next item of the
// current chunk or, when that is exhausted, of the next chunks of the counter `queue`: chunk u is the items from u * chunk
// on, `nchunks` = ceil(total / chunk) of them (0: no items, every wavefront leaves at once).  Returns false for lanes that
// wanted but found the counter past the last chunk: they are done for good.
__device__ __forceinline__ bool batch_take(BatchWork &w, bool &queue_empty, bool want, unsigned int *queue, uint32_t chunk,
                                           uint32_t total, uint32_t nchunks, uint32_t &item) {
    bool got = false;
    for (;;) {
        const bool still = want && !got;
        const unsigned long long m = __ballot(still);
        if (m == 0ull) break;
        if (w.next >= w.end) { // wave-uniform: chunk exhausted, take the next one
            if (queue_empty) break;
            uint32_t u = 0u;
            if ((threadIdx.x & 63) == 0) u = atomicAdd(queue, 1u);
            u = rfl(u);
            if (u >= nchunks) { queue_empty = true; break; }
            const uint32_t begin = u * chunk; // < total < 2^31
            w.next = rfl(begin);
            w.end = rfl(total - begin < chunk ? total : begin + chunk);
            continue;
        }
        const uint32_t k = w.next + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        w.next = rfl(w.next + (uint32_t)__popcll(m));
        if (still && k < w.end) {
            item = k;
            got = true;
        }
    }
    return got;
}
