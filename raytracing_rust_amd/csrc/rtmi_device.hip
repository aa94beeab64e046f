// rtmi_device.hip — gfx950 (MI355X, CDNA4) device path of the per-pixel render loop.
//
// Persistent wavefronts (256 CUs x 16) take units = (8x8 pixel tile, 16 samples) from a global counter; the
// 64 lanes of a wavefront take (sample, pixel) items of its unit dynamically: a lane whose path ended
// starts the next item at once, whatever its pixel, so all lanes stay busy although path lengths differ
// (1..51 hit queries, src/color.rs:6-23).  Every finished path stores its radiance in a per-sample
// buffer in HBM; a resolve kernel adds the samples of a pixel in sample order (tests/test.rs:65-70).
// The recursion of `color` is unrolled into the throughput form L += T*emitted; T *= attenuation.
// Random numbers are Philox4x32-10 counter streams keyed per (pixel, sample), so the result is
// independent of scheduling, tiling, unit size and the number of GPUs.  BVH traversal is cooperative:
// the lanes are workers on a wave-shared LIFO of (ray, node) entries in LDS (rtmi_bvh_coop.hpp).
// No MFMA: there is no dense contraction on this path.
//
// Arithmetic follows the fp32 contract of DESIGN.md: op order as written here, no FMA
// contraction (-ffp-contract=off), IEEE / and sqrt, transcendental functions from
// include/rtmi_math.h.  Every device function cites the reference lines it implements.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <time.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "rtmi.h"
#include "rtmi_math.h"

#include "rtmi_kernels.hpp"
#include "rtmi_render_launch.hpp"
#include "rtmi_probe_path_launch.hpp"
#include "rtmi_f64_types.hpp"
#include "rtmi_f64_plan.hpp"
#include "rtmi_adaptive.h"
#include "rtmi_adaptive_launch.hpp"
#include "rtmi_features.h"
#include "rtmi_features_launch.hpp"
#include "rtmi_nee.h"
#include "rtmi_env.h"
#include "rtmi_adaptive_nee.h"
#include "rtmi_roulette.h"
#include "rtmi_light_coop.h"
#include "rtmi_roulette_coop.h"
#include "rtmi_light_tree.h"
#include "rtmi_light_launch.hpp"
#include "rtmi_session.h"
#include "rtmi_session_launch.hpp"
#include "rtmi_query.h"
#include "rtmi_query_launch.hpp"
#include "rtmi_frame_launch.hpp"
#include "rtmi_hostkit.hpp"
#include "rtmi_host.hpp"

// ======================================================================================
// the launchers of rtmi_render_launch.hpp: the only place where the kernels of this unit are launched
// ======================================================================================
hipError_t rtmi_render_launch(const RenderLaunch &k, uint32_t blocks, hipStream_t stream, const DevScene &sc, const DevCamera &cam,
                              const DevParams &P) {
    const dim3 grid(blocks), block(64 * WAVES_PER_BLOCK);
#define RTMI_LAUNCH(KERN, F, S, PR, LDS) hipLaunchKernelGGL((KERN<F, S, PR>), grid, block, LDS, stream, sc, cam, P)
#define RTMI_LAUNCH_COOP(S, PR, W, E, I) return rtmi_launch_lds(&rtmi_render_coop<S, PR, W, E, I>, grid, block, k.coop_lds, stream, sc, cam, P)
    if (k.bcoop) {
        const dim3 blk(RTMI_BLK_THREADS);
        if (k.sigf) hipLaunchKernelGGL((rtmi_render_bcoop<true, false>), grid, blk, k.bcoop_lds, stream, sc, cam, P);
        else hipLaunchKernelGGL((rtmi_render_bcoop<false, false>), grid, blk, k.bcoop_lds, stream, sc, cam, P);
    } else if (k.coop) {
        if (k.inst) { // instanced primitives, media inside transforms: their own instantiations (no diagnostics builds)
            // (with k.prof there is no instantiation: the host has refused that call)
            // level 2 (DEFERRED items, list scans, nested media; its group state parked in LDS) also serves the scenes that
            // need level 1 only when they have trees: measured faster there than level 1's own instantiation (forced on
            // final_scene -5.2 % against -7.8 %, random_spheres -3.4 % / -3.1 %); without trees level 1 is the faster one
            // (cornell_box -9.5 % against -18 %) — profiles/r04_experiments/inst_levels_ab3_parked.log
            if (k.insd) {
                if (k.sigf) RTMI_LAUNCH_COOP(true, false, 4, true, 2);
                else if (k.ext) RTMI_LAUNCH_COOP(false, false, 4, true, 2);
                else RTMI_LAUNCH_COOP(false, false, 4, false, 2);
            } else {
                RTMI_LAUNCH_COOP(false, false, 4, false, 1);
            }
        }
        else if (k.prof) RTMI_LAUNCH_COOP(false, true, 3, true, 0);
        else if (k.sigf) RTMI_LAUNCH_COOP(true, false, 4, true, 0);
        else if (k.wps == 3) RTMI_LAUNCH_COOP(false, false, 3, true, 0);
        else if (k.wps == 5) RTMI_LAUNCH_COOP(false, false, 5, true, 0);
        else if (k.one_tree) return rtmi_launch_lds(&rtmi_render_coop<false, false, 4, true, 0, true>, grid, block, k.coop_lds, stream, sc, cam, P);
        else if (k.ext) RTMI_LAUNCH_COOP(false, false, 4, true, 0);
        else RTMI_LAUNCH_COOP(false, false, 4, false, 0);
    } else if (!k.async) {
        if (k.prof) { if (k.fast) RTMI_LAUNCH(rtmi_render_kernel, true, false, true, 0); else RTMI_LAUNCH(rtmi_render_kernel, false, false, true, 0); }
        else if (k.fast && k.sigf) RTMI_LAUNCH(rtmi_render_kernel, true, true, false, 0);
        else if (k.fast) RTMI_LAUNCH(rtmi_render_kernel, true, false, false, 0);
        else if (k.sigf) RTMI_LAUNCH(rtmi_render_kernel, false, true, false, 0);
        else RTMI_LAUNCH(rtmi_render_kernel, false, false, false, 0);
    } else {
        if (k.prof) { if (k.fast) RTMI_LAUNCH(rtmi_render_async, true, false, true, k.dyn_lds); else RTMI_LAUNCH(rtmi_render_async, false, false, true, k.dyn_lds); }
        else if (k.fast && k.sigf) RTMI_LAUNCH(rtmi_render_async, true, true, false, k.dyn_lds);
        else if (k.fast) RTMI_LAUNCH(rtmi_render_async, true, false, false, k.dyn_lds);
        else if (k.sigf) RTMI_LAUNCH(rtmi_render_async, false, true, false, k.dyn_lds);
        else RTMI_LAUNCH(rtmi_render_async, false, false, false, k.dyn_lds);
    }
#undef RTMI_LAUNCH
#undef RTMI_LAUNCH_COOP
    return hipGetLastError();
}

hipError_t rtmi_render_launch_resolve(hipStream_t stream, const Rad3 *samples, double *partial, rtmi_texel *out, const DevParams &P,
                                      bool first, bool last, bool progressive) {
    const uint32_t ntex = P.ntiles_local * 64u;
    hipLaunchKernelGGL(rtmi_resolve_kernel, dim3((ntex + 255) / 256), dim3(256), 0, stream, samples, partial, out, P, first ? 1 : 0,
                       last ? 1 : 0, progressive ? 1 : 0);
    return hipGetLastError();
}

hipError_t rtmi_render_launch_pass_end(hipStream_t stream, unsigned int *status, unsigned int units, unsigned int pass_spp, bool last) {
    hipLaunchKernelGGL(rtmi_pass_end_kernel, dim3(1), dim3(1), 0, stream, status, units, pass_spp, last ? 1 : 0);
    return hipGetLastError();
}

hipError_t rtmi_render_launch_probe_math(int op, const float *x, const float *y, float *out, uint32_t n) {
    hipLaunchKernelGGL(rtmi_math_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, op, x, y, out, n);
    return hipGetLastError();
}

hipError_t rtmi_render_launch_probe_xform(const rtmi_xform *xf, int count, const float *a, const float *b, float *out, uint32_t n) {
    hipLaunchKernelGGL(rtmi_xform_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, xf, count, a, b, out, n);
    return hipGetLastError();
}

hipError_t rtmi_render_launch_probe_philox(const uint32_t *ctr, const uint32_t *key, uint32_t *out, uint32_t n) {
    hipLaunchKernelGGL(rtmi_philox_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, ctr, key, out, n);
    return hipGetLastError();
}

hipError_t rtmi_render_launch_probe_geom(int op, const DevScene &sc, const float *in, float *out, uint32_t n) {
    hipLaunchKernelGGL(rtmi_geom_probe_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, op, sc, in, out, n);
    return hipGetLastError();
}

// ======================================================================================
// host side of the C ABI
// ======================================================================================
static thread_local std::string g_err;

extern "C" const char *rtmi_last_error(void) { return g_err.c_str(); }
// the message rtmi_last_error returns, set by the entry points of the other translation units (rtmi_denoise.hip)
RTMI_HIDDEN int rtmi_fail(int code, const char *msg) {
    g_err = msg;
    return code;
}

#ifndef RTMI_BUILD_HASH
#define RTMI_BUILD_HASH "unknown"
#endif
extern "C" const char *rtmi_build_hash(void) { return RTMI_BUILD_HASH; }

// Per-sample buffers outlive their handle, one per device: a destroyed handle parks its buffer here and the next
// handle on that device takes it over when it is large enough.  Why: hipMalloc of tens of GB right after a hipFree of
// the same size stalls for SECONDS now and then on this stack (profiles/r04_experiments/first_call_probe.log: 0.3 ms
// nine times, then 4.6 s and 5.0 s for the same 25 GB; the r03 bench record shows one such stall as a 1.3 s first
// call), and a host that renders one image per handle (rtmi_render_multi, Camera::render — the reference's usage
// model is one render per process, tests/test.rs:802-838) would meet it again and again.  At most one buffer per device
// is parked; rtmi_release_cached() returns the memory.
namespace {
struct ParkedSamples { void *ptr = nullptr; size_t bytes = 0; };
std::mutex g_parked_mu;
std::map<int, ParkedSamples> g_parked;
// takes the parked buffer of `device` if it holds at least `need` bytes
bool parked_take(int device, size_t need, void **ptr, size_t *bytes) {
    std::lock_guard<std::mutex> lock(g_parked_mu);
    auto it = g_parked.find(device);
    if (it == g_parked.end() || !it->second.ptr || it->second.bytes < need) return false;
    *ptr = it->second.ptr; *bytes = it->second.bytes;
    g_parked.erase(it);
    return true;
}
size_t parked_bytes(int device) {
    std::lock_guard<std::mutex> lock(g_parked_mu);
    auto it = g_parked.find(device);
    return it == g_parked.end() ? 0 : it->second.bytes;
}
// frees what is parked on `device` (the current HIP device must be `device`)
void parked_drop(int device) {
    std::lock_guard<std::mutex> lock(g_parked_mu);
    auto it = g_parked.find(device);
    if (it == g_parked.end()) return;
    if (it->second.ptr) (void)hipFree(it->second.ptr);
    g_parked.erase(it);
}
// parks the allocation of `from` (no kernel uses it any more) unless a larger one is parked already; the loser is freed
void parked_give(int device, DeviceBuf<Rad3> &from) {
    size_t bytes = 0;
    void *const ptr = from.give(&bytes);
    std::lock_guard<std::mutex> lock(g_parked_mu);
    ParkedSamples &slot = g_parked[device];
    if (slot.ptr && slot.bytes >= bytes) { (void)hipFree(ptr); return; }
    if (slot.ptr) (void)hipFree(slot.ptr);
    slot.ptr = ptr; slot.bytes = bytes;
}
} // namespace

extern "C" void rtmi_release_cached(void) {
    int cur = 0;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    std::lock_guard<std::mutex> lock(g_parked_mu);
    for (auto &kv : g_parked)
        if (kv.second.ptr && hipSetDevice(kv.first) == hipSuccess) (void)hipFree(kv.second.ptr);
    g_parked.clear();
    if (have_cur) (void)hipSetDevice(cur);
}

extern "C" int rtmi_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

template <typename T>
static int upload(rtmi_scene *s, const T *src, size_t n, const T **dst) {
    *dst = nullptr;
    size_t bytes = (n ? n : 1) * sizeof(T);
    void *p = nullptr;
    HIP_TRY(s->allocs.add(&p, bytes));
    if (n) HIP_TRY(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
    *dst = reinterpret_cast<const T *>(p);
    return RTMI_OK;
}

int validate(const rtmi_scene_desc *d) {
    if (!d) return fail(RTMI_ERR_INVALID, "desc is NULL");
    if (d->abi_version != RTMI_ABI_VERSION) return fail(RTMI_ERR_INVALID, "abi_version mismatch");
    if (d->n_items == 0 || !d->items) return fail(RTMI_ERR_INVALID, "scene has no items");
    if (d->max_bvh_depth > RTMI_MAX_BVH_DEPTH)
        return fail(RTMI_ERR_UNSUPPORTED, "BVH deeper than RTMI_MAX_BVH_DEPTH");
    if (d->n_prims >= (1u << 28)) return fail(RTMI_ERR_UNSUPPORTED, "too many primitives");
    if ((d->n_prims && (!d->prim_a || !d->prim_b || !d->prim_meta)) || (d->n_nodes && !d->nodes) || (d->n_xforms && !d->xforms) ||
        (d->n_materials && !d->materials) || (d->n_textures && !d->textures) || (d->n_perlin && !d->perlin) ||
        (d->n_images && !d->images) || (d->image_bytes && !d->image_data))
        return fail(RTMI_ERR_INVALID, "a non-zero count comes with a NULL array");
    auto prim_ok = [&](int64_t i) { return i >= 0 && (uint64_t)i < d->n_prims; };
    for (uint32_t i = 0; i < d->n_prims; i++) {
        const rtmi_prim_meta &m = d->prim_meta[i];
        if (m.type < 0 || m.type > RTMI_PRIM_CUBE) return fail(RTMI_ERR_INVALID, "bad primitive type");
        if (m.material < 0 || (uint32_t)m.material >= d->n_materials)
            return fail(RTMI_ERR_INVALID, "primitive material out of range");
        const uint32_t xfc = (m.flags >> RTMI_PRIMFLAG_XF_COUNT_SHIFT) & RTMI_PRIM_XF_MAX, xff = m.flags >> RTMI_PRIMFLAG_XF_FIRST_SHIFT;
        if (xfc != 0u && ((uint64_t)xff + xfc > d->n_xforms)) return fail(RTMI_ERR_INVALID, "primitive transform range out of bounds");
        for (uint32_t k = 0; k < xfc; k++) // (gate and inner-medium records are no transforms: never inside a chain)
            if (d->xforms[xff + k].kind > RTMI_XF_ROTATE_Z) return fail(RTMI_ERR_INVALID, "a gate or inner-medium record inside a primitive's transform chain");
    }
    for (uint32_t i = 0; i < d->n_xforms; i++)
        if (d->xforms[i].kind < RTMI_XF_TRANSLATE || d->xforms[i].kind > RTMI_XF_INNER_MEDIUM) return fail(RTMI_ERR_INVALID, "bad transform kind");
    for (uint32_t i = 0; i < d->n_nodes; i++) {
        const int32_t ch[2] = {d->nodes[i].left, d->nodes[i].right};
        for (int c = 0; c < 2; c++) {
            if (ch[c] >= 0) {
                if ((uint32_t)ch[c] >= d->n_nodes) return fail(RTMI_ERR_INVALID, "BVH child out of range");
            } else {
                uint32_t type = ((uint32_t)ch[c] >> 28) & 7u, idx = (uint32_t)ch[c] & 0x0fffffffu;
                if (type > RTMI_PRIM_CUBE || !prim_ok(idx)) return fail(RTMI_ERR_INVALID, "BVH leaf out of range");
                if ((int)type != d->prim_meta[idx].type) return fail(RTMI_ERR_INVALID, "BVH leaf type mismatch");
            }
        }
    }
    // alternative-tree records: children in range, leaves typed like the primitive they name
    if (d->n_alt_nodes && !d->alt_nodes) return fail(RTMI_ERR_INVALID, "n_alt_nodes without alt_nodes");
    // the traversals address a 128-B node record by a 32-bit byte offset and keep a node index in 25 bits of a pool entry
    if (d->n_alt_nodes >= (1u << 25)) return fail(RTMI_ERR_UNSUPPORTED, "too many alternative tree nodes");
    for (uint32_t i = 0; i < d->n_alt_nodes; i++)
        for (int c = 0; c < 4; c++) {
            const int32_t ch = d->alt_nodes[i].child[c];
            if (ch == RTMI_NO_CHILD) continue;
            if (ch >= 0) {
                if ((uint32_t)ch >= d->n_alt_nodes) return fail(RTMI_ERR_INVALID, "alternative tree child out of range");
            } else {
                const uint32_t type = ((uint32_t)ch >> 28) & 7u, idx = (uint32_t)ch & 0x0fffffffu;
                if (type > RTMI_PRIM_CUBE || !prim_ok(idx)) return fail(RTMI_ERR_INVALID, "alternative tree leaf out of range");
                if ((int)type != d->prim_meta[idx].type) return fail(RTMI_ERR_INVALID, "alternative tree leaf type mismatch");
            }
        }
    // Walk every tree from its item's root.  The kernels size their traversal stacks from the DECLARED depths
    // (fixed RTMI_MAX_BVH_DEPTH-entry LDS stack per lane; pool spill capacity), and a persistent wavefront that
    // follows a child cycle never ends: each node may be reached once (no cycles, no shared subtrees) and no
    // deeper than declared.  Depth of a root = 1, as the lowering counts it.
    std::vector<uint8_t> seen_bin(d->n_nodes, 0), seen_alt(d->n_alt_nodes, 0);
    std::vector<std::pair<uint32_t, uint32_t>> todo; // (node, depth)
    const auto walk = [&](bool alt, uint32_t root, uint32_t declared, const char *what) -> int {
        std::vector<uint8_t> &seen = alt ? seen_alt : seen_bin;
        todo.clear();
        todo.emplace_back(root, 1u);
        while (!todo.empty()) {
            const uint32_t n = todo.back().first, depth = todo.back().second;
            todo.pop_back();
            if (seen[n]) return fail(RTMI_ERR_INVALID, std::string(what) + ": a node is reached twice (cycle or shared subtree)");
            seen[n] = 1;
            if (depth > declared) return fail(RTMI_ERR_INVALID, std::string(what) + " is deeper than the declared depth");
            if (alt) {
                for (int c = 0; c < 4; c++) {
                    const int32_t ch = d->alt_nodes[n].child[c];
                    if (ch >= 0 && ch != RTMI_NO_CHILD) todo.emplace_back((uint32_t)ch, depth + 1u);
                }
            } else {
                const int32_t l = d->nodes[n].left, r = d->nodes[n].right;
                if (l >= 0) todo.emplace_back((uint32_t)l, depth + 1u);
                // right == left is legal: BVHNode::new over ONE element stores it on both sides (bvh.rs:44-45); the
                // kernels visit it once.  Any other repeated reference is caught by `seen`.
                if (r >= 0 && r != l) todo.emplace_back((uint32_t)r, depth + 1u);
            }
        }
        return RTMI_OK;
    };
    bool scan_open = false;
    for (uint32_t i = 0; i < d->n_items; i++) {
        const rtmi_item &it = d->items[i];
        if (it.kind == RTMI_ITEM_LIST) {
            if (it.count < 0) return fail(RTMI_ERR_INVALID, "item primitive count is negative");
            if (it.count > 0 && (!prim_ok(it.first) || !prim_ok((int64_t)it.first + it.count - 1)))
                return fail(RTMI_ERR_INVALID, "item primitive range out of bounds");
        } else if (it.kind == RTMI_ITEM_BVH) {
            if (it.first < 0 || (uint32_t)it.first >= d->n_nodes) return fail(RTMI_ERR_INVALID, "item BVH root out of range");
            if (int rc = walk(false, (uint32_t)it.first, d->max_bvh_depth, "BVH")) return rc;
            if (it.alt_first >= 0) {
                if ((uint32_t)it.alt_first >= d->n_alt_nodes || !d->prim_gate || !d->alt_nodes)
                    return fail(RTMI_ERR_INVALID, "item alternative tree out of range or prim_gate missing");
                if (d->alt_max_depth > 64u) return fail(RTMI_ERR_UNSUPPORTED, "alternative tree deeper than 64");
                if (int rc = walk(true, (uint32_t)it.alt_first, d->alt_max_depth, "alternative tree")) return rc;
            }
        } else {
            return fail(RTMI_ERR_INVALID, "bad item kind");
        }
        if (it.xform_count < 0 || it.xform_first < 0 || (uint32_t)(it.xform_first + it.xform_count) > d->n_xforms)
            return fail(RTMI_ERR_INVALID, "item transform range out of bounds");
        if ((it.flags & RTMI_ITEMFLAG_MEDIUM) &&
            (it.medium_material < 0 || (uint32_t)it.medium_material >= d->n_materials))
            return fail(RTMI_ERR_INVALID, "medium material out of range");
        if ((int32_t)((it.flags >> RTMI_ITEMFLAG_MEDIUM_OUTER_SHIFT) & 15u) > it.xform_count)
            return fail(RTMI_ERR_INVALID, "more outer medium transforms than the item has transforms");
        for (int32_t k = 0; k < it.xform_count; k++) // (the gate records are no transforms: never inside a chain)
            if (d->xforms[it.xform_first + k].kind > RTMI_XF_ROTATE_Z) return fail(RTMI_ERR_INVALID, "a gate record inside an item's transform chain");
        if (it.flags & RTMI_ITEMFLAG_NESTED_MEDIUM) { // a medium whose boundary is a medium: the inner density behind the chain (rtmi.h)
            const uint32_t at = (uint32_t)(it.xform_first + it.xform_count) + (((it.flags & RTMI_ITEMFLAG_DEFERRED) && it.kind == RTMI_ITEM_BVH) ? 2u : 0u);
            if (!(it.flags & RTMI_ITEMFLAG_MEDIUM) || at >= d->n_xforms || d->xforms[at].kind != RTMI_XF_INNER_MEDIUM)
                return fail(RTMI_ERR_INVALID, "a NESTED_MEDIUM item must be a MEDIUM with its RTMI_XF_INNER_MEDIUM record behind its transform chain");
        }
        { // list scans that were children of a BVHNode (rtmi.h): BEGIN on the first member, members only inside, one terminator
            const uint32_t ls = it.flags & (RTMI_ITEMFLAG_LISTSCAN_BEGIN | RTMI_ITEMFLAG_LISTSCAN_MEMBER | RTMI_ITEMFLAG_LISTSCAN_END);
            if (ls && !(it.flags & RTMI_ITEMFLAG_DEFERRED)) return fail(RTMI_ERR_INVALID, "a LISTSCAN item must be DEFERRED");
            if (ls & RTMI_ITEMFLAG_LISTSCAN_END) {
                if (ls != RTMI_ITEMFLAG_LISTSCAN_END || !scan_open || it.kind != RTMI_ITEM_LIST || it.count != 0 || it.first < 0 ||
                    (it.flags & (RTMI_ITEMFLAG_MEDIUM | RTMI_ITEMFLAG_SAVE_T0)))
                    return fail(RTMI_ERR_INVALID, "the terminator of a list scan is a LIST item of no primitives behind its members, `first` = its position in the tree");
                scan_open = false;
                continue;
            }
            if (ls & RTMI_ITEMFLAG_LISTSCAN_BEGIN) {
                if (scan_open || !(ls & RTMI_ITEMFLAG_LISTSCAN_MEMBER)) return fail(RTMI_ERR_INVALID, "LISTSCAN_BEGIN inside an open list scan, or not on a member");
                scan_open = true;
            }
            if (scan_open != ((ls & RTMI_ITEMFLAG_LISTSCAN_MEMBER) != 0u))
                return fail(RTMI_ERR_INVALID, "every item between LISTSCAN_BEGIN and the terminator is a LISTSCAN_MEMBER, and no other is");
            if ((ls & RTMI_ITEMFLAG_LISTSCAN_MEMBER) && it.kind == RTMI_ITEM_BVH && !(it.flags & RTMI_ITEMFLAG_MEDIUM))
                return fail(RTMI_ERR_UNSUPPORTED, "a BVH as a member of a list scan is supported as a medium's boundary only");
        }
        if (it.flags & RTMI_ITEMFLAG_DEFERRED) { // a medium or an instanced subtree that was a child of a BVHNode (rtmi.h)
            const int32_t G = (int32_t)((it.flags >> RTMI_ITEMFLAG_GATE_OUTER_SHIFT) & 15u);
            if (it.kind == RTMI_ITEM_LIST) {
                if (!(it.flags & (RTMI_ITEMFLAG_MEDIUM | RTMI_ITEMFLAG_LISTSCAN_MEMBER)) || it.count < 1 || !d->prim_gate)
                    return fail(RTMI_ERR_INVALID, "a DEFERRED item of kind LIST must be a MEDIUM or a member of a list scan, with at least one primitive, and prim_gate must be given");
            } else {
                if (G > it.xform_count || (uint32_t)(it.xform_first + it.xform_count) + 2u > d->n_xforms ||
                    d->xforms[it.xform_first + it.xform_count].kind != RTMI_XF_GATE_MIN || d->xforms[it.xform_first + it.xform_count + 1].kind != RTMI_XF_GATE_MAX)
                    return fail(RTMI_ERR_INVALID, "a DEFERRED item of kind BVH needs its two gate records behind its transform chain");
            }
            if ((it.flags & RTMI_ITEMFLAG_MEDIUM) && G > (int32_t)((it.flags >> RTMI_ITEMFLAG_MEDIUM_OUTER_SHIFT) & 15u))
                return fail(RTMI_ERR_INVALID, "a DEFERRED medium's enclosing transforms must be among those that wrap the medium");
        }
    }
    if (scan_open) return fail(RTMI_ERR_INVALID, "a list scan without its terminator");
    for (uint32_t i = 0; i < d->n_materials; i++) {
        const rtmi_material &m = d->materials[i];
        if (m.kind < 0 || m.kind > RTMI_MAT_ISOTROPIC) return fail(RTMI_ERR_INVALID, "bad material kind");
        if (m.kind != RTMI_MAT_DIELECTRIC && (m.tex < 0 || (uint32_t)m.tex >= d->n_textures))
            return fail(RTMI_ERR_INVALID, "material texture out of range");
    }
    for (uint32_t i = 0; i < d->n_textures; i++) {
        const rtmi_texture &t = d->textures[i];
        switch (t.kind) {
        case RTMI_TEX_SOLID: break;
        case RTMI_TEX_CHECKER:
            if (t.i0 < 0 || t.i1 < 0 || (uint32_t)t.i0 >= d->n_textures || (uint32_t)t.i1 >= d->n_textures)
                return fail(RTMI_ERR_INVALID, "checker child out of range");
            break;
        case RTMI_TEX_NOISE:
            if (t.i0 < 0 || (uint32_t)t.i0 >= d->n_perlin) return fail(RTMI_ERR_INVALID, "perlin table out of range");
            break;
        case RTMI_TEX_IMAGE:
            if (t.i0 < 0 || (uint32_t)t.i0 >= d->n_images) return fail(RTMI_ERR_INVALID, "image out of range");
            break;
        default: return fail(RTMI_ERR_INVALID, "bad texture kind");
        }
    }
    { // checkers nest (texture.rs:28-48 is generic over its children); the device follows at most 16 levels, and a checker
      // that reaches itself would never end: longest checker chain below every texture, by 17 rounds of relaxation
        std::vector<uint8_t> depth(d->n_textures, 0);
        for (int round = 0; round <= 16; round++)
            for (uint32_t i = 0; i < d->n_textures; i++) {
                const rtmi_texture &t = d->textures[i];
                if (t.kind != RTMI_TEX_CHECKER) continue;
                const uint8_t below = depth[t.i0] > depth[t.i1] ? depth[t.i0] : depth[t.i1];
                depth[i] = (uint8_t)(below + 1);
                if (depth[i] > 16) return fail(RTMI_ERR_INVALID, "checker textures nested deeper than 16 levels, or a checker that reaches itself");
            }
    }
    for (uint32_t i = 0; i < d->n_images; i++) {
        const rtmi_image &im = d->images[i];
        if (im.nx == 0 || im.ny == 0 || im.offset + 3ull * im.nx * im.ny > d->image_bytes)
            return fail(RTMI_ERR_INVALID, "image outside image_data");
    }
    return RTMI_OK;
}

extern "C" int rtmi_scene_create(const rtmi_scene_desc *d, int device, rtmi_scene **out) {
    if (!out) return fail(RTMI_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int rc = validate(d);
    if (rc) return rc;
    int ndev = rtmi_device_count();
    if (ndev <= 0) return fail(RTMI_ERR_DEVICE, "no HIP device available (the rtmi path has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(RTMI_ERR_INVALID, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    rtmi_scene *s = new (std::nothrow) rtmi_scene();
    if (!s) return fail(RTMI_ERR_NOMEM, "out of host memory");
    s->device = device;
    s->meta = *d;
    const float4 *nodes4 = nullptr;
    {
        // device copy of the items: a ConstantMedium whose boundary is one static sphere (the common case:
        // tests/test.rs:471-483) carries that sphere in its unused root-box words, marked by a device-only flag bit,
        // so the kernel's fused two-root boundary query needs no dependent loads of the primitive's meta and planes
        std::vector<rtmi_item> items(d->items, d->items + d->n_items);
        for (rtmi_item &it : items) {
            it.flags &= (RTMI_ITEMFLAG_FLIP | RTMI_ITEMFLAG_MEDIUM | (15u << RTMI_ITEMFLAG_MEDIUM_OUTER_SHIFT) | RTMI_ITEMFLAG_SAVE_T0 |
                         RTMI_ITEMFLAG_DEFERRED | (15u << RTMI_ITEMFLAG_GATE_OUTER_SHIFT) | RTMI_ITEMFLAG_NESTED_MEDIUM |
                         RTMI_ITEMFLAG_LISTSCAN_BEGIN | RTMI_ITEMFLAG_LISTSCAN_MEMBER | RTMI_ITEMFLAG_LISTSCAN_END);
            if ((it.flags & RTMI_ITEMFLAG_MEDIUM) && !(it.flags & (RTMI_ITEMFLAG_DEFERRED | RTMI_ITEMFLAG_NESTED_MEDIUM)) && it.kind == RTMI_ITEM_LIST && it.count == 1 &&
                d->prim_meta[it.first].type == RTMI_PRIM_SPHERE &&
                ((d->prim_meta[it.first].flags >> RTMI_PRIMFLAG_XF_COUNT_SHIFT) & RTMI_PRIM_XF_MAX) == 0u) {
                // (a sphere with a transform chain of its own — ConstantMedium(HittableList[Traslate(Sphere)]) — takes the
                // general boundary query, which applies the chain; the fused query reads the raw centre)
                it.flags |= RTMI_ITEMFLAG_DEV_MEDIUM_SPHERE;
                memcpy(it.root_min, d->prim_a + (size_t)it.first * 4, 3 * sizeof(float));
                it.root_max[0] = d->prim_a[(size_t)it.first * 4 + 3];
            }
            if ((it.flags & RTMI_ITEMFLAG_MEDIUM) && !(it.flags & RTMI_ITEMFLAG_DEV_MEDIUM_SPHERE)) s->all_sphere_media = false;
        }
        std::vector<DevItem> ditems(d->n_items);
        for (uint32_t i = 0; i < d->n_items; i++) {
            DevItem &D = ditems[i];
            memset(&D, 0, sizeof(D));
            D.it = items[i];
            if (items[i].xform_count > 0) D.x0 = d->xforms[items[i].xform_first];     // ranges checked by validate()
            if (items[i].xform_count > 1) D.x1 = d->xforms[items[i].xform_first + 1];
        }
        rc = upload(s, ditems.data(), d->n_items, &s->dev.items);
    }
    if (!rc) rc = upload(s, reinterpret_cast<const float4 *>(d->prim_a), d->n_prims, &s->dev.prim_a);
    if (!rc) rc = upload(s, reinterpret_cast<const float4 *>(d->prim_b), d->n_prims, &s->dev.prim_b);
    if (!rc) rc = upload(s, d->prim_meta, d->n_prims, &s->dev.meta);
    if (!rc && d->prim_gate) rc = upload(s, reinterpret_cast<const float4 *>(d->prim_gate), (size_t)d->n_prims * 2, &s->dev.gate);
    if (!rc) {
        // device copy of the nodes: the reserved words carry the child references in the 26-bit encoding of the
        // cooperative traversal's work pool (rtmi_bvh_coop.hpp), so a node visit does not re-encode them
        std::vector<rtmi_bvh_node> nodes(d->nodes, d->nodes + d->n_nodes);
        const auto enc = [](int32_t ref) -> int32_t {
            if (ref >= 0) return ref;
            const uint32_t u = (uint32_t)ref;
            return (int32_t)((1u << 25) | (((u >> 28) & 7u) << 22) | (u & 0x003fffffu));
        };
        for (rtmi_bvh_node &n : nodes) { n.pad[0] = enc(n.left); n.pad[1] = enc(n.right); }
        rc = upload(s, reinterpret_cast<const float4 *>(nodes.data()), (size_t)d->n_nodes * 4, &nodes4);
        if (!rc && d->n_alt_nodes && d->alt_nodes) { // 4-wide alternative trees: children stored pool-encoded
            std::vector<rtmi_bvh4_node> alt(d->alt_nodes, d->alt_nodes + d->n_alt_nodes);
            for (rtmi_bvh4_node &n : alt)
                for (int c = 0; c < 4; c++) {
                    if (n.child[c] == RTMI_NO_CHILD) { // empty slot: a box no ray can enter, whatever the host wrote
                        n.child[c] = (int32_t)0xffffffffu;
                        const float big = 3.40282346638528859811704183484516925e+38f;
                        n.minx[c] = n.miny[c] = n.minz[c] = big;
                        n.maxx[c] = n.maxy[c] = n.maxz[c] = -big;
                    }
                    else n.child[c] = enc(n.child[c]); // range-checked by validate()
                }
            if (!rc) rc = upload(s, reinterpret_cast<const float4 *>(alt.data()), (size_t)d->n_alt_nodes * 8, &s->dev.nodes4);
        }
    }
    if (!rc) { // leaf records: see DevScene
        std::vector<float> lr((size_t)d->n_prims * 20, 0.0f);
        for (uint32_t i = 0; i < d->n_prims; i++) {
            float *r = &lr[(size_t)i * 20];
            memcpy(r, d->prim_a + (size_t)i * 4, 16);
            memcpy(r + 4, d->prim_b + (size_t)i * 4, 16);
            memcpy(r + 8, &d->prim_meta[i], 16);
            if (d->prim_gate) memcpy(r + 12, d->prim_gate + (size_t)i * 8, 32);
        }
        rc = upload(s, reinterpret_cast<const float4 *>(lr.data()), (size_t)d->n_prims * 5, &s->dev.leaf_rec);
    }
    if (!rc) { // shading records: see DevScene
        const auto fill = [&](float *r, int32_t material) {
            const rtmi_material &m = d->materials[material];
            memcpy(r + 4, &m, 16);
            if (m.kind != RTMI_MAT_DIELECTRIC) memcpy(r + 8, &d->textures[m.tex], 32);
        };
        std::vector<float> sp((size_t)d->n_prims * 16, 0.0f), sm((size_t)d->n_materials * 16, 0.0f);
        for (uint32_t i = 0; i < d->n_prims; i++) {
            memcpy(&sp[(size_t)i * 16], d->prim_a + (size_t)i * 4, 16);
            fill(&sp[(size_t)i * 16], d->prim_meta[i].material);
        }
        for (uint32_t i = 0; i < d->n_materials; i++) fill(&sm[(size_t)i * 16], (int32_t)i);
        rc = upload(s, reinterpret_cast<const float4 *>(sp.data()), (size_t)d->n_prims * 4, &s->dev.shade_prim);
        if (!rc) rc = upload(s, reinterpret_cast<const float4 *>(sm.data()), (size_t)d->n_materials * 4, &s->dev.shade_mat);
    }
    if (!rc) rc = upload(s, d->xforms, d->n_xforms, &s->dev.xforms);
    if (!rc) rc = upload(s, d->materials, d->n_materials, &s->dev.mats);
    if (!rc) rc = upload(s, d->textures, d->n_textures, &s->dev.texs);
    if (!rc) rc = upload(s, d->perlin, d->n_perlin, &s->dev.perlin);
    if (!rc) rc = upload(s, d->images, d->n_images, &s->dev.images);
    if (!rc) rc = upload(s, d->image_data, (size_t)d->image_bytes, &s->dev.image_data);
    if (rc) {
        rtmi_scene_destroy(s);
        return rc;
    }
    s->dev.nodes = nodes4;
    for (uint32_t i = 0; i < d->n_items; i++)
        if (d->items[i].kind == RTMI_ITEM_BVH && d->items[i].alt_first >= 0) s->has_alt = true;
    s->all_alt = s->has_alt;
    for (uint32_t i = 0; i < d->n_items; i++)
        if (d->items[i].kind == RTMI_ITEM_BVH && d->items[i].alt_first < 0) s->all_alt = false;
    s->dev.n_items = d->n_items;
    s->dev.has_prim_xf = 0u;
    for (uint32_t i = 0; i < d->n_prims; i++)
        if ((d->prim_meta[i].flags >> RTMI_PRIMFLAG_XF_COUNT_SHIFT) & RTMI_PRIM_XF_MAX) s->dev.has_prim_xf = 1u;
    s->dev.has_medium_outer = 0u;
    for (uint32_t i = 0; i < d->n_items; i++)
        if (((d->items[i].flags >> RTMI_ITEMFLAG_MEDIUM_OUTER_SHIFT) & 15u) || (d->items[i].flags & (RTMI_ITEMFLAG_SAVE_T0 | RTMI_ITEMFLAG_DEFERRED | RTMI_ITEMFLAG_NESTED_MEDIUM)))
            s->dev.has_medium_outer = 1u; // (deferred media ride in the same instantiations as media inside transforms)
    for (uint32_t i = 0; i < d->n_items; i++)
        if (d->items[i].flags & (RTMI_ITEMFLAG_DEFERRED | RTMI_ITEMFLAG_NESTED_MEDIUM)) s->has_deferred = true;
    for (uint32_t i = 0; i < d->n_items; i++)
        if (d->items[i].flags & (RTMI_ITEMFLAG_SAVE_T0 | RTMI_ITEMFLAG_DEFERRED | RTMI_ITEMFLAG_NESTED_MEDIUM)) s->needs_insd = true;
    // one word more than the status words: the chunk counter of the radiance queries (rtmi_radiance.h)
    if (s->status.alloc((RTMI_STATUS_WORDS + 1) * sizeof(unsigned int)) != hipSuccess ||
        hipMemset(s->status.ptr, 0, (RTMI_STATUS_WORDS + 1) * sizeof(unsigned int)) != hipSuccess) {
        rtmi_scene_destroy(s);
        return fail(RTMI_ERR_DEVICE, "allocating the status word failed");
    }
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
        s->slots = cus * 4 * 5; // 4 SIMDs x up to 5 wavefronts: capacity of the spill buffer; a launch uses cus * 4 * its waves per SIMD
    }
    for (int i = 0; i < 3; i++)
        if (hipEventCreate(&s->ev[i].e) != hipSuccess) {
            rtmi_scene_destroy(s);
            return fail(RTMI_ERR_DEVICE, "hipEventCreate failed");
        }
    if (hipEventCreateWithFlags(&s->busy.e, hipEventDisableTiming) != hipSuccess) {
        rtmi_scene_destroy(s);
        return fail(RTMI_ERR_DEVICE, "hipEventCreate failed");
    }
    *out = s;
    return RTMI_OK;
}

// The members free themselves (rtmi_hostkit.hpp); only the per-sample buffer has somewhere else to go.  Works on the
// half-built handle of a failed rtmi_scene_create as well.
extern "C" void rtmi_scene_destroy(rtmi_scene *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->samples.ptr) { // parked for the next handle on this device (see g_parked); no kernel may still write it
        if (s->busy_recorded) (void)hipEventSynchronize(s->busy.e);
        parked_give(s->device, s->samples);
    }
    delete s;
}

extern "C" uint32_t rtmi_local_tiles(const rtmi_render_params *p) {
    if (!p || p->tile_world == 0) return 0;
    return local_tiles_of(p, p->tile_rank);
}

int check_params(const rtmi_render_params *p) {
    if (!p) return fail(RTMI_ERR_INVALID, "params is NULL");
    if (p->nx == 0 || p->ny == 0 || p->ns == 0) return fail(RTMI_ERR_INVALID, "nx, ny and ns must be positive");
    if ((uint64_t)p->nx * p->ny > 0xffffffffull) return fail(RTMI_ERR_UNSUPPORTED, "image too large");
    if (p->ns >= (1u << 26)) return fail(RTMI_ERR_UNSUPPORTED, "ns must be below 2^26");
    if (p->tile_world == 0 || p->tile_rank >= p->tile_world) return fail(RTMI_ERR_INVALID, "bad tile_rank/tile_world");
    return RTMI_OK;
}

// pinned host mirror of a texel buffer (grow-only)
int grow_host_texels(PinnedBuf<rtmi_texel> &h, size_t ntex) {
    HIP_TRY(h.grow(ntex * sizeof(rtmi_texel)));
    return RTMI_OK;
}

// the handle's framebuffer for `ntex` texels and its pinned host mirror
int reserve_texels(rtmi_scene *s, size_t ntex) {
    if (int rc = grow(s, s->texels, ntex * sizeof(rtmi_texel))) return rc;
    return grow_host_texels(s->h_texels, ntex);
}

// adaptive sampling's buffers (include/rtmi_adaptive.h; NEE shares them), grown together for T tiles.  Each knows its own
// size and is empty after a failed allocation, so a call goes on only when all four hold T tiles.
int grow_adaptive(rtmi_scene *s, uint32_t T) {
    const size_t tiles = T;
    int rc;
    if ((rc = grow(s, s->ad_state, tiles * 64 * 9 * sizeof(double))) || (rc = grow(s, s->ad_lists, (2 * tiles + 1) * sizeof(uint32_t))) ||
        (rc = grow(s, s->ad_stderr, tiles * 64 * 3 * sizeof(float))) || (rc = grow(s, s->ad_spp, tiles * 64 * sizeof(uint32_t))))
        return rc;
    return RTMI_OK;
}
// adaptive sampling's first list of active tiles: all of them (NEE's resolve walks it as well)
static int list_all_tiles(rtmi_scene *s, uint32_t T, hipStream_t stream) {
    std::vector<uint32_t> all(T);
    for (uint32_t t = 0; t < T; t++) all[t] = t;
    HIP_TRY(hipMemcpyAsync(s->ad_lists.ptr, all.data(), (size_t)T * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream)); // (`all` is pageable and goes out of scope)
    return RTMI_OK;
}

int ensure_streams(rtmi_scene *s) {
    if (!s->stream.s) HIP_TRY(hipStreamCreateWithFlags(&s->stream.s, hipStreamNonBlocking));
    if (!s->copy_stream.s) {
        // The progress polls must not queue behind the render.  The runtime gives streams at most GPU_MAX_HW_QUEUES
        // hardware queues per priority and shares the least used one beyond that (with 2, the two streams of a handle
        // landed on one queue and every poll waited for the whole render); another priority is another pool.
        int least = 0, greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_TRY(hipStreamCreateWithPriority(&s->copy_stream.s, hipStreamNonBlocking, greatest));
    }
    return RTMI_OK;
}

// start of a blocking call on the handle's own stream (the caller holds s->mu and has selected s->device): no earlier
// render of this handle may still run, the buffers of the call may be reallocated
int begin_blocking(rtmi_scene *s) {
    if (int rc = ensure_streams(s)) return rc;
    if (s->busy_recorded) HIP_TRY(hipEventSynchronize(s->busy.e));
    return RTMI_OK;
}

// Replaces an attached table (the caller holds s->mu and has selected s->device), in this order: waits for the render
// that may read the old one, drops the old buffers, clears the flag (NULL: the table has none), then `fill` allocates
// and copies (a detach returns RTMI_OK at once).  After a failure the flag is false and every buffer is empty or owned.
template <typename Fill, typename... Old>
static int replace_attached(rtmi_scene *s, bool *flag, Fill &&fill, Old &...old) {
    if (s->busy_recorded) HIP_TRY(hipEventSynchronize(s->busy.e));
    hipError_t released = hipSuccess;
    ((released = released == hipSuccess ? old.release() : released), ...);
    HIP_TRY(released);
    if (flag) *flag = false;
    return fill();
}

// argument checks of the whole-image modes (adaptive sampling, features, NEE) after their NULL checks, in this order
int check_mode_params(const rtmi_render_params *p, uint32_t accepted, const char *flags_msg, const char *world_msg) {
    if (int rc = check_params(p)) return rc;
    if (p->flags & ~accepted) return fail(RTMI_ERR_UNSUPPORTED, flags_msg);
    if (p->tile_world != 1) return fail(RTMI_ERR_UNSUPPORTED, world_msg);
    return RTMI_OK;
}

DevCamera dev_camera(const rtmi_camera *cam) {
    DevCamera C;
    C.origin = F3{cam->origin[0], cam->origin[1], cam->origin[2]};
    C.llc = F3{cam->lower_left_corner[0], cam->lower_left_corner[1], cam->lower_left_corner[2]};
    C.horizontal = F3{cam->horizontal[0], cam->horizontal[1], cam->horizontal[2]};
    C.vertical = F3{cam->vertical[0], cam->vertical[1], cam->vertical[2]};
    C.u = F3{cam->u[0], cam->u[1], cam->u[2]};
    C.v = F3{cam->v[0], cam->v[1], cam->v[2]};
    C.time0 = cam->time0; C.time1 = cam->time1; C.lens_radius = cam->lens_radius;
    return C;
}

// pruned traversal needs the BVH boxes to contain their moving spheres at every ray time (camera.rs:65)
bool boxes_valid(const rtmi_scene *s, const rtmi_camera *cam) {
    const float cam_t_lo = cam->time0 < cam->time1 ? cam->time0 : cam->time1, cam_t_hi = cam->time0 < cam->time1 ? cam->time1 : cam->time0;
    return cam_t_lo >= s->meta.bvh_time_lo && cam_t_hi <= s->meta.bvh_time_hi;
}

// the DevParams every f32 render call fills alike; the pass plan, the buffers and the traversal plan come later
DevParams dev_params(const rtmi_scene *s, const rtmi_render_params *p) {
    DevParams P{};
    P.nx = p->nx; P.ny = p->ny; P.ns = p->ns; P.max_depth = p->max_depth; P.t_min = p->t_min;
    P.key0 = (uint32_t)p->seed; P.key1 = (uint32_t)(p->seed >> 32);
    P.tile_rank = p->tile_rank; P.tile_world = p->tile_world; P.tiles_x = tiles_x_of(p);
    P.ntiles_local = local_tiles_of(p, p->tile_rank);
    P.stack_depth = s->meta.max_bvh_depth + 1u;
    P.shade_threshold = p->shade_threshold ? (p->shade_threshold > 64u ? 64u : p->shade_threshold) : 40u; // tuned on C2..C5 (r02 sweep: 16..48)
    P.status = s->status.ptr;
    P.queue = s->status.ptr + 1;
    P.sky = (p->flags & RTMI_FLAG_SKY) ? 1u : 0u;
    P.ext = ((p->flags & RTMI_FLAG_FACE_FORWARD) ? RTMI_EXT_FACE_FORWARD : 0u) | ((p->flags & RTMI_FLAG_UV_BOOK) ? RTMI_EXT_UV_BOOK : 0u) |
            ((p->flags & RTMI_FLAG_TEST_OVERFLOW) ? RTMI_EXT_TEST_OVERFLOW : 0u);
    return P;
}

#ifndef RTMI_COOP_CAP
#define RTMI_COOP_CAP 512u
#endif
#ifndef RTMI_BLK_CAP /* entries of the workgroup's shared stack: 40 000 B of LDS per workgroup, four workgroups per CU */
#define RTMI_BLK_CAP 2432u
#endif
// Traversal plan of the BVH-walking kernels: P.use_alt, P.spill_cap, P.coop_cap and P.spill (grown when the kernel is
// the cooperative one); `ext` = the extended instantiation of the cooperative kernel.
int plan_traversal(rtmi_scene *s, const rtmi_render_params *p, bool coop, DevParams &P, bool &ext) {
    // LDS part of the traversal stack: 512 entries cover the deepest stack ever seen on the reference scenes
    // (447); deeper stacks continue in global memory (64 * (depth + 2) entries per wavefront, the bound of the
    // depth-first order), so the LDS footprint (7.7 KB per wavefront) does not depend on the tree depth
    const bool use_alt = s->dev.gate != nullptr && s->has_alt && !(p->flags & RTMI_FLAG_REF_TREE);
    P.use_alt = use_alt ? 1u : 0u;
    const uint32_t deepest = (use_alt && s->meta.alt_max_depth > s->meta.max_bvh_depth) ? s->meta.alt_max_depth : s->meta.max_bvh_depth;
    P.spill_cap = 64u * (deepest + 2u);
    if (use_alt) { // a 4-wide visit leaves up to three pending entries per level
        const uint32_t wide = 64u * (3u * s->meta.alt_max_depth + 2u);
        if (wide > P.spill_cap) P.spill_cap = wide;
    }
    // the lean kernel (no gates, no spill code) serves scenes without BVH items; everything else takes the extended
    // one with a 512-entry LDS part
    // (lean = scenes WITHOUT any BVH: its instantiation also carries the LDS word ring of the RNG, which pays exactly
    // there, see rtmi_rng.hpp)
    ext = use_alt || s->meta.n_nodes != 0u;
    P.coop_cap = ext ? RTMI_COOP_CAP : P.spill_cap;
    if (coop)
        if (int rc = grow(s, s->spill, (size_t)s->slots * P.spill_cap * sizeof(uint2))) return rc;
    P.spill = s->spill.ptr;
    return RTMI_OK;
}

// Pass protocol of the status words (rtmi_types.hpp), which progress reporting reads: a call starts with its overflow
// word, the unit counter and the finished-units / finished-samples words at zero (the sticky word stays) ...
int begin_passes(rtmi_scene *s, hipStream_t stream) {
    HIP_TRY(hipMemsetAsync(s->status.ptr, 0, 2 * sizeof(unsigned int), stream));
    HIP_TRY(hipMemsetAsync(s->status.ptr + 3, 0, 2 * sizeof(unsigned int), stream));
    s->units_total = 0;
    return RTMI_OK;
}
// ... and every pass ends with rtmi_pass_end_kernel: the pass's units from [1] to [3], its samples onto [4]
static int units_done(rtmi_scene *s, uint64_t *units) { // read through the copy stream while a launch runs
    unsigned int w[RTMI_STATUS_WORDS] = {0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(w, s->status.ptr, sizeof(w), hipMemcpyDeviceToHost, s->copy_stream.s));
    HIP_TRY(hipStreamSynchronize(s->copy_stream.s));
    *units = (uint64_t)w[3] + w[1]; // finished passes + units handed out in the running one
    return RTMI_OK;
}

// this call's overflow word of a scene whose kernels have finished
int check_overflow(rtmi_scene *s) {
    unsigned int st = 0;
    HIP_TRY(hipMemcpy(&st, s->status.ptr, sizeof(st), hipMemcpyDeviceToHost));
    if (st != 0) {
        HIP_TRY(hipMemset(s->status.ptr + 2, 0, sizeof(unsigned int))); // reported here: not again by rtmi_scene_status
        return fail(RTMI_ERR_DEVICE, "cooperative traversal pool overflow (results invalid, texels poisoned): use RTMI_FLAG_SYNC");
    }
    return RTMI_OK;
}
void fill_stats(rtmi_scene *s, const rtmi_render_params *p, rtmi_stats *stats, float ms_render, float ms_all,
                       PassCounts counts) {
    stats->render_ms = ms_render;
    stats->kernel_ms = ms_all;
    // samples actually traced: pixels inside the image that belong to local tiles
    uint64_t pix = 0;
    const uint32_t txn = tiles_x_of(p), nl = local_tiles_of(p, p->tile_rank);
    for (uint32_t lt = 0; lt < nl; lt++) {
        const uint32_t t = lt * p->tile_world + p->tile_rank;
        const uint32_t ty = t / txn, tx = t % txn;
        const uint32_t w = (tx * RTMI_TILE + RTMI_TILE <= p->nx) ? RTMI_TILE : p->nx - tx * RTMI_TILE;
        const uint32_t h = (ty * RTMI_TILE + RTMI_TILE <= p->ny) ? RTMI_TILE : p->ny - ty * RTMI_TILE;
        pix += (uint64_t)w * h;
    }
    stats->samples = pix * p->ns;
    stats->tiles = nl; stats->chunks = counts.chunks; stats->blocks = counts.blocks; stats->kernel = s->last_kernel;
    // diagnostic knob (rtmi.h): the instantiation of the cooperative kernel rides in bits 8..15, for rtmi_stats_instantiation
    if (p->flags & RTMI_KNOB_REPORT_INST) stats->kernel |= s->last_inst << 8;
}
// the same from the scene's events: ev[0] start, ev[1] before the last resolve, ev[2] end (all completed)
int fill_stats_from_events(rtmi_scene *s, const rtmi_render_params *p, rtmi_stats *stats, PassCounts counts) {
    float ms_r = 0.f, ms_all = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms_r, s->ev[0].e, s->ev[1].e));
    HIP_TRY(hipEventElapsedTime(&ms_all, s->ev[0].e, s->ev[2].e));
    fill_stats(s, p, stats, ms_r, ms_all, counts);
    return RTMI_OK;
}

// Plan of one render call: unit size, samples per pass; (re)allocates the per-sample buffer and the f64 sums.
// slot_bytes: the size of one per-sample slot (rtmi_render_features stores 32-B FeatSlots).
int plan_and_reserve(rtmi_scene *s, const rtmi_render_params *p, uint32_t ntiles_local, uint32_t &chunk_spp,
                            uint32_t &pass_ns, size_t slot_bytes) {
    // ---- per-sample buffer and passes.  Every finished path stores its radiance (12 B) in
    // samples[local tile][sample of the pass][pixel]; the resolve kernel adds them in sample order.  With
    // 288 GB of HBM the whole sample range normally fits (headline: 25 GB); otherwise the range is rendered
    // in passes and the f64 sums are carried between them — the same additions in the same order.
    const size_t per_sample = (size_t)ntiles_local * 64 * slot_bytes;
    size_t want = p->sample_buffer_bytes ? (size_t)p->sample_buffer_bytes : ((size_t)45 << 30);
    if (want > ((size_t)45 << 30)) want = (size_t)45 << 30; // slots are addressed with 32 bits (< 2^32 x 12 B = 48 GiB)
    uint64_t max_pass = want / per_sample;
    if (max_pass < 1) max_pass = 1;
    if (max_pass > p->ns) max_pass = p->ns;
    if (max_pass * per_sample > s->samples.bytes) {
        if (!p->sample_buffer_bytes) { // default budget: never more than 3/4 of what is free on the device
            size_t free_b = 0, total_b = 0;
            HIP_TRY(hipMemGetInfo(&free_b, &total_b));
            const size_t avail = (free_b + s->samples.bytes + parked_bytes(s->device)) / 4 * 3;
            if (max_pass * per_sample > avail) max_pass = avail / per_sample ? avail / per_sample : 1;
        }
        if (max_pass * per_sample > s->samples.bytes) {
            const size_t need = max_pass * per_sample;
            void *taken = nullptr;
            size_t taken_bytes = 0;
            if (parked_take(s->device, need, &taken, &taken_bytes)) { // a destroyed handle's buffer: no hipMalloc
                if (s->samples.ptr) { // (smaller than the one taken) another handle may take it next: no render of this one may still write it
                    if (s->busy_recorded) HIP_TRY(hipEventSynchronize(s->busy.e));
                    parked_give(s->device, s->samples);
                }
                s->samples.adopt(taken, taken_bytes);
            } else {
                parked_drop(s->device); // too small to serve this call: its memory may be what the allocation needs
                if (int rc = grow(s, s->samples, need)) return rc;
            }
        }
    }
    // unit = (tile, chunk of the sample range), the grain of the persistent wavefronts' queue.  Lanes
    // take (sample, pixel) items dynamically and a wavefront moves on to the next unit without
    // draining, so units can be small: the launch ends within about one heavy unit of the last
    // wavefront.  Small images still get a few units per wavefront slot.
    if (p->spp_chunks) {
        chunk_spp = (p->ns + p->spp_chunks - 1) / p->spp_chunks;
    } else {
        chunk_spp = 16u;
        const uint64_t want_units = (uint64_t)s->slots * 4u;
        if ((uint64_t)ntiles_local * ((p->ns + chunk_spp - 1) / chunk_spp) < want_units) {
            const uint64_t per_tile = (want_units + ntiles_local - 1) / ntiles_local;
            chunk_spp = (uint32_t)((p->ns + per_tile - 1) / per_tile);
        }
    }
    if (chunk_spp > max_pass) chunk_spp = (uint32_t)max_pass;
    if (chunk_spp < 1u) chunk_spp = 1u;
    // one pass when everything fits (its last chunk may be shorter); otherwise whole chunks per pass
    pass_ns = max_pass >= p->ns ? p->ns : (uint32_t)(max_pass / chunk_spp) * chunk_spp;
    return grow(s, s->partial, (size_t)ntiles_local * 64 * 3 * sizeof(double)); // f64 sums carried between passes
}

// (Re)allocates what a render with these parameters needs BEFORE the caller starts its event clock: an allocation of tens
// of GB can stall the host for seconds (see g_parked), and the kernel_ms of rtmi_stats are kernel time.  The caller holds s->mu.
int reserve_before_clock(rtmi_scene *s, const rtmi_render_params *p) {
    const uint32_t ntiles_local = local_tiles_of(p, p->tile_rank);
    if (ntiles_local == 0) return RTMI_OK;
    if (s->busy_recorded) HIP_TRY(hipEventSynchronize(s->busy.e)); // the buffer may be reallocated: no render may still use it
    uint32_t chunk_spp = 0, pass_ns = 0;
    return plan_and_reserve(s, p, ntiles_local, chunk_spp, pass_ns);
}

extern "C" int rtmi_render_prepare(rtmi_scene *s, const rtmi_render_params *p) {
    if (!s) return fail(RTMI_ERR_INVALID, "NULL argument");
    int rc = check_params(p);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    return reserve_before_clock(s, p);
}

// the enqueue itself; the caller holds s->mu
int render_device_locked(rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params *p, void *d_texels,
                                void *stream_, rtmi_stats *stats) {
    if (!s || !cam || !d_texels) return fail(RTMI_ERR_INVALID, "NULL argument");
    int rc = check_params(p);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    // device side of the thread model: this render starts after the previous one of this handle has finished (a no-op
    // when both were given the same stream)
    if (s->busy_recorded) HIP_TRY(hipStreamWaitEvent(stream, s->busy.e, 0));
    BusyMark busy_mark{s, stream};

    DevParams P = dev_params(s, p);
    if (P.ntiles_local == 0) {
        if (stats) memset(stats, 0, sizeof(*stats));
        return RTMI_OK;
    }
    P.path_sig = reinterpret_cast<unsigned long long *>(p->path_sig);
    if (p->flags & RTMI_FLAG_PATH_SIG) {
        if (!p->path_sig) return fail(RTMI_ERR_INVALID, "RTMI_FLAG_PATH_SIG needs params.path_sig");
        HIP_TRY(hipMemsetAsync(P.path_sig, 0, (size_t)P.ntiles_local * 64 * sizeof(unsigned long long), stream));
    }

    uint32_t chunk_spp = 0, pass_ns = 0;
    rc = plan_and_reserve(s, p, P.ntiles_local, chunk_spp, pass_ns);
    if (rc) return rc;
    P.chunk_spp = chunk_spp;
    P.pass_stride = pass_ns;
    P.samples = s->samples.ptr;
    const DevCamera C = dev_camera(cam);

    if (stats) HIP_TRY(hipEventRecord(s->ev[0].e, stream));
    const bool fast = (p->flags & RTMI_FLAG_FAST_CULL) != 0u && boxes_valid(s, cam), sigf = (p->flags & RTMI_FLAG_PATH_SIG) != 0u;
    const size_t dyn_lds = (size_t)WAVES_PER_BLOCK * 2u * P.stack_depth * 64u * sizeof(uint32_t);
    const bool prof = (p->flags & RTMI_FLAG_PROFILE) != 0u, sync = (p->flags & RTMI_FLAG_SYNC) != 0u;
    if (prof) {
        if (!p->prof) return fail(RTMI_ERR_INVALID, "RTMI_FLAG_PROFILE needs params.prof");
        P.prof = reinterpret_cast<unsigned long long *>(p->prof);
        HIP_TRY(hipMemsetAsync(P.prof, 0, 2 * RTMI_PROF_SLOTS * sizeof(unsigned long long), stream));
    }
    // kernel selection: default = two-phase schedule, cooperative traversal when fast-cull is on
    // (it implements the fast-cull semantics); RTMI_FLAG_SYNC = per-lane traversal; RTMI_FLAG_ASYNC =
    // per-lane state machine (kept for comparison)
    const bool async = (p->flags & RTMI_FLAG_ASYNC) != 0u && !s->has_deferred;
    const bool coop_ok = s->meta.n_prims < (1u << 22) && s->meta.n_nodes < (1u << 25); // (n_alt_nodes < 2^25: validate())
    const bool coop = fast && !sync && !async && coop_ok;
    if ((rc = begin_passes(s, stream))) return rc;
    bool ext = false;
    if ((rc = plan_traversal(s, p, coop, P, ext))) return rc;
    if (p->flags & (1u << 11)) { // test knob: the extended kernel with a pool this small that it spills all the time
        ext = true;
        P.coop_cap = 256u;
    }
    // persistent grid: as many wavefronts as the kernel instantiation keeps resident (4 SIMDs x its waves per SIMD)
    const uint32_t wps_req = (p->flags >> 8) & 7u; // experiment knob: requested waves per SIMD (0 = default)
    const bool inst = s->dev.has_prim_xf != 0u || s->dev.has_medium_outer != 0u; // the rare compositions: own instantiations
    const uint32_t wps_run = (coop && !prof && !sigf && !inst && (wps_req == 3u || wps_req == 5u)) ? wps_req : (coop && prof ? 3u : 4u);
    const uint64_t run_slots = (uint64_t)(s->slots / 20) * 4u * wps_run;
    // workgroup-cooperative traversal (rtmi_bvh_block.hpp): alternative trees only, no diagnostics build
    const bool bcoop = coop && (p->flags & RTMI_FLAG_BLOCK_COOP) != 0u && P.use_alt && s->all_alt && !prof && !inst &&
                       wps_req == 0u;
    const size_t bcoop_lds = (size_t)RTMI_BLK_LDS_WORDS(RTMI_BLK_CAP) * sizeof(uint32_t);
    // (test knob bit 11: a stack so small that rounds are throttled all the time — room for 64 visits when it is full)
    if (bcoop) P.coop_cap = (p->flags & (1u << 11)) ? 3u * RTMI_BLK_THREADS + 64u : RTMI_BLK_CAP;
    s->last_kernel = bcoop ? RTMI_KERNEL_BLOCK_COOP : coop ? RTMI_KERNEL_WAVE_COOP : async ? RTMI_KERNEL_ASYNC : RTMI_KERNEL_PERLANE;
    // The one-tree instantiation of the cooperative kernel (rtmi_onetree.hip): the default one's shape for the scenes that
    // execute a single one of its four traversal copies — every tree gated and walked through its alternative tree, every
    // medium bounded by a static sphere.  Properties of the scene and of the call, never of the data a kernel meets: the
    // general instantiation renders everything else.  The small-pool knob (bit 11) reaches it (it keeps the spill path);
    // knob value 4 of the waves-per-SIMD bits asks for the general instantiation (tests, A/B inside one build).
    const bool one_tree = coop && !bcoop && ext && !inst && !sigf && !prof && wps_req == 0u && P.use_alt != 0u &&
                          !(p->flags & RTMI_FLAG_REF_TREE) && s->all_alt && s->all_sphere_media;
    s->last_inst = !coop || bcoop ? RTMI_INST_NONE : one_tree ? RTMI_INST_COOP_ONE_TREE : RTMI_INST_COOP_GENERAL;
    const bool insd = inst && (s->needs_insd || ext || sigf); // the level-2 instantiations (below) park their group state in LDS
    const size_t coop_lds = (size_t)WAVES_PER_BLOCK * CoopLds{P.coop_cap, ext, insd}.words() * sizeof(uint32_t);
    // two-phase kernels: persistent wavefronts that take units from the queue; async kernel: one block per unit
    // (workgroup-cooperative kernel: resident workgroups of RTMI_BLK_WAVES wavefronts; every wavefront takes units)
    const uint64_t max_blocks = async ? ~0ull : bcoop ? run_slots / RTMI_BLK_WAVES : run_slots;
    const RenderLaunch launch{bcoop, coop, async, inst, insd, prof, sigf, fast, ext, one_tree, wps_req, coop_lds, bcoop_lds, dyn_lds};
    PassCounts counts;
    rc = run_passes(s, P, stream, 0, p->ns, true, max_blocks, async ? WAVES_PER_BLOCK : 1u, counts,
                    [&](uint32_t blocks, bool first, bool last) -> int {
                        // instanced primitives, media inside transforms: their own instantiations (no diagnostics builds)
                        if (!bcoop && coop && inst && prof) return fail(RTMI_ERR_UNSUPPORTED, "the profiling build has no instantiation for instanced primitives / media inside transforms");
                        HIP_TRY(rtmi_render_launch(launch, blocks, stream, s->dev, C, P));
                        if (stats && last) HIP_TRY(hipEventRecord(s->ev[1].e, stream));
                        HIP_TRY(rtmi_render_launch_resolve(stream, s->samples.ptr, s->partial.ptr, reinterpret_cast<rtmi_texel *>(d_texels), P,
                                                           first, last, (p->flags & RTMI_FLAG_PROGRESSIVE) != 0u));
                        return RTMI_OK;
                    });
    if (rc || !stats) return rc;
    HIP_TRY(hipEventRecord(s->ev[2].e, stream));
    HIP_TRY(hipEventSynchronize(s->ev[2].e));
    if ((rc = fill_stats_from_events(s, p, stats, counts))) return rc;
    return check_overflow(s); // (the kernels have finished: ev[2] was waited for)
}

extern "C" int rtmi_render_device(rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params *p, void *d_texels,
                                  void *stream_, rtmi_stats *stats) {
    if (!s) return fail(RTMI_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lock(s->mu);
    return render_device_locked(s, cam, p, d_texels, stream_, stats);
}

extern "C" int rtmi_scene_status(rtmi_scene *s, uint32_t *overflows) {
    if (!s) return fail(RTMI_ERR_INVALID, "scene is NULL");
    std::lock_guard<std::mutex> lock(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());
    unsigned int st = 0;
    HIP_TRY(hipMemcpy(&st, s->status.ptr + 2, sizeof(st), hipMemcpyDeviceToHost));
    if (overflows) *overflows = st;
    if (st != 0) {
        HIP_TRY(hipMemset(s->status.ptr + 2, 0, sizeof(unsigned int)));
        return fail(RTMI_ERR_DEVICE, "cooperative traversal pool overflow in an earlier render call (its texels are poisoned): use RTMI_FLAG_SYNC");
    }
    return RTMI_OK;
}

extern "C" int rtmi_untile(const rtmi_render_params *p, const rtmi_texel *g, float *out_linear, uint8_t *out_rgb8) {
    int rc = check_params(p);
    if (rc) return rc;
    if (!g) return fail(RTMI_ERR_INVALID, "gathered buffer is NULL");
    const uint32_t txn = tiles_x_of(p), tyn = tiles_y_of(p);
    const size_t stride = (size_t)local_tiles_of(p, 0) * 64; // every rank padded to rank 0's size
    for (uint32_t ty = 0; ty < tyn; ty++)
        for (uint32_t tx = 0; tx < txn; tx++) {
            const uint32_t t = ty * txn + tx;
            const uint32_t rank = t % p->tile_world, lt = t / p->tile_world;
            const rtmi_texel *src = g + rank * stride + (size_t)lt * 64;
            for (uint32_t ly = 0; ly < RTMI_TILE; ly++) {
                const uint32_t row = ty * RTMI_TILE + ly;
                if (row >= p->ny) break;
                for (uint32_t lx = 0; lx < RTMI_TILE; lx++) {
                    const uint32_t px = tx * RTMI_TILE + lx;
                    if (px >= p->nx) break;
                    const rtmi_texel &e = src[ly * RTMI_TILE + lx];
                    if (e.rgb8 & RTMI_TEXEL_POISON)
                        return fail(RTMI_ERR_DEVICE, "framebuffer holds poisoned texels (traversal pool overflow in the launch that wrote them)");
                    const size_t o = ((size_t)row * p->nx + px) * 3;
                    if (out_linear) { out_linear[o] = e.r; out_linear[o + 1] = e.g; out_linear[o + 2] = e.b; }
                    if (out_rgb8) {
                        out_rgb8[o] = (uint8_t)(e.rgb8 & 255u);
                        out_rgb8[o + 1] = (uint8_t)((e.rgb8 >> 8) & 255u);
                        out_rgb8[o + 2] = (uint8_t)((e.rgb8 >> 16) & 255u);
                    }
                }
            }
        }
    return RTMI_OK;
}

// ---- blocking host API ---------------------------------------------------------------------------------
// Waits for `done_ev` of every listed scene; meanwhile (about every 50 ms) reads the devices' unit counters through
// their copy streams and reports progress to the caller's callback — what src/progressbar.rs:6-58 only pretends to.
int wait_with_progress(rtmi_scene *const *scenes, hipEvent_t *done_ev, uint32_t n, const rtmi_render_params *p) {
    rtmi_progress_fn fn = reinterpret_cast<rtmi_progress_fn>(static_cast<uintptr_t>(p->progress_fn));
    void *user = reinterpret_cast<void *>(static_cast<uintptr_t>(p->progress_user));
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) total += scenes[i]->units_total;
    bool cancelled = false;
    uint64_t shown = 0;
    if (fn) {
        for (;;) {
            bool all_done = true;
            uint64_t done = 0;
            for (uint32_t i = 0; i < n; i++) {
                rtmi_scene *s = scenes[i];
                HIP_TRY(hipSetDevice(s->device));
                const hipError_t q = hipEventQuery(done_ev[i]);
                if (q == hipErrorNotReady) {
                    all_done = false;
                    uint64_t d = 0;
                    if (int rc = units_done(s, &d)) return rc;
                    done += d < s->units_total ? d : s->units_total;
                } else if (q == hipSuccess) {
                    done += s->units_total;
                } else {
                    return fail(RTMI_ERR_DEVICE, std::string("hipEventQuery: ") + hipGetErrorString(q));
                }
            }
            if (all_done) break;
            if (done < shown) done = shown; // the two words are read without a lock: keep the report monotone
            shown = done;
            if (!cancelled && fn(done, total, user) != 0) cancelled = true;
            struct timespec ts = {0, 50 * 1000 * 1000};
            nanosleep(&ts, nullptr);
        }
    }
    for (uint32_t i = 0; i < n; i++) {
        HIP_TRY(hipSetDevice(scenes[i]->device));
        HIP_TRY(hipEventSynchronize(done_ev[i]));
    }
    if (fn && !cancelled && fn(total, total, user) != 0) cancelled = true;
    return cancelled ? fail(RTMI_ERR_CANCELLED, "cancelled by the progress callback") : RTMI_OK;
}

extern "C" int rtmi_render(rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params *p_in, float *out_linear,
                           uint8_t *out_rgb8, uint64_t *out_path_sig, rtmi_stats *stats) {
    if (!s) return fail(RTMI_ERR_INVALID, "scene is NULL");
    int rc = check_params(p_in);
    if (rc) return rc;
    if (p_in->tile_world != 1) return fail(RTMI_ERR_INVALID, "rtmi_render renders the whole image: tile_world must be 1");
    std::lock_guard<std::mutex> lock(s->mu); // the whole call: it works in the handle's texel / signature buffers
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = ensure_streams(s))) return rc;
    rtmi_render_params p = *p_in;
    const size_t ntex = (size_t)rtmi_local_tiles(&p) * 64;
    if ((rc = reserve_texels(s, ntex))) return rc;
    p.flags &= ~RTMI_FLAG_PATH_SIG;
    p.path_sig = 0;
    if (out_path_sig) {
        if ((rc = grow(s, s->d_sig, ntex * sizeof(unsigned long long)))) return rc;
        p.flags |= RTMI_FLAG_PATH_SIG;
        p.path_sig = reinterpret_cast<uint64_t>(s->d_sig.ptr);
    }
    if (p.progress_fn) {
        // asynchronous launch, then wait and report progress; stats from the scene's events afterwards
        if ((rc = reserve_before_clock(s, &p))) return rc;
        HIP_TRY(hipEventRecord(s->ev[0].e, s->stream.s));
        rc = render_device_locked(s, cam, &p, s->texels.ptr, s->stream.s, nullptr);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(s->ev[2].e, s->stream.s));
        rtmi_scene *one[1] = {s};
        rc = wait_with_progress(one, &s->ev[2].e, 1, &p);
        if (rc) return rc;
        if ((rc = check_overflow(s))) return rc;
        if (stats) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, s->ev[0].e, s->ev[2].e));
            fill_stats(s, &p, stats, ms, ms);
        }
    } else {
        rtmi_stats local{};
        rc = render_device_locked(s, cam, &p, s->texels.ptr, s->stream.s, stats ? stats : &local);
        if (rc) return rc;
    }
    HIP_TRY(hipMemcpy(s->h_texels.ptr, s->texels.ptr, ntex * sizeof(rtmi_texel), hipMemcpyDeviceToHost));
    if (out_path_sig && (rc = download_untiled<1>(&p, s->d_sig.ptr, ntex, out_path_sig))) return rc;
    return rtmi_untile(&p, s->h_texels.ptr, out_linear, out_rgb8);
}

// RTMI_FLAG_PROGRESSIVE: the framebuffer of the running rtmi_render call as it stands (called from its progress callback:
// the calling thread holds s->mu, so none is taken here)
extern "C" int rtmi_partial_image(rtmi_scene *s, const rtmi_render_params *p_in, float *out_linear, uint8_t *out_rgb8,
                                  uint32_t *spp_done) {
    if (!s || !spp_done) return fail(RTMI_ERR_INVALID, "NULL argument");
    int rc = check_params(p_in);
    if (rc) return rc;
    if (p_in->tile_world != 1) return fail(RTMI_ERR_INVALID, "rtmi_partial_image serves rtmi_render: tile_world must be 1");
    *spp_done = 0;
    rtmi_render_params p = *p_in;
    const size_t ntex = (size_t)rtmi_local_tiles(&p) * 64;
    if (!s->texels.ptr || ntex * sizeof(rtmi_texel) > s->texels.bytes || !s->copy_stream.s) return fail(RTMI_ERR_INVALID, "no rtmi_render call of this size is running on the handle");
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = grow_host_texels(s->h_partial, ntex))) return rc;
    unsigned int w[RTMI_STATUS_WORDS] = {0, 0, 0, 0, 0}, w2[RTMI_STATUS_WORDS] = {0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(w, s->status.ptr, sizeof(w), hipMemcpyDeviceToHost, s->copy_stream.s));
    HIP_TRY(hipStreamSynchronize(s->copy_stream.s));
    if (w[4] == 0u) return RTMI_OK; // no pass has finished: nothing to show yet
    for (int attempt = 0; attempt < 2; attempt++) { // a consistent snapshot unless passes end faster than the copy
        HIP_TRY(hipMemcpyAsync(s->h_partial.ptr, s->texels.ptr, ntex * sizeof(rtmi_texel), hipMemcpyDeviceToHost, s->copy_stream.s));
        HIP_TRY(hipMemcpyAsync(w2, s->status.ptr, sizeof(w2), hipMemcpyDeviceToHost, s->copy_stream.s));
        HIP_TRY(hipStreamSynchronize(s->copy_stream.s));
        if (w2[4] == w[4]) break;
        w[4] = w2[4];
    }
    *spp_done = w[4] < p.ns ? w[4] : p.ns;
    return rtmi_untile(&p, s->h_partial.ptr, out_linear, out_rgb8);
}

// P3 writer — tests/test.rs:59,79
extern "C" size_t rtmi_ppm_p3(uint32_t nx, uint32_t ny, const uint8_t *rgb8, char *buf, size_t cap) {
    const size_t need = 40 + (size_t)nx * ny * 12;
    if (!buf || cap < need || !rgb8) return need;
    size_t n = (size_t)snprintf(buf, cap, "P3\n%u %u\n255\n", nx, ny);
    static const char digits[] = "0123456789";
    const size_t npx = (size_t)nx * ny;
    char *w = buf + n;
    for (size_t i = 0; i < npx * 3; i++) {
        const unsigned v = rgb8[i];
        if (v >= 100) { *w++ = digits[v / 100]; *w++ = digits[(v / 10) % 10]; *w++ = digits[v % 10]; }
        else if (v >= 10) { *w++ = digits[v / 10]; *w++ = digits[v % 10]; }
        else { *w++ = digits[v]; }
        *w++ = (i % 3 == 2) ? '\n' : ' ';
    }
    return (size_t)(w - buf);
}

// streaming writer: P3 text identical to rtmi_ppm_p3, or binary P6
extern "C" int rtmi_write_ppm(const char *path, uint32_t nx, uint32_t ny, const uint8_t *rgb8, int format) {
    if (!path || !rgb8) return fail(RTMI_ERR_INVALID, "rtmi_write_ppm: path or rgb8 is NULL");
    if (format != 3 && format != 6) return fail(RTMI_ERR_INVALID, "rtmi_write_ppm: format must be 3 (P3 text) or 6 (P6 binary)");
    FILE *f = fopen(path, "wb");
    if (!f) return fail(RTMI_ERR_INVALID, "rtmi_write_ppm: cannot open the output file");
    bool ok = fprintf(f, "P%d\n%u %u\n255\n", format, nx, ny) > 0;
    const size_t total = (size_t)nx * ny * 3;
    if (format == 6) {
        ok = ok && fwrite(rgb8, 1, total, f) == total;
    } else {
        static const char digits[] = "0123456789";
        std::vector<char> chunk((size_t)1 << 20);
        const size_t per_chunk = chunk.size() / 4; // <= 4 characters per value
        for (size_t i0 = 0; ok && i0 < total; i0 += per_chunk) {
            const size_t i1 = i0 + per_chunk < total ? i0 + per_chunk : total;
            char *w = chunk.data();
            for (size_t i = i0; i < i1; i++) {
                const unsigned v = rgb8[i];
                if (v >= 100) { *w++ = digits[v / 100]; *w++ = digits[(v / 10) % 10]; *w++ = digits[v % 10]; }
                else if (v >= 10) { *w++ = digits[v / 10]; *w++ = digits[v % 10]; }
                else { *w++ = digits[v]; }
                *w++ = (i % 3 == 2) ? '\n' : ' ';
            }
            const size_t n = (size_t)(w - chunk.data());
            ok = fwrite(chunk.data(), 1, n, f) == n;
        }
    }
    ok = (fclose(f) == 0) && ok;
    return ok ? RTMI_OK : fail(RTMI_ERR_INVALID, "rtmi_write_ppm: write failed");
}

// ---- probes (parity tests call these through the C ABI) ------------------------------
extern "C" int rtmi_probe_math(int op, const float *x, const float *y, float *out, uint32_t n) {
    if (rtmi_device_count() <= 0) return fail(RTMI_ERR_DEVICE, "no HIP device available");
    if (n == 0) return RTMI_OK;
    float *dx, *dy, *dout;
    const auto layout = [&](Carve256 &c) { dx = c.take<float>(n); dy = c.take<float>(n); dout = c.take<float>(n); };
    DeviceArena mem;
    HIP_TRY(mem.alloc(layout));
    HIP_TRY(hipMemcpy(dx, x, (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dy, y ? y : x, (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_TRY(rtmi_render_launch_probe_math(op, dx, dy, dout, n));
    HIP_TRY(hipMemcpy(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RTMI_OK;
}
extern "C" int rtmi_probe_xform(const rtmi_xform *xforms, uint32_t count, const float *a, const float *b, float *out, uint32_t n) {
    if (rtmi_device_count() <= 0) return fail(RTMI_ERR_DEVICE, "no HIP device available");
    if (n == 0) return RTMI_OK;
    rtmi_xform *dx;
    float *da, *db, *dout;
    const auto layout = [&](Carve256 &c) {
        dx = c.take<rtmi_xform>(count ? count : 1); da = c.take<float>((size_t)n * 3); db = c.take<float>((size_t)n * 3);
        dout = c.take<float>((size_t)n * 13);
    };
    DeviceArena mem;
    HIP_TRY(mem.alloc(layout));
    if (count) HIP_TRY(hipMemcpy(dx, xforms, count * sizeof(rtmi_xform), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(da, a, (size_t)n * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(db, b, (size_t)n * 12, hipMemcpyHostToDevice));
    HIP_TRY(rtmi_render_launch_probe_xform(dx, (int)count, da, db, dout, n));
    HIP_TRY(hipMemcpy(out, dout, (size_t)n * 13 * 4, hipMemcpyDeviceToHost));
    return RTMI_OK;
}
extern "C" int rtmi_probe_geom(int op, const float *prim_a, const float *prim_b, const rtmi_prim_meta *meta, uint32_t n_prims,
                               const rtmi_xform *xforms, uint32_t n_xforms, const float *in, float *out, uint32_t n) {
    if (rtmi_device_count() <= 0) return fail(RTMI_ERR_DEVICE, "no HIP device available");
    if (op < RTMI_PROBE_GEOM_PRIM || op > RTMI_PROBE_GEOM_UV) return fail(RTMI_ERR_INVALID, "rtmi_probe_geom: unknown op");
    if (n == 0) return RTMI_OK;
    if (!in || !out || (n_prims && (!prim_a || !prim_b || !meta)) || (n_xforms && !xforms))
        return fail(RTMI_ERR_INVALID, "rtmi_probe_geom: missing array");
    uint32_t has_prim_xf = 0u;
    for (uint32_t p = 0; p < n_prims; p++) {
        const uint32_t cnt = (meta[p].flags >> RTMI_PRIMFLAG_XF_COUNT_SHIFT) & RTMI_PRIM_XF_MAX;
        const uint64_t first = meta[p].flags >> RTMI_PRIMFLAG_XF_FIRST_SHIFT;
        if (meta[p].type < RTMI_PRIM_SPHERE || meta[p].type > RTMI_PRIM_CUBE) return fail(RTMI_ERR_INVALID, "rtmi_probe_geom: primitive type");
        if (cnt && first + cnt > n_xforms) return fail(RTMI_ERR_INVALID, "rtmi_probe_geom: transform chain out of range");
        if (cnt) has_prim_xf = 1u;
    }
    if (op == RTMI_PROBE_GEOM_PRIM || op == RTMI_PROBE_GEOM_MEDIUM) {
        for (uint32_t i = 0; i < n; i++) {
            int32_t idx;
            memcpy(&idx, in + (size_t)RTMI_PROBE_GEOM_IN * i + 9, 4);
            if (idx < 0 || (uint32_t)idx >= n_prims) return fail(RTMI_ERR_INVALID, "rtmi_probe_geom: primitive index out of range");
            int32_t lead;
            memcpy(&lead, in + (size_t)RTMI_PROBE_GEOM_IN * (i & ~63u) + 9, 4);
            if (op == RTMI_PROBE_GEOM_PRIM && idx != lead)
                return fail(RTMI_ERR_INVALID, "rtmi_probe_geom: PRIM cases must share one primitive per 64");
        }
    }
    std::vector<float> lr((size_t)(n_prims ? n_prims : 1) * 20, 0.0f); // leaf records as rtmi_scene_create builds them
    for (uint32_t p = 0; p < n_prims; p++) {
        float *r = &lr[(size_t)p * 20];
        memcpy(r, prim_a + (size_t)p * 4, 16);
        memcpy(r + 4, prim_b + (size_t)p * 4, 16);
        memcpy(r + 8, &meta[p], 16);
    }
    float *d_rec, *d_in, *d_out;
    rtmi_xform *d_xf;
    const auto layout = [&](Carve256 &c) {
        d_rec = c.take<float>(lr.size()); d_xf = c.take<rtmi_xform>(n_xforms ? n_xforms : 1);
        d_in = c.take<float>((size_t)n * RTMI_PROBE_GEOM_IN); d_out = c.take<float>((size_t)n * RTMI_PROBE_GEOM_OUT);
    };
    DeviceArena mem;
    HIP_TRY(mem.alloc(layout));
    HIP_TRY(hipMemcpy(d_rec, lr.data(), lr.size() * 4, hipMemcpyHostToDevice));
    if (n_xforms) HIP_TRY(hipMemcpy(d_xf, xforms, n_xforms * sizeof(rtmi_xform), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_in, in, (size_t)n * RTMI_PROBE_GEOM_IN * 4, hipMemcpyHostToDevice));
    DevScene sc;
    memset(&sc, 0, sizeof(sc));
    sc.leaf_rec = reinterpret_cast<const float4 *>(d_rec);
    sc.xforms = d_xf;
    sc.has_prim_xf = has_prim_xf;
    HIP_TRY(rtmi_render_launch_probe_geom(op, sc, d_in, d_out, n));
    HIP_TRY(hipMemcpy(out, d_out, (size_t)n * RTMI_PROBE_GEOM_OUT * 4, hipMemcpyDeviceToHost));
    return RTMI_OK;
}
extern "C" int rtmi_probe_path(rtmi_scene *s, int op, const rtmi_camera *cams, uint32_t n_cams, const rtmi_xform *xforms, uint32_t n_xforms,
                               const float *in, const uint32_t *words, float *out, uint32_t n) {
    if (rtmi_device_count() <= 0) return fail(RTMI_ERR_DEVICE, "no HIP device available");
    if (op < RTMI_PROBE_PATH_CAMERA || op > RTMI_PROBE_PATH_BOUNCE) return fail(RTMI_ERR_INVALID, "rtmi_probe_path: unknown op");
    if (op == RTMI_PROBE_PATH_BOUNCE && !s) return fail(RTMI_ERR_INVALID, "rtmi_probe_path: BOUNCE needs a scene");
    if (n == 0) return RTMI_OK;
    if (!in || !words || !out || (n_cams && !cams) || (n_xforms && !xforms)) return fail(RTMI_ERR_INVALID, "rtmi_probe_path: missing array");
    for (uint32_t i = 0; i < n; i++) { // everything a lane indexes with, before any launch
        const float *a = in + (size_t)RTMI_PROBE_PATH_IN * i;
        if (op == RTMI_PROBE_PATH_CAMERA) {
            uint32_t w[5];
            memcpy(w, a, sizeof(w));
            if (w[0] >= n_cams) return fail(RTMI_ERR_INVALID, "rtmi_probe_path: camera index out of range");
            if (w[1] == 0u || w[2] == 0u || w[3] >= w[1] || w[4] >= w[2]) return fail(RTMI_ERR_INVALID, "rtmi_probe_path: pixel outside the image");
        } else if (op == RTMI_PROBE_PATH_XFORM_ROUNDTRIP) {
            int32_t fc[2];
            memcpy(fc, a + 7, sizeof(fc));
            if (fc[0] < 0 || fc[1] < 0 || (uint32_t)fc[1] > RTMI_PRIM_XF_MAX || (uint64_t)fc[0] + (uint64_t)fc[1] > n_xforms)
                return fail(RTMI_ERR_INVALID, "rtmi_probe_path: transform chain out of range");
        } else if (op == RTMI_PROBE_PATH_BOUNCE) { // max_depth and the flags are a launch's: one value each
            if (memcmp(a + 10, in + 10, 8) != 0) return fail(RTMI_ERR_INVALID, "rtmi_probe_path: BOUNCE cases differ in max_depth or flags");
        }
    }
    for (uint32_t k = 0; k < n_xforms; k++)
        if (xforms[k].kind < RTMI_XF_TRANSLATE || xforms[k].kind > RTMI_XF_ROTATE_Z) return fail(RTMI_ERR_INVALID, "rtmi_probe_path: transform kind");
    uint32_t bounce_words[2] = {0u, 0u}; // BOUNCE: max_depth and flags, the same in every case (checked above)
    std::unique_lock<std::mutex> lock;
    if (op == RTMI_PROBE_PATH_BOUNCE) {
        memcpy(bounce_words, in + 10, sizeof(bounce_words));
        if (bounce_words[1] & ~(uint32_t)(RTMI_FLAG_FACE_FORWARD | RTMI_FLAG_UV_BOOK)) return fail(RTMI_ERR_INVALID, "rtmi_probe_path: BOUNCE flags");
        lock = std::unique_lock<std::mutex>(s->mu); // the handle is read under its mutex only; no device work before this
        HIP_TRY(hipSetDevice(s->device));
        if (int rc = begin_blocking(s)) return rc;
    }
    std::vector<DevCamera> dc(n_cams ? n_cams : 1);
    for (uint32_t c = 0; c < n_cams; c++) dc[c] = dev_camera(&cams[c]);
    DevCamera *d_cams;
    rtmi_xform *d_xf;
    float *d_in, *d_out;
    uint32_t *d_words;
    const auto layout = [&](Carve256 &c) {
        d_cams = c.take<DevCamera>(dc.size()); d_xf = c.take<rtmi_xform>(n_xforms ? n_xforms : 1);
        d_in = c.take<float>((size_t)n * RTMI_PROBE_PATH_IN); d_words = c.take<uint32_t>((size_t)n * RTMI_PROBE_PATH_WORDS);
        d_out = c.take<float>((size_t)n * RTMI_PROBE_PATH_OUT);
    };
    DeviceArena mem;
    HIP_TRY(mem.alloc(layout));
    HIP_TRY(hipMemcpy(d_cams, dc.data(), dc.size() * sizeof(DevCamera), hipMemcpyHostToDevice));
    if (n_xforms) HIP_TRY(hipMemcpy(d_xf, xforms, n_xforms * sizeof(rtmi_xform), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_in, in, (size_t)n * RTMI_PROBE_PATH_IN * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_words, words, (size_t)n * RTMI_PROBE_PATH_WORDS * 4, hipMemcpyHostToDevice));
    PathProbe B;
    memset(&B, 0, sizeof(B));
    B.cams = d_cams; B.xforms = d_xf; B.in = d_in; B.words = d_words; B.out = d_out; B.n = n;
    if (op == RTMI_PROBE_PATH_BOUNCE) {
        B.sc = s->dev;
        B.max_depth = bounce_words[0];
        B.ext = ((bounce_words[1] & RTMI_FLAG_FACE_FORWARD) ? RTMI_EXT_FACE_FORWARD : 0u) |
                ((bounce_words[1] & RTMI_FLAG_UV_BOOK) ? RTMI_EXT_UV_BOOK : 0u);
    }
    HIP_TRY(rtmi_probe_path_launch(op, B));
    HIP_TRY(hipMemcpy(out, d_out, (size_t)n * RTMI_PROBE_PATH_OUT * 4, hipMemcpyDeviceToHost));
    return RTMI_OK;
}
extern "C" int rtmi_probe_stream(int kind, uint64_t seed, const uint8_t *script, uint32_t steps, uint32_t *out, uint32_t n) {
    if (rtmi_device_count() <= 0) return fail(RTMI_ERR_DEVICE, "no HIP device available");
    if (kind < 0 || kind > 2) return fail(RTMI_ERR_INVALID, "rtmi_probe_stream: unknown kind");
    if (steps < 1u || steps > RTMI_PROBE_STREAM_MAX_STEPS) return fail(RTMI_ERR_INVALID, "rtmi_probe_stream: steps out of range");
    if (n == 0) return RTMI_OK;
    if (!script || !out) return fail(RTMI_ERR_INVALID, "rtmi_probe_stream: missing array");
    const size_t cells = (size_t)n * steps;
    for (size_t c = 0; c < cells; c++)
        if (script[c] > 4u) return fail(RTMI_ERR_INVALID, "rtmi_probe_stream: script byte above 4");
    uint8_t *d_script;
    uint32_t *d_out;
    const auto layout = [&](Carve256 &c) { d_script = c.take<uint8_t>(cells); d_out = c.take<uint32_t>(cells * 3); };
    DeviceArena mem;
    HIP_TRY(mem.alloc(layout));
    HIP_TRY(hipMemcpy(d_script, script, cells, hipMemcpyHostToDevice));
    HIP_TRY(rtmi_probe_stream_launch(kind, (uint32_t)seed, (uint32_t)(seed >> 32), d_script, steps, d_out, n));
    HIP_TRY(hipMemcpy(out, d_out, cells * 3 * 4, hipMemcpyDeviceToHost));
    return RTMI_OK;
}
extern "C" int rtmi_probe_philox(const uint32_t *ctr, const uint32_t *key, uint32_t *out, uint32_t n) {
    if (rtmi_device_count() <= 0) return fail(RTMI_ERR_DEVICE, "no HIP device available");
    if (n == 0) return RTMI_OK;
    uint32_t *dc, *dk, *dout;
    const auto layout = [&](Carve256 &c) {
        dc = c.take<uint32_t>((size_t)n * 4); dk = c.take<uint32_t>((size_t)n * 2); dout = c.take<uint32_t>((size_t)n * 4);
    };
    DeviceArena mem;
    HIP_TRY(mem.alloc(layout));
    HIP_TRY(hipMemcpy(dc, ctr, (size_t)n * 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dk, key, (size_t)n * 8, hipMemcpyHostToDevice));
    HIP_TRY(rtmi_render_launch_probe_philox(dc, dk, dout, n));
    HIP_TRY(hipMemcpy(out, dout, (size_t)n * 16, hipMemcpyDeviceToHost));
    return RTMI_OK;
}

// ======================================================================================
// f64 render mode (include/rtmi_f64.h): attach, blocking render, probe.  The kernels are in rtmi_f64.hip.
// ======================================================================================
extern "C" int rtmi_scene_attach_f64(rtmi_scene *s, const rtmi_scene_f64 *w) {
    if (!s || !w) return fail(RTMI_ERR_INVALID, "NULL argument");
    const rtmi_scene_desc &m = s->meta;
    if (w->n_items != m.n_items || w->n_prims != m.n_prims || w->n_nodes != m.n_nodes || w->n_xforms != m.n_xforms ||
        w->n_materials != m.n_materials || w->n_textures != m.n_textures || w->n_perlin != m.n_perlin)
        return fail(RTMI_ERR_INVALID, "rtmi_scene_attach_f64: counts differ from the handle's scene description");
    struct Plane { const double *src; size_t n; const double **dst; const char *name; };
    DevSceneF64 d{};
    const Plane planes[] = {
        {w->prim_a, (size_t)w->n_prims * 4, &d.prim_a, "prim_a"}, {w->prim_b, (size_t)w->n_prims * 4, &d.prim_b, "prim_b"},
        {w->prim_dt, (size_t)w->n_prims, &d.prim_dt, "prim_dt"}, {w->nodes, (size_t)w->n_nodes * 12, &d.nodes, "nodes"},
        {w->xforms, (size_t)w->n_xforms * 4, &d.xforms, "xforms"},
        {w->item_neg_inv_density, (size_t)w->n_items, &d.item_nid, "item_neg_inv_density"},
        {w->item_root, (size_t)w->n_items * 6, &d.item_root, "item_root"},
        {w->material_param, (size_t)w->n_materials, &d.mparam, "material_param"},
        {w->texture_f, (size_t)w->n_textures * 4, &d.texf, "texture_f"},
        {w->perlin_ranvec, (size_t)w->n_perlin * 768, &d.ranvec, "perlin_ranvec"}};
    for (const Plane &p : planes)
        if (p.n && !p.src) return fail(RTMI_ERR_INVALID, std::string("rtmi_scene_attach_f64: plane ") + p.name + " is NULL");
    // prim_gate is part of the description (rtmi_scene_f64) but the exact walk of this mode does not read it
    if (w->n_prims && !w->prim_gate) return fail(RTMI_ERR_INVALID, "rtmi_scene_attach_f64: plane prim_gate is NULL");
    std::lock_guard<std::mutex> lock(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    const auto fill = [&]() -> int { // (a running f64 render may read the old planes)
        for (const Plane &p : planes) {
            void *dp = nullptr;
            HIP_TRY(s->f64_allocs.add(&dp, (p.n ? p.n : 1) * sizeof(double)));
            if (p.n) HIP_TRY(hipMemcpy(dp, p.src, p.n * sizeof(double), hipMemcpyHostToDevice));
            *p.dst = static_cast<const double *>(dp);
        }
        s->f64 = d;
        s->has_f64 = true;
        return RTMI_OK;
    };
    return replace_attached(s, &s->has_f64, fill, s->f64_allocs);
}

extern "C" int rtmi_render_f64(rtmi_scene *s, const rtmi_camera_f64 *cam, const rtmi_render_params *p_in, double t_min,
                               double *out_linear, uint8_t *out_rgb8, uint64_t *out_path_sig, rtmi_stats *stats) {
    if (!s || !cam) return fail(RTMI_ERR_INVALID, "NULL argument");
    int rc = check_params(p_in);
    if (rc) return rc;
    rtmi_render_params p = *p_in;
    if (out_path_sig) p.flags |= RTMI_FLAG_PATH_SIG;
    if (p.tile_world != 1) return fail(RTMI_ERR_INVALID, "rtmi_render_f64 renders the whole image: tile_world must be 1");
    const uint32_t unsupported = RTMI_FLAG_PROGRESSIVE | RTMI_FLAG_ASYNC | RTMI_FLAG_BLOCK_COOP | RTMI_FLAG_PROFILE | RTMI_FLAG_TEST_OVERFLOW;
    if (p.flags & unsupported) return fail(RTMI_ERR_UNSUPPORTED, "rtmi_render_f64: PROGRESSIVE, ASYNC, BLOCK_COOP, PROFILE and TEST_OVERFLOW are not supported in the f64 mode");
    if (s->needs_insd) return fail(RTMI_ERR_UNSUPPORTED, "rtmi_render_f64: scenes with DEFERRED, LISTSCAN or NESTED_MEDIUM items are not supported in the f64 mode");
    std::lock_guard<std::mutex> lock(s->mu);
    if (!s->has_f64) return fail(RTMI_ERR_INVALID, "rtmi_render_f64: no f64 planes attached (rtmi_scene_attach_f64)");
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = begin_blocking(s))) return rc;
    hipStream_t st = s->stream.s;
    const uint32_t ntiles = local_tiles_of(&p, 0);
    const bool sig = (p.flags & RTMI_FLAG_PATH_SIG) != 0u;
    // passes (rtmi_f64_plan.hpp): RTMI_SAMPLE_SLOT_BYTES_F64 per pixel sample, at most 45 GiB and 2^32 - 1 slots per pass;
    // the default budget is half the free HBM
    const size_t per_sample = (size_t)ntiles * 64 * RTMI_SAMPLE_SLOT_BYTES_F64;
    size_t free_b = 0;
    if (!p.sample_buffer_bytes) {
        size_t total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    }
    uint32_t chunk_spp = 0, pass_ns = 0;
    if (!rtmi_f64_plan(ntiles, p.ns, p.sample_buffer_bytes, free_b, (uint64_t)s->slots * 4u, p.spp_chunks, chunk_spp, pass_ns))
        return fail(RTMI_ERR_UNSUPPORTED, "rtmi_render_f64: image too large for one sample per pass");
    double *d_acc = nullptr, *d_lin = nullptr;
    uint32_t *d_q = nullptr, *d_queue = nullptr;
    unsigned long long *d_sig = nullptr;
    const size_t texels = (size_t)ntiles * 64;
    if (grow(s, s->f64_samples, (size_t)pass_ns * per_sample)) // grows to the largest pass planned
        return fail(RTMI_ERR_NOMEM, "rtmi_render_f64: hipMalloc of the per-sample buffer failed");
    double *const d_samples = s->f64_samples.ptr;
    // call-local device memory, one allocation freed on every return path
    const auto layout = [&](Carve256 &c) {
        d_acc = c.take<double>(texels * 3); d_lin = c.take<double>(texels * 3);
        d_q = c.take<uint32_t>(texels); d_queue = c.take<uint32_t>(1);
        if (sig) d_sig = c.take<unsigned long long>(texels);
    };
    DeviceArena scratch;
    if (scratch.alloc(layout) != hipSuccess) return fail(RTMI_ERR_NOMEM, "rtmi_render_f64: hipMalloc failed");
    if (sig) HIP_TRY(hipMemsetAsync(d_sig, 0, texels * sizeof(unsigned long long), st));
    DevParams P{};
    P.nx = p.nx; P.ny = p.ny; P.ns = p.ns; P.max_depth = p.max_depth;
    P.t_min = (float)t_min;
    P.key0 = (uint32_t)p.seed; P.key1 = (uint32_t)(p.seed >> 32);
    P.tile_rank = 0; P.tile_world = 1; P.tiles_x = tiles_x_of(&p); P.ntiles_local = ntiles;
    P.chunk_spp = chunk_spp;
    P.pass_stride = pass_ns;
    P.path_sig = d_sig;
    P.shade_threshold = p.shade_threshold ? p.shade_threshold : 40u;
    if (P.shade_threshold > 64u) P.shade_threshold = 64u;
    P.queue = d_queue;
    P.sky = (p.flags & RTMI_FLAG_SKY) ? 1u : 0u;
    P.ext = ((p.flags & RTMI_FLAG_FACE_FORWARD) ? RTMI_EXT_FACE_FORWARD : 0u) | ((p.flags & RTMI_FLAG_UV_BOOK) ? RTMI_EXT_UV_BOOK : 0u);
    DevParamsF64 Q{};
    Q.t_min = t_min;
    Q.samples = d_samples;
    DevCameraF64 C{};
    C.origin = D3{cam->origin[0], cam->origin[1], cam->origin[2]};
    C.llc = D3{cam->lower_left_corner[0], cam->lower_left_corner[1], cam->lower_left_corner[2]};
    C.horizontal = D3{cam->horizontal[0], cam->horizontal[1], cam->horizontal[2]};
    C.vertical = D3{cam->vertical[0], cam->vertical[1], cam->vertical[2]};
    C.u = D3{cam->u[0], cam->u[1], cam->u[2]};
    C.v = D3{cam->v[0], cam->v[1], cam->v[2]};
    C.time0 = cam->time0; C.time1 = cam->time1; C.lens_radius = cam->lens_radius;
    const uint32_t blocks = (uint32_t)(s->slots / 20) * 4u * 2u; // CUs x 4 SIMDs x 2 wavefronts (the kernel's occupancy: 255 VGPRs)
    HIP_TRY(hipEventRecord(s->ev[0].e, st));
    float ms_render = 0.0f;
    for (uint32_t s0 = 0; s0 < p.ns; s0 += pass_ns) {
        const uint32_t cnt = p.ns - s0 < pass_ns ? p.ns - s0 : pass_ns;
        P.pass_s0 = s0; P.pass_cnt = cnt;
        P.nchunks = (cnt + chunk_spp - 1) / chunk_spp;
        HIP_TRY(hipMemsetAsync(d_queue, 0, sizeof(uint32_t), st));
        HIP_TRY(hipEventRecord(s->ev[1].e, st));
        HIP_TRY(rtmi_f64_launch_render(sig, blocks, st, s->dev, s->f64, C, P, Q));
        HIP_TRY(hipEventRecord(s->ev[2].e, st));
        HIP_TRY(rtmi_f64_launch_resolve(st, d_samples, d_acc, d_lin, d_q, P, s0 == 0, s0 + cnt >= p.ns));
        HIP_TRY(hipEventSynchronize(s->ev[2].e));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, s->ev[1].e, s->ev[2].e));
        ms_render += ms;
    }
    HIP_TRY(hipEventRecord(s->ev[1].e, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (out_linear && (rc = download_untiled<3>(&p, d_lin, texels, out_linear))) return rc;
    if (out_rgb8) {
        std::vector<uint32_t> q((size_t)p.nx * p.ny);
        if ((rc = download_untiled<1>(&p, d_q, texels, q.data()))) return rc;
        for (size_t o = 0; o < q.size(); o++)
            for (int ch = 0; ch < 3; ch++) out_rgb8[3 * o + ch] = (uint8_t)((q[o] >> (8 * ch)) & 255u);
    }
    if (out_path_sig && (rc = download_untiled<1>(&p, d_sig, texels, out_path_sig))) return rc;
    if (stats) {
        float ms_all = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms_all, s->ev[0].e, s->ev[1].e));
        fill_stats(s, &p, stats, ms_render, ms_all);
        stats->kernel = RTMI_KERNEL_PERLANE;
    }
    return RTMI_OK;
}

extern "C" int rtmi_probe_math_f64(int op, const double *x, const double *y, double *out, uint32_t n) {
    if (op < 0 || op > 5) return fail(RTMI_ERR_INVALID, "rtmi_probe_math_f64: unknown op");
    if (!x || !out || ((op == 2 || op == 4) && !y)) return fail(RTMI_ERR_INVALID, "NULL argument");
    if (n == 0) return RTMI_OK;
    if (rtmi_device_count() <= 0) return fail(RTMI_ERR_DEVICE, "no HIP device available");
    double *dx, *dy, *dout;
    const size_t bytes = (size_t)n * sizeof(double);
    const auto layout = [&](Carve256 &c) { dx = c.take<double>(n); dy = c.take<double>(n); dout = c.take<double>(n); };
    DeviceArena mem;
    hipError_t e = mem.alloc(layout);
    if (e == hipSuccess) e = hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dy, y ? y : x, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = rtmi_f64_launch_probe(op, dx, dy, dout, n);
    if (e == hipSuccess) e = hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(RTMI_ERR_DEVICE, std::string("rtmi_probe_math_f64: ") + hipGetErrorString(e));
    return RTMI_OK;
}

// ---- adaptive sampling (include/rtmi_adaptive.h) ---------------------------------------------------------------------
// the checks of the noise target, after those of the params (rtmi_render_adaptive and the entries of rtmi_adaptive_nee.h)
int check_adaptive(const rtmi_render_params *p, const rtmi_adaptive *a) {
    if (a->min_spp < 2u) return fail(RTMI_ERR_INVALID, "min_spp must be at least 2 (a variance needs two samples)");
    if (a->min_spp > p->ns) return fail(RTMI_ERR_INVALID, "min_spp must not exceed ns");
    if (a->step_spp == 0u) return fail(RTMI_ERR_INVALID, "step_spp must be positive");
    if (!std::isfinite(a->abs_tol) || !(a->abs_tol >= 0.0) || !std::isfinite(a->rel_tol) || !(a->rel_tol >= 0.0))
        return fail(RTMI_ERR_INVALID, "abs_tol and rel_tol must be finite and non-negative");
    return RTMI_OK;
}

// the buffers of an adaptive call for T tiles, before the clock starts: framebuffer, adaptive state, the pinned count
// word and the per-sample buffer for the largest step (every tile, max(min_spp, step_spp) samples)
static int adaptive_reserve(rtmi_scene *s, const rtmi_render_params &p, const rtmi_adaptive *a, uint32_t T) {
    int rc;
    if ((rc = reserve_texels(s, (size_t)T * 64)) || (rc = grow_adaptive(s, T))) return rc;
    HIP_TRY(s->h_ad_count.grow(64));
    rtmi_render_params q = p;
    q.ns = a->min_spp > a->step_spp ? a->min_spp : (a->step_spp < p.ns ? a->step_spp : p.ns);
    uint32_t chunk_spp = 0, pass_ns = 0;
    return plan_and_reserve(s, &q, T, chunk_spp, pass_ns);
}

// Steps of samples per active tile; after every step the adaptive resolve retires the converged tiles and lists the
// others, and the host reads the count back (4 B) and plans the next step for that many tiles, so a small active set
// still gets enough units to fill the chip.  The per-sample buffer holds the active tiles only (indexed by list position).
// Shared by rtmi_render_adaptive and the entries of rtmi_adaptive_nee.h.  launch(blocks, tiles) enqueues the mode's
// render kernel on s->stream.s for the pass fields of P over the active list `tiles` and returns an RTMI code; `kernel` is
// the label of rtmi_stats.kernel, `wps` the waves per SIMD that kernel keeps resident (the persistent grid).  The caller
// holds s->mu, has checked every argument, called begin_blocking and adaptive_reserve and filled P with the mode's
// traversal plan.
// adaptive_steps_device: enqueue, wait and check overflow; texels, standard errors and counts stay in the scene's device
// buffers (the frame handle, rtmi_frame_launch.hpp, stops here).  adaptive_download: their copies to the host.
template <typename Launch>
static int adaptive_steps_device(rtmi_scene *s, const rtmi_render_params &p, const rtmi_adaptive *a, DevParams &P, uint32_t kernel,
                                 uint32_t wps, PassCounts &counts, Launch &&launch) {
    int rc;
    hipStream_t stream = s->stream.s;
    const uint32_t T = local_tiles_of(&p, 0);
    const uint64_t run_slots = (uint64_t)(s->slots / 20) * 4u * wps;
    s->last_kernel = kernel;

    rtmi_progress_fn fn = reinterpret_cast<rtmi_progress_fn>(static_cast<uintptr_t>(p.progress_fn));
    void *user = reinterpret_cast<void *>(static_cast<uintptr_t>(p.progress_user));
    const uint64_t total = (uint64_t)T * p.ns; // tile-samples: every tile at ns
    uint64_t settled = 0, shown = 0;           // tile-samples of finished steps, retired tiles counted at ns
    bool cancelled = false;

    if ((rc = begin_passes(s, stream)) || (rc = list_all_tiles(s, T, stream))) return rc;
    HIP_TRY(hipEventRecord(s->ev[0].e, stream));
    uint32_t *lists[2] = {s->ad_lists.ptr, s->ad_lists.ptr + T}, *count = s->ad_lists.ptr + 2 * (size_t)T;
    uint32_t n_active = T, n = 0, cur = 0;
    AdaptiveResolve A;
    A.n_out = count;
    A.state = s->ad_state.ptr; A.texels = s->texels.ptr; A.stderr_out = s->ad_stderr.ptr; A.spp_out = s->ad_spp.ptr;
    A.abs_tol = a->abs_tol; A.rel_tol = a->rel_tol; A.ns = p.ns;
    while (n_active > 0 && n < p.ns && !cancelled) {
        const uint32_t c = n == 0 ? a->min_spp : (a->step_spp < p.ns - n ? a->step_spp : p.ns - n);
        rtmi_render_params q = p;
        q.ns = c;
        uint32_t chunk_spp = 0, pass_ns = 0;
        if ((rc = plan_and_reserve(s, &q, n_active, chunk_spp, pass_ns))) return rc;
        P.ntiles_local = n_active; P.chunk_spp = chunk_spp; P.pass_stride = pass_ns; P.samples = s->samples.ptr;
        HIP_TRY(hipMemsetAsync(count, 0, sizeof(uint32_t), stream));
        A.tiles_in = lists[cur]; A.tiles_out = lists[cur ^ 1];
        const uint64_t units_before = s->units_total;
        // samples [n, n + c) in sub-passes when the per-sample buffer does not hold the step
        rc = run_passes(s, P, stream, n, c, false, run_slots, 1u, counts, [&](uint32_t blocks, bool first, bool last) -> int {
            if (int lrc = launch(blocks, (const uint32_t *)lists[cur])) return lrc;
            A.first = (n == 0 && first) ? 1 : 0;
            A.decide = last ? 1 : 0;
            HIP_TRY(rtmi_adaptive_launch_resolve(stream, s->samples.ptr, P, A));
            return RTMI_OK;
        });
        if (rc) return rc;
        const uint64_t units_step = s->units_total - units_before;
        HIP_TRY(hipMemcpyAsync(s->h_ad_count.ptr, count, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipEventRecord(s->ev[1].e, stream));
        // wait for the step; meanwhile report progress from the unit counters (as wait_with_progress does)
        const uint64_t step_ts = (uint64_t)n_active * c;
        while (fn) {
            const hipError_t qe = hipEventQuery(s->ev[1].e);
            if (qe == hipSuccess) break;
            if (qe != hipErrorNotReady) return fail(RTMI_ERR_DEVICE, std::string("hipEventQuery: ") + hipGetErrorString(qe));
            uint64_t u = 0;
            if ((rc = units_done(s, &u))) return rc;
            u = u > units_before ? u - units_before : 0;
            if (u > units_step) u = units_step;
            uint64_t done = settled + (units_step ? step_ts * u / units_step : 0);
            if (done < shown) done = shown;
            shown = done;
            if (!cancelled && fn(done, total, user) != 0) cancelled = true;
            struct timespec ts = {0, 50 * 1000 * 1000};
            nanosleep(&ts, nullptr);
        }
        HIP_TRY(hipEventSynchronize(s->ev[1].e));
        const uint32_t next = *s->h_ad_count.ptr;
        settled += (uint64_t)(n_active - next) * (p.ns - n) + (uint64_t)next * c; // a retired tile counts at ns
        n += c;
        n_active = next;
        cur ^= 1;
    }
    HIP_TRY(hipEventRecord(s->ev[2].e, stream));
    HIP_TRY(hipEventSynchronize(s->ev[2].e));
    if (fn && !cancelled && fn(total, total, user) != 0) cancelled = true;
    if (cancelled) return fail(RTMI_ERR_CANCELLED, "cancelled by the progress callback");
    return check_overflow(s);
}
static int adaptive_download(rtmi_scene *s, const rtmi_render_params &p, const PassCounts &counts, float *out_linear,
                             uint8_t *out_rgb8, float *out_stderr, uint32_t *out_spp, rtmi_stats *stats) {
    int rc;
    const size_t ntex = (size_t)local_tiles_of(&p, 0) * 64;
    HIP_TRY(hipMemcpy(s->h_texels.ptr, s->texels.ptr, ntex * sizeof(rtmi_texel), hipMemcpyDeviceToHost));
    if (out_stderr && (rc = download_untiled<3>(&p, s->ad_stderr.ptr, ntex, out_stderr))) return rc;
    const size_t npix = (size_t)p.nx * p.ny;
    std::vector<uint32_t> spp_local(out_spp ? 0 : npix);
    uint32_t *spp = out_spp ? out_spp : spp_local.data();
    if ((rc = download_untiled<1>(&p, s->ad_spp.ptr, ntex, spp))) return rc;
    if (stats) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, s->ev[0].e, s->ev[2].e));
        fill_stats(s, &p, stats, ms, ms, counts); // first launch to last resolve, the per-step read-backs included
        stats->samples = 0;                       // the samples traced: every pixel's own count
        for (size_t o = 0; o < npix; o++) stats->samples += spp[o];
    }
    return rtmi_untile(&p, s->h_texels.ptr, out_linear, out_rgb8);
}
template <typename Launch>
static int adaptive_steps(rtmi_scene *s, const rtmi_render_params &p, const rtmi_adaptive *a, DevParams &P, uint32_t kernel,
                          uint32_t wps, float *out_linear, uint8_t *out_rgb8, float *out_stderr, uint32_t *out_spp,
                          rtmi_stats *stats, Launch &&launch) {
    PassCounts counts;
    if (int rc = adaptive_steps_device(s, p, a, P, kernel, wps, counts, launch)) return rc;
    return adaptive_download(s, p, counts, out_linear, out_rgb8, out_stderr, out_spp, stats);
}

// ---- one host path for the estimators of the whole-image modes -----------------------------------------------------------
// The plain estimator, next-event estimation (rtmi_nee.h), environment lighting (rtmi_env.h) or both, in a fixed render, in
// adaptive sampling's step loop (rtmi_adaptive.h, rtmi_adaptive_nee.h) and under Russian roulette (rtmi_roulette.h).  The
// entry points differ in their argument checks and in the kernel they launch; what surrounds the launches is here.

// the checks of rtmi_env_render-style options, in `name`'s words
static int check_env_opts(const char *name, const rtmi_env_render *o) {
    if (o->nee > 1u) return fail(RTMI_ERR_INVALID, std::string(name) + ": nee must be 0 or 1");
    if (!(o->env_select_p > 0.0f && o->env_select_p <= 1.0f))
        return fail(RTMI_ERR_INVALID, std::string(name) + ": env_select_p must be in (0, 1]");
    return RTMI_OK;
}
static int refuse_sky(const char *name, uint32_t flags) {
    if (flags & RTMI_FLAG_SKY)
        return fail(RTMI_ERR_INVALID, std::string(name) + ": RTMI_FLAG_SKY is refused, the map replaces the sky");
    return RTMI_OK;
}
// The estimator of an entry that selects it by an RTMI_ROULETTE_* value (rtmi_roulette.h): the roulette renders, the sessions
// and the batch modes.  env_select_p is read where both the lights and the map are sampled.  lit_estimator: the same of an
// entry that holds the two choices themselves.  null_scene must outlive the Estimator.
Estimator lit_estimator(const char *name, bool nee, bool env, float env_select_p, const char *null_scene) {
    return Estimator{name, nee, env, env_select_p, null_scene, "no light table attached (rtmi_scene_attach_lights)"};
}
Estimator estimator_of(const char *name, uint32_t estimator, float env_select_p, const char *null_scene) {
    const bool nee = estimator == RTMI_ROULETTE_NEE || estimator == RTMI_ROULETTE_ENV_NEE;
    const bool env = estimator == RTMI_ROULETTE_ENV || estimator == RTMI_ROULETTE_ENV_NEE;
    return lit_estimator(name, nee, env, nee && env ? env_select_p : 1.0f, null_scene);
}
// The checks of that selection, two because each entry has checks of its own between them: the value, and what the chosen
// estimator refuses of env_select_p (read, and checked, only where both are sampled) and of the flags.
int check_estimator(const char *name, uint32_t estimator) {
    if (estimator > RTMI_ROULETTE_ENV_NEE)
        return fail(RTMI_ERR_INVALID, std::string(name) + ": estimator must be one of RTMI_ROULETTE_* (0..3)");
    return RTMI_OK;
}
int check_estimator_opts(const char *name, uint32_t estimator, float env_select_p, uint32_t flags) {
    const rtmi_env_render eo{1u, env_select_p};
    if (estimator == RTMI_ROULETTE_ENV_NEE)
        if (int rc = check_env_opts(name, &eo)) return rc;
    const bool env = estimator == RTMI_ROULETTE_ENV || estimator == RTMI_ROULETTE_ENV_NEE;
    return env ? refuse_sky(name, flags) : RTMI_OK;
}

static DevEnv dev_env(const rtmi_scene *s, float p_env) {
    const size_t H = s->env_h, n = (size_t)s->env_w * s->env_h;
    DevEnv E;
    E.texels = s->env_texels.ptr;
    E.row_cdf = s->env_tables.ptr; E.row_p = s->env_tables.ptr + H; E.col_cdf = s->env_tables.ptr + 2 * H; E.col_p = s->env_tables.ptr + 2 * H + n;
    E.w = s->env_w; E.h = s->env_h;
    E.p_env = p_env;
    return E;
}
// The light table and the map as the kernels of this estimator read them (the caller has checked that they are attached);
// empty where it reads none.  p_env: the map's share of the light samples (rtmi_env.h).
void dev_lighting(const rtmi_scene *s, bool nee, bool env, float env_select_p, DevLights &L, DevEnv &E) {
    L = DevLights{};
    E = DevEnv{};
    if (nee) { L.lights = s->nee_lights.ptr; L.prim_light = s->nee_prim_light.ptr; L.n = s->nee_n; }
    if (env) E = dev_env(s, !s->env_sampled ? 0.0f : (s->nee_n > 0u ? env_select_p : 1.0f));
}

// the map and the light table the estimator reads are attached to the handle (the caller holds s->mu)
int check_attached(const Estimator &m, const rtmi_scene *s) {
    if (m.env && !s->has_env)
        return fail(RTMI_ERR_INVALID, std::string(m.name) + ": no environment map attached (rtmi_scene_attach_env)");
    if (m.nee && !s->has_lights) return fail(RTMI_ERR_INVALID, std::string(m.name) + ": " + m.no_lights);
    return RTMI_OK;
}
// the same among the argument checks of the sparse and per-pixel entries: of a handle that is there, under its lock
int check_attached_early(const Estimator &m, const rtmi_scene *s_in) {
    if (!s_in) return RTMI_OK;
    rtmi_scene *s = const_cast<rtmi_scene *>(s_in);
    std::lock_guard<std::mutex> lock(s->mu);
    return check_attached(m, s);
}
// The end of an entry point's checks and the start of its device work, in this order: the handle, its lock, what the
// estimator needs attached, then the device, no earlier render of the handle running, the busy mark.
int begin_call(RenderCall &c, const Estimator &m, rtmi_scene *s) {
    if (!s) return fail(RTMI_ERR_INVALID, m.null_scene);
    c.lock = std::unique_lock<std::mutex>(s->mu);
    if (int rc = check_attached(m, s)) return rc;
    if (m.tree && !s->has_light_tree)
        return fail(RTMI_ERR_INVALID, std::string(m.name) + ": no light tree attached (rtmi_scene_attach_light_tree)");
    HIP_TRY(hipSetDevice(s->device));
    if (int rc = begin_blocking(s)) return rc;
    c.busy.s = s; c.busy.st = s->stream.s;
    return RTMI_OK;
}
void kernel_args(RenderCall &c, const Estimator &m, const rtmi_scene *s, const rtmi_camera *cam,
                        const rtmi_render_params &p) {
    c.P = dev_params(s, &p);
    c.C = dev_camera(cam);
    c.fast = (p.flags & RTMI_FLAG_FAST_CULL) != 0u && boxes_valid(s, cam);
    dev_lighting(s, m.nee, m.env, m.env_select_p, c.L, c.E);
}
// RTMI_FLAG_LIGHT_COOP (rtmi_light_coop.h), after kernel_args: the selection of the cooperative kernel (the rule of
// rtmi_render_adaptive: level-0 scenes under fast-cull, no SYNC) and, where it runs, its traversal plan in c.P.
// RTMI_FLAG_ROULETTE_COOP (rtmi_roulette_coop.h) is the same rule under the roulette entries' flag: `flag` names the
// entry's own bit, `wps` the waves per SIMD its cooperative kernel was compiled for.
static uint32_t light_coop_bits(const rtmi_render_params *p, uint32_t flag = RTMI_FLAG_LIGHT_COOP) { // the bits the flag adds to an entry's accepted ones
    return (p && (p->flags & flag)) ? (flag | (1u << 11)) : 0u;
}
int plan_light_coop(RenderCall &c, rtmi_scene *s, const rtmi_render_params &p, uint32_t flag, uint32_t wps) {
    const bool coop_ok = s->meta.n_prims < (1u << 22) && s->meta.n_nodes < (1u << 25); // (n_alt_nodes < 2^25: validate())
    const bool inst = s->dev.has_prim_xf != 0u || s->dev.has_medium_outer != 0u;
    c.coop = (p.flags & flag) != 0u && c.fast && !(p.flags & RTMI_FLAG_SYNC) && coop_ok && !inst;
    if (!c.coop) return RTMI_OK;
    c.wps = wps;
    if (int rc = plan_traversal(s, &p, true, c.P, c.ext)) return rc;
    if (p.flags & (1u << 11)) { // test knob, as in render_device_locked: a pool this small that it spills all the time
        c.ext = true;
        c.P.coop_cap = 256u;
    }
    c.coop_lds = (size_t)WAVES_PER_BLOCK * CoopLds{c.P.coop_cap, c.ext, false}.words() * sizeof(uint32_t);
    return RTMI_OK;
}
// the persistent grid of the call's render kernel, in wavefronts: CUs x 4 SIMDs x the waves per SIMD it was compiled for
uint64_t light_run_slots(const rtmi_scene *s, const RenderCall &c) {
    return (uint64_t)(s->slots / 20) * 4u * c.wps;
}
// the cooperative launch of a lighting entry's callable: the fixed render's pass (tiles = NULL) or one over the active list
int launch_light_coop(const RenderCall &c, const Estimator &m, rtmi_scene *s, bool sig, uint32_t blocks, const uint32_t *tiles) {
    HIP_TRY(rtmi_light_coop_launch_render(tiles != nullptr, sig, c.ext, m.nee, m.env, blocks, c.coop_lds, s->stream.s, s->dev, c.C,
                                          c.P, tiles, c.L, c.E));
    return RTMI_OK;
}
// begin_call, adaptive sampling's buffers and the kernel arguments: what precedes adaptive_steps
static int begin_adaptive(RenderCall &c, const Estimator &m, rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params &p,
                          const rtmi_adaptive *a) {
    int rc;
    if ((rc = begin_call(c, m, s)) || (rc = adaptive_reserve(s, p, a, local_tiles_of(&p, 0)))) return rc;
    kernel_args(c, m, s, cam, p);
    return RTMI_OK;
}

// The fixed-sample-count render of rtmi_render_nee and rtmi_render_env: the estimator's per-lane kernel, or under
// RTMI_FLAG_LIGHT_COOP its cooperative one (c.coop: the callable launches that), TILE_LIST = false,
// in passes of the render's plan; adaptive sampling's resolve over the list of all tiles carries sum, m and M2 between
// passes and writes texels and standard errors after the last one.  launch(c, sig, blocks) enqueues the render kernel on
// s->stream.s for the pass fields of c.P and returns an RTMI code.  The caller has checked every argument.
// render_fixed_device: after begin_call, enqueue, wait and check overflow; texels, standard errors and signatures stay in
// the scene's device buffers (the frame handle, rtmi_frame_launch.hpp, stops here).  render_fixed adds their copies to the host.
template <typename Launch>
static int render_fixed_device(RenderCall &c, const Estimator &m, rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params &p,
                               bool sig, rtmi_stats *stats, Launch &&launch) {
    int rc;
    hipStream_t stream = s->stream.s;
    const uint32_t T = local_tiles_of(&p, 0);
    const size_t ntex = (size_t)T * 64;
    if ((rc = reserve_texels(s, ntex)) || (rc = grow_adaptive(s, T)) ||
        (sig && (rc = grow(s, s->d_sig, ntex * sizeof(unsigned long long)))))
        return rc;
    uint32_t chunk_spp = 0, pass_ns = 0;
    if ((rc = plan_and_reserve(s, &p, T, chunk_spp, pass_ns))) return rc;

    kernel_args(c, m, s, cam, p);
    if ((rc = plan_light_coop(c, s, p))) return rc;
    DevParams &P = c.P;
    P.chunk_spp = chunk_spp; P.pass_stride = pass_ns; P.samples = s->samples.ptr;
    P.path_sig = sig ? s->d_sig.ptr : nullptr;
    const uint64_t run_slots = light_run_slots(s, c);
    s->last_kernel = c.coop ? RTMI_KERNEL_WAVE_COOP : RTMI_KERNEL_PERLANE;

    if ((rc = begin_passes(s, stream))) return rc;
    if (sig) HIP_TRY(hipMemsetAsync(s->d_sig.ptr, 0, ntex * sizeof(unsigned long long), stream));
    if ((rc = list_all_tiles(s, T, stream))) return rc;
    AdaptiveResolve A;
    A.tiles_in = s->ad_lists.ptr; A.tiles_out = s->ad_lists.ptr + T; A.n_out = s->ad_lists.ptr + 2 * (size_t)T;
    A.state = s->ad_state.ptr; A.texels = s->texels.ptr; A.stderr_out = s->ad_stderr.ptr; A.spp_out = s->ad_spp.ptr;
    A.abs_tol = 0.0; A.rel_tol = 0.0; A.ns = p.ns; // the last pass retires every tile at ns
    PassCounts counts;
    HIP_TRY(hipEventRecord(s->ev[0].e, stream));
    rc = run_passes(s, P, stream, 0, p.ns, true, run_slots, 1u, counts, [&](uint32_t blocks, bool first, bool last) -> int {
        if (int lrc = launch(c, sig, blocks)) return lrc;
        if (last) HIP_TRY(hipEventRecord(s->ev[1].e, stream));
        A.first = first ? 1 : 0;
        A.decide = last ? 1 : 0;
        if (last) HIP_TRY(hipMemsetAsync(A.n_out, 0, sizeof(uint32_t), stream));
        HIP_TRY(rtmi_adaptive_launch_resolve(stream, s->samples.ptr, P, A));
        return RTMI_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipEventRecord(s->ev[2].e, stream));
    rtmi_scene *one[1] = {s};
    if ((rc = wait_with_progress(one, &s->ev[2].e, 1, &p))) return rc;
    if ((rc = check_overflow(s))) return rc;
    return stats ? fill_stats_from_events(s, &p, stats, counts) : RTMI_OK;
}
template <typename Launch>
static int render_fixed(const Estimator &m, rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params &p, float *out_linear,
                        uint8_t *out_rgb8, float *out_stderr, uint64_t *out_path_sig, rtmi_stats *stats, Launch &&launch) {
    RenderCall c;
    int rc;
    if ((rc = begin_call(c, m, s)) || (rc = render_fixed_device(c, m, s, cam, p, out_path_sig != nullptr, stats, launch))) return rc;
    const size_t ntex = (size_t)local_tiles_of(&p, 0) * 64;
    HIP_TRY(hipMemcpy(s->h_texels.ptr, s->texels.ptr, ntex * sizeof(rtmi_texel), hipMemcpyDeviceToHost));
    if (out_stderr && (rc = download_untiled<3>(&p, s->ad_stderr.ptr, ntex, out_stderr))) return rc;
    if (out_path_sig && (rc = download_untiled<1>(&p, s->d_sig.ptr, ntex, out_path_sig))) return rc;
    return rtmi_untile(&p, s->h_texels.ptr, out_linear, out_rgb8);
}

// The plain estimator's adaptive render after begin_call: adaptive sampling's buffers, the kernel arguments, the kernel
// selection and adaptive_steps_device (rtmi_render_adaptive; the frame handle with min_spp == ns, step_spp == 1).
static int adaptive_plain_device(RenderCall &c, const Estimator &m, rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params &p,
                                 const rtmi_adaptive *a, PassCounts &counts) {
    int rc;
    if ((rc = adaptive_reserve(s, p, a, local_tiles_of(&p, 0)))) return rc;
    kernel_args(c, m, s, cam, p);
    DevParams &P = c.P;
    // kernel selection as in render_device_locked; the rare compositions (level-1/2 instantiations there) run per-lane
    const bool fast = c.fast, sync = (p.flags & RTMI_FLAG_SYNC) != 0u;
    const bool coop_ok = s->meta.n_prims < (1u << 22) && s->meta.n_nodes < (1u << 25); // (n_alt_nodes < 2^25: validate())
    const bool inst = s->dev.has_prim_xf != 0u || s->dev.has_medium_outer != 0u;
    const bool coop = fast && !sync && coop_ok && !inst;
    bool ext = false;
    if ((rc = plan_traversal(s, &p, coop, P, ext))) return rc;
    const int which = coop ? (ext ? RTMI_AD_COOP_EXT : RTMI_AD_COOP_LEAN) : (fast ? RTMI_AD_PERLANE_FAST : RTMI_AD_PERLANE);
    const size_t coop_lds = (size_t)WAVES_PER_BLOCK * CoopLds{P.coop_cap, ext, false}.words() * sizeof(uint32_t);
    return adaptive_steps_device(s, p, a, P, coop ? RTMI_KERNEL_WAVE_COOP : RTMI_KERNEL_PERLANE, 4u, counts,
                                 [&](uint32_t blocks, const uint32_t *tiles) -> int {
                                     HIP_TRY(rtmi_adaptive_launch_render(which, blocks, coop ? coop_lds : 0, s->stream.s, s->dev, c.C,
                                                                         P, tiles));
                                     return RTMI_OK;
                                 });
}

extern "C" int rtmi_render_adaptive(rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params *p_in,
                                    const rtmi_adaptive *a, float *out_linear, uint8_t *out_rgb8, float *out_stderr,
                                    uint32_t *out_spp, rtmi_stats *stats) {
    // every argument check comes before the first use of the handle (and of the device)
    if (!p_in || !a || !cam) return fail(RTMI_ERR_INVALID, "NULL argument");
    int rc = check_mode_params(p_in, RTMI_FLAG_FAST_CULL | RTMI_FLAG_SYNC | RTMI_FLAG_REF_TREE | RTMI_FLAG_SKY | RTMI_FLAG_FACE_FORWARD |
                                         RTMI_FLAG_UV_BOOK,
                               "adaptive sampling accepts the flags FAST_CULL, SYNC, REF_TREE, SKY, FACE_FORWARD and "
                               "UV_BOOK only (not PATH_SIG, PROFILE, ASYNC, BLOCK_COOP, PROGRESSIVE, TEST_OVERFLOW)",
                               "adaptive sampling renders the whole image: tile_world must be 1");
    if (rc) return rc;
    if ((rc = check_adaptive(p_in, a))) return rc;
    const Estimator m{"rtmi_render_adaptive", false, false, 1.0f, "scene is NULL", ""};
    RenderCall c;
    PassCounts counts;
    if ((rc = begin_call(c, m, s)) || (rc = adaptive_plain_device(c, m, s, cam, *p_in, a, counts))) return rc;
    return adaptive_download(s, *p_in, counts, out_linear, out_rgb8, out_stderr, out_spp, stats);
}

// ---- first-hit features (include/rtmi_features.h) ---------------------------------------------------------------------
// The per-lane features kernel (rtmi_features.hip) in passes of the render's plan, sized for 32-B slots; a resolve per
// pass carries the f64 sums and writes the planes after the last one.  Progress and cancellation as rtmi_render's.
// features_device: under the scene's lock and after begin_blocking, enqueue, wait and check overflow; the four planes stay
// in s->ft_planes.ptr, the signatures in s->d_sig.ptr (the frame handle, rtmi_frame_launch.hpp, stops here).  The entry adds the
// copies to the host.
static int features_device(rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params &p, bool sig, rtmi_stats *stats) {
    int rc;
    hipStream_t stream = s->stream.s;
    const uint32_t T = local_tiles_of(&p, 0);
    const size_t ntex = (size_t)T * 64, npix = (size_t)p.nx * p.ny;
    if ((rc = grow(s, s->ft_state, ntex * 8 * sizeof(double))) ||
        (rc = grow(s, s->ft_planes, npix * 8 * sizeof(float))) ||
        (sig && (rc = grow(s, s->d_sig, ntex * sizeof(unsigned long long)))))
        return rc;
    // the per-sample buffer, planned for 32-B slots, before the clock starts
    uint32_t chunk_spp = 0, pass_ns = 0;
    if ((rc = plan_and_reserve(s, &p, T, chunk_spp, pass_ns, RTMI_FEAT_SLOT_BYTES))) return rc;

    DevParams P = dev_params(s, &p);
    P.chunk_spp = chunk_spp; P.pass_stride = pass_ns; P.samples = s->samples.ptr;
    const DevCamera C = dev_camera(cam);
    const bool fast = (p.flags & RTMI_FLAG_FAST_CULL) != 0u && boxes_valid(s, cam);
    P.path_sig = sig ? s->d_sig.ptr : nullptr;
    const uint64_t run_slots = (uint64_t)(s->slots / 20) * 4u * 4u;
    s->last_kernel = RTMI_KERNEL_PERLANE;

    if ((rc = begin_passes(s, stream))) return rc;
    if (sig) HIP_TRY(hipMemsetAsync(s->d_sig.ptr, 0, ntex * sizeof(unsigned long long), stream));
    FeaturesResolve R;
    R.slots = reinterpret_cast<const FeatSlot *>(s->samples.ptr);
    R.state = s->ft_state.ptr;
    R.albedo = s->ft_planes.ptr; R.normal = s->ft_planes.ptr + npix * 3; R.depth = s->ft_planes.ptr + npix * 6;
    R.hits = reinterpret_cast<uint32_t *>(s->ft_planes.ptr + npix * 7);
    PassCounts counts;
    HIP_TRY(hipEventRecord(s->ev[0].e, stream));
    rc = run_passes(s, P, stream, 0, p.ns, true, run_slots, 1u, counts, [&](uint32_t blocks, bool first, bool last) -> int {
        HIP_TRY(rtmi_features_launch_render(fast, sig, blocks, stream, s->dev, C, P));
        if (last) HIP_TRY(hipEventRecord(s->ev[1].e, stream));
        R.first = first ? 1 : 0;
        R.last = last ? 1 : 0;
        HIP_TRY(rtmi_features_launch_resolve(stream, P, R));
        return RTMI_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipEventRecord(s->ev[2].e, stream));
    rtmi_scene *one[1] = {s};
    if ((rc = wait_with_progress(one, &s->ev[2].e, 1, &p))) return rc;
    if ((rc = check_overflow(s))) return rc;
    return stats ? fill_stats_from_events(s, &p, stats, counts) : RTMI_OK;
}
extern "C" int rtmi_render_features(rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params *p_in, float *out_albedo,
                                    float *out_normal, float *out_depth, uint32_t *out_hits, uint64_t *out_path_sig,
                                    rtmi_stats *stats) {
    // every argument check comes before the first use of the handle (and of the device)
    if (!p_in || !cam) return fail(RTMI_ERR_INVALID, "NULL argument");
    int rc = check_mode_params(p_in, RTMI_FLAG_FAST_CULL | RTMI_FLAG_SYNC | RTMI_FLAG_REF_TREE | RTMI_FLAG_SKY | RTMI_FLAG_FACE_FORWARD |
                                         RTMI_FLAG_UV_BOOK | RTMI_FLAG_PATH_SIG,
                               "features accept the flags FAST_CULL, SYNC, REF_TREE, SKY, FACE_FORWARD, UV_BOOK and "
                               "PATH_SIG only (not PROFILE, ASYNC, BLOCK_COOP, PROGRESSIVE, TEST_OVERFLOW)",
                               "features cover the whole image: tile_world must be 1");
    if (rc) return rc;
    if (!s) return fail(RTMI_ERR_INVALID, "scene is NULL");
    std::lock_guard<std::mutex> lock(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = begin_blocking(s))) return rc;
    const rtmi_render_params &p = *p_in;
    BusyMark busy_mark{s, s->stream.s};
    if ((rc = features_device(s, cam, p, out_path_sig != nullptr, stats))) return rc;
    const size_t ntex = (size_t)local_tiles_of(&p, 0) * 64, npix = (size_t)p.nx * p.ny;
    const float *planes = s->ft_planes.ptr;
    if (out_albedo) HIP_TRY(hipMemcpy(out_albedo, planes, npix * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (out_normal) HIP_TRY(hipMemcpy(out_normal, planes + npix * 3, npix * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (out_depth) HIP_TRY(hipMemcpy(out_depth, planes + npix * 6, npix * sizeof(float), hipMemcpyDeviceToHost));
    if (out_hits) HIP_TRY(hipMemcpy(out_hits, planes + npix * 7, npix * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (out_path_sig && (rc = download_untiled<1>(&p, s->d_sig.ptr, ntex, out_path_sig))) return rc;
    return RTMI_OK;
}

// ---- ray queries (include/rtmi_query.h) ---------------------------------------------------------------------------------
// The checks both forms of an entry share, in this order: params, flags, scene; *go = false: n == 0, nothing to launch.
// Then, for a batch with rays, the ray and output pointers.
static int query_check(const char *name, const rtmi_scene *s, const rtmi_query_params *p, const void *rays, const void *out, bool *go) {
    *go = false;
    if (!p) return fail(RTMI_ERR_INVALID, std::string(name) + ": params is NULL");
    if (p->flags & ~RTMI_FLAG_FAST_CULL)
        return fail(RTMI_ERR_UNSUPPORTED, std::string(name) + ": ray queries accept the flags 0 and FAST_CULL only");
    if (!s) return fail(RTMI_ERR_INVALID, std::string(name) + ": scene is NULL");
    if (p->n == 0) return RTMI_OK;
    if (!rays) return fail(RTMI_ERR_INVALID, std::string(name) + ": rays is NULL");
    if (!out) return fail(RTMI_ERR_INVALID, std::string(name) + ": output is NULL");
    *go = true;
    return RTMI_OK;
}
// what the host forms refuse of a ray; the device forms take the caller's word
int query_check_rays(const char *name, const rtmi_ray *rays, const float *time, uint32_t n) {
    const auto bad = [&](uint32_t i, const char *what) {
        return fail(RTMI_ERR_INVALID, std::string(name) + ": ray " + std::to_string(i) + " " + what);
    };
    for (uint32_t i = 0; i < n; i++) {
        const rtmi_ray &r = rays[i];
        bool finite = std::isfinite(r.t_min) && !std::isnan(r.t_max) && r.t_max != -std::numeric_limits<float>::infinity();
        for (int k = 0; k < 3; k++) finite = finite && std::isfinite(r.o[k]) && std::isfinite(r.d[k]);
        if (time) finite = finite && std::isfinite(time[i]);
        if (!finite) return bad(i, "has a non-finite component");
        if (r.d[0] == 0.0f && r.d[1] == 0.0f && r.d[2] == 0.0f) return bad(i, "has a zero direction");
        if (r.t_min > r.t_max) return bad(i, "has t_min > t_max");
    }
    return RTMI_OK;
}
// The pruned closest-hit traversal needs the BVH boxes to hold at every ray time (boxes_valid): with a time plane the
// scene's range must be unbounded, without one it must contain 0.  Wave-uniform, decided here.
bool query_fast(const rtmi_scene *s, const rtmi_query_params *p, bool has_time) {
    if (!(p->flags & RTMI_FLAG_FAST_CULL)) return false;
    const float lo = s->meta.bvh_time_lo, hi = s->meta.bvh_time_hi;
    if (has_time) return lo <= -RTMI_FLT_MAX && hi >= RTMI_FLT_MAX; // no MovingSphere inside a BVH (rtmi.h)
    return lo <= 0.0f && 0.0f <= hi;
}
static QueryBatch query_batch(const rtmi_scene *s, const rtmi_query_params *p, const void *d_rays, const void *d_time, void *d_out,
                              bool any) {
    QueryBatch B{};
    B.prim_gaps = s->q_flip_gaps.ptr;
    B.item_gaps = s->q_flip_gaps.ptr ? s->q_flip_gaps.ptr + s->meta.n_prims : nullptr;
    B.rays = reinterpret_cast<const float4 *>(d_rays);
    B.time = reinterpret_cast<const float *>(d_time);
    if (any) B.occluded = reinterpret_cast<uint8_t *>(d_out); else B.hits = reinterpret_cast<float4 *>(d_out);
    B.n = p->n;
    const uint64_t key = p->seed + p->first_ray; // mod 2^64
    B.key0 = (uint32_t)key; B.key1 = (uint32_t)(key >> 32);
    return B;
}
// the asynchronous forms: enqueued on the caller's stream behind the handle's previous call, like rtmi_render_device
static int query_device(const char *name, bool any, rtmi_scene *s, const rtmi_query_params *p, const void *d_rays, const void *d_time,
                        void *d_out, void *stream_) {
    bool go;
    if (int rc = query_check(name, s, p, d_rays, d_out, &go)) return rc;
    if (!go) return RTMI_OK;
    AsyncCall c;
    if (int rc = c.begin(Estimator{name, false, false, 1.0f, "scene is NULL", ""}, s, stream_)) return rc;
    HIP_TRY(rtmi_query_launch(any, query_fast(s, p, d_time != nullptr), c.stream, s->dev, query_batch(s, p, d_rays, d_time, d_out, any)));
    return RTMI_OK;
}
// the blocking forms: the batch goes through the handle's query buffers (none of its render scratch) on its own stream
static int query_host(const char *name, bool any, rtmi_scene *s, const rtmi_query_params *p, const rtmi_ray *rays, const float *time,
                      void *out, double *kernel_ms) {
    bool go;
    int rc;
    if ((rc = query_check(name, s, p, rays, out, &go))) return rc;
    if (kernel_ms) *kernel_ms = 0.0;
    if (!go) return RTMI_OK;
    if ((rc = query_check_rays(name, rays, time, p->n))) return rc;
    const Estimator m{name, false, false, 1.0f, "scene is NULL", ""};
    RenderCall c;
    if ((rc = begin_call(c, m, s))) return rc;
    hipStream_t stream = s->stream.s;
    const size_t n = p->n, out_bytes = any ? n : n * sizeof(rtmi_hit);
    if ((rc = grow(s, s->q_rays, n * sizeof(rtmi_ray))) ||
        (time && (rc = grow(s, s->q_time, n * sizeof(float)))) || (rc = grow(s, s->q_out, out_bytes)))
        return rc;
    HIP_TRY(hipMemcpyAsync(s->q_rays.ptr, rays, n * sizeof(rtmi_ray), hipMemcpyHostToDevice, stream));
    if (time) HIP_TRY(hipMemcpyAsync(s->q_time.ptr, time, n * sizeof(float), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(s->ev[0].e, stream));
    HIP_TRY(rtmi_query_launch(any, query_fast(s, p, time != nullptr), stream, s->dev,
                              query_batch(s, p, s->q_rays.ptr, time ? s->q_time.ptr : nullptr, s->q_out.ptr, any)));
    HIP_TRY(hipEventRecord(s->ev[1].e, stream));
    HIP_TRY(hipMemcpyAsync(out, s->q_out.ptr, out_bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (kernel_ms) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, s->ev[0].e, s->ev[1].e));
        *kernel_ms = (double)ms;
    }
    return RTMI_OK;
}
extern "C" int rtmi_scene_attach_flips(rtmi_scene *s, const uint32_t *prim_gaps, uint32_t n_prims, const uint32_t *item_gaps,
                                       uint32_t n_items) {
    const char *name = "rtmi_scene_attach_flips";
    if (!s) return fail(RTMI_ERR_INVALID, std::string(name) + ": scene is NULL");
    const bool detach = !prim_gaps && !item_gaps;
    if (!detach && (n_prims != s->meta.n_prims || n_items != s->meta.n_items))
        return fail(RTMI_ERR_INVALID, std::string(name) + ": the counts are not the scene's");
    if (!detach && ((n_prims && !prim_gaps) || (n_items && !item_gaps))) return fail(RTMI_ERR_INVALID, std::string(name) + ": NULL array");
    std::lock_guard<std::mutex> lock(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    const auto fill = [&]() -> int { // (a running query may read the old table)
        if (detach) return RTMI_OK;
        HIP_TRY(s->q_flip_gaps.alloc(((size_t)n_prims + n_items + 1u) * sizeof(uint32_t)));
        uint32_t *const d = s->q_flip_gaps.ptr;
        if (n_prims) HIP_TRY(hipMemcpy(d, prim_gaps, (size_t)n_prims * sizeof(uint32_t), hipMemcpyHostToDevice));
        if (n_items) HIP_TRY(hipMemcpy(d + n_prims, item_gaps, (size_t)n_items * sizeof(uint32_t), hipMemcpyHostToDevice));
        return RTMI_OK;
    };
    return replace_attached(s, nullptr, fill, s->q_flip_gaps);
}
extern "C" int rtmi_trace(rtmi_scene *s, const rtmi_query_params *p, const rtmi_ray *rays, const float *time, rtmi_hit *hits_out,
                          double *kernel_ms) {
    return query_host("rtmi_trace", false, s, p, rays, time, hits_out, kernel_ms);
}
extern "C" int rtmi_occluded(rtmi_scene *s, const rtmi_query_params *p, const rtmi_ray *rays, const float *time, uint8_t *occluded_out,
                             double *kernel_ms) {
    return query_host("rtmi_occluded", true, s, p, rays, time, occluded_out, kernel_ms);
}
extern "C" int rtmi_trace_device(rtmi_scene *s, const rtmi_query_params *p, const void *d_rays, const void *d_time, void *d_hits,
                                 void *stream) {
    return query_device("rtmi_trace_device", false, s, p, d_rays, d_time, d_hits, stream);
}
extern "C" int rtmi_occluded_device(rtmi_scene *s, const rtmi_query_params *p, const void *d_rays, const void *d_time,
                                    void *d_occluded, void *stream) {
    return query_device("rtmi_occluded_device", true, s, p, d_rays, d_time, d_occluded, stream);
}

// ---- next-event estimation (include/rtmi_nee.h) -------------------------------------------------------------------------
// The light table of a description: the eligible occurrences (item, prim) in item order, primitives in the order the item
// reaches them.  Host code only (no HIP call), so the CPU tests can call it.
static int nee_lights_of(const rtmi_scene_desc *d, std::vector<rtmi_light> &out) {
    out.clear();
    if (!d) return fail(RTMI_ERR_INVALID, "NULL argument");
    if (d->abi_version != RTMI_ABI_VERSION) return fail(RTMI_ERR_INVALID, "rtmi_lights_from_desc: abi_version mismatch");
    if ((d->n_items && !d->items) || (d->n_prims && (!d->prim_a || !d->prim_b || !d->prim_meta)) ||
        (d->n_nodes && !d->nodes) || (d->n_materials && !d->materials) || (d->n_textures && !d->textures))
        return fail(RTMI_ERR_INVALID, "rtmi_lights_from_desc: a non-empty array is NULL");
    // every (item, prim) the world list can report, and how many items reach each primitive
    std::vector<std::pair<int32_t, int32_t>> occ;
    std::vector<int32_t> last_item(d->n_prims, -1);
    std::vector<uint32_t> n_items_of(d->n_prims, 0u);
    auto reach = [&](int32_t it, int64_t prim) -> bool {
        if (prim < 0 || prim >= (int64_t)d->n_prims) return false;
        if (last_item[prim] != it) { last_item[prim] = it; n_items_of[prim]++; occ.push_back({it, (int32_t)prim}); }
        return true;
    };
    for (uint32_t it = 0; it < d->n_items; it++) {
        const rtmi_item &I = d->items[it];
        if (I.kind == RTMI_ITEM_LIST) {
            for (int64_t k = 0; k < I.count; k++)
                if (!reach((int32_t)it, (int64_t)I.first + k)) return fail(RTMI_ERR_INVALID, "rtmi_lights_from_desc: primitive out of range");
        } else if (I.kind == RTMI_ITEM_BVH) {
            if (I.first < 0 || (uint32_t)I.first >= d->n_nodes) return fail(RTMI_ERR_INVALID, "rtmi_lights_from_desc: root out of range");
            std::vector<int32_t> stack{I.first};
            uint64_t visits = 0;
            while (!stack.empty()) {
                const int32_t n = stack.back();
                stack.pop_back();
                if (++visits > 2ull * d->n_nodes + 2ull) return fail(RTMI_ERR_INVALID, "rtmi_lights_from_desc: the tree is not a tree");
                for (const int32_t c : {d->nodes[n].left, d->nodes[n].right}) {
                    if (c >= 0) {
                        if ((uint32_t)c >= d->n_nodes) return fail(RTMI_ERR_INVALID, "rtmi_lights_from_desc: node out of range");
                        stack.push_back(c);
                    } else if (!reach((int32_t)it, (int64_t)((uint32_t)c & 0x0fffffffu))) {
                        return fail(RTMI_ERR_INVALID, "rtmi_lights_from_desc: primitive out of range");
                    }
                }
            }
        } else {
            return fail(RTMI_ERR_INVALID, "rtmi_lights_from_desc: unknown item kind");
        }
    }
    std::sort(occ.begin(), occ.end());
    double total = 0.0;
    for (const auto &o : occ) {
        const rtmi_item &I = d->items[o.first];
        const rtmi_prim_meta &M = d->prim_meta[o.second];
        const float *A = d->prim_a + (size_t)o.second * 4;
        if (n_items_of[o.second] != 1u) continue;              // reported by more than one item: not one occurrence
        if (I.xform_count != 0 || (I.flags & RTMI_ITEMFLAG_MEDIUM)) continue;
        if ((M.flags >> RTMI_PRIMFLAG_XF_COUNT_SHIFT) & RTMI_PRIM_XF_MAX) continue;
        if (M.material < 0 || (uint32_t)M.material >= d->n_materials) continue;
        const rtmi_material &m = d->materials[M.material];
        if (m.kind != RTMI_MAT_DIFFUSE_LIGHT) continue;
        double area;
        if (M.type == RTMI_PRIM_RECT) {
            if (!(A[0] < A[2]) || !(A[1] < A[3])) continue;      // never hit (rect.rs)
            area = ((double)A[2] - (double)A[0]) * ((double)A[3] - (double)A[1]);
        } else if (M.type == RTMI_PRIM_SPHERE ||
                   (M.type == RTMI_PRIM_MSPHERE && d->prim_b[(size_t)o.second * 4] == 0.0f && d->prim_b[(size_t)o.second * 4 + 1] == 0.0f &&
                    d->prim_b[(size_t)o.second * 4 + 2] == 0.0f && std::isfinite(M.inv_dt) && std::isfinite(d->prim_b[(size_t)o.second * 4 + 3]))) {
            // (a MSPHERE without displacement is how the lowerings store a static Sphere among moving ones: c0 at all times)
            if (!(A[3] > 0.0f) || !std::isfinite(A[0]) || !std::isfinite(A[1]) || !std::isfinite(A[2])) continue;
            area = 4.0 * M_PI * (double)A[3] * (double)A[3];
        } else {
            continue;                                            // MSPHERE, CUBE
        }
        double w = 1.0;
        if (m.tex >= 0 && (uint32_t)m.tex < d->n_textures && d->textures[m.tex].kind == RTMI_TEX_SOLID) {
            const rtmi_texture &t = d->textures[m.tex];
            w = std::max(std::max((double)t.f0, (double)t.f1), (double)t.f2);
        }
        if (!(w > 0.0) || !std::isfinite(area * w) || !(area > 0.0)) continue;
        rtmi_light L{};
        L.item = o.first; L.prim = o.second; L.kind = M.type == RTMI_PRIM_RECT ? RTMI_PRIM_RECT : RTMI_PRIM_SPHERE;
        L.material = M.material;
        L.area = area; L.weight = w;
        out.push_back(L);
        total += area * w;
    }
    double c = 0.0;
    for (size_t i = 0; i < out.size(); i++) {
        out[i].select_p = out[i].area * out[i].weight / total;
        c += out[i].select_p;
        out[i].cdf = i + 1 == out.size() ? 1.0 : c;
    }
    return RTMI_OK;
}

extern "C" int rtmi_lights_from_desc(const rtmi_scene_desc *desc, rtmi_light *out, uint32_t cap, uint32_t *count) {
    if (!desc || !count || (cap && !out)) return fail(RTMI_ERR_INVALID, "NULL argument");
    std::vector<rtmi_light> v;
    const int rc = nee_lights_of(desc, v);
    if (rc) return rc;
    for (size_t i = 0; i < v.size() && i < cap; i++) out[i] = v[i];
    *count = (uint32_t)v.size();
    return RTMI_OK;
}

extern "C" int rtmi_scene_attach_lights(rtmi_scene *s, const rtmi_scene_desc *d) {
    if (!s || !d) return fail(RTMI_ERR_INVALID, "NULL argument");
    const rtmi_scene_desc &m = s->meta;
    if (d->n_items != m.n_items || d->n_prims != m.n_prims || d->n_nodes != m.n_nodes || d->n_xforms != m.n_xforms ||
        d->n_materials != m.n_materials || d->n_textures != m.n_textures)
        return fail(RTMI_ERR_INVALID, "rtmi_scene_attach_lights: counts differ from the handle's scene description");
    std::vector<rtmi_light> v;
    int rc = nee_lights_of(d, v);
    if (rc) return rc;
    std::vector<NeeLight> dl(v.size() ? v.size() : 1);
    std::vector<int32_t> pl(d->n_prims ? d->n_prims : 1, -1);
    for (size_t i = 0; i < v.size(); i++) {
        NeeLight &L = dl[i];
        const float *A = d->prim_a + (size_t)v[i].prim * 4;
        L.geo = make_float4(A[0], A[1], A[2], A[3]);
        L.k = d->prim_b[(size_t)v[i].prim * 4];
        L.plane = v[i].kind == RTMI_PRIM_RECT ? (int32_t)((d->prim_meta[v[i].prim].flags >> RTMI_PRIMFLAG_PLANE_SHIFT) & 3u) : -1;
        L.item = v[i].item; L.prim = v[i].prim;
        L.area = (float)v[i].area; L.p_sel = (float)v[i].select_p; L.cdf = (float)v[i].cdf;
        L.pad = 0;
        pl[v[i].prim] = (int32_t)i;
    }
    std::lock_guard<std::mutex> lock(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    const auto fill = [&]() -> int { // (a running NEE render may read the old table)
        s->has_light_tree = false; // its leaves index the table it was built over (rtmi_light_tree.h)
        s->rl_on = s->rl_ready = false; // ... and so do the tables of a handle that follows its lights (rtmi_relight.h)
        HIP_TRY(s->nee_lights.alloc(dl.size() * sizeof(NeeLight)));
        HIP_TRY(s->nee_prim_light.alloc(pl.size() * sizeof(int32_t)));
        HIP_TRY(hipMemcpy(s->nee_lights.ptr, dl.data(), dl.size() * sizeof(NeeLight), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(s->nee_prim_light.ptr, pl.data(), pl.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        s->nee_n = (uint32_t)v.size();
        s->has_lights = true;
        return RTMI_OK;
    };
    return replace_attached(s, &s->has_lights, fill, s->nee_lights, s->nee_prim_light);
}

// ---- light tree (include/rtmi_light_tree.h) -----------------------------------------------------------------------------
extern "C" int rtmi_scene_attach_light_tree(rtmi_scene *s, const rtmi_scene_desc *d) {
    if (!s || !d) return fail(RTMI_ERR_INVALID, "rtmi_scene_attach_light_tree: NULL argument");
    const rtmi_scene_desc &m = s->meta;
    if (d->n_items != m.n_items || d->n_prims != m.n_prims || d->n_nodes != m.n_nodes || d->n_xforms != m.n_xforms ||
        d->n_materials != m.n_materials || d->n_textures != m.n_textures)
        return fail(RTMI_ERR_INVALID, "rtmi_scene_attach_light_tree: counts differ from the handle's scene description");
    std::vector<rtmi_light_node> nodes;
    std::vector<rtmi_light_path> paths;
    int rc = rtmi_light_tree_build(d, nodes, paths); // every check of the description comes before the first use of the device
    if (rc) return rc;
    bool has_lights;
    {
        std::lock_guard<std::mutex> lock(s->mu);
        has_lights = s->has_lights;
    }
    if (!has_lights && (rc = rtmi_scene_attach_lights(s, d))) return rc;
    std::lock_guard<std::mutex> lock(s->mu);
    if (s->nee_n * 2u != (uint32_t)nodes.size())
        return fail(RTMI_ERR_INVALID, "rtmi_scene_attach_light_tree: the attached light table is not this description's");
    HIP_TRY(hipSetDevice(s->device));
    const auto fill = [&]() -> int { // (a running render may read the old tree)
        const size_t nn = std::max<size_t>(nodes.size(), 2), np = std::max<size_t>(paths.size(), 1);
        s->rl_on = s->rl_ready = false; // the tables of a handle that follows its lights hold the old tree's slots (rtmi_relight.h)
        HIP_TRY(s->lt_nodes.alloc(nn * sizeof(rtmi_light_node))); // hipMalloc aligns to 256 B
        HIP_TRY(s->lt_paths.alloc(np * sizeof(rtmi_light_path)));
        HIP_TRY(hipMemset(s->lt_nodes.ptr, 0, nn * sizeof(rtmi_light_node)));
        HIP_TRY(hipMemset(s->lt_paths.ptr, 0, np * sizeof(rtmi_light_path)));
        if (!nodes.empty()) {
            HIP_TRY(hipMemcpy(s->lt_nodes.ptr, nodes.data(), nodes.size() * sizeof(rtmi_light_node), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(s->lt_paths.ptr, paths.data(), paths.size() * sizeof(rtmi_light_path), hipMemcpyHostToDevice));
        }
        s->lt_n = (uint32_t)nodes.size();
        s->has_light_tree = true;
        return RTMI_OK;
    };
    return replace_attached(s, &s->has_light_tree, fill, s->lt_nodes, s->lt_paths);
}

static DevLightTree dev_light_tree(const rtmi_scene *s) {
    DevLightTree T;
    T.nodes = s->lt_nodes.ptr; T.paths = s->lt_paths.ptr; T.n = s->lt_n;
    return T;
}

extern "C" int rtmi_probe_light_tree(rtmi_scene *s, int op, const float *points, const void *aux, uint32_t n, uint32_t *out_light,
                                     float *out_p) {
    const bool pick = op == RTMI_LIGHT_TREE_PROBE_PICK;
    if (!s) return fail(RTMI_ERR_INVALID, "rtmi_probe_light_tree: scene is NULL");
    if (!pick && op != RTMI_LIGHT_TREE_PROBE_PMF) return fail(RTMI_ERR_INVALID, "rtmi_probe_light_tree: unknown op");
    if (n > 0u && (!points || !aux || !out_p || (pick && !out_light))) return fail(RTMI_ERR_INVALID, "rtmi_probe_light_tree: NULL argument");
    std::lock_guard<std::mutex> lock(s->mu);
    if (!s->has_light_tree)
        return fail(RTMI_ERR_INVALID, "rtmi_probe_light_tree: no light tree attached (rtmi_scene_attach_light_tree)");
    if (n == 0u) return RTMI_OK;
    if (s->lt_n == 0u) return fail(RTMI_ERR_INVALID, "rtmi_probe_light_tree: the tree is empty (the scene has no eligible light)");
    if (!pick)
        for (uint32_t k = 0; k < n; k++)
            if (static_cast<const uint32_t *>(aux)[k] >= s->lt_n / 2u)
                return fail(RTMI_ERR_INVALID, "rtmi_probe_light_tree: a light index is outside the table");
    HIP_TRY(hipSetDevice(s->device));
    if (int rc = begin_blocking(s)) return rc;
    // one device buffer, freed on every return
    float *dpts, *dp;
    uint32_t *daux, *dlight;
    const auto layout = [&](Carve16 &c) {
        dpts = c.take<float>((size_t)n * 3); daux = c.take<uint32_t>(n); dlight = c.take<uint32_t>(n); dp = c.take<float>(n);
    };
    DeviceArena buf;
    HIP_TRY(buf.alloc<16>(layout));
    HIP_TRY(hipMemcpyAsync(dpts, points, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, s->stream.s));
    HIP_TRY(hipMemcpyAsync(daux, aux, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream.s));
    HIP_TRY(rtmi_light_tree_launch_probe(op, dev_light_tree(s), dpts, daux, n, dlight, dp, s->stream.s));
    if (pick) HIP_TRY(hipMemcpyAsync(out_light, dlight, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream.s));
    HIP_TRY(hipMemcpyAsync(out_p, dp, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s->stream.s));
    HIP_TRY(hipStreamSynchronize(s->stream.s));
    return RTMI_OK;
}

// render_fixed's launch of the table's NEE kernel or of the environment kernel (m.env), per-lane or cooperative (c.coop)
static int launch_lit_fixed(const RenderCall &c, const Estimator &m, rtmi_scene *s, bool sig, uint32_t blocks) {
    if (c.coop) return launch_light_coop(c, m, s, sig, blocks, nullptr);
    if (m.env)
        HIP_TRY(rtmi_env_launch_render(c.fast, sig, m.nee, blocks, s->stream.s, s->dev, c.C, c.P, c.L, c.E));
    else
        HIP_TRY(rtmi_nee_launch_render(c.fast, sig, blocks, s->stream.s, s->dev, c.C, c.P, c.L));
    return RTMI_OK;
}

// The per-lane NEE kernel (rtmi_nee.hip), or the cooperative one (rtmi_light_coop.hip), in render_fixed; under
// RTMI_FLAG_LIGHT_TREE the per-lane kernel of rtmi_light_tree.hip.
extern "C" int rtmi_render_nee(rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params *p_in, float *out_linear,
                               uint8_t *out_rgb8, float *out_stderr, uint64_t *out_path_sig, rtmi_stats *stats) {
    // every argument check comes before the first use of the device
    if (!p_in || !cam) return fail(RTMI_ERR_INVALID, "NULL argument");
    int rc = check_mode_params(p_in, RTMI_FLAG_FAST_CULL | RTMI_FLAG_SYNC | RTMI_FLAG_REF_TREE | RTMI_FLAG_SKY | RTMI_FLAG_FACE_FORWARD |
                                         RTMI_FLAG_UV_BOOK | RTMI_FLAG_PATH_SIG | RTMI_FLAG_LIGHT_TREE | light_coop_bits(p_in),
                               "NEE accepts the flags FAST_CULL, SYNC, REF_TREE, SKY, FACE_FORWARD, UV_BOOK and "
                               "PATH_SIG only (not PROFILE, ASYNC, BLOCK_COOP, PROGRESSIVE, TEST_OVERFLOW)",
                               "NEE renders the whole image: tile_world must be 1");
    if (rc) return rc;
    const bool tree = (p_in->flags & RTMI_FLAG_LIGHT_TREE) != 0u;
    if (tree && (p_in->flags & RTMI_FLAG_LIGHT_COOP))
        return fail(RTMI_ERR_UNSUPPORTED, "rtmi_render_nee: the flags LIGHT_TREE and LIGHT_COOP do not combine (rtmi_light_tree.h)");
    Estimator m{"rtmi_render_nee", true, false, 1.0f, "scene is NULL",
                "no light table attached (rtmi_scene_attach_lights)"};
    m.tree = tree;
    return render_fixed(m, s, cam, *p_in, out_linear, out_rgb8, out_stderr, out_path_sig, stats,
                        [&](const RenderCall &c, bool sig, uint32_t blocks) -> int {
                            if (tree && !c.coop) {
                                HIP_TRY(rtmi_light_tree_launch_render(c.fast, sig, blocks, s->stream.s, s->dev, c.C, c.P, c.L,
                                                                      dev_light_tree(s)));
                                return RTMI_OK;
                            }
                            return launch_lit_fixed(c, m, s, sig, blocks);
                        });
}

// ---- environment lighting (include/rtmi_env.h) ------------------------------------------------------------------------
extern "C" int rtmi_scene_attach_env(rtmi_scene *s, const rtmi_env_map *map) {
    if (!s) return fail(RTMI_ERR_INVALID, "scene is NULL");
    EnvTables t;
    std::vector<float4> tex;
    if (map) { // every check of the map comes before the first use of the device
        if (int rc = rtmi_env_build_tables(map, t)) return rc;
        tex.resize((size_t)map->width * map->height);
        for (size_t k = 0; k < tex.size(); k++) tex[k] = make_float4(map->rgb[3 * k], map->rgb[3 * k + 1], map->rgb[3 * k + 2], 0.0f);
    }
    std::lock_guard<std::mutex> lock(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    const auto fill = [&]() -> int { // (a running render may read the old map)
        if (!map) return RTMI_OK;
        const size_t n = tex.size(), H = map->height;
        HIP_TRY(s->env_texels.alloc(n * sizeof(float4)));
        HIP_TRY(s->env_tables.alloc((2 * H + 2 * n) * sizeof(float)));
        HIP_TRY(hipMemcpy(s->env_texels.ptr, tex.data(), n * sizeof(float4), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(s->env_tables.ptr, t.row_cdf.data(), H * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(s->env_tables.ptr + H, t.row_p.data(), H * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(s->env_tables.ptr + 2 * H, t.col_cdf.data(), n * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(s->env_tables.ptr + 2 * H + n, t.col_p.data(), n * sizeof(float), hipMemcpyHostToDevice));
        s->env_w = map->width; s->env_h = map->height;
        s->env_sampled = t.total > 0.0;
        s->has_env = true;
        return RTMI_OK;
    };
    return replace_attached(s, &s->has_env, fill, s->env_texels, s->env_tables);
}

// The per-lane environment kernel (rtmi_env.hip), or the cooperative one (rtmi_light_coop.hip), in render_fixed.
extern "C" int rtmi_render_env(rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params *p_in, const rtmi_env_render *opts,
                               float *out_linear, uint8_t *out_rgb8, float *out_stderr, uint64_t *out_path_sig, rtmi_stats *stats) {
    // every argument check comes before the first use of the device
    if (!p_in || !cam || !opts) return fail(RTMI_ERR_INVALID, "NULL argument");
    const char *name = "rtmi_render_env";
    int rc;
    if ((rc = check_params(p_in)) || (rc = refuse_sky(name, p_in->flags))) return rc;
    rc = check_mode_params(p_in, RTMI_FLAG_FAST_CULL | RTMI_FLAG_SYNC | RTMI_FLAG_REF_TREE | RTMI_FLAG_FACE_FORWARD | RTMI_FLAG_UV_BOOK |
                                     RTMI_FLAG_PATH_SIG | light_coop_bits(p_in),
                           "environment renders accept the flags FAST_CULL, SYNC, REF_TREE, FACE_FORWARD, UV_BOOK and PATH_SIG "
                           "only (not PROFILE, ASYNC, BLOCK_COOP, PROGRESSIVE, TEST_OVERFLOW)",
                           "environment renders render the whole image: tile_world must be 1");
    if (rc || (rc = check_env_opts(name, opts))) return rc;
    const bool nee = opts->nee != 0u;
    const Estimator m{name, nee, true, opts->env_select_p, "scene is NULL",
                      "nee = 1 needs the light table (rtmi_scene_attach_lights)"};
    return render_fixed(m, s, cam, *p_in, out_linear, out_rgb8, out_stderr, out_path_sig, stats,
                        [&](const RenderCall &c, bool sig, uint32_t blocks) -> int { return launch_lit_fixed(c, m, s, sig, blocks); });
}

// ---- adaptive sampling with NEE or environment lighting (include/rtmi_adaptive_nee.h) ---------------------------------
// adaptive sampling's step loop (adaptive_steps) with the per-lane kernel of rtmi_adaptive_nee.hip, or under
// RTMI_FLAG_LIGHT_COOP the cooperative one of rtmi_light_coop.hip: rtmi_render_nee's or rtmi_render_env's estimator over
// the active-tile list
static int adaptive_lit(const Estimator &m, rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params &p,
                        const rtmi_adaptive *a, float *out_linear, uint8_t *out_rgb8, float *out_stderr, uint32_t *out_spp,
                        rtmi_stats *stats) {
    RenderCall c;
    int rc;
    if ((rc = begin_adaptive(c, m, s, cam, p, a)) || (rc = plan_light_coop(c, s, p))) return rc;
    return adaptive_steps(s, p, a, c.P, c.coop ? RTMI_KERNEL_WAVE_COOP : RTMI_KERNEL_PERLANE, c.wps, out_linear, out_rgb8,
                          out_stderr, out_spp, stats, [&](uint32_t blocks, const uint32_t *tiles) -> int {
                              if (c.coop) return launch_light_coop(c, m, s, false, blocks, tiles);
                              HIP_TRY(rtmi_adaptive_nee_launch_render(c.fast, m.nee, m.env, blocks, s->stream.s, s->dev, c.C,
                                                                      c.P, tiles, c.L, c.E));
                              return RTMI_OK;
                          });
}

extern "C" int rtmi_render_adaptive_nee(rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params *p_in,
                                        const rtmi_adaptive *a, float *out_linear, uint8_t *out_rgb8, float *out_stderr,
                                        uint32_t *out_spp, rtmi_stats *stats) {
    // every argument check comes before the first use of the handle (and of the device)
    if (!p_in || !a || !cam) return fail(RTMI_ERR_INVALID, "NULL argument");
    int rc = check_mode_params(p_in, RTMI_ADAPTIVE_NEE_FLAGS | RTMI_FLAG_SKY | light_coop_bits(p_in),
                               "adaptive NEE accepts the flags FAST_CULL, SYNC, REF_TREE, SKY, FACE_FORWARD and UV_BOOK only "
                               "(not PATH_SIG, PROFILE, ASYNC, BLOCK_COOP, PROGRESSIVE, TEST_OVERFLOW)",
                               "adaptive NEE renders the whole image: tile_world must be 1");
    if (rc || (rc = check_adaptive(p_in, a))) return rc;
    const Estimator m{"rtmi_render_adaptive_nee", true, false, 1.0f, "scene is NULL",
                      "no light table attached (rtmi_scene_attach_lights)"};
    return adaptive_lit(m, s, cam, *p_in, a, out_linear, out_rgb8, out_stderr, out_spp, stats);
}

extern "C" int rtmi_render_adaptive_env(rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params *p_in,
                                        const rtmi_env_render *opts, const rtmi_adaptive *a, float *out_linear,
                                        uint8_t *out_rgb8, float *out_stderr, uint32_t *out_spp, rtmi_stats *stats) {
    // every argument check comes before the first use of the handle (and of the device)
    if (!p_in || !a || !cam || !opts) return fail(RTMI_ERR_INVALID, "NULL argument");
    const char *name = "rtmi_render_adaptive_env";
    int rc;
    if ((rc = check_params(p_in)) || (rc = refuse_sky(name, p_in->flags))) return rc;
    rc = check_mode_params(p_in, RTMI_ADAPTIVE_NEE_FLAGS | light_coop_bits(p_in),
                           "adaptive environment renders accept the flags FAST_CULL, SYNC, REF_TREE, FACE_FORWARD and UV_BOOK "
                           "only (not PATH_SIG, PROFILE, ASYNC, BLOCK_COOP, PROGRESSIVE, TEST_OVERFLOW)",
                           "adaptive environment renders render the whole image: tile_world must be 1");
    if (rc || (rc = check_adaptive(p_in, a)) || (rc = check_env_opts(name, opts))) return rc;
    const Estimator m{name, opts->nee != 0u, true, opts->env_select_p, "scene is NULL",
                      "nee = 1 needs the light table (rtmi_scene_attach_lights)"};
    return adaptive_lit(m, s, cam, *p_in, a, out_linear, out_rgb8, out_stderr, out_spp, stats);
}

// ---- Russian-roulette path termination (include/rtmi_roulette.h) ------------------------------------------------------
// Both entries are adaptive sampling's step loop (adaptive_steps) over the per-lane kernels of rtmi_roulette.hip, or under
// RTMI_FLAG_ROULETTE_COOP (rtmi_roulette_coop.h) the cooperative ones of rtmi_roulette_coop.hip (plan_light_coop); the
// fixed render is the single step of ns samples over the list of all tiles (tolerances 0: every tile retires at ns), as
// the resolve of render_fixed.  `a` = NULL: the fixed entry.
static int render_roulette(const char *name, rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params *p_in,
                           const rtmi_roulette *o, const rtmi_adaptive *a, float *out_linear, uint8_t *out_rgb8,
                           float *out_stderr, uint32_t *out_spp, uint32_t *out_bounces, rtmi_stats *stats) {
    const std::string nm = std::string(name) + ": ", null_scene = nm + "scene is NULL";
    int rc = check_params(p_in);
    if (rc) return rc;
    if ((rc = check_estimator(name, o->estimator))) return rc;
    if (o->min_depth == 0u) return fail(RTMI_ERR_INVALID, nm + "min_depth must be at least 1");
    if (!std::isfinite(o->q_min) || !(o->q_min > 0.0f && o->q_min <= 1.0f)) return fail(RTMI_ERR_INVALID, nm + "q_min must be in (0, 1]");
    const bool nee = o->estimator == RTMI_ROULETTE_NEE || o->estimator == RTMI_ROULETTE_ENV_NEE;
    const bool env = o->estimator == RTMI_ROULETTE_ENV || o->estimator == RTMI_ROULETTE_ENV_NEE;
    if ((rc = check_estimator_opts(name, o->estimator, o->env_select_p, p_in->flags))) return rc;
    if (p_in->flags & RTMI_FLAG_PATH_SIG)
        return fail(RTMI_ERR_UNSUPPORTED, nm + "PATH_SIG is refused: a roulette path has no counterpart to compare a signature with");
    const std::string flags_msg = nm + "roulette renders accept the flags FAST_CULL, SYNC, REF_TREE, SKY, FACE_FORWARD and UV_BOOK "
                                       "only (not PATH_SIG, PROFILE, ASYNC, BLOCK_COOP, PROGRESSIVE, TEST_OVERFLOW)";
    const std::string world_msg = nm + "roulette renders render the whole image: tile_world must be 1";
    if ((rc = check_mode_params(p_in, RTMI_ADAPTIVE_NEE_FLAGS | RTMI_FLAG_SKY | light_coop_bits(p_in, RTMI_FLAG_ROULETTE_COOP),
                                flags_msg.c_str(), world_msg.c_str())))
        return rc;
    if (a && (rc = check_adaptive(p_in, a))) return rc;
    const rtmi_render_params &p = *p_in;
    const rtmi_adaptive fixed{p.ns, 1u, 0.0, 0.0}; // one step of ns samples
    if (!a) a = &fixed;
    const Estimator m = estimator_of(name, o->estimator, o->env_select_p, null_scene.c_str());
    RenderCall c;
    if ((rc = begin_adaptive(c, m, s, cam, p, a)) ||
        (rc = plan_light_coop(c, s, p, RTMI_FLAG_ROULETTE_COOP, rtmi_roulette_coop_wps(nee, env))))
        return rc;
    const size_t ntex = (size_t)local_tiles_of(&p, 0) * 64;
    if ((rc = grow(s, s->rr_bounces, ntex * sizeof(uint32_t)))) return rc;
    HIP_TRY(hipMemsetAsync(s->rr_bounces.ptr, 0, ntex * sizeof(uint32_t), s->stream.s));
    const DevRoulette R{s->rr_bounces.ptr, o->min_depth, o->q_min};
    rc = adaptive_steps(s, p, a, c.P, c.coop ? RTMI_KERNEL_WAVE_COOP : RTMI_KERNEL_PERLANE, c.wps, out_linear, out_rgb8,
                        out_stderr, out_spp, stats, [&](uint32_t blocks, const uint32_t *tiles) -> int {
                            if (c.coop) {
                                HIP_TRY(rtmi_roulette_coop_launch_render(c.ext, nee, env, blocks, c.coop_lds, s->stream.s, s->dev,
                                                                         c.C, c.P, tiles, c.L, c.E, R));
                                return RTMI_OK;
                            }
                            HIP_TRY(rtmi_roulette_launch_render(c.fast, nee, env, blocks, s->stream.s, s->dev, c.C, c.P, tiles,
                                                                c.L, c.E, R));
                            return RTMI_OK;
                        });
    if (rc) return rc;
    if (out_bounces && (rc = download_untiled<1>(&p, s->rr_bounces.ptr, ntex, out_bounces))) return rc;
    return RTMI_OK;
}

extern "C" int rtmi_render_roulette(rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params *p_in, const rtmi_roulette *opts,
                                    float *out_linear, uint8_t *out_rgb8, float *out_stderr, uint32_t *out_bounces,
                                    rtmi_stats *stats) {
    // every argument check comes before the first use of the handle (and of the device)
    if (!p_in || !cam || !opts) return fail(RTMI_ERR_INVALID, "rtmi_render_roulette: NULL argument");
    return render_roulette("rtmi_render_roulette", s, cam, p_in, opts, nullptr, out_linear, out_rgb8, out_stderr, nullptr,
                           out_bounces, stats);
}

extern "C" int rtmi_render_adaptive_roulette(rtmi_scene *s, const rtmi_camera *cam, const rtmi_render_params *p_in,
                                             const rtmi_roulette *opts, const rtmi_adaptive *a, float *out_linear,
                                             uint8_t *out_rgb8, float *out_stderr, uint32_t *out_spp, uint32_t *out_bounces,
                                             rtmi_stats *stats) {
    if (!p_in || !cam || !opts || !a) return fail(RTMI_ERR_INVALID, "rtmi_render_adaptive_roulette: NULL argument");
    return render_roulette("rtmi_render_adaptive_roulette", s, cam, p_in, opts, a, out_linear, out_rgb8, out_stderr, out_spp,
                           out_bounces, stats);
}

extern "C" int rtmi_probe_env(rtmi_scene *s, int op, const float *in, float *out, uint32_t n) {
    if (!s || (n > 0u && (!in || !out))) return fail(RTMI_ERR_INVALID, "NULL argument");
    if (op != RTMI_ENV_PROBE_LOOKUP && op != RTMI_ENV_PROBE_SAMPLE) return fail(RTMI_ERR_INVALID, "rtmi_probe_env: unknown op");
    std::lock_guard<std::mutex> lock(s->mu);
    if (!s->has_env) return fail(RTMI_ERR_INVALID, "rtmi_probe_env: no environment map attached (rtmi_scene_attach_env)");
    if (n == 0u) return RTMI_OK;
    HIP_TRY(hipSetDevice(s->device));
    if (int rc = begin_blocking(s)) return rc;
    const size_t nin = (size_t)n * (op == RTMI_ENV_PROBE_LOOKUP ? 3u : 2u), nout = (size_t)n * 4u;
    float *din, *dout; // one device buffer, freed on every return
    const auto layout = [&](Carve16 &c) { din = c.take<float>(nin); dout = c.take<float>(nout); };
    DeviceArena buf;
    HIP_TRY(buf.alloc<16>(layout));
    HIP_TRY(hipMemcpyAsync(din, in, nin * sizeof(float), hipMemcpyHostToDevice, s->stream.s));
    HIP_TRY(rtmi_env_launch_probe(op, dev_env(s, s->env_sampled ? 1.0f : 0.0f), din, dout, n, s->stream.s));
    HIP_TRY(hipMemcpyAsync(out, dout, nout * sizeof(float), hipMemcpyDeviceToHost, s->stream.s));
    HIP_TRY(hipStreamSynchronize(s->stream.s));
    return RTMI_OK;
}

// ---- the frame pipeline's seams (rtmi_frame_launch.hpp, include/rtmi_frame.h) ------------------------------------------
// The device halves of the two renders of a frame, under one hold on the scene.  rtmi_frame.hip runs the rest of the frame
// on s->stream.s before it ends the hold.
struct RtmiFrameHold {
    RenderCall c;
    rtmi_scene *s = nullptr;
};
static Estimator frame_estimator(const RtmiFrameLit &m, const std::string &null_scene) {
    return lit_estimator(m.name, m.nee, m.env, m.env ? m.env_select_p : 1.0f, null_scene.c_str());
}
int rtmi_frame_hold_begin(rtmi_scene *s, const RtmiFrameLit &m, RtmiFrameHold **hold) {
    *hold = nullptr;
    const std::string null_scene = std::string(m.name) + ": scene is NULL";
    RtmiFrameHold *h = new (std::nothrow) RtmiFrameHold;
    if (!h) return fail(RTMI_ERR_NOMEM, std::string(m.name) + ": out of host memory");
    if (int rc = begin_call(h->c, frame_estimator(m, null_scene), s)) {
        delete h;
        return rc;
    }
    h->s = s;
    *hold = h;
    return RTMI_OK;
}
void rtmi_frame_hold_end(RtmiFrameHold *hold) { delete hold; } // ~RenderCall: the busy mark, then the lock
int rtmi_frame_enqueue_lit(RtmiFrameHold *hold, const RtmiFrameLit &fm, const rtmi_camera *cam, const rtmi_render_params &p,
                           rtmi_stats *stats) {
    rtmi_scene *s = hold->s;
    const Estimator m = frame_estimator(fm, "");
    if (!fm.nee && !fm.env) {
        const rtmi_adaptive a{p.ns, 1u, 0.0, 0.0};
        PassCounts counts;
        if (int rc = adaptive_plain_device(hold->c, m, s, cam, p, &a, counts)) return rc;
        if (stats) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, s->ev[0].e, s->ev[2].e));
            fill_stats(s, &p, stats, ms, ms, counts); // every tile stops at ns: the samples are fill_stats'
        }
        return RTMI_OK;
    }
    return render_fixed_device(hold->c, m, s, cam, p, false, stats,
                               [&](const RenderCall &c, bool sig, uint32_t blocks) -> int { return launch_lit_fixed(c, m, s, sig, blocks); });
}
int rtmi_frame_enqueue_first_hits(RtmiFrameHold *hold, const rtmi_camera *cam, const rtmi_render_params &p) {
    return features_device(hold->s, cam, p, false, nullptr);
}
RtmiFramePlanes rtmi_frame_planes(const RtmiFrameHold *hold, const rtmi_render_params &p) {
    const rtmi_scene *s = hold->s;
    const size_t npix = (size_t)p.nx * p.ny;
    return RtmiFramePlanes{s->device, s->stream.s, s->texels.ptr, s->ad_stderr.ptr, s->ft_planes.ptr, s->ft_planes.ptr + npix * 3, s->ft_planes.ptr + npix * 6,
                           reinterpret_cast<const uint32_t *>(s->ft_planes.ptr + npix * 7)};
}
