// rtmi_multi.hip — several GPUs of this process behind one handle (rtmi_multi of include/rtmi.h; host code only,
// DESIGN.md §40): the lazily bound RCCL, the communicator sets and the multi-device entry points, on the plain render
// (render_device_locked and its helpers, rtmi_host.hpp).
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "rtmi_host.hpp"

// ---- several GPUs of this process behind one handle: scene replicated, tiles t % n, one gather on devices[0] -----
// RCCL is bound lazily (dlopen) so that single-GPU users of librtmi.so do not load it; inside a PyTorch process the
// soname resolves to the copy torch already mapped.
namespace {
struct RcclApi {
    void *lib = nullptr;
    int (*CommInitAll)(void **, int, const int *) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Gather)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr; // rccl.h ncclGather
    const char *(*GetErrorString)(int) = nullptr;
    std::string err;
    bool load() {
        if (lib) return true;
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (lib) break;
        }
        if (!lib) { err = std::string("dlopen(librccl.so.1): ") + (dlerror() ? dlerror() : "not found"); return false; }
        CommInitAll = reinterpret_cast<decltype(CommInitAll)>(dlsym(lib, "ncclCommInitAll"));
        CommDestroy = reinterpret_cast<decltype(CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
        GroupStart = reinterpret_cast<decltype(GroupStart)>(dlsym(lib, "ncclGroupStart"));
        GroupEnd = reinterpret_cast<decltype(GroupEnd)>(dlsym(lib, "ncclGroupEnd"));
        Gather = reinterpret_cast<decltype(Gather)>(dlsym(lib, "ncclGather"));
        GetErrorString = reinterpret_cast<decltype(GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
        if (!CommInitAll || !CommDestroy || !GroupStart || !GroupEnd || !Gather || !GetErrorString) {
            err = "librccl lacks one of ncclCommInitAll/ncclCommDestroy/ncclGroupStart/ncclGroupEnd/ncclGather/ncclGetErrorString";
            dlclose(lib); lib = nullptr;
            return false;
        }
        return true;
    }
};
RcclApi g_rccl;
std::mutex g_rccl_mutex;
// Communicator sets are expensive to make (ncclCommInitAll) and RCCL allows ONE thread at a time to enqueue on a
// communicator: a set belongs to exactly one rtmi_multi handle while that handle lives (checked out at create,
// handed back at destroy) and is kept for the next handle on the same device list afterwards, so that one-shot
// calls (rtmi_render_multi) do not pay the initialisation per image and two live handles on one device list never
// share communicators.  Sets live for the process lifetime.
struct CommSet {
    std::vector<void *> comms;
    bool busy = false;
};
std::map<std::vector<int>, std::vector<CommSet *>> g_comm_pool;
// RTMI_FORCE_RCCL=1 (environment, read at every rtmi_multi_create): also a ONE-entry device list gets a communicator,
// so that the whole collective path — dlopen, ncclCommInitAll, grouped ncclGather on the render stream — runs on a
// single GPU (tests, and bench.py's abi_multi leg at N = 1).  Without it a one-device handle needs no exchange.
bool force_rccl() {
    const char *e = getenv("RTMI_FORCE_RCCL");
    return e && *e && *e != '0';
}
} // namespace
#define RCCL_TRY(expr)                                                                                        \
    do {                                                                                                      \
        int r_ = (expr);                                                                                      \
        if (r_ != 0) return fail(RTMI_ERR_DEVICE, std::string(#expr) + ": " + g_rccl.GetErrorString(r_));     \
    } while (0)

// The persistent multi-device handle.  Everything a render needs between calls lives here; rtmi_multi_render only
// enqueues kernels and the one gather, waits, copies the gathered framebuffer out and un-tiles it.
struct RTMI_HIDDEN rtmi_multi {
    std::vector<int> devices;
    bool distinct = true;
    std::vector<rtmi_scene *> scenes;    // one per listed device (a device listed twice holds two scenes)
    std::vector<DeviceBuf<rtmi_texel>> texels; // per device: tile-packed local framebuffer (grow-only)
    DeviceBuf<rtmi_texel> gathered;      // on devices[0]: n x stride texels, rank-major
    PinnedBuf<rtmi_texel> h_gathered;    // its pinned host mirror
    CommSet *commset = nullptr;          // RCCL communicators (distinct devices; n > 1 or RTMI_FORCE_RCCL), checked out at create
    std::mutex mu;                       // render calls on one handle serialise (rtmi.h, thread model)
};

extern "C" void rtmi_multi_destroy(rtmi_multi *m) {
    if (!m) return;
    for (size_t i = 0; i < m->texels.size(); i++) // each device's buffer is released with that device selected
        if (m->texels[i].ptr) { (void)hipSetDevice(m->devices[i]); (void)m->texels[i].release(); }
    if (m->gathered.ptr) { (void)hipSetDevice(m->devices[0]); (void)m->gathered.release(); }
    for (rtmi_scene *s : m->scenes) rtmi_scene_destroy(s);
    if (m->commset) { // back to the pool: the next handle on this device list takes it over
        std::lock_guard<std::mutex> lock(g_rccl_mutex);
        m->commset->busy = false;
    }
    delete m;
}

extern "C" int rtmi_multi_create(const rtmi_scene_desc *desc, const int *devices, uint32_t n, rtmi_multi **out) {
    if (!out) return fail(RTMI_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!desc || !devices || n == 0) return fail(RTMI_ERR_INVALID, "NULL argument or empty device list");
    int rc = validate(desc);
    if (rc) return rc;
    const int ndev = rtmi_device_count();
    if (ndev <= 0) return fail(RTMI_ERR_DEVICE, "no HIP device available (the rtmi path has no CPU fallback)");
    rtmi_multi *m = new (std::nothrow) rtmi_multi();
    if (!m) return fail(RTMI_ERR_NOMEM, "out of host memory");
    struct Guard { rtmi_multi *m; ~Guard() { if (m) rtmi_multi_destroy(m); } } guard{m};
    for (uint32_t i = 0; i < n; i++) {
        if (devices[i] < 0 || devices[i] >= ndev) return fail(RTMI_ERR_INVALID, "device index out of range");
        for (uint32_t k = 0; k < i; k++) m->distinct = m->distinct && devices[k] != devices[i];
    }
    m->devices.assign(devices, devices + n);
    m->scenes.assign(n, nullptr);
    m->texels = std::vector<DeviceBuf<rtmi_texel>>(n);
    // uploads to all devices at once: one host thread per device (hipMalloc / hipMemcpy of one device do not wait for
    // another's; the derived records — leaf, shading, pool-encoded nodes — are built per thread as well)
    std::vector<int> rcs(n, RTMI_OK);
    std::vector<std::string> errs(n);
    {
        std::vector<std::thread> th;
        for (uint32_t i = 0; i < n; i++)
            th.emplace_back([&, i]() {
                rcs[i] = rtmi_scene_create(desc, devices[i], &m->scenes[i]);
                if (rcs[i] == RTMI_OK) {
                    (void)hipSetDevice(devices[i]);
                    rcs[i] = ensure_streams(m->scenes[i]);
                }
                if (rcs[i] != RTMI_OK) errs[i] = rtmi_last_error(); // the message is thread-local
            });
        for (std::thread &t : th) t.join();
    }
    for (uint32_t i = 0; i < n; i++)
        if (rcs[i] != RTMI_OK) return fail(rcs[i], "device " + std::to_string(devices[i]) + ": " + errs[i]);
    if (m->distinct && (n > 1 || force_rccl())) { // communicators at create, not in the first render
        std::lock_guard<std::mutex> lock(g_rccl_mutex);
        if (!g_rccl.load()) return fail(RTMI_ERR_DEVICE, g_rccl.err);
        std::vector<CommSet *> &pool = g_comm_pool[m->devices];
        for (CommSet *c : pool)
            if (!c->busy) { m->commset = c; break; }
        if (!m->commset) {
            CommSet *c = new CommSet();
            c->comms.assign(n, nullptr);
            int r = g_rccl.CommInitAll(c->comms.data(), (int)n, devices);
            if (r != 0) { delete c; return fail(RTMI_ERR_DEVICE, std::string("ncclCommInitAll: ") + g_rccl.GetErrorString(r)); }
            pool.push_back(c);
            m->commset = c;
        }
        m->commset->busy = true;
    }
    guard.m = nullptr;
    *out = m;
    return RTMI_OK;
}

extern "C" int rtmi_multi_collective(const rtmi_multi *m) {
    if (!m) return -1;
    return m->commset ? RTMI_COLLECTIVE_RCCL : (m->devices.size() > 1 ? RTMI_COLLECTIVE_PEER_COPY : RTMI_COLLECTIVE_NONE);
}

// whole-image parameters -> per-device parameters; validates what the multi-device entry points accept
static int multi_params(const rtmi_multi *m, const rtmi_render_params *p_in, std::vector<rtmi_render_params> &params) {
    int rc = check_params(p_in);
    if (rc) return rc;
    if (p_in->tile_world != 1 || p_in->tile_rank != 0)
        return fail(RTMI_ERR_INVALID, "multi-device render calls render the whole image: tile_rank/tile_world must be 0/1");
    if (p_in->flags & (RTMI_FLAG_PATH_SIG | RTMI_FLAG_PROFILE)) return fail(RTMI_ERR_INVALID, "PATH_SIG / PROFILE are single-device diagnostics");
    const uint32_t n = (uint32_t)m->devices.size();
    params.assign(n, *p_in);
    for (uint32_t i = 0; i < n; i++) { params[i].tile_world = n; params[i].tile_rank = i; }
    return RTMI_OK;
}
// framebuffers of a render of this size (grow-only); every rank padded to rank 0's size (the largest)
static int multi_reserve_texels(rtmi_multi *m, const rtmi_render_params *p0) {
    const uint32_t n = (uint32_t)m->devices.size();
    const size_t want = (size_t)local_tiles_of(p0, 0) * 64 * sizeof(rtmi_texel);
    // what every buffer holds: the smallest one decides (a buffer whose allocation failed is empty)
    size_t have = m->gathered.bytes / n;
    for (uint32_t i = 0; i < n; i++) have = std::min(have, m->texels[i].bytes);
    if (want > have) {
        for (uint32_t i = 0; i < n; i++) {
            HIP_TRY(hipSetDevice(m->devices[i]));
            HIP_TRY(m->texels[i].alloc(want));
            // ranks with fewer tiles than rank 0 never write their padding: zero it once
            HIP_TRY(hipMemset(m->texels[i].ptr, 0, want));
        }
        HIP_TRY(hipSetDevice(m->devices[0]));
        HIP_TRY(m->gathered.alloc((size_t)n * want));
    }
    return grow_host_texels(m->h_gathered, m->gathered.bytes / sizeof(rtmi_texel));
}

extern "C" int rtmi_multi_prepare(rtmi_multi *m, const rtmi_render_params *p_in) {
    if (!m) return fail(RTMI_ERR_INVALID, "NULL argument");
    std::vector<rtmi_render_params> params;
    int rc = multi_params(m, p_in, params);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(m->mu);
    if ((rc = multi_reserve_texels(m, &params[0]))) return rc;
    for (size_t i = 0; i < m->scenes.size(); i++)
        if ((rc = rtmi_render_prepare(m->scenes[i], &params[i]))) return rc;
    return RTMI_OK;
}

extern "C" int rtmi_multi_render(rtmi_multi *m, const rtmi_camera *cam, const rtmi_render_params *p_in, float *out_linear,
                                 uint8_t *out_rgb8, rtmi_stats *stats) {
    if (!m || !cam) return fail(RTMI_ERR_INVALID, "NULL argument");
    std::vector<rtmi_render_params> params;
    int rc = multi_params(m, p_in, params);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(m->mu);
    const uint32_t n = (uint32_t)m->devices.size();
    if ((rc = multi_reserve_texels(m, &params[0]))) return rc;
    // rank-major layout of the gathered buffer uses THIS call's stride (the buffers may be larger from an earlier call)
    const size_t stride = (size_t)local_tiles_of(&params[0], 0) * 64;
    std::vector<hipEvent_t> done(n);
    // every device renders its tiles on its own stream, all concurrently
    for (uint32_t i = 0; i < n; i++) {
        rtmi_scene *s = m->scenes[i];
        std::lock_guard<std::mutex> slock(s->mu);
        HIP_TRY(hipSetDevice(m->devices[i]));
        if ((rc = reserve_before_clock(s, &params[i]))) return rc;
        HIP_TRY(hipEventRecord(s->ev[0].e, s->stream.s));
        if ((rc = render_device_locked(s, cam, &params[i], m->texels[i].ptr, s->stream.s, nullptr))) return rc;
        HIP_TRY(hipEventRecord(s->ev[1].e, s->stream.s));
        done[i] = s->ev[2].e;
    }
    // the ONE exchange of the path: tile-packed framebuffers -> devices[0]
    if (m->commset) {
        RCCL_TRY(g_rccl.GroupStart());
        for (uint32_t i = 0; i < n; i++) {
            HIP_TRY(hipSetDevice(m->devices[i]));
            // (recvbuff is read on the root only; the others pass a valid device pointer rather than NULL for argument checkers)
            RCCL_TRY(g_rccl.Gather(m->texels[i].ptr, i == 0 ? m->gathered.ptr : m->texels[i].ptr, stride * sizeof(rtmi_texel), /*ncclInt8*/ 0, 0, m->commset->comms[i], m->scenes[i]->stream.s));
        }
        RCCL_TRY(g_rccl.GroupEnd());
    } else {
        for (uint32_t i = 0; i < n; i++) {
            HIP_TRY(hipSetDevice(m->devices[i]));
            HIP_TRY(hipMemcpyPeerAsync(m->gathered.ptr + (size_t)i * stride, m->devices[0], m->texels[i].ptr, m->devices[i], stride * sizeof(rtmi_texel), m->scenes[i]->stream.s));
        }
    }
    for (uint32_t i = 0; i < n; i++) {
        HIP_TRY(hipSetDevice(m->devices[i]));
        HIP_TRY(hipEventRecord(m->scenes[i]->ev[2].e, m->scenes[i]->stream.s));
    }
    if ((rc = wait_with_progress(m->scenes.data(), done.data(), n, p_in))) return rc;
    if (stats) memset(stats, 0, sizeof(*stats));
    for (uint32_t i = 0; i < n; i++) {
        HIP_TRY(hipSetDevice(m->devices[i]));
        if ((rc = check_overflow(m->scenes[i]))) return rc;
        if (stats) {
            rtmi_stats one{};
            if ((rc = fill_stats_from_events(m->scenes[i], &params[i], &one))) return rc;
            stats->samples += one.samples; stats->tiles += one.tiles; stats->kernel = one.kernel;
            if (one.render_ms > stats->render_ms) stats->render_ms = one.render_ms;
            if (one.kernel_ms > stats->kernel_ms) stats->kernel_ms = one.kernel_ms;
        }
    }
    HIP_TRY(hipSetDevice(m->devices[0]));
    HIP_TRY(hipMemcpy(m->h_gathered.ptr, m->gathered.ptr, (size_t)n * stride * sizeof(rtmi_texel), hipMemcpyDeviceToHost));
    return rtmi_untile(&params[0], m->h_gathered.ptr, out_linear, out_rgb8);
}

// one-shot form: create + render + destroy (pays uploads, allocations and the communicator look-up on every call)
extern "C" int rtmi_render_multi(const rtmi_scene_desc *desc, const int *devices, uint32_t n, const rtmi_camera *cam,
                                 const rtmi_render_params *p_in, float *out_linear, uint8_t *out_rgb8, rtmi_stats *stats) {
    if (!desc || !devices || !cam || n == 0) return fail(RTMI_ERR_INVALID, "NULL argument or empty device list");
    int rc = check_params(p_in);
    if (rc) return rc;
    if (p_in->tile_world != 1 || p_in->tile_rank != 0)
        return fail(RTMI_ERR_INVALID, "rtmi_render_multi renders the whole image: tile_rank/tile_world must be 0/1");
    if (p_in->flags & (RTMI_FLAG_PATH_SIG | RTMI_FLAG_PROFILE)) return fail(RTMI_ERR_INVALID, "PATH_SIG / PROFILE are single-device diagnostics");
    rtmi_multi *m = nullptr;
    if ((rc = rtmi_multi_create(desc, devices, n, &m))) return rc;
    rc = rtmi_multi_render(m, cam, p_in, out_linear, out_rgb8, stats);
    const std::string keep = rtmi_last_error(); // destroy must not lose the message
    rtmi_multi_destroy(m);
    if (rc) (void)fail(rc, keep);
    return rc;
}
