// rtmi_hostkit.hpp — the host-side helpers the translation units share: the refusal composer, the device check, the
// "return on a HIP error" macro and the owners of device memory, pinned memory, a stream and an event.  Everything is static
// inline, so librtmi.so exports nothing from here.  What stays with each unit: whether out-of-memory answers RTMI_ERR_NOMEM,
// the order in which a handle is torn down, and the caller-visible scratch layouts.  See DESIGN.md §34 and §36.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "rtmi.h"
#include "rtmi_carve.hpp"

// not exported: the handles that hold an arena are marked with it too, so that their implicit destructors stay inside
#define RTMI_HIDDEN __attribute__((visibility("hidden")))

// rtmi_device.hip: sets the message of rtmi_last_error, returns `code`
RTMI_HIDDEN int rtmi_fail(int code, const char *msg);

static inline int fail(int code, const std::string &name, const char *msg) { return rtmi_fail(code, (name + ": " + msg).c_str()); }

static inline bool finite_f(float v) { return v == v && v - v == 0.0f; }

static inline bool misaligned(const void *p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1u)) != 0u; }

// "is this device index usable": `prefix` is the complete start of the message ("", "rtmi_temporal_create: ")
static inline int device_ok(const std::string &prefix, int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return rtmi_fail(RTMI_ERR_DEVICE, (prefix + "no HIP device available").c_str());
    if (device < 0 || device >= n) return rtmi_fail(RTMI_ERR_DEVICE, (prefix + "device index out of range").c_str());
    return RTMI_OK;
}

// Return from the enclosing entry when `expr` is a HIP error.  prefix: the complete start of the message; oom_is_nomem:
// whether hipErrorOutOfMemory answers RTMI_ERR_NOMEM (the entry's header says which); text: the expression as the entry
// wrote it.  Each unit fixes its policy in a one-line alias that passes #expr, so the text is not macro-expanded first.
#define RTMI_HIP_TRY(prefix, oom_is_nomem, expr, text)                                                                 \
    do {                                                                                                               \
        const hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess)                                                                                          \
            return rtmi_fail((oom_is_nomem) && e_ == hipErrorOutOfMemory ? RTMI_ERR_NOMEM : RTMI_ERR_DEVICE,           \
                             (std::string(prefix) + text ": " + hipGetErrorString(e_)).c_str());                      \
    } while (0)

// One device allocation, freed by the destructor (or by release(), where a handle's destroy function fixes the moment).
struct RTMI_HIDDEN DeviceArena {
    char *base = nullptr;
    size_t bytes = 0;
    DeviceArena() = default;
    DeviceArena(const DeviceArena &) = delete;
    DeviceArena &operator=(const DeviceArena &) = delete;
    ~DeviceArena() { release(); }
    void release() {
        if (base) (void)hipFree(base);
        base = nullptr;
        bytes = 0;
    }
    // measures `layout` (a function of a Carve<Align> &) against no base, allocates its total on the current device and runs
    // it again against the allocation; the pointers `layout` stored are valid after hipSuccess only
    template <size_t Align = 256, typename Layout>
    hipError_t alloc(Layout &&layout) {
        Carve<Align> measure;
        layout(measure);
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&base), measure.total());
        if (e != hipSuccess) return e;
        bytes = measure.total();
        Carve<Align> pieces(base);
        layout(pieces);
        return hipSuccess;
    }
};

// One typed grow-only buffer that knows its size: device memory (hipMalloc), or with Pinned host memory (hipHostMalloc).
// Freed by the destructor, or by release() where a handle fixes the moment; empty (ptr NULL, bytes 0) after a failure.
template <typename T, bool Pinned = false>
struct RTMI_HIDDEN DeviceBuf {
    T *ptr = nullptr;
    size_t bytes = 0;
    DeviceBuf() = default;
    DeviceBuf(const DeviceBuf &) = delete;
    DeviceBuf &operator=(const DeviceBuf &) = delete;
    ~DeviceBuf() { (void)release(); }
    hipError_t release() {
        T *const old = give();
        return !old ? hipSuccess : Pinned ? hipHostFree(old) : hipFree(old);
    }
    // frees what it holds and allocates `want` bytes on the current device
    hipError_t alloc(size_t want) {
        hipError_t e = release();
        void *p = nullptr;
        if (e == hipSuccess) e = Pinned ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want);
        if (e == hipSuccess) adopt(p, want);
        return e;
    }
    // grow-only: no call when `want` bytes are there already
    hipError_t grow(size_t want) { return want <= bytes ? hipSuccess : alloc(want); }
    // hands the allocation to the caller, who frees it or gives it to another owner (adopt); nothing is held afterwards
    T *give(size_t *had = nullptr) {
        T *const p = ptr;
        if (had) *had = bytes;
        ptr = nullptr;
        bytes = 0;
        return p;
    }
    // takes over an allocation of `n` bytes; the buffer must be empty
    void adopt(void *p, size_t n) { ptr = static_cast<T *>(p), bytes = n; }
};
template <typename T>
using PinnedBuf = DeviceBuf<T, true>;

// Device allocations made one by one and freed together (a scene's arrays: one allocation per array).
struct RTMI_HIDDEN DeviceList {
    std::vector<void *> all;
    DeviceList() = default;
    DeviceList(const DeviceList &) = delete;
    DeviceList &operator=(const DeviceList &) = delete;
    ~DeviceList() { (void)release(); }
    hipError_t add(void **out, size_t bytes) {
        all.reserve(all.size() + 1); // (so that the allocation cannot be lost to a failing push_back)
        const hipError_t e = hipMalloc(out, bytes);
        if (e == hipSuccess) all.push_back(*out);
        return e;
    }
    hipError_t release() {
        for (void *p : all) (void)hipFree(p);
        all.clear();
        return hipSuccess;
    }
};

// One stream, destroyed by the destructor; create() makes a non-blocking one.
struct RTMI_HIDDEN DeviceStream {
    hipStream_t s = nullptr;
    DeviceStream() = default;
    DeviceStream(const DeviceStream &) = delete;
    DeviceStream &operator=(const DeviceStream &) = delete;
    ~DeviceStream() {
        if (s) (void)hipStreamDestroy(s);
    }
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
};

// One event, destroyed by the destructor (the handle creates it: timing or not is its choice).
struct RTMI_HIDDEN DeviceEvent {
    hipEvent_t e = nullptr;
    DeviceEvent() = default;
    DeviceEvent(const DeviceEvent &) = delete;
    DeviceEvent &operator=(const DeviceEvent &) = delete;
    ~DeviceEvent() {
        if (e) (void)hipEventDestroy(e);
    }
};
