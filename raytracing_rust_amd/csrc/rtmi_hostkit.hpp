// rtmi_hostkit.hpp — the host-side helpers the translation units share: the refusal composer, the device check, the
// "return on a HIP error" macro and the owners of one device allocation and of one stream.  Everything is static inline, so
// librtmi.so exports nothing from here.  What stays with each unit: whether out-of-memory answers RTMI_ERR_NOMEM, the order
// in which a handle is torn down, and the caller-visible scratch layouts.  See DESIGN.md §34.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

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

// One non-blocking stream, destroyed by the destructor.
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
