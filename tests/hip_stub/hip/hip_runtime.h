// A stand-in for <hip/hip_runtime.h> on the host: only the calls csrc/rtmi_hostkit.hpp names, backed by malloc/free, so that
// tests/test_hostkit_owners.py can run the owners under the address and undefined-behaviour sanitizers without a device.
// It counts the live allocations and the calls, and refuses one allocation on request.
#pragma once

#include <cstddef>
#include <cstdlib>

enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 };
typedef struct hipStubStream *hipStream_t;
typedef struct hipStubEvent *hipEvent_t;
enum { hipHostMallocDefault = 0, hipStreamNonBlocking = 1 };

inline int hip_stub_live_device = 0, hip_stub_live_pinned = 0, hip_stub_live_objects = 0; // allocations not yet freed
inline int hip_stub_calls = 0;                                                            // every memory call made
inline int hip_stub_refuse = 0; // the next allocation fails when this is 1 (counts down otherwise)

inline const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : "invalid value"; }
inline hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }

inline hipError_t hip_stub_alloc(void **p, size_t bytes, int *live) {
    hip_stub_calls++;
    *p = nullptr;
    if (hip_stub_refuse && --hip_stub_refuse == 0) return hipErrorOutOfMemory;
    if (!(*p = malloc(bytes ? bytes : 1))) return hipErrorOutOfMemory;
    ++*live;
    return hipSuccess;
}
inline hipError_t hip_stub_free(void *p, int *live) {
    hip_stub_calls++;
    if (p) { free(p); --*live; }
    return hipSuccess;
}
inline hipError_t hipMalloc(void **p, size_t bytes) { return hip_stub_alloc(p, bytes, &hip_stub_live_device); }
inline hipError_t hipFree(void *p) { return hip_stub_free(p, &hip_stub_live_device); }
inline hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return hip_stub_alloc(p, bytes, &hip_stub_live_pinned); }
inline hipError_t hipHostFree(void *p) { return hip_stub_free(p, &hip_stub_live_pinned); }
inline hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return hip_stub_alloc(reinterpret_cast<void **>(s), 1, &hip_stub_live_objects); }
inline hipError_t hipStreamDestroy(hipStream_t s) { return hip_stub_free(s, &hip_stub_live_objects); }
inline hipError_t hipEventCreate(hipEvent_t *e) { return hip_stub_alloc(reinterpret_cast<void **>(e), 1, &hip_stub_live_objects); }
inline hipError_t hipEventDestroy(hipEvent_t e) { return hip_stub_free(e, &hip_stub_live_objects); }
