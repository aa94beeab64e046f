// rtmi_carve.hpp — one allocation carved into aligned pieces.  Pure C++17, no HIP: tests/test_carve_layout.py compiles it
// with g++ under the sanitizers.  See DESIGN.md §34.
//
// A layout is a function of a Carve: it takes its pieces in order and keeps the pointers.  It is run twice, once against no
// base to learn the total and once against the allocation (DeviceArena::alloc of rtmi_hostkit.hpp does both), so the size
// that is allocated is by construction the end of the last piece handed out: there is no second, hand-written sum.
#pragma once

#include <cstddef>
#include <cstdint>

template <size_t Align>
class Carve {
    static_assert(Align != 0 && (Align & (Align - 1)) == 0, "the alignment is a power of two");
    uintptr_t base_; // an integer, so that measuring against no base does no arithmetic on a null pointer
    size_t used_ = 0;

public:
    explicit Carve(void *base = nullptr) : base_(reinterpret_cast<uintptr_t>(base)) {}
    static constexpr size_t round(size_t bytes) { return (bytes + (Align - 1)) & ~(Align - 1); }
    // the next piece: `count` elements of T, starting at a multiple of Align from the base; an empty piece takes no room
    template <typename T>
    T *take(size_t count) {
        T *r = reinterpret_cast<T *>(base_ + used_);
        used_ += round(count * sizeof(T));
        return r;
    }
    size_t total() const { return used_; } // the end of the last piece
};

using Carve256 = Carve<256>; // the image units: every plane starts on a 256-byte boundary
using Carve16 = Carve<16>;   // the probes of rtmi_device.hip and rtmi_batch.hip
