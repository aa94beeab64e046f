"""The owners of csrc/rtmi_hostkit.hpp (DeviceBuf, PinnedBuf, DeviceList, DeviceArena, DeviceStream, DeviceEvent), on the host.

The three handles (rtmi_scene in rtmi_host.hpp, rtmi_multi in rtmi_multi.hip, rtmi_session in rtmi_session.hip) keep all their device and pinned memory in these owners and free nothing by hand, so a
mistake here is a leak or a double free in every entry point, and no image test sees either.  This compiles the header
alone against tests/hip_stub (the HIP calls it names, backed by malloc/free, with counters), under the address, leak and
undefined-behaviour sanitizers, and runs it as a child process; nothing is loaded into Python.  DESIGN.md §36."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing_rust_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
STUB = os.path.join(ROOT, "tests", "hip_stub")

PROG = r"""
#include "rtmi_hostkit.hpp"
#include <cstdio>
#include <cstring>
int rtmi_fail(int code, const char *) { return code; }
#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)

template <bool Pinned> static int buffer(const char *only) {
    int &live = Pinned ? hip_stub_live_pinned : hip_stub_live_device;
    const auto is = [&](const char *name) { return !strcmp(only, "all") || !strcmp(only, name); };
    if (is("grow")) { // a smaller or equal size: same pointer, no call; a larger one: one free, one allocation, the new size
        DeviceBuf<double, Pinned> b;
        int calls = hip_stub_calls;
        CHECK(b.ptr == nullptr && b.bytes == 0 && b.grow(0) == hipSuccess && hip_stub_calls == calls);
        CHECK(b.grow(64) == hipSuccess && b.ptr && b.bytes == 64 && live == 1 && hip_stub_calls == calls + 1);
        b.ptr[7] = 1.0; // (the sanitizer checks the extent)
        double *const first = b.ptr;
        calls = hip_stub_calls;
        CHECK(b.grow(64) == hipSuccess && b.grow(8) == hipSuccess && b.grow(0) == hipSuccess);
        CHECK(b.ptr == first && b.bytes == 64 && hip_stub_calls == calls);
        CHECK(b.grow(4096) == hipSuccess && b.bytes == 4096 && live == 1 && hip_stub_calls == calls + 2);
        b.ptr[511] = 1.0;
    }
    CHECK(live == 0);
    if (is("refuse")) { // a refused allocation: empty, size 0, the old block freed once; a later grow works
        DeviceBuf<char, Pinned> b;
        CHECK(b.grow(16) == hipSuccess && live == 1);
        hip_stub_refuse = 1;
        CHECK(b.grow(32) == hipErrorOutOfMemory && b.ptr == nullptr && b.bytes == 0 && live == 0);
        CHECK(b.grow(8) == hipSuccess && b.ptr && b.bytes == 8 && live == 1);
        b.ptr[7] = 1;
    }
    CHECK(live == 0);
    if (is("release")) { // release(), then the destructor: freed once
        DeviceBuf<int, Pinned> b;
        CHECK(b.alloc(40) == hipSuccess && live == 1);
        const int calls = hip_stub_calls;
        CHECK(b.release() == hipSuccess && b.ptr == nullptr && b.bytes == 0 && live == 0 && hip_stub_calls == calls + 1);
        CHECK(b.release() == hipSuccess && hip_stub_calls == calls + 1);
    }
    CHECK(live == 0);
    if (is("give")) { // handed away: nothing left to free; another owner adopts it and frees it
        size_t had = 0;
        int *p;
        DeviceBuf<int, Pinned> other;
        int calls;
        {
            DeviceBuf<int, Pinned> b;
            CHECK(b.alloc(40) == hipSuccess);
            calls = hip_stub_calls;
            p = b.give(&had);
            CHECK(p && had == 40 && b.ptr == nullptr && b.bytes == 0);
        }
        CHECK(live == 1 && hip_stub_calls == calls);
        other.adopt(p, had);
        CHECK(other.ptr == p && other.bytes == 40 && other.grow(40) == hipSuccess && hip_stub_calls == calls);
    }
    CHECK(live == 0);
    return 0;
}

static int others(const char *only) {
    const auto is = [&](const char *name) { return !strcmp(only, "all") || !strcmp(only, name); };
    if (is("list")) { // every element freed, by release() and by the destructor; a refused one is not listed
        DeviceList l;
        void *p[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int i = 0; i < 3; i++) CHECK(l.add(&p[i], 8 + i) == hipSuccess && p[i]);
        hip_stub_refuse = 1;
        CHECK(l.add(&p[3], 8) == hipErrorOutOfMemory && l.all.size() == 3 && hip_stub_live_device == 3);
        CHECK(l.release() == hipSuccess && l.all.empty() && hip_stub_live_device == 0);
        CHECK(l.add(&p[0], 8) == hipSuccess && l.add(&p[1], 8) == hipSuccess && hip_stub_live_device == 2);
    }
    CHECK(hip_stub_live_device == 0);
    if (is("arena")) {
        DeviceArena a;
        char *x = nullptr, *y = nullptr;
        CHECK(a.alloc([&](Carve256 &c) { x = c.take<char>(3); y = c.take<char>(5); }) == hipSuccess);
        CHECK(x == a.base && y == x + 256 && a.bytes == 512 && hip_stub_live_device == 1);
        y[255] = 1;
    }
    CHECK(hip_stub_live_device == 0);
    if (is("objects")) {
        DeviceStream s;
        DeviceEvent e, never_created;
        CHECK(s.create() == hipSuccess && hipEventCreate(&e.e) == hipSuccess && hip_stub_live_objects == 2);
    }
    CHECK(hip_stub_live_objects == 0);
    return 0;
}

int main(int argc, char **argv) {
    const char *only = argc > 1 ? argv[1] : "all";
    if (!strcmp(only, "leak")) { // the harness itself: a block the stub handed out and nobody freed must fail the run
        DeviceBuf<char> b;
        if (b.alloc(24) != hipSuccess) return 1;
        (void)b.give();
        printf("live %d\n", hip_stub_live_device);
        fflush(stdout); // (the leak report ends the process before the buffers of stdio are written)
        return 0;
    }
    if (int rc = buffer<false>(only)) return rc;
    if (int rc = buffer<true>(only)) return 10 + rc;
    if (int rc = others(only)) return 20 + rc;
    CHECK(hip_stub_live_device == 0 && hip_stub_live_pinned == 0 && hip_stub_live_objects == 0);
    printf("ok\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def owners(tmp_path_factory):
    d = tmp_path_factory.mktemp("owners")
    src, exe = d / "owners.cpp", d / "owners"
    src.write_text(PROG)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + STUB, "-I" + CSRC, "-I" + INCLUDE, str(src), "-o", str(exe)], check=True)

    def run(what):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
        return subprocess.run([str(exe), what], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    return run


@pytest.mark.parametrize("what", ["grow", "refuse", "release", "give", "list", "arena", "objects", "all"])
def test_owners_free_exactly_once_and_leave_nothing(owners, what):
    """device and pinned owner alike: the stub's live counts are 0 at exit and the sanitizers are silent"""
    r = owners(what)
    assert (r.returncode, r.stdout.decode()) == (0, "ok\n") and b"Sanitizer" not in r.stderr, r.stderr.decode()


def test_a_leak_would_be_seen(owners):
    """the same build does fail on an allocation that is handed away and never freed"""
    r = owners("leak")
    assert r.stdout.decode() == "live 1\n"
    assert r.returncode != 0 and b"LeakSanitizer" in r.stderr
