"""The carve of one allocation into aligned pieces (csrc/rtmi_carve.hpp), on the host.

Every unit that keeps several planes in one device allocation lists them once, as a sequence of takes; the sequence is run
against no base to learn the size to allocate and again against the allocation.  A total that fell short of the last piece
would be a device buffer overrun that no image test sees, so this compiles the header alone, under the address and
undefined-behaviour sanitizers, and checks the arithmetic: alignment, no overlap, total = end of the last piece, the two
runs agree.  It also replays the take sequences of the frame handle, the temporal handle and rtmi_denoise's staging and
compares their totals with the sums those units used to write out by hand."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing_rust_amd", "csrc")
BASE = 0x7F0000000000  # a multiple of 256 that stands for the allocation; nothing is read or written through it

# arguments: cases separated by "/", each "align count size count size ...": take<T>(count) with sizeof(T) == size
# one line per case: "measured_offset:carved_offset ..." for the pieces, then "| measured_total carved_total"
PROG = r"""
#include "rtmi_carve.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
template <size_t N> struct El { char b[N]; };
template <size_t A> static uintptr_t take(Carve<A> &c, size_t count, size_t size) {
    switch (size) {
    case 1: return reinterpret_cast<uintptr_t>(c.template take<El<1>>(count));
    case 4: return reinterpret_cast<uintptr_t>(c.template take<El<4>>(count));
    case 8: return reinterpret_cast<uintptr_t>(c.template take<El<8>>(count));
    case 16: return reinterpret_cast<uintptr_t>(c.template take<El<16>>(count));
    }
    abort();
}
template <size_t A> static void run(char **arg, int n) {
    const uintptr_t base = %dull;
    Carve<A> measure, carve(reinterpret_cast<void *>(base));
    for (int i = 0; i + 1 < n; i += 2) {
        const size_t count = strtoull(arg[i], 0, 10), size = strtoull(arg[i + 1], 0, 10);
        const uintptr_t m = take(measure, count, size), r = take(carve, count, size);
        printf("%%llu:%%llu ", (unsigned long long)m, (unsigned long long)(r - base));
    }
    printf("| %%llu %%llu\n", (unsigned long long)measure.total(), (unsigned long long)carve.total());
}
int main(int argc, char **argv) {
    for (int i = 1; i < argc;) {
        int end = i;
        while (end < argc && strcmp(argv[end], "/")) end++;
        const int align = atoi(argv[i]);
        if (align == 16) run<16>(argv + i + 1, end - i - 1);
        else if (align == 256) run<256>(argv + i + 1, end - i - 1);
        else abort();
        i = end + 1;
    }
    return 0;
}
""" % BASE


@pytest.fixture(scope="module")
def carve(tmp_path_factory):
    d = tmp_path_factory.mktemp("carve")
    src, exe = d / "carve.cpp", d / "carve"
    src.write_text(PROG)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, str(src), "-o", str(exe)], check=True)

    def run(cases):
        """cases: (align, [(count, size), ...]) -> per case ([measured offsets], [carved offsets], measured total, carved total)"""
        args = []
        for align, takes in cases:
            args += [str(align)] + [str(v) for t in takes for v in t] + ["/"]
        out = subprocess.run([str(exe)] + args, check=True, stdout=subprocess.PIPE).stdout.decode().split("\n")
        res = []
        for ln in [ln for ln in out if ln]:
            pieces, totals = ln.split("|")
            pairs = [p.split(":") for p in pieces.split()]
            tm, tr = totals.split()
            res.append(([int(m) for m, _ in pairs], [int(r) for _, r in pairs], int(tm), int(tr)))
        assert len(res) == len(cases)
        return res
    return run


def up(b, a=256):
    return (b + a - 1) // a * a


SIZES = [0, 1, 255, 256, 257, 3 * 5 * 3, 12 * (2**31 - 1)]


@pytest.mark.parametrize("align", [16, 256])
def test_pieces_are_aligned_disjoint_and_total_is_the_end_of_the_last(carve, align):
    assert BASE % 256 == 0
    orders = [SIZES, SIZES[::-1], [s for s in SIZES for _ in range(2)]] + [[s] for s in SIZES]
    res = carve([(align, [(s, 1) for s in order]) for order in orders])
    for order, (measured, carved, total_m, total_c) in zip(orders, res):
        assert measured == carved and total_m == total_c  # measuring and carving the same layout agree
        end = 0
        for off, size in zip(carved, order):
            assert off % align == 0 and (BASE + off) % align == 0
            assert off >= end  # starts after the previous piece's last byte
            end = off + size
        assert total_c == carved[-1] + up(order[-1], align) >= end
        assert total_c % align == 0


def test_typed_takes_count_elements(carve):
    # take<T>(count) is count * sizeof(T) bytes, also past 2^32
    (m, c, tm, tc), = carve([(256, [(5, 4), (3, 16), (2**31 - 1, 8), (1, 1)])])
    assert m == c == [0, 256, 512, 512 + up(8 * (2**31 - 1))] and tm == tc == c[-1] + 256


@pytest.mark.parametrize("align", [16, 256])
def test_empty_layout_has_total_zero(carve, align):
    assert carve([(align, [])]) == [([], [], 0, 0)]


# ---- the units' layouts: the takes as the units make them, the totals as their parent wrote them by hand -------------------
IMAGES = [(1, 1), (5, 3), (1920, 1080)]


def denoise_work_takes(n, iterations):  # rtmi_denoise_layout
    return [(n, 16), (n, 16), (n, 16), (n, 8)] if iterations else []


def denoise_work_bytes(n, iterations):  # the parent's rtmi_denoise_scratch_bytes
    return 3 * up(n * 16) + up(n * 8) if iterations else 0


def history_takes(n):  # rtmi_temporal_history_layout
    return [(n, 16)] * 6


@pytest.mark.parametrize("temporal", [True, False])
@pytest.mark.parametrize("iterations", [0, 5])
def test_frame_alloc_total(carve, temporal, iterations):
    cases, want = [], []
    for nx, ny in IMAGES:
        n = nx * ny
        takes = (history_takes(n) if temporal else []) + [(n * 3, 4), (n * 3, 4)]
        if temporal:
            takes += [(n * 3, 4), (n * 3, 4), (n, 4), (n, 8)]
        takes += denoise_work_takes(n, iterations) + [(n * 3, 4), (n * 3, 1), (1, 4)]
        cases.append((256, takes))
        f3, f2, f1, b3 = up(n * 12), up(n * 8), up(n * 4), up(n * 3)
        hist = 6 * up(n * 16) if temporal else 0
        work = up(denoise_work_bytes(n, iterations))
        want.append(hist + 2 * f3 + (2 * f3 + f1 + f2 if temporal else 0) + work + f3 + b3 + 256)
    assert [r[3] for r in carve(cases)] == want


def test_temporal_alloc_total(carve):
    cases, want = [], []
    for nx, ny in IMAGES:
        n = nx * ny
        cases.append((256, history_takes(n) + [(n * 3, 4)] * 6 + [(n, 4), (n, 4), (n, 8)]))
        f4, f3, f2, f1 = up(n * 16), up(n * 12), up(n * 8), up(n * 4)
        want.append(6 * f4 + 6 * f3 + 2 * f1 + f2)
    res = carve(cases)
    assert [r[3] for r in res] == want
    for (nx, ny), (_m, offs, _tm, _tc) in zip(IMAGES, res):  # the history's planes where the parent's carve put them
        assert offs[:6] == [k * up(nx * ny * 16) for k in range(6)]


@pytest.mark.parametrize("lum", [True, False])
@pytest.mark.parametrize("iterations", [0, 5])
def test_denoise_staging_total(carve, lum, iterations):
    cases, want = [], []
    for nx, ny in IMAGES:
        n = nx * ny
        takes = [(n * 3, 4)] * 3 + [(n, 4)] + ([(n * 3, 4)] if lum else [])
        takes += denoise_work_takes(n, iterations) + [(n * 3, 4), (n * 3, 1)]
        cases.append((256, takes))
        f3, f1, b3 = up(n * 12), up(n * 4), up(n * 3)
        want.append(3 * f3 + f1 + (f3 if lum else 0) + denoise_work_bytes(n, iterations) + f3 + b3)
    assert [r[3] for r in carve(cases)] == want
