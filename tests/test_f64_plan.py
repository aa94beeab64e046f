"""The pass plan of the f64 render mode (csrc/rtmi_f64_plan.hpp), on the host.

The f64 kernel takes its (sample, pixel) items from the work queue of the fp32 kernels, which computes per-sample slot
indices in 32 bits: a pass must hold fewer than 2^32 slots, or the kernel's writes wrap to low slots that the resolve
then reads twice while the high ones stay unwritten.  The buffer is also capped at 45 GiB like the fp32 one.  This compiles
the planner rtmi_render_f64 calls and checks, over a grid of image sizes, sample counts, budgets and free memory, that
every plan respects both limits and covers the sample range in whole chunks."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing_rust_amd", "csrc")
MAX_SLOTS = 2**32 - 1
MAX_BYTES = 45 << 30

PROG = r"""
#include "rtmi_f64_plan.hpp"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv) {
    for (int i = 1; i + 5 < argc + 1; i += 6) {
        uint32_t c = 0, p = 0;
        const bool ok = rtmi_f64_plan(strtoull(argv[i], 0, 10), (uint32_t)strtoul(argv[i + 1], 0, 10), strtoull(argv[i + 2], 0, 10),
                                      strtoull(argv[i + 3], 0, 10), strtoull(argv[i + 4], 0, 10), (uint32_t)strtoul(argv[i + 5], 0, 10), c, p);
        printf("%d %u %u\n", ok ? 1 : 0, c, p);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("f64_plan")
    src, exe = d / "plan.cpp", d / "plan"
    src.write_text(PROG)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)], check=True)

    def run(cases):
        args = [str(v) for case in cases for v in case]
        out = subprocess.run([str(exe)] + args, check=True, stdout=subprocess.PIPE).stdout.decode().split("\n")
        return [tuple(int(t) for t in ln.split()) for ln in out if ln]
    return run


def tiles(nx, ny):
    return ((nx + 7) // 8) * ((ny + 7) // 8)


def test_plans_stay_below_2_32_slots_and_45_gib(plan):
    cases = []
    for nx, ny in [(8, 8), (400, 225), (800, 800), (1920, 1080), (3840, 2160), (7680, 4320), (16384, 16384)]:
        for ns in [1, 7, 56, 520, 1000, 2100, 5000, 100000]:
            for budget in [0, 1, 24 * 64 * tiles(nx, ny) * 5, 200 << 30]:
                for free in [0, 64 << 30, 288 << 30]:
                    for chunks in [0, 3]:
                        cases.append((tiles(nx, ny), ns, budget, free, 1024, chunks))
    res = plan(cases)
    assert len(res) == len(cases)
    for (nt, ns, budget, free, _u, _c), (ok, chunk, pas) in zip(cases, res):
        assert ok, (nt, ns)
        slots = nt * 64
        assert 1 <= pas <= ns and 1 <= chunk <= pas
        assert pas * slots <= MAX_SLOTS, (nt, ns, budget, free, pas)
        assert pas == 1 or pas * slots * 24 <= MAX_BYTES
        assert pas == ns or pas % chunk == 0  # whole chunks per pass, the last pass takes the rest
        if budget >= 24 * slots:
            assert pas == 1 or pas * slots * 24 <= budget


def test_renders_beyond_2_32_slots_run_in_passes(plan):
    # the sizes at which a single pass would wrap: 1920x1080 at 2100 spp, 4K at 520 spp (texels x ns > 2^32)
    for nx, ny, ns in [(1920, 1080, 2100), (3840, 2160, 520), (1920, 1080, 5000)]:
        assert tiles(nx, ny) * 64 * ns > MAX_SLOTS
        (ok, chunk, pas), = plan([(tiles(nx, ny), ns, 0, 288 << 30, 1024, 0)])
        assert ok and pas < ns and tiles(nx, ny) * 64 * pas <= MAX_SLOTS


def test_image_too_large_for_one_sample_per_pass_is_refused(plan):
    (ok, _c, _p), = plan([(2**26 + 1, 1, 0, 1 << 40, 0, 0)])  # 2^32 + 64 padded pixels
    assert ok == 0
