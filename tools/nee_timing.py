"""Times next-event estimation (include/rtmi_nee.h) against the default render and its per-lane form, and measures the
time to equal noise.  Needs a GPU.  Prints one JSON line per (scene, mode) and one per scene with the figure of merit.

    python tools/nee_timing.py                      # cornell_box 800x800, lit_smoke 800x800, lit_final_scene 1920x1080
    python tools/nee_timing.py --ns 16 --repeats 2  # a shorter run

Every call is blocking; its time is the span between two HIP events on the null stream around it (tools/denoise_timing.py).
One warm-up call per mode, then the modes alternate `repeats` times and the median is reported.  The standard errors come
from render_adaptive(min_spp = ns) (render()'s image and its Welford plane) and from render_nee; median over the pixels
whose default mean is not zero.  Figure of merit: t_nee * (sigma_nee / sigma_def)^2 / t_def, the time NEE needs for the
default render's noise relative to the default render's time (< 1: NEE is worth it).  Kernel times per launch come from a
separate rocprofv3 --kernel-trace --stats run of this tool.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from denoise_timing import Events  # noqa: E402
from raytracing_rust_amd import Host, abi, scenes  # noqa: E402
import scenes_extra  # noqa: E402

CASES = [("cornell_box", 800, 800), ("lit_smoke", 800, 800), ("lit_final_scene", 1920, 1080)]


def _build(host, name, nx, ny):
    if name in scenes.SCENES:
        return scenes.build(host, name, nx, ny, seed=1)
    return scenes_extra.build(host, name, nx, ny, seed=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--scenes", default=",".join(c[0] for c in CASES))
    args = ap.parse_args()
    host = Host()
    ev = Events()
    fc = abi.RTMI_FLAG_FAST_CULL
    for name, nx, ny in CASES:
        if name not in args.scenes.split(","):
            continue
        cam, world = _build(host, name, nx, ny)
        sc = host.lower(world).upload(0, nee=True)
        ns = args.ns
        modes = {"render": lambda: sc.render(cam, nx, ny, ns, seed=42, flags=fc),
                 "render_sync": lambda: sc.render(cam, nx, ny, ns, seed=42, flags=fc | abi.RTMI_FLAG_SYNC),
                 "render_nee": lambda: sc.render_nee(cam, nx, ny, ns, seed=42, flags=fc)}
        times = {m: [] for m in modes}
        for fn in modes.values():
            fn()  # warm-up
        for _ in range(args.repeats):
            for m, fn in modes.items():
                times[m].append(ev.time_ms(fn)[0])
        d = sc.render_adaptive(cam, nx, ny, ns, min_spp=ns, step_spp=1, seed=42, flags=fc)
        n = sc.render_nee(cam, nx, ny, ns, seed=42, flags=fc)
        lit = d["linear"].sum(-1) > 0
        sig_def = float(np.median(d["stderr"].mean(-1)[lit])) if lit.any() else float("nan")
        sig_nee = float(np.median(n["stderr"].mean(-1)[lit])) if lit.any() else float("nan")
        sig = {"render": sig_def, "render_sync": sig_def, "render_nee": sig_nee}
        med = {m: float(np.median(t)) for m, t in times.items()}
        for m in modes:
            print(json.dumps({"scene": name, "nx": nx, "ny": ny, "ns": ns, "mode": m, "seconds": med[m] / 1e3,
                              "msamples_per_s": nx * ny * ns / (med[m] / 1e3) / 1e6, "median_stderr": sig[m],
                              "repeats_ms": times[m]}), flush=True)
        fom = med["render_nee"] * (sig_nee / sig_def) ** 2 / med["render"]
        print(json.dumps({"scene": name, "stderr_ratio": sig_nee / sig_def, "time_ratio": med["render_nee"] / med["render"],
                          "time_ratio_vs_sync": med["render_nee"] / med["render_sync"], "time_to_equal_noise": fom}),
              flush=True)
        host.free_all()


if __name__ == "__main__":
    main()
