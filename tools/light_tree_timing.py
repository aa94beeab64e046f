"""Times rtmi_render_nee with the light tree (include/rtmi_light_tree.h) against the same call with the light table, and
measures the time to equal noise.  Needs a GPU.  Prints one JSON line per (scene, mode) and one per scene with the figure
of merit.

    python tools/light_tree_timing.py                      # the five scenes of DESIGN.md §25
    python tools/light_tree_timing.py --ns 16 --repeats 2  # a shorter run
    python tools/light_tree_timing.py --table-only         # render_nee alone: runs on a tree without the feature too

Every call is blocking; its time is the span between two HIP events on the null stream around it (tools/denoise_timing.py).
One warm-up call per mode, then the modes alternate `repeats` times and the median is reported.  Noise: sigma = the median,
over the pixels lit in both, of the standard deviation of a pixel's mean across `--seeds` independent renders
(noise_ratio; rms_ratio is the root of the mean variance instead, which the few pixels that see a lamp's edge rule under
either selection).  A pixel's own Welford stderr is reported too (stderr_ratio, median over those pixels, first seed) but is
not the yardstick: under many small lights the table's noise is rare bright BSDF hits that most pixels do not see in 64
samples, and their own stderr under-reports it.  Figure of merit: t_tree * noise_ratio^2 / t_table, the
time the tree needs for the table's noise relative to the table's time (< 1: the tree is worth it).  cornell_box has one
light: its row is the pure overhead of the walk's one load.
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

CASES = [("cornell_box", 800, 800), ("lit_random_spheres", 1200, 800), ("lit_final_scene", 1920, 1080),
         ("lamp_grid_16", 1200, 800), ("lamp_grid_64", 1200, 800)]


def _build(host, name, nx, ny):
    if name.startswith("lamp_grid_"):
        import light_tree_scenes as lts

        g = int(name.rsplit("_", 1)[1])
        return lts.lamp_grid_camera(host, nx, ny, g), lts.lamp_grid(host, g)
    if name in scenes.SCENES:
        return scenes.build(host, name, nx, ny, seed=1)
    return scenes_extra.build(host, name, nx, ny, seed=7 if name == "lit_random_spheres" else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--scenes", default=",".join(c[0] for c in CASES))
    ap.add_argument("--table-only", action="store_true")
    ap.add_argument("--seeds", type=int, default=8)
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
        modes = {"table": lambda: sc.render_nee(cam, nx, ny, ns, seed=42, flags=fc)}
        if not args.table_only:
            sc.attach_light_tree()
            modes["tree"] = lambda: sc.render_nee(cam, nx, ny, ns, seed=42, flags=fc, light_tree=True)
        times = {m: [] for m in modes}
        out = {m: fn() for m, fn in modes.items()}  # warm-up, and the images the noise is read from
        for _ in range(args.repeats):
            for m, fn in modes.items():
                times[m].append(ev.time_ms(fn)[0])
        lit = np.ones((ny, nx), bool)
        for o in out.values():
            lit &= o["linear"].sum(-1) > 0
        sig = {m: float(np.median(o["stderr"].mean(-1)[lit])) if lit.any() else float("nan") for m, o in out.items()}
        # the variance of a pixel's mean across seeds (running sums: the images are large)
        calls = {"table": lambda k: sc.render_nee(cam, nx, ny, ns, seed=42 + k, flags=fc),
                 "tree": lambda k: sc.render_nee(cam, nx, ny, ns, seed=42 + k, flags=fc, light_tree=True)}
        noise, rms = {}, {}
        for m in modes:
            s1, s2 = np.zeros((ny, nx, 3)), np.zeros((ny, nx, 3))
            for k in range(args.seeds):
                img = (out[m] if k == 0 else calls[m](k))["linear"].astype(np.float64)
                s1 += img
                s2 += img * img
            var = (s2 - s1 * s1 / args.seeds) / max(args.seeds - 1, 1)
            ok = lit.any() and args.seeds > 1
            noise[m] = float(np.median(np.sqrt(np.maximum(var.mean(-1)[lit], 0.0)))) if ok else float("nan")
            rms[m] = float(np.sqrt(var.mean(-1)[lit].mean())) if ok else float("nan")
        med = {m: float(np.median(t)) for m, t in times.items()}
        for m in modes:
            print(json.dumps({"scene": name, "lights": int(len(sc.lights())), "nx": nx, "ny": ny, "ns": ns, "mode": m,
                              "ms": med[m], "msamples_per_s": nx * ny * ns / (med[m] / 1e3) / 1e6, "noise": noise[m],
                              "median_stderr": sig[m], "repeats_ms": times[m]}), flush=True)
        if "tree" in modes:
            r = noise["tree"] / noise["table"]
            print(json.dumps({"scene": name, "noise_ratio": r, "rms_ratio": rms["tree"] / rms["table"], "stderr_ratio": sig["tree"] / sig["table"],
                              "time_ratio": med["tree"] / med["table"],
                              "time_to_equal_noise": med["tree"] * r ** 2 / med["table"]}), flush=True)
        host.free_all()


if __name__ == "__main__":
    main()
