"""Times windowed adaptive sampling (Scene.render_windowed, include/rtmi_window.h) at the radii 0, 1, 2 and 4 against the
tile-adaptive entry (Scene.render_adaptive(nee=True)) and the fixed render at the cap (Scene.render_nee).  Needs a GPU.

    python tools/window_timing.py                                # rows to stdout and to profiles/window/timing.jsonl
    python tools/window_timing.py --scenes cornell_box --repeats 4 --out /dev/null
    python tools/window_timing.py --design                       # the table of profiles/window/timing.jsonl into DESIGN.md §33

The scenes, the lattices and the tolerances are those of tools/pixelwise_timing.py: one process, per scene one uploaded scene,
NEE, FAST_CULL, rel_tol 0.05, abs_tol 0.  Modes, alternating in this order: `fixed`, render_nee at the cap; `tile`,
render_adaptive(nee=True); `window_r0` .. `window_r4`, render_windowed(out="torch") with that radius followed by a
synchronize of its stream (radius 0 is the per-pixel entry's launch sequence).  Every mode makes two warm-up calls, then
`--repeats` calls; a call's time is the host clock around it.  Rows hold the median, the range and every repeat, the paths
traced, the RMSE against render_nee at --reference-spp under another seed, and the histogram of the per-pixel counts.  The
cost of an empty step at radius 1: the device form with tolerances so loose that every pixel retires at min_spp runs one real
step and steps - 1 empty ones (select, path kernel and step kernel over an empty list, and the spread over the whole image);
the row `empty_step` holds its median time, that of the one-step run with ns = min_spp, and their difference per empty step.

The spread kernel's own duration comes from kernel traces (profiles/window/spread_kernel_trace.jsonl).
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
from pixelwise_timing import LATTICES  # noqa: E402
from sparse_timing import CASES, median  # noqa: E402

RADII = (0, 1, 2, 4)
MODES = ("fixed", "tile") + tuple("window_r%d" % r for r in RADII)
BEGIN, END = "<!-- window_timing:begin -->", "<!-- window_timing:end -->"


def table(rows):
    out = ["| scene, lattice | " + " | ".join(("fixed at the cap", "tile-adaptive") + tuple("r = %d" % r for r in RADII)) + " | empty step, r = 1 |",
           "|" + "---|" * (len(MODES) + 2)]
    keys = dict.fromkeys((r["scene"], r["lattice"]) for r in rows)
    for scene, lattice in keys:
        by = {r["mode"]: r for r in rows if r["scene"] == scene and r["lattice"] == lattice}
        fixed = by["fixed"]

        def cell(r):
            return "%.1f ms (%.1f–%.1f), %.0f %% of the paths, rmse %.4f" % (
                r["median_ms"], r["min_ms"], r["max_ms"], 100.0 * r["paths"] / fixed["paths"], r["rmse"])

        out.append("| %s %d×%d, %d + %d·k ≤ %d | %s | %.3f ms |" % (
            scene, fixed["nx"], fixed["ny"], fixed["min_spp"], fixed["step_spp"], fixed["cap"], " | ".join(cell(by[m]) for m in MODES),
            by["empty_step"]["per_empty_step_ms"]))
    return "\n".join(out)


def design(jsonl):
    rows = [json.loads(line) for line in open(jsonl)]
    path = os.path.join(HERE, "DESIGN.md")
    text = open(path).read()
    a, b = text.index(BEGIN) + len(BEGIN), text.index(END)
    open(path, "w").write(text[:a] + "\n" + table(rows) + "\n" + text[b:])
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(CASES))
    ap.add_argument("--lattices", default=",".join(LATTICES))
    ap.add_argument("--rel-tol", type=float, default=0.05)
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--reference-spp", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "window", "timing.jsonl"))
    ap.add_argument("--design", action="store_true")
    args = ap.parse_args()
    if args.design:
        return design(args.out)
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import numpy as np
    import scenes_extra
    import torch
    from raytracing_rust_amd import Host, abi, scenes

    host = Host()
    fc = abi.RTMI_FLAG_FAST_CULL
    rows = []
    for name in args.scenes.split(","):
        nx, ny, look_from, look_at, vfov = CASES[name]
        build = scenes.build if name in scenes.SCENES else scenes_extra.build
        _, world = build(host, name, nx, ny, seed=1)
        sc = host.lower(world).upload(0, nee=True)
        cam = scenes.set_camera(host, nx, ny, look_from, look_at, vertical_fov=vfov)
        truth = sc.render_nee(cam, nx, ny, args.reference_spp, seed=99, flags=fc)["linear"].astype(np.float64)
        stream = torch.cuda.current_stream(sc.device)
        for lattice in args.lattices.split(","):
            lo, step, cap = LATTICES[lattice]
            px = dict(abs_tol=0.0, rel_tol=args.rel_tol, estimator="nee", seed=1, flags=fc)

            def run(mode):
                """the timed call of a mode; it returns the mode's result dict"""
                if mode == "fixed":
                    return lambda: sc.render_nee(cam, nx, ny, cap, seed=1, flags=fc)
                if mode == "tile":
                    return lambda: sc.render_adaptive(cam, nx, ny, cap, lo, step, abs_tol=0.0, rel_tol=args.rel_tol, nee=True, seed=1, flags=fc)
                radius = int(mode[len("window_r"):])

                def device():
                    out = sc.render_windowed(cam, nx, ny, cap, lo, step, radius=radius, out="torch", **px)
                    stream.synchronize()
                    return out
                return device

            calls = {m: run(m) for m in MODES}
            times = {m: [] for m in MODES}
            last = {}
            for m in MODES:  # warm-up
                for _ in range(2):
                    calls[m]()
            for _ in range(args.repeats):
                for m in MODES:
                    t0 = time.perf_counter()
                    last[m] = calls[m]()
                    times[m].append((time.perf_counter() - t0) * 1e3)
            for m in MODES:
                out = last[m]
                windowed = m.startswith("window")
                lin = out["linear"].cpu().numpy() if windowed else out["linear"]
                spp = None if m == "fixed" else out["spp"].cpu().numpy().view(np.uint32) if windowed else out["spp"]
                paths = nx * ny * cap if m == "fixed" else out["stats"]["samples"] if m == "tile" else out["samples"]()
                row = {"scene": name, "nx": nx, "ny": ny, "lattice": lattice, "min_spp": lo, "step_spp": step, "cap": cap, "rel_tol": args.rel_tol,
                       "mode": m, "median_ms": median(times[m]), "min_ms": min(times[m]), "max_ms": max(times[m]), "repeats_ms": times[m],
                       "paths": int(paths), "rmse": float(np.sqrt(np.mean((lin.astype(np.float64) - truth) ** 2))),
                       "reference_spp": args.reference_spp}
                if spp is not None:
                    row["spp_histogram"] = dict(zip(*[a.tolist() for a in np.unique(spp, return_counts=True)]))
                    row["paths_in_image"] = int(spp.astype(np.int64).sum())  # the tile entry also traces the lanes outside the image
                rows.append(row)
            del last
            # an empty step of the device form at radius 1
            steps = 1 + -(-(cap - lo) // step)
            loose = dict(px, abs_tol=1e30, rel_tol=1e30)
            t_loose, t_one = [], []
            for k in range(2 + args.repeats):
                for t, ns in ((t_loose, cap), (t_one, lo)):
                    t0 = time.perf_counter()
                    out = sc.render_windowed(cam, nx, ny, ns, lo, step, radius=1, out="torch", **loose)
                    stream.synchronize()
                    if k >= 2:
                        t.append((time.perf_counter() - t0) * 1e3)
            assert out["samples"]() == nx * ny * lo
            rows.append({"scene": name, "nx": nx, "ny": ny, "lattice": lattice, "mode": "empty_step", "radius": 1, "steps": steps,
                         "loose_median_ms": median(t_loose), "one_step_median_ms": median(t_one),
                         "per_empty_step_ms": (median(t_loose) - median(t_one)) / max(steps - 1, 1), "loose_ms": t_loose, "one_step_ms": t_one})
        host.free_all()
        torch.cuda.empty_cache()
    text = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text)
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
