"""Times per-pixel adaptive sampling (Scene.render_pixelwise, include/rtmi_pixelwise.h) against the tile-adaptive entry of
the parent commit (Scene.render_adaptive(nee=True)) and against the fixed render at the cap (Scene.render_nee).  Needs a GPU.

    python tools/pixelwise_timing.py                                # rows to stdout and to profiles/pixelwise/timing.jsonl
    python tools/pixelwise_timing.py --scenes cornell_box --repeats 4 --out /dev/null
    python tools/pixelwise_timing.py --summarise X_results.db       # per-kernel durations of a rocprofv3 --kernel-trace run
    python tools/pixelwise_timing.py --design                       # the table of profiles/pixelwise/timing.jsonl into DESIGN.md §32

One process, per scene one uploaded scene, NEE, FAST_CULL.  Two lattices: min = step = 64 under a cap of 1000 (the one of
DESIGN.md §11's table) and min = step = 8 under a cap of 64, both with rel_tol 0.05 and abs_tol 0.  Modes, alternating in this
order: `fixed`, render_nee at the cap; `tile`, render_adaptive(nee=True); `pixelwise`, render_pixelwise, blocking, numpy
planes; `pixelwise_device`, render_pixelwise(out="torch") followed by a synchronize of its stream (nothing is copied to the
host).  Every mode makes two warm-up calls, then `--repeats` calls; a call's time is the host clock around it.  Rows hold the
median, the range and every repeat, the paths traced, the RMSE against render_nee at --reference-spp under another seed, and
the histogram of the per-pixel counts.  The cost of an empty step: the device form with tolerances so loose that every pixel
retires at min_spp runs one real step and steps - 1 empty ones (select, path kernel and step kernel over an empty list); the
row `empty_step` holds its median time, that of the one-step run with ns = min_spp, and their difference per empty step.

The kernels' own durations come from a run of this tool under `rocprofv3 --kernel-trace --stats`, in a run of its own
(`--out /dev/null --repeats 2`); `--summarise` reduces the trace to medians per kernel.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
from sparse_timing import CASES, median, summarise  # noqa: E402

LATTICES = {"cap1000": (64, 64, 1000), "cap64": (8, 8, 64)}
MODES = ("fixed", "tile", "pixelwise", "pixelwise_device")
BEGIN, END = "<!-- pixelwise_timing:begin -->", "<!-- pixelwise_timing:end -->"


def table(rows):
    out = ["| scene, lattice | fixed at the cap | tile-adaptive | per pixel, blocking | per pixel, device form | empty step |",
           "|---|---|---|---|---|---|"]
    keys = dict.fromkeys((r["scene"], r["lattice"]) for r in rows)
    for scene, lattice in keys:
        by = {r["mode"]: r for r in rows if r["scene"] == scene and r["lattice"] == lattice}
        fixed = by["fixed"]

        def cell(r):
            return "%.1f ms (%.1f–%.1f), %.0f %% of the paths, rmse %.4f" % (
                r["median_ms"], r["min_ms"], r["max_ms"], 100.0 * r["paths"] / fixed["paths"], r["rmse"])

        e = by["empty_step"]
        out.append("| %s %d×%d, %d + %d·k ≤ %d | %s | %s | %s | %s | %.3f ms |" % (
            scene, fixed["nx"], fixed["ny"], fixed["min_spp"], fixed["step_spp"], fixed["cap"], cell(fixed), cell(by["tile"]),
            cell(by["pixelwise"]), cell(by["pixelwise_device"]), e["per_empty_step_ms"]))
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
    ap.add_argument("--modes", default=",".join(MODES), help="a subset for a traced run; --design needs all four")
    ap.add_argument("--rel-tol", type=float, default=0.05)
    ap.add_argument("--pass-spp", type=int, default=0, help="samples per pixel and launch of render_pixelwise (0: a whole step)")
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--reference-spp", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "pixelwise", "timing.jsonl"))
    ap.add_argument("--summarise", metavar="TRACE", help="X_results.db or X_kernel_trace.csv of a rocprofv3 --kernel-trace run")
    ap.add_argument("--design", action="store_true")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
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
        truth = sc.render_nee(cam, nx, ny, args.reference_spp, seed=99, flags=fc)["linear"].astype(np.float64) if args.reference_spp else None
        stream = torch.cuda.current_stream(sc.device)
        for lattice in args.lattices.split(","):
            lo, step, cap = LATTICES[lattice]
            px = dict(abs_tol=0.0, rel_tol=args.rel_tol, estimator="nee", seed=1, pass_spp=args.pass_spp, flags=fc)

            def run(mode):
                """the timed call of a mode; it returns the mode's result dict"""
                if mode == "fixed":
                    return lambda: sc.render_nee(cam, nx, ny, cap, seed=1, flags=fc)
                if mode == "tile":
                    return lambda: sc.render_adaptive(cam, nx, ny, cap, lo, step, abs_tol=0.0, rel_tol=args.rel_tol, nee=True, seed=1, flags=fc)
                if mode == "pixelwise":
                    return lambda: sc.render_pixelwise(cam, nx, ny, cap, lo, step, **px)

                def device():
                    out = sc.render_pixelwise(cam, nx, ny, cap, lo, step, out="torch", **px)
                    stream.synchronize()
                    return out
                return device

            modes = args.modes.split(",")
            calls = {m: run(m) for m in modes}
            times = {m: [] for m in modes}
            last = {}
            for m in modes:  # warm-up
                for _ in range(2):
                    calls[m]()
            for _ in range(args.repeats):
                for m in modes:
                    t0 = time.perf_counter()
                    last[m] = calls[m]()
                    times[m].append((time.perf_counter() - t0) * 1e3)
            for m in modes:
                out = last[m]
                lin = out["linear"].cpu().numpy() if m == "pixelwise_device" else out["linear"]
                spp = None if m == "fixed" else out["spp"].cpu().numpy().view(np.uint32) if m == "pixelwise_device" else out["spp"]
                paths = nx * ny * cap if m == "fixed" else out["stats"]["samples"] if m == "tile" else \
                    out["samples"]() if m == "pixelwise_device" else out["samples"]
                row = {"scene": name, "nx": nx, "ny": ny, "lattice": lattice, "min_spp": lo, "step_spp": step, "cap": cap, "rel_tol": args.rel_tol,
                       "pass_spp": args.pass_spp, "mode": m, "median_ms": median(times[m]), "min_ms": min(times[m]), "max_ms": max(times[m]),
                       "repeats_ms": times[m], "paths": int(paths)}
                if truth is not None:
                    row["rmse"] = float(np.sqrt(np.mean((lin.astype(np.float64) - truth) ** 2)))
                    row["reference_spp"] = args.reference_spp
                if spp is not None:
                    row["spp_histogram"] = dict(zip(*[a.tolist() for a in np.unique(spp, return_counts=True)]))
                    row["paths_in_image"] = int(spp.astype(np.int64).sum())  # the tile entry also traces the lanes outside the image
                rows.append(row)
            del last
            # an empty step of the device form
            steps = 1 + -(-(cap - lo) // step)
            loose = dict(px, abs_tol=1e30, rel_tol=1e30)
            t_loose, t_one = [], []
            for k in range(2 + args.repeats):
                for t, ns in ((t_loose, cap), (t_one, lo)):
                    t0 = time.perf_counter()
                    out = sc.render_pixelwise(cam, nx, ny, ns, lo, step, out="torch", **loose)
                    stream.synchronize()
                    if k >= 2:
                        t.append((time.perf_counter() - t0) * 1e3)
            assert out["samples"]() == nx * ny * lo
            rows.append({"scene": name, "nx": nx, "ny": ny, "lattice": lattice, "mode": "empty_step", "steps": steps, "loose_median_ms": median(t_loose),
                         "one_step_median_ms": median(t_one), "per_empty_step_ms": (median(t_loose) - median(t_one)) / max(steps - 1, 1),
                         "loose_ms": t_loose, "one_step_ms": t_one})
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
