"""Times the re-trace of the pixels a reconstruction could not serve (Scene.refine_pixels, include/rtmi_sparse.h) behind an
upscaled frame (Upscaler.render), against the upscaled frame alone and the full-resolution frame (Frame.render).  Needs a GPU.

    python tools/sparse_timing.py                                # rows to stdout and to profiles/sparse/timing.jsonl
    python tools/sparse_timing.py --scenes cornell_box --repeats 4 --out /dev/null
    python tools/sparse_timing.py --quality                      # adds the RMSE rows (a 4096-spp reference per scene)
    python tools/sparse_timing.py --summarise X_results.db       # per-kernel durations of a rocprofv3 --kernel-trace run
    python tools/sparse_timing.py --design                       # the table of profiles/sparse/timing.jsonl into DESIGN.md §31

One process: per scene a full-resolution Frame and an Upscaler at scale 2 on one uploaded scene, NEE, 4 spp,
out="torch" (no plane passes through the host).  Modes, alternating in this order: frame_full; upscaler; upscaler followed
by refine_pixels of class 3; the same of classes 2 and 3, both at ns = 4 and a budget of half the image.  Every mode makes two
warm-up calls, then `--repeats` calls.  The camera moves between the calls as in tools/upscale_timing.py.  A call's time
is the host clock around it: every call timed here is blocking (refine_pixels reads its two counts back), and the timed
region is the whole Python call as a frame loop pays it.  Rows hold the median, the range and every repeat, and the counts
of re-traced pixels of the last repeat; the last row per scene has the ratios of the medians.  The frame and upscaler code
is the parent commit's (no kernel or entry of it changed), so those rows are the parent's figures, measured in the same
process and minute.

The kernels' own durations come from a run of this tool under `rocprofv3 --kernel-trace --stats`, in a run of its own
(`--out /dev/null`: a traced run's host times are not kept); `--summarise` reduces the trace to medians per kernel and, with
the path counts of the run, to the time per traced path of rtmi_sparse_kernel beside rtmi_nee_kernel's.
"""
import argparse
import csv
import json
import os
import re
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"cornell_box": (800, 800, (278.0, 278.0, -800.0), (278.0, 278.0, 0.0), 40.0),
         "lit_final_scene": (1920, 1080, (478.0, 278.0, -600.0), (278.0, 278.0, 0.0), 40.0)}
REFINES = {"refine_3": (3,), "refine_23": (2, 3)}
BEGIN, END = "<!-- sparse_timing:begin -->", "<!-- sparse_timing:end -->"


def median(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def summarise(path):
    """Median, range and every launch of each kernel's duration in a rocprofv3 kernel trace (the .db or the .csv), µs."""
    per = {}
    if path.endswith(".db"):  # rocprofv3's default output: its `kernels` view, in launch order
        import sqlite3

        for name, ns in sqlite3.connect(path).execute("select name, duration from kernels order by start"):
            per.setdefault(re.sub(r"\(.*", "", name), []).append(ns / 1e3)
    else:  # --output-format csv: X_kernel_trace.csv
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = re.sub(r"\(.*", "", row["Kernel_Name"])
                per.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    for name in sorted(per):
        v = per[name]
        print(json.dumps({"kernel": name, "launches": len(v), "median_us": median(v), "min_us": min(v), "max_us": max(v),
                          "launches_us": [round(x, 1) for x in v]}))
    return 0


def table(rows):
    out = ["| scene | `Frame`, full size | `Upscaler`, scale 2 | + re-trace of class 3 | + re-trace of classes 2, 3 |", "|---|---|---|---|---|"]
    for scene in dict.fromkeys(r["scene"] for r in rows):
        by = {r["mode"]: r for r in rows if r["scene"] == scene and "mode" in r}
        full = by["frame_full"]["median_ms"]
        cell = lambda r: "%.2f (%.2f–%.2f)" % (r["median_ms"], r["min_ms"], r["max_ms"])  # noqa: E731
        cells = [cell(by["frame_full"]), "%s, %.2f×" % (cell(by["upscaler"]), by["upscaler"]["median_ms"] / full)]
        for m in REFINES:
            r = by[m]
            cells.append("%s, %.2f×; %d of %d pixels" % (cell(r), r["median_ms"] / full, r["refined"][0], r["nx"] * r["ny"]))
        out.append("| %s %d×%d | %s |" % (scene, by["frame_full"]["nx"], by["frame_full"]["ny"], " | ".join(cells)))
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
    ap.add_argument("--ns", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--quality", action="store_true", help="also RMSE against render_nee at --reference-spp over the re-traced pixels")
    ap.add_argument("--reference-spp", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "sparse", "timing.jsonl"))
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

        def cam(k):
            return scenes.set_camera(host, nx, ny, (look_from[0] + 2.0 * k,) + look_from[1:], look_at, vertical_fov=vfov)

        frame = sc.frame(nx, ny, estimator="nee", flags=fc)
        ups = sc.upscaler(nx, ny, scale=2.0, estimator="nee", flags=fc)
        budget = nx * ny // 2
        refined = {}

        def run(mode, k):
            if mode == "frame_full":
                return frame.render(cam(k), args.ns, seed=k, out="torch")
            planes = ups.render(cam(k), args.ns, seed=k, out="torch")
            if mode in REFINES:
                planes = sc.refine_pixels(cam(k), planes, classes=REFINES[mode], ns=args.ns, estimator="nee", seed=k, budget=budget, flags=fc)
                refined[mode] = planes["refined"]
            return planes

        modes = ["frame_full", "upscaler"] + list(REFINES)
        times = {m: [] for m in modes}
        for k in range(2):  # warm-up, every shape
            for m in modes:
                run(m, k)
        for k in range(2, args.repeats + 2):
            for m in modes:
                t0 = time.perf_counter()
                run(m, k)
                times[m].append((time.perf_counter() - t0) * 1e3)
        for m in modes:
            row = {"scene": name, "nx": nx, "ny": ny, "ns": args.ns, "mode": m, "low": [ups.lx, ups.ly], "median_ms": median(times[m]),
                   "min_ms": min(times[m]), "max_ms": max(times[m]), "repeats_ms": times[m]}
            if m in refined:
                row["refined"], row["budget"] = list(refined[m]), budget
            rows.append(row)
        full = median(times["frame_full"])
        rows.append(dict({"scene": name, "summary": True},
                         **{"%s_over_frame_full" % m: median(times[m]) / full for m in modes[1:]},
                         **{"%s_every_repeat_faster" % m: max(times[m]) < min(times["frame_full"]) for m in modes[1:]}))
        if args.quality:  # a fresh history, frame 0: before and after the re-trace against a converged render
            truth = torch.from_numpy(sc.render_nee(cam(0), nx, ny, args.reference_spp, seed=99, flags=fc)["linear"]).reshape(-1, 3).double()
            for m, classes in REFINES.items():
                ups.reset()
                planes = ups.render(cam(0), args.ns, seed=0, out="torch")
                px = torch.isin(planes["cls"].reshape(-1).cpu(), torch.tensor(classes, dtype=torch.uint8)).nonzero().reshape(-1)
                before = planes["linear"].reshape(-1, 3).cpu().double()[px]
                out = sc.refine_pixels(cam(0), planes, classes=classes, ns=args.ns, estimator="nee", seed=0, flags=fc)
                after = out["linear"].reshape(-1, 3).cpu().double()[px]
                rmse = lambda a: float(np.sqrt(((a - truth[px]) ** 2).mean().item()))  # noqa: E731
                rows.append({"scene": name, "quality": m, "pixels": int(px.numel()), "refined": list(out["refined"]), "ns": args.ns,
                             "reference_spp": args.reference_spp, "rmse_before": rmse(before), "rmse_after": rmse(after)})
        host.free_all()
    text = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text)
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
