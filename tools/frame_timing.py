"""Times the frame pipeline (Frame.render, include/rtmi_frame.h) against the chain it replaces (Scene.render_temporal) as
the parent commit built it, and the one-shot entries of this tree against the parent's.  Needs a GPU.

    python tools/frame_timing.py --parent <parent tree>            # both trees, alternating; one JSON row per (scene, tree, mode)
    python tools/frame_timing.py                                   # this tree alone
    python tools/frame_timing.py --worker --scenes cornell_box     # one process of one tree (what the driver starts)

<parent tree> is a checkout of the parent commit built beside this one (`git worktree add`, then `python -m
raytracing_rust_amd.build` in it).  A process can hold one build of the package, so the driver starts one worker process
per tree and round, this tree and the parent in turn, `--rounds` times; a worker builds each scene once, makes one warm-up
call per mode and then `--repeats` calls per mode with the modes alternating.  The camera moves between the calls of a
mode (look_from.x + 2 per frame, the path of tests/test_gpu_frame.py), so the push reprojects.  A call's time is the host
clock around it: every call timed here is blocking and ends in a device synchronise.  Rows hold the median, the range
and every repeat.  4 spp NEE, as DESIGN.md §28 records it.

Modes: frame_numpy and frame_torch (this tree: Frame.render to host arrays, and with out="torch"), render_temporal and
render_nee (both trees).  The last row per scene is the verdict: every repeat of either frame mode against every repeat of
the parent's render_temporal.
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"cornell_box": (800, 800, (278.0, 278.0, -800.0), (278.0, 278.0, 0.0), 40.0),
         "lit_final_scene": (1920, 1080, (478.0, 278.0, -600.0), (278.0, 278.0, 0.0), 40.0)}


def worker(args):
    tree = os.path.abspath(args.tree or HERE)
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    import numpy as np  # noqa: F401
    import scenes_extra
    from raytracing_rust_amd import Host, Scene, Temporal, abi, scenes

    host = Host()
    fc = abi.RTMI_FLAG_FAST_CULL
    for name in args.scenes.split(","):
        nx, ny, look_from, look_at, vfov = CASES[name]
        build = scenes.build if name in scenes.SCENES else scenes_extra.build
        _, world = build(host, name, nx, ny, seed=1)
        sc = host.lower(world).upload(0, nee=True)

        def cam(k):
            return scenes.set_camera(host, nx, ny, (look_from[0] + 2.0 * k,) + look_from[1:], look_at, vertical_fov=vfov)

        t = Temporal(nx, ny)
        modes = {"render_temporal": lambda k: sc.render_temporal(t, cam(k), nx, ny, args.ns, nee=True, seed=k, flags=fc),
                 "render_nee": lambda k: sc.render_nee(cam(k), nx, ny, args.ns, seed=k, flags=fc)}
        if hasattr(Scene, "frame"):
            f_np, f_t = sc.frame(nx, ny, estimator="nee", flags=fc), sc.frame(nx, ny, estimator="nee", flags=fc)
            modes["frame_numpy"] = lambda k: f_np.render(cam(k), args.ns, seed=k)
            modes["frame_torch"] = lambda k: f_t.render(cam(k), args.ns, seed=k, out="torch")
        times = {m: [] for m in modes}
        for fn in modes.values():
            fn(0)  # warm-up: code objects, the scene's scratch, torch's context
        for k in range(1, args.repeats + 1):
            for m, fn in modes.items():
                t0 = time.perf_counter()
                fn(k)
                times[m].append((time.perf_counter() - t0) * 1e3)
        for m in modes:
            print(json.dumps({"worker": True, "scene": name, "nx": nx, "ny": ny, "ns": args.ns, "mode": m, "repeats_ms": times[m]}),
                  flush=True)
        host.free_all()


def driver(args):
    trees = [("this", HERE)] + ([("parent", os.path.abspath(args.parent))] if args.parent else [])
    rows = {}
    for _ in range(args.rounds):
        for label, tree in trees:
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--scenes", args.scenes, "--ns", str(args.ns),
                   "--repeats", str(args.repeats)]
            out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=args.worker_timeout).stdout
            for line in out.splitlines():
                if line.startswith("{"):
                    r = json.loads(line)
                    key = (r["scene"], label, r["mode"])
                    rows.setdefault(key, dict(r, tree=label, repeats_ms=[]))["repeats_ms"] += r["repeats_ms"]
    for (scene, label, mode), r in rows.items():
        ms = sorted(r["repeats_ms"])
        r.pop("worker")
        r.update(median_ms=ms[len(ms) // 2] if len(ms) % 2 else 0.5 * (ms[len(ms) // 2 - 1] + ms[len(ms) // 2]), min_ms=ms[0],
                 max_ms=ms[-1], rounds=args.rounds)
        print(json.dumps(r), flush=True)
    ok = True
    for scene in args.scenes.split(","):
        base = rows.get((scene, "parent", "render_temporal"))
        if not base:
            continue
        verdict = {"scene": scene, "verdict": True}
        for mode in ("frame_numpy", "frame_torch"):
            f = rows[(scene, "this", mode)]
            verdict[mode + "_every_repeat_faster"] = f["max_ms"] < base["min_ms"]
            verdict[mode + "_saved_ms"] = base["median_ms"] - f["median_ms"]
            verdict[mode + "_speedup"] = base["median_ms"] / f["median_ms"]
            ok = ok and f["max_ms"] < base["min_ms"]
        for mode in ("render_temporal", "render_nee"):  # the one-shot entries: this tree within the parent's spread
            a, b = rows[(scene, "this", mode)], rows[(scene, "parent", mode)]
            verdict[mode + "_this_over_parent"] = a["median_ms"] / b["median_ms"]
            verdict[mode + "_within_spread"] = a["median_ms"] <= b["max_ms"] and b["median_ms"] <= a["max_ms"]
        print(json.dumps(verdict), flush=True)
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--scenes", default=",".join(CASES))
    ap.add_argument("--ns", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--worker-timeout", type=float, default=240.0)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", help="(worker) the tree whose package to time; default: this one")
    args = ap.parse_args()
    if args.worker:
        worker(args)
        return 0
    return driver(args)


if __name__ == "__main__":
    sys.exit(main())
