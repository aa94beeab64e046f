"""Timings of the lights that follow a scene update (include/rtmi_relight.h) on the GPU of this machine.  One
JSON line per measurement on stdout (and appended to --out), each with the library's build hash:

  follow     the device-form update of every lamp of a scene with follow_lights() on: host time of the enqueue, time to
             completion, and the GPU time of the update's kernels between two events
  plain      the GPU time of the same update with following off (scatter and refit alone): the difference to `follow` is the
             relight kernel's own time
  reattach   what a caller had to do before: the blocking update plus the wrapper's re-attach of the table and the tree

Scenes: cornell_box (1 light) and lit_random_spheres (20) of the tests' scene set, and grids of 256 and 4096 lamps with the
geometry of tests/light_tree_scenes.py's lamp_grid — in a list, not under a BVHNode: a tree of rects cannot be refit
(rtmi_update.h), so its lamps cannot move at all.  A scene whose lamps sit in an item that cannot be refit is reported so.
Every figure is the median of --reps runs after --warmup warm-up runs, with the minimum and the maximum beside it.

    python tools/relight_timing.py [--reps 20] [--warmup 3] [--out profiles/relight/timing.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from raytracing_rust_amd import Host, abi  # noqa: E402


def spread(samples):
    s = sorted(samples)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "n": len(s)}


def timed(fn, reps, warmup, sync=None):
    out = []
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        if k >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return spread(out)


def lamp_list(host, g, bright_every=4, le=20.0):
    """lamp_grid(g) of tests/light_tree_scenes.py with the lamps in the world list"""
    world = host.HittableList()
    half = max(40.0, g * 1.5)
    world.push(host.Rect(host.PLANE_XY, -half, -half, half, half, 0.0, host.Lambertian(host.SolidTexture(0.7, 0.7, 0.7))))
    for i in range(g):
        for k in range(g):
            bright = bright_every and (i * g + k) % bright_every == bright_every - 1
            cx, cy = (i - (g - 1) / 2) * 2.0, (k - (g - 1) / 2) * 2.0
            e = 5.0 * le if bright else le
            world.push(host.Rect(host.PLANE_XY, cx - 0.1, cy - 0.1, cx + 0.1, cy + 0.1, 1.0, host.DiffuseLight(host.SolidTexture(e, e, e))))
    return world


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import light_tree_scenes

    host = Host()
    build = (abi.load_rtmi().rtmi_build_hash() or b"").decode()
    lines = []

    def emit(**kw):
        kw["build"] = build
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    worlds = {"cornell_box": lambda: light_tree_scenes.build(host, "cornell_box", 64, 64)[1],
              "lit_random_spheres": lambda: light_tree_scenes.build(host, "lit_random_spheres", 64, 64)[1],
              "lamps256": lambda: lamp_list(host, 16), "lamps4096": lambda: lamp_list(host, 64, 0)}
    for name, make in worlds.items():
        scene = host.lower(make()).upload(0, light_tree=True)
        d = scene.desc()
        a = np.ctypeslib.as_array(d.prim_a, shape=(d.n_prims, 4)).copy()
        b = np.ctypeslib.as_array(d.prim_b, shape=(d.n_prims, 4)).copy()
        lights = scene.lights()
        first, count = int(lights["prim"].min()), int(lights["prim"].max() - lights["prim"].min() + 1)
        emit(what="scene", scene=name, lights=len(lights), prims=int(d.n_prims), first=first, count=count)
        a1 = a.copy()
        for L in lights:  # a rect travels along its plane's first axis, a sphere along x
            p = int(L["prim"])
            a1[p, [0, 2]] += np.float32(1e-3)
            if L["kind"] != abi.PRIM_RECT:
                a1[p, 2] = a[p, 2]
        s = slice(first, first + count)
        try:
            scene.update_prims(first, a[s], b[s])
        except Exception as e:  # the lamps share an item that cannot be refit
            emit(what="refused", scene=name, why=str(e)[:160])
            host.free_all()
            continue
        turn = [0]

        def reattach():  # following off: the wrapper derives table and tree again from the description and uploads them
            turn[0] ^= 1
            scene.update_prims(first, (a1 if turn[0] else a)[s], b[s])

        emit(what="reattach", scene=name, ms=timed(reattach, args.reps, args.warmup))
        tensors = [(torch.tensor(x[s], device="cuda"), torch.tensor(b[s], device="cuda")) for x in (a, a1)]
        torch.cuda.synchronize()
        scene.follow_lights()

        def device():
            turn[0] ^= 1
            scene.update_prims(first, *tensors[turn[0]])

        emit(what="follow", form="device, enqueue", scene=name, ms=timed(device, args.reps, args.warmup))
        torch.cuda.synchronize()
        emit(what="follow", form="device, to completion", scene=name, ms=timed(device, args.reps, args.warmup, torch.cuda.synchronize))

        def gpu_ms(call):
            out = []
            for k in range(args.warmup + args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                torch.cuda.synchronize()
                if k >= args.warmup:
                    out.append(e0.elapsed_time(e1))
            return spread(out)

        emit(what="follow", form="device, kernels", scene=name, ms=gpu_ms(device))
        scene.follow_lights(False)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def plain():  # the entry itself: the wrapper refuses tensors for a range with emitters while following is off
            ta, tb = tensors[0]
            host._check(host.lib.rthu_update_prims_device(scene.h, first, count, C.c_void_p(ta.data_ptr()), C.c_void_p(tb.data_ptr()), stream))

        emit(what="plain", form="device, kernels", scene=name, ms=gpu_ms(plain))
        host.free_all()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
