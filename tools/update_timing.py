"""Timings of the scene updates (include/rtmi_update.h) on the GPU of this machine.  One JSON line per
measurement on stdout (and appended to --out), each with the library's build hash:

  update     one update_prims call over every refittable item of a scene, blocking (numpy planes, with the host description's
             refit) and through the device entry (torch planes; host time of the enqueue and time to completion)
  recreate   the only alternative without the entries: build the world again, lower it, destroy and create the handle,
             attach the light table, the light tree and a 2048 x 1024 environment map
  staleness  render time of the updated handle (topology of the old positions) against a scene lowered afresh at the same
             positions, after moving every sphere of the 485-sphere cluster by 1 %, 10 % and 100 % of the cluster's extent

Every figure is the median of --reps runs after --warmup warm-up runs, with the minimum and the maximum beside it.

    python tools/update_timing.py [--reps 20] [--warmup 3] [--out profiles/update/timing.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raytracing_rust_amd import Host, abi, env_from_sky, scenes  # noqa: E402


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


def cluster_world(host, centres, radius, seed=9):
    """485 static spheres under one BVH, a ground sphere and an emitter"""
    host.seed_scene_rng(seed)
    solid = host.SolidTexture
    mats = [host.Lambertian(solid(0.6, 0.6, 0.6)), host.Metal(solid(0.8, 0.7, 0.5), 0.1), host.Lambertian(solid(0.7, 0.2, 0.2))]
    world = host.HittableList()
    world.push(host.BVHNode([host.Sphere(tuple(float(v) for v in c), radius, mats[k % 3]) for k, c in enumerate(centres)], 0.0, 1.0))
    world.push(host.Sphere((4.0, -1000.5, 4.0), 1000.0, mats[0]))
    world.push(host.Rect(1, 0.0, 0.0, 8.0, 8.0, 14.0, host.DiffuseLight(solid(5.0, 5.0, 5.0))))
    return world


def cluster_centres(n=485, seed=4):
    rng = np.random.RandomState(seed)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    cells = np.array([(x, y, z) for y in range(side) for z in range(side) for x in range(side)][:n], np.float64)
    return (cells + rng.uniform(-0.2, 0.2, cells.shape)).astype(np.float32)


def refit_ranges(scene):
    """(first, count) of every refittable item's primitives: the leaves of a BVH item are one run"""
    d, out = scene.desc(), []
    for i in np.flatnonzero(scene.refittable()):
        stack, prims = [d.items[i].first], []
        while stack:
            n = d.nodes[stack.pop()]
            for ref in {n.left, n.right}:
                (prims if ref < 0 else stack).append(ref & 0x0fffffff if ref < 0 else ref)
        out.append((min(prims), max(prims) - min(prims) + 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    host = Host()
    build = (abi.load_rtmi().rtmi_build_hash() or b"").decode()
    lines = []

    def emit(**kw):
        kw["build"] = build
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    env = env_from_sky(2048, 1024)
    centres = cluster_centres()
    worlds = {"final_scene": lambda: scenes.build(host, "final_scene", 640, 360, seed=1)[1],
              "cluster485": lambda: cluster_world(host, centres, 0.25)}
    for name, make in worlds.items():
        scene = host.lower(make()).upload(0)
        scene.attach_light_tree()
        scene.attach_env(env)
        d = scene.desc()
        a = np.ctypeslib.as_array(d.prim_a, shape=(d.n_prims, 4)).copy()
        b = np.ctypeslib.as_array(d.prim_b, shape=(d.n_prims, 4)).copy()
        ranges = refit_ranges(scene)
        prims = sum(c for _, c in ranges)
        emit(what="scene", scene=name, items=int(d.n_items), prims=int(d.n_prims), nodes=int(d.n_nodes), alt_nodes=int(d.n_alt_nodes),
             refittable_items=len(ranges), refittable_prims=prims)
        if not ranges:
            continue
        # the calls alternate between the scene's planes and a copy moved by 1e-3 (a cube's max travels with its min)
        cube = np.array([d.prim_meta[p].type == abi.PRIM_CUBE for p in range(d.n_prims)])
        step = np.float32(1e-3)
        a1, b1 = a.copy(), b.copy()
        a1[:, :3] += step
        a1[:, 3] += np.where(cube, step, np.float32(0))
        b1[:, :2] += np.where(cube, step, np.float32(0))[:, None]
        turn = [0]

        def blocking():
            turn[0] ^= 1
            pa, pb = (a1, b1) if turn[0] else (a, b)
            for f, c in ranges:
                scene.update_prims(f, pa[f:f + c], pb[f:f + c])

        emit(what="update", form="blocking", scene=name, ms=timed(blocking, args.reps, args.warmup))
        ta, tb = torch.tensor(a1, device="cuda"), torch.tensor(b1, device="cuda")
        torch.cuda.synchronize()

        def device():
            for f, c in ranges:
                scene.update_prims(f, ta[f:f + c], tb[f:f + c])

        emit(what="update", form="device, enqueue", scene=name, ms=timed(device, args.reps, args.warmup))
        torch.cuda.synchronize()
        emit(what="update", form="device, to completion", scene=name, ms=timed(device, args.reps, args.warmup, torch.cuda.synchronize))

        def recreate():
            fresh = host.lower(make()).upload(0)
            fresh.attach_light_tree()
            fresh.attach_env(env)

        emit(what="recreate", scene=name, ms=timed(recreate, max(3, args.reps // 4), 1))
        host.free_all()

    # ---- how fast the kept topology goes stale
    nx, ny, ns = 640, 360, 8
    extent = float(centres.max() - centres.min())
    rng = np.random.RandomState(12)
    for fraction in (0.0, 0.01, 0.1, 1.0):
        cam = scenes.set_camera(host, nx, ny, (14.0, 9.0, 20.0), (4.0, 3.0, 4.0), vertical_fov=35.0)  # (free_all frees it too)
        moved = (centres + rng.uniform(-1.0, 1.0, centres.shape) * fraction * extent).astype(np.float32)
        upd = host.lower(cluster_world(host, centres, 0.25)).upload(0)
        old = host.lower(cluster_world(host, centres, 0.25))
        d = old.desc()
        a = np.ctypeslib.as_array(d.prim_a, shape=(d.n_prims, 4)).copy()
        where = {tuple(c.tolist()): k for k, c in enumerate(centres)}
        for p in range(d.n_prims):
            k = where.get(tuple(a[p, :3].tolist()))
            if k is not None:
                a[p, :3] = moved[k]
        (f, c), = refit_ranges(upd)
        upd.update_prims(f, a[f:f + c])
        fresh = host.lower(cluster_world(host, moved, 0.25)).upload(0)
        res = {}
        for label, sc in (("updated", upd), ("fresh", fresh)):
            ms = []
            for k in range(args.warmup + args.reps):
                r = sc.render(cam, nx, ny, ns, seed=3, flags=abi.RTMI_FLAG_FAST_CULL)
                if k >= args.warmup:
                    ms.append(r["stats"]["kernel_ms"])
            res[label] = spread(ms)
        emit(what="staleness", scene="cluster485", moved_by=fraction, image="%dx%dx%d" % (nx, ny, ns), kernel_ms=res,
             ratio=res["updated"]["median"] / res["fresh"]["median"])
        host.free_all()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
