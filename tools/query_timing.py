"""Times the ray queries (include/rtmi_query.h): trace and occluded on the device forms, against the only other route to
first hits, render_features(ns=1).  Needs a GPU and torch.  Prints one JSON line per (scene, ray set, flags, query) and one
per scene for the yardstick.

    python tools/query_timing.py                         # final_scene, random_spheres, cornell_box at 1920x1080
    python tools/query_timing.py --nx 640 --ny 360 --runs 3 --inner 2   # a shorter run

Ray sets: the nx*ny pixel-centre rays of the scene's camera (primary_rays), and as many bounce rays — from the hit points
of the primary rays (repeated in order where some missed), along standard-normal directions, t_min = 0.001.  A query is
enqueued `inner` times on torch's current stream between two events of that stream; after one warm-up window the median
of `runs` windows is reported, the four (flags, query) variants of a ray set alternating.  The yardstick is the kernel_ms
that render_features(ns=1) reports at the same size; it also samples the pixel and the lens, evaluates the albedo textures
and is followed by a resolve that is not counted.  Kernel times per launch come from a separate
rocprofv3 --kernel-trace --stats run of this tool.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raytracing_rust_amd import Host, abi, primary_rays, scenes  # noqa: E402

SCENES = ["final_scene", "random_spheres", "cornell_box"]


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=1920)
    ap.add_argument("--ny", type=int, default=1080)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--scenes", default=",".join(SCENES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("query_timing needs a GPU")
    dev = torch.device("cuda", 0)
    host = Host()
    nx, ny = args.nx, args.ny
    n = nx * ny
    for name in args.scenes.split(","):
        cam, world = scenes.build(host, name, nx, ny, seed=1)
        sc = host.lower(world).upload(0)
        feat = [sc.render_features(cam, nx, ny, 1, seed=42, flags=abi.RTMI_FLAG_FAST_CULL)["stats"]["kernel_ms"] for _ in range(4)]
        yard_ms = float(np.median(feat[1:]))  # the first call warms up
        print(json.dumps({"scene": name, "nx": nx, "ny": ny, "yardstick": "render_features(ns=1) kernel_ms", "ms": yard_ms,
                          "mrays_per_s": n / yard_ms / 1e3, "calls_ms": feat}), flush=True)
        o, d = (torch.from_numpy(a.reshape(-1, 3)).to(dev) for a in primary_rays(cam, nx, ny))
        first = sc.trace(o, d)
        hits = torch.nonzero(first["hit"]).flatten()
        gen = torch.Generator(device=dev)
        gen.manual_seed(7)
        bo = first["p"][hits[torch.arange(n, device=dev) % hits.numel()]].contiguous()
        bd = torch.randn((n, 3), generator=gen, device=dev, dtype=torch.float32)
        for set_name, (ro, rd) in (("primary", (o, d)), ("bounce", (bo, bd))):
            variants = {(q, f): (lambda q=q, f=f: getattr(sc, q)(ro, rd, flags=f))
                        for f in (abi.RTMI_FLAG_FAST_CULL, 0) for q in ("trace", "occluded")}
            times = {k: [] for k in variants}
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for run in range(args.runs + 1):
                for k, fn in variants.items():
                    a.record()
                    for _ in range(args.inner):
                        fn()
                    b.record()
                    b.synchronize()
                    if run:  # window 0 warms up
                        times[k].append(a.elapsed_time(b) / args.inner)
            n_hit = int(sc.occluded(ro, rd).sum().item())
            for (q, f), t in times.items():
                ms = float(np.median(t))
                print(json.dumps({"scene": name, "rays": set_name, "n": n, "hit_fraction": n_hit / n, "query": q,
                                  "flags": "FAST_CULL" if f else "0", "ms": ms, "mrays_per_s": n / ms / 1e3,
                                  "speed_vs_yardstick": yard_ms / ms, "windows_ms": t}), flush=True)
        host.free_all()


if __name__ == "__main__":
    main()
