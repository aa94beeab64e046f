"""Times the radiance queries (include/rtmi_radiance.h) on the device form, against the one-shot render of the same
estimator and scene on the per-lane kernel.  Needs a GPU and torch.  Prints one JSON line per row.

    python tools/radiance_timing.py                                   # every scene at 1920x1080, spp 16
    python tools/radiance_timing.py --nx 640 --ny 360 --runs 3        # a shorter run
    python tools/radiance_timing.py --chunks 256,1024,4096            # the chunk size of the refill, per row

Workload: the nx*ny pixel-centre rays of the scene's camera (primary_rays) with `spp` paths each, on final_scene under
RTMI_FLAG_SKY, lit_final_scene, random_spheres under a sky map and cornell_box, for every estimator the scene supports;
and for each scene's first estimator the incoherent bounce set of tools/query_timing.py (from the hit points of the primary
rays along standard-normal directions).  A call is enqueued on torch's current stream between two events of that stream;
after one warm-up call the median of `runs` calls is reported.  That window holds the counter's memset, the path kernel
and the resolve kernel.
Yardstick: kernel_ms of the one-shot render (render with RTMI_FLAG_SYNC, render_nee, render_env; coop=False: the per-lane
kernel) at nx x ny, ns = spp: the same number of paths from nearly the same rays (it jitters the pixel and samples the
lens and the shutter), resolve not counted.  --chunks sets RTMI_RADIANCE_CHUNK, the cap of the chunk a wavefront takes
from the counter (default: RTMI_RADIANCE_CHUNK of csrc/rtmi_radiance_launch.hpp).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from raytracing_rust_amd import Host, abi, env_from_sky, primary_rays, scenes  # noqa: E402

FC, SKY = abi.RTMI_FLAG_FAST_CULL, abi.RTMI_FLAG_SKY
# scene: (builder module, device flags, map, estimators)
ROWS = [("final_scene", FC | SKY, False, ["plain"]), ("lit_final_scene", FC, False, ["plain", "nee"]),
        ("random_spheres", FC, True, ["env", "env_nee"]), ("cornell_box", FC, False, ["plain", "nee"])]


def yardstick(sc, cam, nx, ny, spp, est, flags):
    kw = dict(seed=42, flags=flags)
    if est == "plain":
        call = lambda: sc.render(cam, nx, ny, spp, seed=42, flags=flags | abi.RTMI_FLAG_SYNC)  # noqa: E731
    elif est == "nee":
        call = lambda: sc.render_nee(cam, nx, ny, spp, coop=False, **kw)  # noqa: E731
    else:
        call = lambda: sc.render_env(cam, nx, ny, spp, nee=est == "env_nee", coop=False, **kw)  # noqa: E731
    ms = [call()["stats"]["kernel_ms"] for _ in range(4)]
    return float(np.median(ms[1:])), ms  # the first call warms up


def main():
    import torch

    import scenes_extra

    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=1920)
    ap.add_argument("--ny", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--scenes", default=",".join(r[0] for r in ROWS))
    ap.add_argument("--chunks", default="", help="comma-separated caps of the refill chunk (RTMI_RADIANCE_CHUNK); empty: the default")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("radiance_timing needs a GPU")
    dev = torch.device("cuda", 0)
    host = Host()
    nx, ny, spp = args.nx, args.ny, args.spp
    n = nx * ny
    chunks = [c for c in args.chunks.split(",") if c] or [""]
    for name, flags, with_map, estimators in ROWS:
        if name not in args.scenes.split(","):
            continue
        cam, world = scenes_extra.build(host, name, nx, ny, seed=1)
        sc = host.lower(world).upload(0)
        if with_map:
            sc.attach_env(env_from_sky(2048, 1024))
        o, d = (torch.from_numpy(a.reshape(-1, 3)).to(dev) for a in primary_rays(cam, nx, ny))
        first = sc.trace(o, d)
        hits = torch.nonzero(first["hit"]).flatten()
        gen = torch.Generator(device=dev)
        gen.manual_seed(7)
        bo = first["p"][hits[torch.arange(n, device=dev) % hits.numel()]].contiguous()
        bd = torch.randn((n, 3), generator=gen, device=dev, dtype=torch.float32)
        for k, est in enumerate(estimators):
            yard_ms, yard_all = yardstick(sc, cam, nx, ny, spp, est, flags)
            print(json.dumps({"scene": name, "estimator": est, "nx": nx, "ny": ny, "spp": spp, "yardstick": "one-shot render, per-lane kernel_ms",
                              "ms": yard_ms, "mpaths_per_s": n * spp / yard_ms / 1e3, "calls_ms": yard_all}), flush=True)
            for set_name, (ro, rd) in (("primary", (o, d)), ("bounce", (bo, bd)))[:2 if k == 0 else 1]:
                for chunk in chunks:
                    if chunk:
                        os.environ["RTMI_RADIANCE_CHUNK"] = chunk
                    else:
                        os.environ.pop("RTMI_RADIANCE_CHUNK", None)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    times = []
                    for run in range(args.runs + 1):
                        a.record()
                        r = sc.radiance(ro, rd, spp=spp, estimator=est, seed=42, flags=flags)
                        b.record()
                        b.synchronize()
                        if run:  # call 0 warms up
                            times.append(a.elapsed_time(b))
                        mean = float(r["mean"].mean().item())
                        del r
                    ms = float(np.median(times))
                    print(json.dumps({"scene": name, "estimator": est, "rays": set_name, "n": n, "spp": spp, "chunk": chunk or "default",
                                      "ms": ms, "mpaths_per_s": n * spp / ms / 1e3, "speed_vs_yardstick": yard_ms / ms,
                                      "mean_radiance": mean, "calls_ms": times}), flush=True)
        os.environ.pop("RTMI_RADIANCE_CHUNK", None)
        host.free_all()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
