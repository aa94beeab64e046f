"""Times the hemisphere gathers (include/rtmi_gather.h) on the device form against the radiance query on the same rays.
Needs a GPU and torch.  Prints one JSON line per row.

    python tools/gather_timing.py                                   # every scene at 1920x1080 points, spp 16
    python tools/gather_timing.py --nx 640 --ny 360 --runs 3        # a shorter run
    python tools/gather_timing.py --irradiance                      # also Scene.irradiance end to end on the same input

Workload: the first hits of the nx*ny pixel-centre rays of the scene's camera (surface hits only, repeated cyclically up to
nx*ny points), normals turned against the ray, `spp` cosine-distributed directions each: final_scene under RTMI_FLAG_SKY
(plain), lit_final_scene (NEE) and cornell_box (NEE).
Gather: rtmi_gather_device with value and stderr, scratch for the whole batch (one slab), between two events of torch's
current stream; after one warm-up call the median of `runs` calls, with their least and greatest.  That window holds the
counter's memset, the path kernel and the resolve.
Yardstick: rtmi_radiance_device alone on the same first rays, already resident on the device: the n*spp rays
(points[i], rtmi_gather_directions[i, s]) in item order with spp = 1, mean and stderr asked for, timed the same way.  Its
paths start along the gather's directions and continue on other Philox streams: the same work statistically, not bit for
bit.  `path_only_ms` is the yardstick without its resolve; `sphere_ms` / `sphere_sh_ms` the SPHERE gather without and with
the SH projection (other directions: compare them with each other).
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

from raytracing_rust_amd import Host, abi, gather_directions, primary_rays  # noqa: E402

FC, SKY = abi.RTMI_FLAG_FAST_CULL, abi.RTMI_FLAG_SKY
ROWS = [("final_scene", FC | SKY, "plain"), ("lit_final_scene", FC, "nee"), ("cornell_box", FC, "nee")]
SEED = 42


def timed(runs, call):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for run in range(runs + 1):
        a.record()
        call()
        b.record()
        b.synchronize()
        if run:  # call 0 warms up
            times.append(a.elapsed_time(b))
    return {"ms": float(np.median(times)), "min_ms": min(times), "max_ms": max(times), "calls_ms": times}


def main():
    import torch

    import scenes_extra

    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=1920)
    ap.add_argument("--ny", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--scenes", default=",".join(r[0] for r in ROWS))
    ap.add_argument("--irradiance", action="store_true", help="also time Scene.irradiance end to end (host directions, n*spp rays)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gather_timing needs a GPU")
    dev = torch.device("cuda", 0)
    host = Host()
    nx, ny, spp = args.nx, args.ny, args.spp
    n = nx * ny
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for name, flags, est in ROWS:
        if name not in args.scenes.split(","):
            continue
        cam, world = scenes_extra.build(host, name, nx, ny, seed=1)
        sc = host.lower(world).upload(0, nee=est == "nee")
        o, d = (torch.from_numpy(a.reshape(-1, 3)).to(dev) for a in primary_rays(cam, nx, ny))
        first = sc.trace(o, d)
        nrm = first["normal"]
        nrm = torch.where(((nrm * d).sum(dim=1) > 0)[:, None], -nrm, nrm)
        keep = torch.nonzero(first["hit"] & (nrm != 0).any(dim=1)).flatten()
        idx = keep[torch.arange(n, device=dev) % keep.numel()]
        pts, nrm = first["p"][idx].contiguous(), nrm[idx].contiguous()
        del first, o, d
        est_id = abi.ROULETTE_ESTIMATORS[est]
        value, stderr = (torch.empty((n, 3), dtype=torch.float32, device=dev) for _ in range(2))
        sh = torch.empty((n, 27), dtype=torch.float32, device=dev)
        samples = torch.empty((n * spp, 3), dtype=torch.float32, device=dev)  # the gather's scratch, the yardstick's d_samples
        row = {"scene": name, "estimator": est, "n": n, "spp": spp, "surface_points": int(keep.numel())}

        def gather(mode, with_sh=False):
            p = abi.GatherParams(n, spp, mode, est_id, flags, 50, 0.001, SEED, 0, 0, 0, 0.5)
            host._check(host.lib.rth_gather_device(sc.h, C.byref(p), ptr(pts), ptr(nrm), None, ptr(value), ptr(stderr),
                                                   ptr(sh) if with_sh else None, ptr(samples), C.c_uint64(n * spp * 12), stream))

        row["gather"] = timed(args.runs, lambda: gather(abi.RTMI_GATHER_COSINE))
        row["mean_irradiance"] = float(value.mean().item())
        row["sphere_ms"] = timed(args.runs, lambda: gather(abi.RTMI_GATHER_SPHERE))["ms"]
        row["sphere_sh_ms"] = timed(args.runs, lambda: gather(abi.RTMI_GATHER_SPHERE, True))["ms"]

        # the yardstick's rays: the host's directions, uploaded once
        pts_h, nrm_h = pts.cpu().numpy(), nrm.cpu().numpy()
        t0 = time.perf_counter()
        dirs = gather_directions(nrm_h, spp, seed=SEED)
        row["host_directions_s"] = time.perf_counter() - t0
        rays = torch.empty((n * spp, 8), dtype=torch.float32, device=dev)
        rays[:, 0:3] = pts.repeat_interleave(spp, dim=0)
        rays[:, 4:7] = torch.from_numpy(dirs.reshape(-1, 3)).to(dev)
        rays[:, 3], rays[:, 7] = 0.001, float("inf")
        del dirs
        mean1, se1 = (torch.empty((n * spp, 3), dtype=torch.float32, device=dev) for _ in range(2))

        def radiance(resolve):
            p = abi.RadianceParams(n * spp, 1, est_id, flags, 50, 0.001, SEED, 0, 0, 0, 0.5)
            host._check(host.lib.rth_radiance_device(sc.h, C.byref(p), ptr(rays), None, ptr(mean1) if resolve else None,
                                                     ptr(se1) if resolve else None, ptr(samples), stream))

        row["yardstick"] = timed(args.runs, lambda: radiance(True))
        row["mean_radiance_times_pi"] = float(mean1.mean().item()) * float(np.pi)
        row["path_only_ms"] = timed(args.runs, lambda: radiance(False))["ms"]
        row["gather_vs_yardstick"] = row["yardstick"]["ms"] / row["gather"]["ms"]
        row["mpaths_per_s"] = n * spp / row["gather"]["ms"] / 1e3
        del rays, mean1, se1
        torch.cuda.empty_cache()
        if args.irradiance:
            t0 = time.perf_counter()
            r = sc.irradiance(pts_h, nrm_h, spp, seed=SEED, estimator=est, flags=flags)
            row["scene_irradiance_s"] = time.perf_counter() - t0
            row["scene_irradiance_mean"] = float(r["irradiance"].mean())
            t0 = time.perf_counter()
            r = sc.gather(pts_h, nrm_h, spp=spp, estimator=est, flags=flags, seed=SEED)
            row["scene_gather_s"] = time.perf_counter() - t0
        print(json.dumps(row), flush=True)
        del pts, nrm, value, stderr, sh, samples
        host.free_all()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
