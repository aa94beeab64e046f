"""Times environment lighting (include/rtmi_env.h) against the plain render with RTMI_FLAG_SKY, and measures the noise of
its two estimators.  Needs a GPU.  Prints one JSON line per (scene, map, mode) and one per (scene, map) with the figure of
merit.

    python tools/env_timing.py                      # random_spheres 1920x1080x64 under the sky map and the sun map
    python tools/env_timing.py --ns 16 --repeats 2  # a shorter run

Every call is blocking; its time is the span between two HIP events on the null stream around it (tools/denoise_timing.py).
One warm-up call per mode, then the modes alternate `repeats` times and the median is reported.  render_sky runs the
default (cooperative) kernel, render_sky_sync the per-lane kernel that render_env is built on.  sigma = the root mean
square of render_env's per-pixel standard errors (Welford, include/rtmi_adaptive.h); under a sun, nee=0's estimate is
low wherever a pixel's samples missed the sun.  Figure of merit: t_nee * (sigma_nee /
sigma_bsdf)^2 / t_bsdf, the time nee=1 needs for nee=0's noise relative to nee=0's time (< 1: NEE is worth it).
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
from raytracing_rust_amd import Host, abi, env_from_sky, scenes  # noqa: E402
import env_ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, default=64)
    ap.add_argument("--nx", type=int, default=1920)
    ap.add_argument("--ny", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    host = Host()
    ev = Events()
    fc = abi.RTMI_FLAG_FAST_CULL
    nx, ny, ns = args.nx, args.ny, args.ns
    cam, world = scenes.build(host, "random_spheres", nx, ny, seed=1)
    sc = host.lower(world).upload(0, nee=True)
    for mapname, m in (("sky", env_from_sky(2048, 1024)), ("sun", env_ref.sun_map())):
        sc.attach_env(m)
        modes = {"render_sky": lambda: sc.render(cam, nx, ny, ns, seed=42, flags=fc | abi.RTMI_FLAG_SKY),
                 "render_sky_sync": lambda: sc.render(cam, nx, ny, ns, seed=42, flags=fc | abi.RTMI_FLAG_SKY | abi.RTMI_FLAG_SYNC),
                 "render_env_nee0": lambda: sc.render_env(cam, nx, ny, ns, nee=False, seed=42, flags=fc),
                 "render_env_nee1": lambda: sc.render_env(cam, nx, ny, ns, nee=True, seed=42, flags=fc)}
        times = {k: [] for k in modes}
        for fn in modes.values():
            fn()  # warm-up
        for _ in range(args.repeats):
            for k, fn in modes.items():
                times[k].append(ev.time_ms(fn)[0])
        b = sc.render_env(cam, nx, ny, ns, nee=False, seed=42, flags=fc)
        n = sc.render_env(cam, nx, ny, ns, nee=True, seed=42, flags=fc)
        sig_b = float(np.sqrt(np.mean(b["stderr"].astype(np.float64) ** 2)))
        sig_n = float(np.sqrt(np.mean(n["stderr"].astype(np.float64) ** 2)))
        med = {k: float(np.median(t)) for k, t in times.items()}
        for k in modes:
            print(json.dumps({"scene": "random_spheres", "map": mapname, "nx": nx, "ny": ny, "ns": ns, "mode": k,
                              "seconds": med[k] / 1e3, "msamples_per_s": nx * ny * ns / (med[k] / 1e3) / 1e6,
                              "repeats_ms": times[k]}), flush=True)
        print(json.dumps({"scene": "random_spheres", "map": mapname, "sigma_nee1": sig_n, "sigma_nee0": sig_b,
                          "stderr_ratio": sig_n / sig_b, "time_ratio": med["render_env_nee1"] / med["render_env_nee0"],
                          "time_to_equal_noise": med["render_env_nee1"] * (sig_n / sig_b) ** 2 / med["render_env_nee0"]}),
              flush=True)
    host.free_all()


if __name__ == "__main__":
    main()
