"""Times rtmi_denoise (include/rtmi_denoise.h) at 1920x1080 on lit_final_scene's planes, against the render it follows,
and measures the denoiser's quality against a converged render.  Needs a GPU.  Prints one JSON line per measurement.

    python tools/denoise_timing.py                 # timing: render_adaptive + render_features, then the denoise calls
    python tools/denoise_timing.py --quality       # display-domain RMSE, noisy and denoised, against a 4096-spp render

Timing: the calls are blocking, so the time between two HIP events on the null stream, one recorded before the call and
one after it returns, is the call's whole duration as the device sees it: host-to-device copies, the three kernels and
the copies back.  Kernel times per launch come from a rocprofv3 --kernel-trace --stats run of this tool.
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

from raytracing_rust_amd import Host, abi, denoise, scenes  # noqa: E402
import scenes_extra  # noqa: E402


class Events:
    """hipEventRecord on the null stream around a blocking call."""

    def __init__(self):
        abi.load_rtmi()
        self.hip = C.CDLL("libamdhip64.so")
        self.a, self.b = C.c_void_p(), C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(self.a)) == 0 and self.hip.hipEventCreate(C.byref(self.b)) == 0

    def time_ms(self, fn):
        assert self.hip.hipEventRecord(self.a, None) == 0
        out = fn()
        assert self.hip.hipEventRecord(self.b, None) == 0 and self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return ms.value, out


def _build(host, name, nx, ny):
    if name in scenes.SCENES:
        return scenes.build(host, name, nx, ny, seed=1)
    return scenes_extra.build(host, name, nx, ny, seed=1)


def timing(args):
    host = Host()
    nx, ny, ns = args.nx, args.ny, args.ns
    cam, world = _build(host, args.scene, nx, ny)
    sc = host.lower(world).upload(0)
    ev = Events()
    fc = abi.RTMI_FLAG_FAST_CULL
    sc.render(cam, nx, ny, ns, seed=42, flags=fc)  # warm-up
    render_ms, r = ev.time_ms(lambda: sc.render(cam, nx, ny, ns, seed=42, flags=fc))
    noisy = sc.render_adaptive(cam, nx, ny, ns, min_spp=ns, step_spp=1, seed=42, flags=fc)
    ft = sc.render_features(cam, nx, ny, ns, seed=42, flags=fc)
    planes = (noisy["linear"], ft["albedo"], ft["normal"], ft["depth"])
    surface = float(np.isfinite(ft["depth"]).mean())
    print(json.dumps({"what": "render", "scene": args.scene, "nx": nx, "ny": ny, "ns": ns, "call_ms": round(render_ms, 3),
                      "kernel_ms": round(r["stats"]["kernel_ms"], 3), "surface_fraction": round(surface, 4)}), flush=True)
    for it in args.iterations:
        for se in (noisy["stderr"], None):
            call = lambda: denoise(*planes, stderr=se, iterations=it)  # noqa: E731
            for _ in range(args.warmup):
                call()
            times = []
            for _ in range(args.reps):
                ms, _out = ev.time_ms(call)
                times.append(ms)
            t0 = time.perf_counter()
            call()
            wall = (time.perf_counter() - t0) * 1e3
            print(json.dumps({"what": "denoise", "iterations": it, "stderr": se is not None, "reps": args.reps,
                              "call_ms_median": round(float(np.median(times)), 3), "call_ms_min": round(min(times), 3),
                              "call_ms_max": round(max(times), 3), "wall_ms": round(wall, 3),
                              "vs_render_call": round(float(np.median(times)) / render_ms, 4)}), flush=True)
    host.free_all()


def display_rmse(a, b):
    da = np.clip(np.sqrt(np.maximum(a.astype(np.float64), 0.0)), 0.0, 1.0)
    db = np.clip(np.sqrt(np.maximum(b.astype(np.float64), 0.0)), 0.0, 1.0)
    return float(np.sqrt(np.mean((da - db) ** 2)))


def quality(args):
    host = Host()
    fc = abi.RTMI_FLAG_FAST_CULL
    n = 128
    for name in args.quality_scenes:
        cam, world = _build(host, name, n, n)
        sc = host.lower(world).upload(0)
        truth = sc.render(cam, n, n, 4096, seed=7, flags=fc)["linear"]
        for ns in (16, 64):
            got = sc.render_denoised(cam, n, n, ns, seed=42, flags=fc)
            noisy = display_rmse(got["noisy"]["linear"], truth)
            den = display_rmse(got["linear"], truth)
            row = {"what": "quality", "scene": name, "size": n, "ns": ns, "truth_mean": round(float(truth.mean()), 5),
                   "truth_max": round(float(truth.max()), 5), "noisy_rmse": round(noisy, 5), "denoised_rmse": round(den, 5),
                   "ratio": round(den / noisy, 4) if noisy > 0 else None}
            if noisy == 0:
                print(json.dumps(row), flush=True)
                continue
            for it in args.sweep_iterations:
                for sl in args.sweep_sigma_l:
                    for npow in args.sweep_normal_power:
                        f = sc.render_features(cam, n, n, ns, seed=42, flags=fc)
                        o = denoise(got["noisy"]["linear"], f["albedo"], f["normal"], f["depth"], stderr=got["noisy"]["stderr"],
                                    iterations=it, sigma_l=sl, normal_power=npow)
                        row["it%d_sl%g_np%d" % (it, sl, npow)] = round(display_rmse(o["linear"], truth) / noisy, 4)
            print(json.dumps(row), flush=True)
        host.free_all()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scene", default="lit_final_scene")
    ap.add_argument("--nx", type=int, default=1920)
    ap.add_argument("--ny", type=int, default=1080)
    ap.add_argument("--ns", type=int, default=64)
    ap.add_argument("--iterations", type=int, nargs="+", default=[5])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--quality-scenes", nargs="+", default=["cornell_box", "cornell_smoke", "cornell_smoke_corrected", "lit_final_scene"])
    ap.add_argument("--sweep-iterations", type=int, nargs="*", default=[])
    ap.add_argument("--sweep-sigma-l", type=float, nargs="*", default=[4.0])
    ap.add_argument("--sweep-normal-power", type=int, nargs="*", default=[128])
    args = ap.parse_args()
    if abi.load_rtmi().rtmi_device_count() < 1:
        sys.exit("denoise_timing.py needs a GPU")
    quality(args) if args.quality else timing(args)


if __name__ == "__main__":
    main()
