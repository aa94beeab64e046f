"""Times rtmi_temporal_push (include/rtmi_temporal.h) at 1920x1080 against one a-trous iteration of rtmi_denoise, on the
planes of cornell_box and of final_scene under RTMI_FLAG_SKY.  Needs a GPU.  Prints one JSON line per measurement.

    python tools/temporal_timing.py --scenes cornell_box                  # the host calls, by HIP events
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/temporal_timing.py --scenes cornell_box --moving-only
    python tools/temporal_timing.py --scenes cornell_box --kernel-stats DIR   # the kernels of that run; no GPU needed

Host calls: push and denoise are blocking, so the time between two HIP events on the null stream, one recorded before the
call and one after it returns, is the call's whole duration as the device sees it: the host-to-device copies, the kernel
and the copies back.  Two frames from cameras 2 units apart are pushed in turn, so every timed push reprojects (the
standing camera's short cut is timed apart).
Kernels: the entries take host pointers and own their streams, so a kernel alone is not bracketed by events of the
caller; its duration comes from the kernel trace of a separate run of this tool, as DESIGN.md §13 does for the denoiser.
--kernel-stats reads that run's kernel trace (the median over the dispatches of a kernel) and relates the push kernel's
time to the bytes it moves (computed here from the shapes and the surface fraction, which the rows of the first form
carry) and to the HBM rates of the MI355X.
"""
import argparse
import ctypes as C
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC = 8.0e12       # bytes/s, the data sheet
HBM_MEASURED = 6.29e12  # bytes/s, a float4 copy on this chip


def push_bytes(n, surface_fraction, with_se):
    """The bytes one push kernel must move for n pixels, each plane and record once (the four taps of a pixel are its
    neighbours' records and come from cache): the input planes, one copy of the history read, the other written, the
    four output planes.  A pixel without a surface reads no albedo and no history."""
    rec = 48 if with_se else 32
    inputs = 12 + 12 + 4 + (12 if with_se else 0)  # linear, normal, depth, stderr
    outputs = 12 + (12 if with_se else 0) + 4 + 8
    surface = inputs + 12 + rec + rec + outputs      # + albedo, history in, history out
    other = inputs + rec + outputs
    return int(n * (surface_fraction * surface + (1.0 - surface_fraction) * other))


class Events:
    """hipEventRecord on the null stream around a blocking call."""

    def __init__(self):
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


def _stats(times):
    return {"call_ms_median": round(float(np.median(times)), 3), "call_ms_min": round(min(times), 3),
            "call_ms_max": round(max(times), 3)}


def measure(args):
    from raytracing_rust_amd import Host, Temporal, abi, denoise, scenes

    if abi.load_rtmi().rtmi_device_count() < 1:
        sys.exit("temporal_timing.py needs a GPU")
    host = Host()
    ev = Events()
    nx, ny, ns = args.nx, args.ny, args.ns
    for name in args.scenes:
        flags = abi.RTMI_FLAG_FAST_CULL | (abi.RTMI_FLAG_SKY if name == "final_scene" else 0)
        _, world = scenes.build(host, name, nx, ny, seed=1)
        sc = host.lower(world).upload(0)
        look_from, look_at, vfov = scenes.SCENES[name][1:]
        frames = []
        for j in range(2):
            cam = scenes.set_camera(host, nx, ny, (look_from[0] + 2.0 * j,) + tuple(look_from[1:]), look_at, vertical_fov=vfov)
            noisy = sc.render_adaptive(cam, nx, ny, ns, min_spp=ns, step_spp=1, seed=42 + j, flags=flags)
            ft = sc.render_features(cam, nx, ny, ns, seed=42 + j, flags=flags)
            frames.append((cam.lower(), noisy["linear"], ft["albedo"], ft["normal"], ft["depth"], noisy["stderr"]))
        surface = float(np.isfinite(frames[1][4]).mean())
        base = {"scene": name, "nx": nx, "ny": ny, "ns": ns, "surface_fraction": round(surface, 4), "reps": args.reps}
        for with_se in (True, False):
            for moving in ((True,) if args.moving_only else (True, False)):
                t = Temporal(nx, ny)
                k = [0]

                def call():
                    cam, lin, alb, nrm, dep, se = frames[k[0] % 2 if moving else 0]
                    k[0] += 1
                    return t.push(cam, lin, alb, nrm, dep, stderr=se if with_se else None, motion=True)

                for _ in range(args.warmup + 1):  # the first push has no history
                    out = call()
                times = [ev.time_ms(call)[0] for _ in range(args.reps)]
                row = dict(base, what="push", stderr=with_se, camera="moving" if moving else "standing",
                           bytes_copied=nx * ny * ((52 if with_se else 40) + (36 if with_se else 24)),
                           kernel_bytes=push_bytes(nx * ny, surface, with_se),
                           mean_history=round(float(out["history"][np.isfinite(frames[0][4])].mean()), 2), **_stats(times))
                print(json.dumps(row), flush=True)
                t.close()
        cam, lin, alb, nrm, dep, se = frames[1]
        for it in (1, 2, 5):
            call = lambda: denoise(lin, alb, nrm, dep, stderr=se, iterations=it)  # noqa: E731
            for _ in range(args.warmup):
                call()
            times = [ev.time_ms(call)[0] for _ in range(args.reps)]
            print(json.dumps(dict(base, what="denoise", iterations=it, stderr=True, **_stats(times))), flush=True)
        host.free_all()


def _durations(directory):
    """{kernel name: [ns per dispatch]} from the run's kernel trace; without one, the (mean, min, max, calls) of its
    statistics table"""
    traces = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if len(traces) == 1:
        rows = list(csv.DictReader(open(traces[0])))
        if rows and {"Kernel_Name", "Start_Timestamp", "End_Timestamp"} <= set(rows[0]):
            out = {}
            for r in rows:
                out.setdefault(r["Kernel_Name"], []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
            return {k: {"calls": len(v), "kernel_us_median": round(float(np.median(v)) / 1e3, 2),
                        "kernel_us_min": round(min(v) / 1e3, 2), "kernel_us_max": round(max(v) / 1e3, 2)} for k, v in out.items()}
    stats = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if len(stats) != 1:
        sys.exit("expected one *kernel_trace.csv or *kernel_stats.csv under %s" % directory)
    return {r["Name"]: {"calls": int(r["Calls"]), "kernel_us_mean": round(float(r["AverageNs"]) / 1e3, 2),
                        "kernel_us_min": round(float(r["MinNs"]) / 1e3, 2), "kernel_us_max": round(float(r["MaxNs"]) / 1e3, 2)}
            for r in csv.DictReader(open(stats[0]))}


def kernel_stats(args):
    """the kernels of a rocprofv3 --kernel-trace --stats run of measure(), beside the bytes of its rows"""
    rows = {}
    if args.rows:
        for line in open(args.rows):
            line = line.strip()
            if line.startswith("{"):
                r = json.loads(line)
                if r.get("what") == "push" and r.get("camera") == "moving":
                    rows[r["stderr"]] = r
    for name, d in sorted(_durations(args.kernel_stats).items()):
        short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if "rtmi_temporal_push_kernel" in name:
            with_se = "<true>" in name
            row = dict(what="push_kernel", scene=args.scenes[0], stderr=with_se, **d)
            if with_se in rows:
                b, s = rows[with_se]["kernel_bytes"], d.get("kernel_us_median", d.get("kernel_us_mean")) * 1e-6
                row.update(kernel_bytes=b, bytes_per_pixel=round(b / (rows[with_se]["nx"] * rows[with_se]["ny"]), 1),
                           tb_per_s=round(b / s / 1e12, 3), share_of_hbm_spec=round(b / s / HBM_SPEC, 3),
                           share_of_hbm_measured=round(b / s / HBM_MEASURED, 3))
        elif "rtmi_denoise_" in name and "_kernel" in name:
            row = dict(what=short, scene=args.scenes[0], **d)
        else:
            continue
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scenes", nargs="+", default=["cornell_box", "final_scene"])
    ap.add_argument("--nx", type=int, default=1920)
    ap.add_argument("--ny", type=int, default=1080)
    ap.add_argument("--ns", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--moving-only", action="store_true", help="skip the standing-camera pushes (for the profiled run)")
    ap.add_argument("--kernel-stats", metavar="DIR", help="read the kernel trace statistics of a profiled run instead of measuring")
    ap.add_argument("--rows", metavar="JSONL", help="with --kernel-stats: the rows of the run, for the bytes a push moves")
    args = ap.parse_args()
    kernel_stats(args) if args.kernel_stats else measure(args)


if __name__ == "__main__":
    main()
