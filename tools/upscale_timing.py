"""Times an upscaled frame (Upscaler.render, include/rtmi_upscale.h) against the full-resolution frame it stands in for
(Frame.render, include/rtmi_frame.h).  Needs a GPU.

    python tools/upscale_timing.py                                  # rows to stdout and to profiles/upscale/timing.jsonl
    python tools/upscale_timing.py --scenes cornell_box --repeats 4 --out /dev/null
    python tools/upscale_timing.py --kernel-ab 12                   # the direct and the staged kernel alternating

One process: per scene a full-resolution Frame and one Upscaler per scale (2 and 1.5) on one uploaded scene, 4 spp NEE,
out="torch" (no plane passes through the host).  Every handle makes two warm-up calls (code objects, the scene's scratch at
that shape, torch's context), then `--repeats` calls with the handles alternating.  The camera moves between the calls
(look_from.x + 2 per frame, the path of tests/test_gpu_frame.py), so the history reprojects.  A call's time is the host
clock around it: every call timed here is blocking and ends in a device synchronise.  Rows hold the median, the range and
every repeat; the last row per scene has the ratios of the medians.  The timed region is the whole Python call, as a frame
loop pays it: the ctypes marshalling and torch.empty of the output tensors included (two for a Frame, three for an Upscaler,
served by torch's caching allocator after the warm-up).  The frame code is the parent commit's (no kernel or
entry of it changed), so the Frame rows are the parent's figures, measured in the same process and minute.

The kernels' own durations come from a run of this tool under `rocprofv3 --kernel-trace --stats`, in a run of its own
(profiles/upscale/kernel_stats.csv): a traced run's host times are not written to the timing file (`--out /dev/null`).
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"cornell_box": (800, 800, (278.0, 278.0, -800.0), (278.0, 278.0, 0.0), 40.0),
         "lit_final_scene": (1920, 1080, (478.0, 278.0, -600.0), (278.0, 278.0, 0.0), 40.0)}
SCALES = (2.0, 1.5)


def median(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def kernel_ab(pairs):
    """The two variants of the reconstruction kernel in turn in one process (RTMI_UPSCALE_VARIANT is read at every launch),
    on random planes with a depth edge; HIP events around each launch for a figure without a trace."""
    sys.path.insert(0, HERE)
    import torch

    from raytracing_rust_amd import upscale

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    nx, ny = 1920, 1080
    for lx, ly in ((960, 540), (1280, 720)):
        def planes(w, h):
            d = torch.where(torch.arange(w, device=dev)[None, :] * h < torch.arange(h, device=dev)[:, None] * w, 2.0, 9.0).float()
            n = torch.nn.functional.normalize(torch.rand((h, w, 3), generator=g, device=dev) + 0.5, dim=2)
            return torch.rand((h, w, 3), generator=g, device=dev), n.contiguous(), d.contiguous()

        a_lo, n_lo, z_lo = planes(lx, ly)
        a, n, z = planes(nx, ny)
        lin = torch.rand((ly, lx, 3), generator=g, device=dev)
        times, first = {"direct": [], "staged": []}, {}
        for k in range(pairs + 2):
            for v in times:
                os.environ["RTMI_UPSCALE_VARIANT"] = v
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = upscale(lin, a_lo, n_lo, z_lo, a, n, z)
                e1.record()
                e1.synchronize()
                if k >= 2:
                    times[v].append(e0.elapsed_time(e1) * 1e3)
                if k == 0:
                    first[v] = out
        assert all(torch.equal(first["direct"][p], first["staged"][p]) for p in ("linear", "rgb8", "cls"))
        for v in ("direct", "staged"):
            print(json.dumps({"kernel_ab": v, "low": [lx, ly], "full": [nx, ny], "median_us": median(times[v]), "min_us": min(times[v]),
                              "max_us": max(times[v]), "pairs": pairs}), flush=True)
    os.environ.pop("RTMI_UPSCALE_VARIANT", None)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(CASES))
    ap.add_argument("--ns", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "upscale", "timing.jsonl"))
    ap.add_argument("--kernel-ab", type=int, default=0, metavar="N",
                    help="instead: N alternating pairs of the direct and the staged kernel on device tensors, 1920x1080 from 960x540 "
                         "and from 1280x720, for a kernel-trace run (the two kernels have different names in the trace)")
    args = ap.parse_args()
    if args.kernel_ab:
        return kernel_ab(args.kernel_ab)
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import scenes_extra
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

        handles = {"frame_full": sc.frame(nx, ny, estimator="nee", flags=fc)}
        sizes = {"frame_full": (nx, ny)}
        for s in SCALES:
            h = sc.upscaler(nx, ny, scale=s, estimator="nee", flags=fc)
            handles["upscaler_x%g" % s] = h
            sizes["upscaler_x%g" % s] = (h.lx, h.ly)
        times = {m: [] for m in handles}
        for k in range(2):  # warm-up, every shape
            for h in handles.values():
                h.render(cam(k), args.ns, seed=k, out="torch")
        for k in range(2, args.repeats + 2):
            for m, h in handles.items():
                t0 = time.perf_counter()
                h.render(cam(k), args.ns, seed=k, out="torch")
                times[m].append((time.perf_counter() - t0) * 1e3)
        for m in handles:
            rows.append({"scene": name, "nx": nx, "ny": ny, "ns": args.ns, "mode": m, "low": list(sizes[m]), "median_ms": median(times[m]),
                         "min_ms": min(times[m]), "max_ms": max(times[m]), "repeats_ms": times[m]})
        full = median(times["frame_full"])
        rows.append(dict({"scene": name, "summary": True},
                         **{"%s_over_frame_full" % m: median(times[m]) / full for m in handles if m != "frame_full"},
                         **{"%s_every_repeat_faster" % m: max(times[m]) < min(times["frame_full"]) for m in handles if m != "frame_full"}))
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
