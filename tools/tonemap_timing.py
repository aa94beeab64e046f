"""Times the tone mapper's device form (rtmi_tonemap_apply_device, include/rtmi_tonemap.h) with HIP events.  Needs a GPU.

    python tools/tonemap_timing.py                      # rows to profiles/tonemap/timing.jsonl and to stdout
    python tools/tonemap_timing.py --out <file> --repeats 16 --batch 50

Sizes 800x800 and 1920x1080; settings AUTO+ACES+SRGB (the defaults) and MANUAL+CLAMP+GAMMA2 (the project's quantiser).
Two images, resident on the device: `spread`, log-uniform over sixteen stops (some 170 bins in use), and `flat`, one grey,
the worst case of the meter's LDS atomics: all 64 lanes of an instruction meet in one bin, as in a sky or a black
background.  A repeat is `--batch` calls enqueued back to back on torch's current stream between two events, reported per
call, so a row is the rate a frame loop sees, launch gaps included; `--repeats` (at least 8) repeats follow one warm-up
batch, and a row holds their median and range.

The entry has no switch that runs one kernel alone, so the calls are chosen to take the kernels apart:
    whole        rgb8 and state: meter, solve, apply (AUTO); solve, apply (MANUAL)
    with_display rgb8, display and state: the same kernels, the apply writing 12 more bytes per channel triple
    state_only   state alone: meter, solve (AUTO); solve (MANUAL)
and the derived rows are differences of medians: apply = whole - state_only, solve = MANUAL's state_only, meter = AUTO's
state_only - MANUAL's state_only.  `bytes` is what the apply kernel moves for the row (12 B read, 3 B or 15 B written per
pixel) and `apply_gbps` that over the derived apply time.  A difference is what a kernel adds to a busy stream, where it
overlaps the launch gaps and tails of its neighbours; it is less than the kernel's own duration.  For the durations run
the tool under `rocprofv3 --kernel-trace --stats`: the apply launches of one setting and size then come in runs of
`--batch`, without and with `display` in turn."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
SIZES = ((800, 800), (1920, 1080))
SETTINGS = {"auto_aces_srgb": dict(exposure="auto", op="aces", oetf="srgb"),
            "manual_clamp_gamma2": dict(exposure="manual", op="clamp", oetf="gamma2")}


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "tonemap", "timing.jsonl"))
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--batch", type=int, default=20)
    args = ap.parse_args()
    if args.repeats < 8:
        ap.error("--repeats must be at least 8")
    import numpy as np
    import torch

    from raytracing_rust_amd import Tonemap, abi

    lib = abi.load_rtmi()
    dev = torch.device("cuda", 0)
    rows = []
    for nx, ny in SIZES:
        n = nx * ny
        rng = np.random.default_rng(nx)
        images = {"spread": (np.exp2(rng.uniform(-8, 8, (ny, nx, 1))) * rng.uniform(0.2, 1.8, (ny, nx, 3))).astype(np.float32),
                  "flat": np.full((ny, nx, 3), 0.5, np.float32)}
        for image, img in images.items():
            lin = torch.from_numpy(img).to(dev)
            rgb8 = torch.empty((ny, nx, 3), dtype=torch.uint8, device=dev)
            disp = torch.empty((ny, nx, 3), dtype=torch.float32, device=dev)
            state = torch.empty(32, dtype=torch.uint8, device=dev)
            med = {}
            for setting, kw in SETTINGS.items():
                with Tonemap(nx, ny, **kw) as tm:
                    calls = {"whole": (rgb8.data_ptr(), None, state.data_ptr()),
                             "with_display": (rgb8.data_ptr(), disp.data_ptr(), state.data_ptr()),
                             "state_only": (None, None, state.data_ptr())}
                    stream = torch.cuda.current_stream(dev)

                    def batch(outs):
                        for _ in range(args.batch):
                            rc = lib.rtmi_tonemap_apply_device(tm.h, lin.data_ptr(), 1 / 60, outs[0], outs[1], outs[2], stream.cuda_stream)
                            if rc:
                                sys.exit("rtmi_tonemap_apply_device failed (%d): %s" % (rc, lib.rtmi_last_error().decode()))

                    times = {m: [] for m in calls}
                    for outs in calls.values():  # warm-up: code objects, clocks
                        batch(outs)
                    torch.cuda.synchronize(dev)
                    for _ in range(args.repeats):  # the calls alternate, so drift falls on all alike
                        for m, outs in calls.items():
                            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            t0.record(stream)
                            batch(outs)
                            t1.record(stream)
                            t1.synchronize()
                            times[m].append(t0.elapsed_time(t1) / args.batch)
                    for m, ms in times.items():
                        med[(setting, m)] = median(ms)
                        rows.append({"nx": nx, "ny": ny, "image": image, "setting": setting, "call": m, "median_ms": median(ms), "min_ms": min(ms),
                                     "max_ms": max(ms), "repeats": args.repeats, "batch": args.batch, "repeats_ms": ms})
            for setting in SETTINGS:
                for call, out_bytes in (("whole", 3), ("with_display", 15)):
                    ms = med[(setting, call)] - med[(setting, "state_only")]
                    b = n * (12 + out_bytes)
                    rows.append({"nx": nx, "ny": ny, "image": image, "setting": setting, "derived": "apply (%s - state_only)" % call, "median_ms": ms,
                                 "bytes": b, "apply_gbps": b / (ms * 1e-3) / 1e9 if ms > 0 else None})
            solve = med[("manual_clamp_gamma2", "state_only")]
            rows.append({"nx": nx, "ny": ny, "image": image, "derived": "solve (MANUAL state_only)", "median_ms": solve})
            meter = med[("auto_aces_srgb", "state_only")] - solve
            rows.append({"nx": nx, "ny": ny, "image": image, "derived": "meter (AUTO state_only - MANUAL state_only)", "median_ms": meter,
                         "bytes": n * 12, "meter_gbps": n * 12 / (meter * 1e-3) / 1e9 if meter > 0 else None})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
            print(json.dumps({k: v for k, v in r.items() if k != "repeats_ms"}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
