"""Times render sessions (include/rtmi_session.h) against the one-shot entries they equal.  Needs a GPU.  Prints one JSON
line per measurement with every repeat.

    python tools/session_timing.py                      # the two scenes of DESIGN.md §22
    python tools/session_timing.py --ns 16 --repeats 3  # a shorter run

The protocol is tools/light_coop_timing.py's: every call is blocking and its time is the span between two HIP events
around it; one warm-up per mode, then the modes alternate `repeats` times in one process and the median is reported.
Per scene: 64 spp as one one-shot call and as 1 x 64, 4 x 16 and 16 x 4 session calls (a fresh session each time, its
creation and destruction outside the span; the image is compared with the one-shot's, bit for bit); one image() read-out;
one merge of two 32-spp sessions; and one refine sequence (2u, cap/2) -> (u, cap/2) -> (0.5u, cap) next to the one-shot
adaptive run with the last call's arguments, u being the median tile noise after min_spp samples.
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
from raytracing_rust_amd import Host, abi, scenes  # noqa: E402
import scenes_extra  # noqa: E402

# scene, nx, ny, coop
CASES = [("cornell_box", 800, 800, False), ("lit_final_scene", 1920, 1080, True)]
PLANES = ("linear", "rgb8", "stderr")


def _build(host, name, nx, ny):
    if name in scenes.SCENES:
        return scenes.build(host, name, nx, ny, seed=1)
    return scenes_extra.build(host, name, nx, ny, seed=1)


def _same(a, b, keys):
    return all(a[k].tobytes() == b[k].tobytes() for k in keys)


def _report(label, times, **more):
    print(json.dumps(dict(label, median_ms=float(np.median(times)), repeats_ms=[float(t) for t in times], **more)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--scenes", default=",".join(c[0] for c in CASES))
    ap.add_argument("--cap", type=int, default=64)
    args = ap.parse_args()
    if args.repeats < 3:
        ap.error("--repeats must be at least 3")
    if args.ns % 16:
        ap.error("--ns must be a multiple of 16")
    host = Host()
    ev = Events()
    fc = abi.RTMI_FLAG_FAST_CULL
    ns = args.ns
    for name, nx, ny, coop in CASES:
        if name not in args.scenes.split(","):
            continue
        cam, world = _build(host, name, nx, ny)
        sc = host.lower(world).upload(0, nee=True)
        label = {"scene": name, "nx": nx, "ny": ny, "ns": ns, "estimator": "nee", "coop": coop}

        def session(**kw):
            return sc.session(cam, nx, ny, estimator="nee", coop=coop, seed=42, flags=fc, **kw)

        def one_shot():
            return sc.render_nee(cam, nx, ny, ns, seed=42, flags=fc, coop=coop)

        def in_calls(calls):
            ses = session()
            ms = ev.time_ms(lambda: [ses.render(ns // calls) for _ in range(calls)])[0]
            img = ses.image()
            ses.close()
            return ms, img

        modes = {"one_shot": lambda: ev.time_ms(one_shot), "session_1x%d" % ns: lambda: in_calls(1),
                 "session_4x%d" % (ns // 4): lambda: in_calls(4), "session_16x%d" % (ns // 16): lambda: in_calls(16)}
        outs = {m: fn()[1] for m, fn in modes.items()}  # warm-up, and the planes to compare
        times = {m: [] for m in modes}
        for _ in range(args.repeats):
            for m, fn in modes.items():
                times[m].append(fn()[0])
        base = float(np.median(times["one_shot"]))
        for m in modes:
            _report(dict(label, mode=m), times[m], over_one_shot=float(np.median(times[m])) / base,
                    same_bits=_same(outs[m], outs["one_shot"], PLANES))

        # one read-out, one merge
        a, b = session(), session(first_sample=ns // 2)
        a.render(ns // 2)
        b.render(ns // 2)
        a.image()
        _report(dict(label, mode="image"), [ev.time_ms(a.image)[0] for _ in range(args.repeats)])
        merges = []
        blob = a.save()
        for _ in range(args.repeats):
            a.load(blob)
            merges.append(ev.time_ms(lambda: a.merge(b))[0])
        _report(dict(label, mode="merge_%d+%d" % (ns // 2, ns // 2)), merges)
        a.close()
        b.close()

        # a refine sequence against the one-shot adaptive run it equals
        cap, mn, step = args.cap, 16, 16
        first = sc.render_adaptive(cam, nx, ny, mn, mn, step, nee=True, seed=42, flags=fc, coop=coop)
        u = float(np.median(first["stderr"].max(-1)))

        def adaptive():
            return sc.render_adaptive(cam, nx, ny, cap, mn, step, abs_tol=0.5 * u, nee=True, seed=42, flags=fc, coop=coop)

        def refine():
            ses = session(lattice=(mn, step))
            ms = ev.time_ms(lambda: [ses.refine(2 * u, 0.0, cap // 2), ses.refine(u, 0.0, cap // 2), ses.refine(0.5 * u, 0.0, cap)])[0]
            img = ses.image()
            ses.close()
            return ms, img

        modes = {"adaptive_one_shot": lambda: ev.time_ms(adaptive), "refine_3_calls": refine}
        outs = {m: fn()[1] for m, fn in modes.items()}
        times = {m: [] for m in modes}
        for _ in range(args.repeats):
            for m, fn in modes.items():
                times[m].append(fn()[0])
        base = float(np.median(times["adaptive_one_shot"]))
        for m in modes:
            _report(dict(label, mode=m, cap=cap, min_spp=mn, step_spp=step, abs_tol=0.5 * u,
                         samples=int(outs["adaptive_one_shot"]["stats"]["samples"])), times[m],
                    over_one_shot=float(np.median(times[m])) / base,
                    same_bits=_same(outs[m], outs["adaptive_one_shot"], PLANES + ("spp",)))
        host.free_all()


if __name__ == "__main__":
    main()
