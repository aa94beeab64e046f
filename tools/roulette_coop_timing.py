"""Times RTMI_FLAG_ROULETTE_COOP (include/rtmi_roulette_coop.h): Russian-roulette renders on the per-lane kernel against the
same renders on the wave-cooperative kernel, and against the non-roulette cooperative form of the same estimator.  Needs a
GPU.  Prints one JSON line per (scene, estimator, mode) with every repeat and one per (scene, estimator) with the ratios,
and writes the same lines to the log.

    python tools/roulette_coop_timing.py                      # the rows of DESIGN.md §20 and one adaptive run
    python tools/roulette_coop_timing.py --ns 16 --repeats 3 --scenes cornell_box,closed_box --no-adaptive

The protocol is tools/light_coop_timing.py's: every call is blocking and its time is the span between two HIP events
around it; one warm-up call per mode, then the modes alternate `repeats` times in one process and the median is reported.
Modes: "perlane" (render_roulette), "coop" (render_roulette(coop=True)) and "off" (render_nee(coop=True),
render_env(coop=True), or render() for the plain estimator: the existing cooperative entry without roulette).  Roulette
runs with min_depth = 3, q_min = 0.05, everything with FAST_CULL.  The baselines are modes of the same build.  `spread` is
the larger max - min of the two roulette modes' repeats and `clear` says whether their medians differ by more than that.
The two roulette modes are compared plane by plane: the flag must not change a bit.  Per row also scatters per sample
(bounces / samples; "off": roulette with min_depth > max_depth), the median per-pixel standard error over the pixels
whose non-roulette mean is not zero, and t_rr * sigma_rr^2 / (t_off * sigma_off^2) for the cooperative pair: below 1 roulette
reaches the same noise sooner.
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
import env_ref  # noqa: E402
import roulette_ref  # noqa: E402
import scenes_extra  # noqa: E402

# scene, nx, ny, map, estimators
CASES = [("lit_final_scene", 1920, 1080, None, ("nee", "plain")), ("lit_random_spheres", 1920, 1080, "sun", ("nee", "env_nee")),
         ("random_spheres", 1920, 1080, "sun", ("env", "env_nee")), ("closed_box", 800, 800, None, ("plain", "nee")),
         ("cornell_box", 800, 800, None, ("nee",)), ("lit_smoke", 800, 800, None, ("nee",))]
ADAPTIVE = ("lit_final_scene", 1920, 1080, 256, 16, 16)  # scene, nx, ny, cap, min_spp, step_spp
RR = dict(min_depth=3, q_min=0.05)
DEFAULT_LOG = os.path.join(ROOT, "profiles", "roulette_coop", "timing.jsonl")


def _build(host, name, nx, ny):
    if name == "closed_box":
        return roulette_ref.box(host, "closed", nx, ny)
    if name in scenes.SCENES:
        return scenes.build(host, name, nx, ny, seed=1)
    return scenes_extra.build(host, name, nx, ny, seed=7 if name == "lit_random_spheres" else 1)


def _same(a, b, keys):
    return all(a[k].tobytes() == b[k].tobytes() for k in keys)


class Log:
    def __init__(self, path):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self.f = open(path, "w")

    def __call__(self, rec):
        line = json.dumps(rec)
        print(line, flush=True)
        self.f.write(line + "\n")
        self.f.flush()


def _race(ev, log, label, modes, repeats, keys, stats=None):
    """modes: {"perlane": fn, "coop": fn[, "off": fn]}; warm-up, alternate, report.  stats(outs) -> extra fields of the
    summary line and per-mode fields."""
    outs = {m: fn() for m, fn in modes.items()}  # warm-up, and the planes to compare
    times = {m: [] for m in modes}
    for _ in range(repeats):
        for m, fn in modes.items():
            times[m].append(ev.time_ms(fn)[0])
    med = {m: float(np.median(t)) for m, t in times.items()}
    per_mode, summary = stats(outs, med) if stats else ({}, {})
    for m in modes:
        log(dict(label, mode=m, kernel_reported=int(outs[m]["stats"]["kernel"]), median_ms=med[m], repeats_ms=times[m],
                 **per_mode.get(m, {})))
    spread = max(max(times[m]) - min(times[m]) for m in ("perlane", "coop"))
    log(dict(label, perlane_over_coop=med["perlane"] / med["coop"], spread_ms=spread,
             clear=abs(med["perlane"] - med["coop"]) > spread, same_bits=_same(outs["perlane"], outs["coop"], keys), **summary))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scenes", default=",".join(c[0] for c in CASES))
    ap.add_argument("--no-adaptive", action="store_true")
    ap.add_argument("--log", default=DEFAULT_LOG)
    args = ap.parse_args()
    if args.repeats < 3:
        ap.error("--repeats must be at least 3")
    host = Host()
    ev = Events()
    log = Log(args.log)
    fc = abi.RTMI_FLAG_FAST_CULL
    ns = args.ns
    for name, nx, ny, mapname, estimators in CASES:
        if name not in args.scenes.split(","):
            continue
        cam, world = _build(host, name, nx, ny)
        sc = host.lower(world).upload(0, nee=True)
        if mapname:
            sc.attach_env(env_ref.sun_map())
        for est in estimators:
            kw = dict(seed=42, flags=fc)

            def rr(coop, est=est):
                return sc.render_roulette(cam, nx, ny, ns, estimator=est, env_select_p=0.5, coop=coop, **RR, **kw)

            if est == "plain":
                def off():
                    return sc.render(cam, nx, ny, ns, **kw)
                stat_off = sc.render_adaptive(cam, nx, ny, ns, min_spp=ns, step_spp=1, **kw)  # render's image with stderr
            elif est == "nee":
                def off():
                    return sc.render_nee(cam, nx, ny, ns, coop=True, **kw)
                stat_off = off()
            else:
                def off(nee=est == "env_nee"):
                    return sc.render_env(cam, nx, ny, ns, nee=nee, env_select_p=0.5, coop=True, **kw)
                stat_off = off()
            none = sc.render_roulette(cam, nx, ny, ns, estimator=est, env_select_p=0.5, min_depth=1 << 30, q_min=1.0, **kw)
            lit = stat_off["linear"].sum(-1) > 0
            sig_off = float(np.median(stat_off["stderr"].mean(-1)[lit]))
            scat_off = float(none["bounces"].sum(dtype=np.uint64)) / (nx * ny * ns)

            def stats(outs, med):
                sig = float(np.median(outs["coop"]["stderr"].mean(-1)[lit]))
                scat = float(outs["coop"]["bounces"].sum(dtype=np.uint64)) / (nx * ny * ns)
                on = dict(median_stderr=sig, scatters_per_sample=scat)
                return ({"perlane": on, "coop": on, "off": dict(median_stderr=sig_off, scatters_per_sample=scat_off)},
                        dict(off_over_coop=med["off"] / med["coop"],
                             time_to_equal_noise=med["coop"] * sig ** 2 / (med["off"] * sig_off ** 2)))

            _race(ev, log, {"scene": name, "nx": nx, "ny": ny, "ns": ns, "map": mapname, "estimator": est, **RR},
                  {"perlane": lambda: rr(False), "coop": lambda: rr(True), "off": off}, args.repeats,
                  ("linear", "rgb8", "stderr", "bounces"), stats)
        host.free_all()
    if not args.no_adaptive:
        name, nx, ny, cap, mn, step = ADAPTIVE
        cam, world = _build(host, name, nx, ny)
        sc = host.lower(world).upload(0, nee=True)

        def adaptive(ns_, tol, coop):
            return sc.render_adaptive_roulette(cam, nx, ny, ns_, mn, step, abs_tol=tol, estimator="nee", seed=42, flags=fc,
                                               coop=coop, **RR)

        first = adaptive(mn, 0.0, False)
        tol = float(np.median(first["stderr"].max(-1)))  # about half the pixels' tiles go on after the first step
        _race(ev, log, {"scene": name, "nx": nx, "ny": ny, "ns": cap, "min_spp": mn, "step_spp": step, "abs_tol": tol,
                        "estimator": "adaptive_nee", **RR},
              {"perlane": lambda: adaptive(cap, tol, False), "coop": lambda: adaptive(cap, tol, True)}, args.repeats,
              ("linear", "rgb8", "stderr", "spp", "bounces"))
        host.free_all()


if __name__ == "__main__":
    main()
