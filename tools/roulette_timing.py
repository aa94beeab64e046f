"""Times Russian-roulette path termination (include/rtmi_roulette.h) against the same estimators without it, and measures
the time to equal noise.  Needs a GPU.  Prints one JSON line per (scene, estimator, mode).

    python tools/roulette_timing.py                        # all five scenes, min_depth {1,2,3,5} x q_min {0.05,0.2}
    python tools/roulette_timing.py --ns 16 --repeats 2 --scenes cornell_box,closed_box

The protocol of tools/nee_timing.py: every call is blocking, its time the span between two HIP events around it; one
warm-up call per mode, then the modes alternate `repeats` times in one process and the median is reported (the repeats
are printed: their spread is the noise of the figures).  "Without" is the same run's render_nee / render_env / render:
for the plain estimator both render (the cooperative kernel) and render with RTMI_FLAG_SYNC (the per-lane kernel the
roulette kernels extend).  Per mode: seconds, the median per-pixel standard error over the pixels whose non-roulette mean
is not zero, and scatters per sample (bounces / samples; without roulette: render_roulette with min_depth > max_depth).
Figure of merit: t_rr * sigma_rr^2 / (t_off * sigma_off^2); below 1 roulette reaches the same noise sooner.
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

# (scene, nx, ny, estimators)
CASES = [("cornell_box", 800, 800, ("plain", "nee")), ("lit_smoke", 800, 800, ("plain", "nee")),
         ("lit_final_scene", 1920, 1080, ("plain", "nee")), ("closed_box", 800, 800, ("plain", "nee")),
         ("random_spheres", 1920, 1080, ("env", "env_nee"))]
MIN_DEPTHS, Q_MINS = (1, 2, 3, 5), (0.05, 0.2)


def _build(host, name, nx, ny):
    if name == "closed_box":
        return roulette_ref.box(host, "closed", nx, ny)
    if name in scenes.SCENES:
        return scenes.build(host, name, nx, ny, seed=1)
    return scenes_extra.build(host, name, nx, ny, seed=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--scenes", default=",".join(c[0] for c in CASES))
    ap.add_argument("--min-depths", default=",".join(str(d) for d in MIN_DEPTHS))
    ap.add_argument("--q-mins", default=",".join(str(q) for q in Q_MINS))
    args = ap.parse_args()
    sweep = [(int(d), float(q)) for d in args.min_depths.split(",") for q in args.q_mins.split(",")]
    host = Host()
    ev = Events()
    fc = abi.RTMI_FLAG_FAST_CULL
    ns = args.ns
    for name, nx, ny, estimators in CASES:
        if name not in args.scenes.split(","):
            continue
        cam, world = _build(host, name, nx, ny)
        sc = host.lower(world).upload(0, nee=True)
        if "env" in estimators:
            sc.attach_env(env_ref.sun_map())
        for est in estimators:
            kw = dict(seed=42, flags=fc)
            if est == "plain":
                off = {"render": lambda: sc.render(cam, nx, ny, ns, **kw),
                       "render_sync": lambda: sc.render(cam, nx, ny, ns, seed=42, flags=fc | abi.RTMI_FLAG_SYNC)}
                stat_off = sc.render_adaptive(cam, nx, ny, ns, min_spp=ns, step_spp=1, **kw)
            elif est == "nee":
                off = {"render_nee": lambda: sc.render_nee(cam, nx, ny, ns, **kw)}
                stat_off = sc.render_nee(cam, nx, ny, ns, **kw)
            else:
                nee = est == "env_nee"
                off = {"render_env": lambda nee=nee: sc.render_env(cam, nx, ny, ns, nee=nee, **kw)}
                stat_off = sc.render_env(cam, nx, ny, ns, nee=nee, **kw)
            on = {"rr_d%d_q%g" % (d, q): (lambda d=d, q=q: sc.render_roulette(cam, nx, ny, ns, estimator=est, min_depth=d,
                                                                                q_min=q, **kw)) for d, q in sweep}
            modes = dict(off, **on)
            times = {m: [] for m in modes}
            outs = {}
            for m, fn in modes.items():
                outs[m] = fn()  # warm-up; its image gives the mode's statistics
            for _ in range(args.repeats):
                for m, fn in modes.items():
                    times[m].append(ev.time_ms(fn)[0])
            lit = stat_off["linear"].sum(-1) > 0
            sig_off = float(np.median(stat_off["stderr"].mean(-1)[lit]))
            none = sc.render_roulette(cam, nx, ny, ns, estimator=est, min_depth=1 << 30, q_min=1.0, **kw)
            scat_off = float(none["bounces"].sum(dtype=np.uint64)) / (nx * ny * ns)
            med = {m: float(np.median(t)) for m, t in times.items()}
            base = next(iter(off))  # render / render_nee / render_env
            for m in modes:
                rec = {"scene": name, "nx": nx, "ny": ny, "ns": ns, "estimator": est, "mode": m, "seconds": med[m] / 1e3,
                       "repeats_ms": times[m]}
                if m in on:
                    sig = float(np.median(outs[m]["stderr"].mean(-1)[lit]))
                    rec.update(median_stderr=sig, scatters_per_sample=float(outs[m]["bounces"].sum(dtype=np.uint64)) / (nx * ny * ns),
                               time_ratio=med[m] / med[base], stderr_ratio=sig / sig_off,
                               time_to_equal_noise=med[m] * sig ** 2 / (med[base] * sig_off ** 2))
                    if est == "plain":
                        rec["time_to_equal_noise_vs_sync"] = med[m] * sig ** 2 / (med["render_sync"] * sig_off ** 2)
                else:
                    rec.update(median_stderr=sig_off, scatters_per_sample=scat_off)
                print(json.dumps(rec), flush=True)
        host.free_all()


if __name__ == "__main__":
    main()
