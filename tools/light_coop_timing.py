"""Times RTMI_FLAG_LIGHT_COOP (include/rtmi_light_coop.h): the lighting estimators on the per-lane kernel against the same
estimators on the wave-cooperative kernel.  Needs a GPU.  Prints one JSON line per (scene, estimator, kernel) with every
repeat, and one per (scene, estimator) with the ratio.

    python tools/light_coop_timing.py                      # the five scenes of DESIGN.md §19 and one adaptive run
    python tools/light_coop_timing.py --ns 16 --repeats 3  # a shorter run

The protocol is tools/nee_timing.py's: every call is blocking and its time is the span between two HIP events around it;
one warm-up call per mode, then the modes alternate `repeats` times in one process and the median is reported.  The
baseline is the per-lane mode of the same build.  `clear` says whether the medians differ by more than the spread
(max - min) of the repeats of both modes.  Every pair is also compared plane by plane: the flag must not change a bit.
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
import scenes_extra  # noqa: E402

# scene, nx, ny, map, estimators
CASES = [("cornell_box", 800, 800, None, ("nee",)), ("lit_smoke", 800, 800, None, ("nee",)),
         ("lit_final_scene", 1920, 1080, None, ("nee",)), ("random_spheres", 1920, 1080, "sun", ("env", "env_nee")),
         ("earth", 1920, 1080, "earth", ("env", "env_nee")), ("lit_random_spheres", 1920, 1080, "sun", ("nee", "env_nee"))]
ADAPTIVE = ("lit_final_scene", 1920, 1080, 256, 16, 16)  # scene, nx, ny, cap, min_spp, step_spp


def _build(host, name, nx, ny):
    if name in scenes.SCENES:
        return scenes.build(host, name, nx, ny, seed=1)
    return scenes_extra.build(host, name, nx, ny, seed=7 if name == "lit_random_spheres" else 1)


def _earth_map():
    data, w, h = scenes.earthmap_rgb8()
    return (np.asarray(data, np.float32).reshape(h, w, 3) / np.float32(255.0)).astype(np.float32)


def _same(a, b, keys):
    return all(a[k].tobytes() == b[k].tobytes() for k in keys)


def _race(ev, label, modes, repeats, keys):
    """modes: {"perlane": fn, "coop": fn}; warm-up, alternate, report."""
    outs = {m: fn() for m, fn in modes.items()}  # warm-up, and the planes to compare
    times = {m: [] for m in modes}
    for _ in range(repeats):
        for m, fn in modes.items():
            times[m].append(ev.time_ms(fn)[0])
    med = {m: float(np.median(t)) for m, t in times.items()}
    for m in modes:
        print(json.dumps(dict(label, kernel=m, kernel_reported=int(outs[m]["stats"]["kernel"]), median_ms=med[m],
                              repeats_ms=times[m])), flush=True)
    spread = max(max(t) - min(t) for t in times.values())
    print(json.dumps(dict(label, perlane_over_coop=med["perlane"] / med["coop"], spread_ms=spread,
                          clear=abs(med["perlane"] - med["coop"]) > spread, same_bits=_same(outs["perlane"], outs["coop"], keys))),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scenes", default=",".join(c[0] for c in CASES))
    ap.add_argument("--no-adaptive", action="store_true")
    args = ap.parse_args()
    if args.repeats < 3:
        ap.error("--repeats must be at least 3")
    host = Host()
    ev = Events()
    fc = abi.RTMI_FLAG_FAST_CULL
    ns = args.ns
    for name, nx, ny, mapname, estimators in CASES:
        if name not in args.scenes.split(","):
            continue
        cam, world = _build(host, name, nx, ny)
        sc = host.lower(world).upload(0, nee=True)
        if mapname:
            sc.attach_env(env_ref.sun_map() if mapname == "sun" else _earth_map())
        for est in estimators:
            if est == "nee":
                def call(coop):
                    return sc.render_nee(cam, nx, ny, ns, seed=42, flags=fc, coop=coop)
            else:
                def call(coop, nee=est == "env_nee"):
                    return sc.render_env(cam, nx, ny, ns, nee=nee, env_select_p=0.5, seed=42, flags=fc, coop=coop)
            _race(ev, {"scene": name, "nx": nx, "ny": ny, "ns": ns, "map": mapname, "estimator": est},
                  {"perlane": lambda: call(False), "coop": lambda: call(True)}, args.repeats, ("linear", "rgb8", "stderr"))
        host.free_all()
    if not args.no_adaptive:
        name, nx, ny, cap, mn, step = ADAPTIVE
        cam, world = _build(host, name, nx, ny)
        sc = host.lower(world).upload(0, nee=True)
        first = sc.render_adaptive(cam, nx, ny, mn, mn, step, nee=True, seed=42, flags=fc)
        tol = float(np.median(first["stderr"].max(-1)))  # about half the pixels' tiles go on after the first step

        def adaptive(coop):
            return sc.render_adaptive(cam, nx, ny, cap, mn, step, abs_tol=tol, nee=True, seed=42, flags=fc, coop=coop)

        _race(ev, {"scene": name, "nx": nx, "ny": ny, "ns": cap, "min_spp": mn, "step_spp": step, "abs_tol": tol,
                   "estimator": "adaptive_nee"},
              {"perlane": lambda: adaptive(False), "coop": lambda: adaptive(True)}, args.repeats,
              ("linear", "rgb8", "stderr", "spp"))
        host.free_all()


if __name__ == "__main__":
    main()
