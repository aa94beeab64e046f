"""Times adaptive sampling with next-event estimation or environment lighting (include/rtmi_adaptive_nee.h) against the
fixed-ns render of the same estimator and against plain adaptive sampling.  Needs a GPU.  Prints one JSON line per
(scene, mode).

    python tools/adaptive_nee_timing.py                     # cornell_box 800x800 (cap 1024); random_spheres 1920x1080 + sun
    python tools/adaptive_nee_timing.py --repeats 2 --cap-env 128

Every call is blocking; its time is the span between two HIP events on the null stream around it (tools/denoise_timing.py).
One warm-up call per mode, then the modes alternate `repeats` times and the median is reported.  Each row gives the
camera paths traced (stats.samples), the time, and the max and RMS difference of its linear image against the fixed
render of the row's reference (`vs`).  cornell_box also reports the tiles that plain adaptive sampling retired at
min_spp with every pixel at mean 0 and stderr 0 (the zero-variance trap), and how many of them adaptive
NEE found lit.
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


def _tile_max(a, nx, ny):
    ty, tx = (ny + 7) // 8, (nx + 7) // 8
    pad = np.full((ty * 8, tx * 8, a.shape[-1]), -np.inf)
    pad[:ny, :nx] = a
    return pad.reshape(ty, 8, tx, 8, -1).max(axis=(1, 3, 4))


def _run(ev, modes, repeats):
    times = {k: [] for k in modes}
    outs = {k: fn() for k, fn in modes.items()}  # warm-up; its output is the row's image
    for _ in range(repeats):
        for k, fn in modes.items():
            times[k].append(ev.time_ms(fn)[0])
    return outs, {k: float(np.median(t)) for k, t in times.items()}, times


def _rows(scene, nx, ny, cap, outs, med, times, vs, extra=None):
    for k, out in outs.items():
        d = out["linear"].astype(np.float64) - outs[vs[k]]["linear"].astype(np.float64)
        row = {"scene": scene, "nx": nx, "ny": ny, "cap": cap, "mode": k, "paths": int(out["stats"]["samples"]),
               "paths_fraction": out["stats"]["samples"] / (nx * ny * cap), "seconds": med[k] / 1e3, "vs": vs[k],
               "max_abs_diff": float(np.abs(d).max()), "rms_diff": float(np.sqrt(np.mean(d * d))), "repeats_ms": times[k]}
        row.update((extra or {}).get(k, {}))
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--cap-env", type=int, default=256)
    ap.add_argument("--step", type=int, default=32)
    ap.add_argument("--rel-tol", type=float, default=0.05)
    args = ap.parse_args()
    host = Host()
    ev = Events()
    fc = abi.RTMI_FLAG_FAST_CULL
    st, rel = args.step, args.rel_tol

    nx, ny, cap = 800, 800, args.cap
    cam, world = scenes.build(host, "cornell_box", nx, ny, seed=1)
    sc = host.lower(world).upload(0, nee=True)
    modes = {"render_nee": lambda: sc.render_nee(cam, nx, ny, cap, seed=42, flags=fc),
             "adaptive_nee": lambda: sc.render_adaptive(cam, nx, ny, cap, st, st, rel_tol=rel, nee=True, seed=42, flags=fc),
             "adaptive_plain": lambda: sc.render_adaptive(cam, nx, ny, cap, st, st, rel_tol=rel, seed=42, flags=fc)}
    outs, med, times = _run(ev, modes, args.repeats)
    p, n = outs["adaptive_plain"], outs["adaptive_nee"]
    black = ((_tile_max(p["linear"], nx, ny) == 0) & (_tile_max(p["stderr"], nx, ny) == 0) &
             (_tile_max(p["spp"][..., None], nx, ny) == st))
    lit_nee = _tile_max(n["linear"], nx, ny) > 0
    _rows("cornell_box", nx, ny, cap, outs, med, times, {k: "render_nee" for k in modes},
          {"adaptive_plain": {"tiles_black_at_min": int(black.sum()), "of_them_lit_under_nee": int((black & lit_nee).sum()),
                              "tiles": int(black.size)}})
    host.free_all()

    nx, ny, cap = 1920, 1080, args.cap_env
    cam, world = scenes.build(host, "random_spheres", nx, ny, seed=1)
    sc = host.lower(world).upload(0, nee=True)
    sc.attach_env(env_ref.sun_map())
    modes = {}
    for nee in (0, 1):
        modes["render_env_nee%d" % nee] = (lambda e: lambda: sc.render_env(cam, nx, ny, cap, nee=bool(e), seed=42, flags=fc))(nee)
        modes["adaptive_env_nee%d" % nee] = (lambda e: lambda: sc.render_adaptive(
            cam, nx, ny, cap, st, st, rel_tol=rel, nee=bool(e), env=True, seed=42, flags=fc))(nee)
    outs, med, times = _run(ev, modes, args.repeats)
    _rows("random_spheres+sun", nx, ny, cap, outs, med, times, {k: "render_env_nee" + k[-1] for k in modes})
    host.free_all()


if __name__ == "__main__":
    main()
