"""Times RTMI_FLAG_BATCH_COOP (include/rtmi_batch_coop.h): the batch modes on the per-lane kernel against the same calls on
the wave-cooperative kernel.  Needs a GPU.  Prints one JSON line per (workload, scene, kernel) with every repeat and one
per (workload, scene) with the ratio, and appends them to profiles/batch_coop/timing.jsonl.

    python tools/batch_coop_timing.py                                  # the table of DESIGN.md §38
    python tools/batch_coop_timing.py --repeats 3 --scenes cornell_box --workloads radiance_primary,gather

The workloads are those of the existing timing tools: radiance_timing.py (1920x1080 rays x 16 samples, primary rays and
incoherent bounce rays), gather_timing.py, sparse_timing.py and pixelwise_timing.py, each on final_scene /
lit_final_scene, random_spheres and cornell_box.  The protocol is tools/light_coop_timing.py's: every call is blocking, its
time is the kernels' span between two HIP events (the call's own kernel_ms; the per-pixel render has none in its dict and
is timed by events around the call); one warm-up call per mode, then the modes alternate `repeats` times in one process
and the median is reported.  The yardstick is the same call without the flag (the unflagged code is the parent commit's:
DESIGN.md §38).  `clear` says whether the medians differ by more than the spread (max - min) of the repeats of both modes.
Every pair is also compared output by output: the flag must not change a bit.
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
from raytracing_rust_amd import Host, abi, primary_rays, scenes  # noqa: E402
import scenes_extra  # noqa: E402

DEFAULT_LOG = os.path.join(ROOT, "profiles", "batch_coop", "timing.jsonl")
# scene, estimator, flags beside FAST_CULL
SCENES = [("lit_final_scene", "nee", 0), ("final_scene", "plain", abi.RTMI_FLAG_SKY), ("random_spheres", "plain", abi.RTMI_FLAG_SKY),
          ("cornell_box", "nee", 0)]
WORKLOADS = ["radiance_primary", "radiance_bounce", "gather", "sparse", "pixelwise"]
NX, NY, SPP = 1920, 1080, 16


def _build(host, name, nx, ny):
    if name in scenes.SCENES:
        return scenes.build(host, name, nx, ny, seed=1)
    return scenes_extra.build(host, name, nx, ny, seed=1)


def _same(a, b, keys):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys)


def _race(ev, log, label, call, repeats, keys):
    """call(coop) -> dict; warm-up, alternate, report."""
    modes = {"perlane": lambda: call(False), "coop": lambda: call(True)}
    outs = {m: fn() for m, fn in modes.items()}  # warm-up, and the outputs to compare
    times = {m: [] for m in modes}
    for _ in range(repeats):
        for m, fn in modes.items():
            ms, out = ev.time_ms(fn)
            times[m].append(float(out["kernel_ms"]) if "kernel_ms" in out else ms)
    med = {m: float(np.median(t)) for m, t in times.items()}
    # kernel_reported: rtmi_stats.kernel, where the entry has stats (the per-pixel render)
    lines = [dict(label, kernel=m, median_ms=med[m], repeats_ms=times[m],
                  **({"kernel_reported": int(outs[m]["kernel"])} if "kernel" in outs[m] else {})) for m in modes]
    spread = max(max(t) - min(t) for t in times.values())
    lines.append(dict(label, perlane_over_coop=med["perlane"] / med["coop"], spread_ms=spread,
                      clear=abs(med["perlane"] - med["coop"]) > spread, same_bits=_same(outs["perlane"], outs["coop"], keys)))
    for line in lines:
        text = json.dumps(line)
        print(text, flush=True)
        log.write(text + "\n")
    log.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scenes", default=",".join(c[0] for c in SCENES))
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--nx", type=int, default=NX)
    ap.add_argument("--ny", type=int, default=NY)
    ap.add_argument("--spp", type=int, default=SPP)
    ap.add_argument("--log", default=DEFAULT_LOG)
    args = ap.parse_args()
    if args.repeats < 3:
        ap.error("--repeats must be at least 3")
    if abi.load_rtmi().rtmi_device_count() < 1:
        sys.exit("batch_coop_timing.py needs a GPU: nothing is measured without one")
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    host, ev = Host(), Events()
    fc = abi.RTMI_FLAG_FAST_CULL
    nx, ny, spp = args.nx, args.ny, args.spp
    want = args.workloads.split(",")
    with open(args.log, "a") as log:
        for name, est, extra in SCENES:
            if name not in args.scenes.split(","):
                continue
            cam, world = _build(host, name, nx, ny)
            sc = host.lower(world).upload(0, nee=est == "nee")
            fl = fc | extra
            base = {"scene": name, "estimator": est, "build": abi.load_rtmi().rtmi_build_hash().decode()}
            o, d = (a.reshape(-1, 3) for a in primary_rays(cam, nx, ny))
            times = None  # rays at time 0: a time plane sends a scene whose BVH time range is bounded to the exact traversal
            first = None
            if "radiance_primary" in want:
                _race(ev, log, dict(base, workload="radiance_primary", rays=nx * ny, spp=spp),
                      lambda coop: sc.radiance(o, d, times, spp=spp, estimator=est, seed=42, flags=fl, coop=coop),
                      args.repeats, ("mean", "stderr"))
            if "radiance_bounce" in want or "gather" in want:
                first = sc.trace(o, d, times, flags=fc)
                at = np.flatnonzero(first["hit"])
                nrm = np.ascontiguousarray(first["normal"][at], np.float32)
                pts = (first["p"][at] + np.float32(0.01) * nrm).astype(np.float32)
            if "radiance_bounce" in want:  # incoherent rays: one seeded direction about every first hit's normal
                rng = np.random.default_rng(7)
                v = rng.normal(size=nrm.shape).astype(np.float32)
                v = np.where((v * nrm).sum(-1, keepdims=True) < 0, -v, v) + nrm
                _race(ev, log, dict(base, workload="radiance_bounce", rays=int(at.size), spp=spp),
                      lambda coop: sc.radiance(pts, v, spp=spp, estimator=est, seed=42, flags=fl, coop=coop),
                      args.repeats, ("mean", "stderr"))
            if "gather" in want:
                _race(ev, log, dict(base, workload="gather", points=int(at.size), spp=spp),
                      lambda coop: sc.gather(pts, nrm, spp=spp, mode="cosine", estimator=est, seed=42, flags=fl, coop=coop),
                      args.repeats, ("value", "stderr"))
            if "sparse" in want:  # a tenth of the image's pixels, scattered
                px = np.random.default_rng(3).permutation(nx * ny)[:nx * ny // 10].astype(np.uint32)
                _race(ev, log, dict(base, workload="sparse", pixels=int(px.size), ns=spp),
                      lambda coop: sc.render_pixels(cam, nx, ny, px, spp, estimator=est, seed=42, flags=fl, coop=coop),
                      args.repeats, ("mean", "stderr"))
            if "pixelwise" in want:
                probe = sc.render_pixelwise(cam, nx, ny, 4, 4, 4, estimator=est, seed=42, flags=fl)
                tol = float(np.median(probe["stderr"].max(-1)))  # about half the pixels go on after the first step
                _race(ev, log, dict(base, workload="pixelwise", nx=nx, ny=ny, cap=4 * spp, min_spp=4, step_spp=4, abs_tol=tol),
                      lambda coop: sc.render_pixelwise(cam, nx, ny, 4 * spp, 4, 4, abs_tol=tol, estimator=est, seed=42, flags=fl,
                                                       coop=coop),
                      args.repeats, ("linear", "rgb8", "stderr", "spp", "counts"))
            host.free_all()


if __name__ == "__main__":
    main()
