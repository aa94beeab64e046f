"""Ray sets and oracle records for the ray-query tests (tests/test_gpu_query.py): the fan and bounce rays of a scene and,
for every ray, the record of the fp32 oracle's Hittable::hit in the device's arithmetic.  Built once per scene and
shared by the tests; nothing here needs a GPU."""
import numpy as np

import scenes_extra
import scenes_random
from oracle.oracle import ARITH_DEVICE
from raytracing_rust_amd import scenes

SEED = 1000  # ray i of a set is traced with the oracle's seed SEED + i
T_MIN = 0.001
INF = float("inf")
NO_HIT = {"hit": False}


def fan(rng, look_from, look_at, n):
    """n rays from look_from along (look_at - look_from) + N(0, (0.15 |look_at - look_from|)^2), rounded to float32"""
    c = np.asarray(look_at, np.float64) - np.asarray(look_from, np.float64)
    d = c + rng.standard_normal((n, 3)) * (0.15 * np.linalg.norm(c))
    return np.tile(np.asarray(look_from, np.float32), (n, 1)), d.astype(np.float32)


def oracle_records(orc, world, o, d, times=None, t_min=T_MIN, t_max=INF, seed=SEED):
    """orc.hit of every ray in a numpy record per field: hit bool [n], t, u, v float32 [n], p, normal float32 [n, 3],
    mat_kind int [n] (-1: no hit); ray i with the seed `seed + i`; t_min, t_max scalars or [n]"""
    n = o.shape[0]
    tmn, tmx = np.broadcast_to(np.asarray(t_min, np.float64), (n,)), np.broadcast_to(np.asarray(t_max, np.float64), (n,))
    out = {"hit": np.zeros(n, bool), "t": np.full(n, np.inf, np.float32), "u": np.zeros(n, np.float32),
           "v": np.zeros(n, np.float32), "p": np.zeros((n, 3), np.float32), "normal": np.zeros((n, 3), np.float32),
           "mat_kind": np.full(n, -1, np.int64)}
    for i in range(n):
        h = orc.hit(world, o[i].astype(np.float64), d[i].astype(np.float64), time=0.0 if times is None else float(times[i]),
                    t_min=float(tmn[i]), t_max=float(tmx[i]), flags=ARITH_DEVICE, seed=seed + i)
        if h is None:
            continue
        out["hit"][i] = True
        for k in ("t", "u", "v"):
            out[k][i] = np.float32(h[k])
        out["p"][i] = h["p"].astype(np.float32)
        out["normal"][i] = h["normal"].astype(np.float32)
        out["mat_kind"][i] = h["mat_kind"]
    return out


def ray_sets(orc, world, look_from, look_at, n, shutter=None, intervals=False):
    """The two ray sets of a world and their oracle records: dict(fan=(o, d, times, t_min, ref), bounce=(...)).  The
    bounce rays start at the fan's hit points with standard-normal directions.  shutter = (t0, t1): a time per ray,
    uniform in the shutter.  intervals: for every surface hit of either set also `near`, the oracle's answer to the same
    ray with t_max = t, nextafter(t, +inf) and nextafter(t, 0) — a list of (ray indices, t_max values, hit flags)."""
    rng = np.random.default_rng(7)
    o, d = fan(rng, look_from, look_at, n)
    times = None if shutter is None else rng.uniform(shutter[0], shutter[1], n).astype(np.float32)
    ref = oracle_records(orc, world, o, d, times)
    sets = {"fan": {"o": o, "d": d, "times": times, "ref": ref}}
    idx = np.flatnonzero(ref["hit"])
    bo = np.ascontiguousarray(ref["p"][idx])
    bd = rng.standard_normal((len(idx), 3)).astype(np.float32)
    bt = None if shutter is None else rng.uniform(shutter[0], shutter[1], len(idx)).astype(np.float32)
    sets["bounce"] = {"o": bo, "d": bd, "times": bt, "ref": oracle_records(orc, world, bo, bd, bt)}
    if intervals:
        for s in sets.values():
            r = s["ref"]
            hits = np.flatnonzero(r["hit"] & (r["mat_kind"] != 4))
            near = []
            for tm in (r["t"][hits], np.nextafter(r["t"][hits], np.float32(np.inf)), np.nextafter(r["t"][hits], np.float32(0.0))):
                got = np.zeros(len(hits), bool)
                for k, i in enumerate(hits):
                    h = orc.hit(world, s["o"][i].astype(np.float64), s["d"][i].astype(np.float64),
                                time=0.0 if s["times"] is None else float(s["times"][i]), t_min=T_MIN, t_max=float(tm[k]),
                                flags=ARITH_DEVICE, seed=SEED + int(i))
                    got[k] = h is not None
                near.append((hits, tm.astype(np.float32), got))
            s["near"] = near
    return sets


def scene_camera(name):
    """(look_from, look_at) of a named scene's camera"""
    table = scenes.SCENES if name in scenes.SCENES else scenes_extra.EXTRA
    return table[name][1], table[name][2]


def build_world(api, name):
    return scenes_extra.build(api, name, 64, 48, seed=1)[1]


def random_fan_camera(host, seed):
    """eye and view centre of scenes_random.random_camera: the lens centre and the centre of its focus plane"""
    c = scenes_random.random_camera(host, seed, 64, 48).lower()
    org = np.array(list(c.origin), np.float64)
    centre = (np.array(list(c.lower_left_corner), np.float64) + 0.5 * np.array(list(c.horizontal), np.float64) +
              0.5 * np.array(list(c.vertical), np.float64))
    return org, centre
