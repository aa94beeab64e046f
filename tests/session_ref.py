"""numpy restatement of the render sessions' state arithmetic (include/rtmi_session.h): the blob layout, the read-out, the
merge, and the refine rule next to the one-shot adaptive rule.  numpy evaluates every operation with one rounding (no
fused operations), as the device units compiled with -ffp-contract=off do.  No GPU."""
import struct

import numpy as np

MAGIC = b"RTMISESS"
VERSION, HEADER, IDENTITY = 1, 216, 196
SEED_OFFSET = 72  # a byte of the identity block the tests change
OPTS = ("estimator", "rr", "min_depth", "q_min", "env_select_p", "first_sample", "min_spp", "step_spp")


def parse_blob(blob):
    """The blob of rtmi_session_export by the header's layout: dict of the header fields, n u32 [tiles],
    state f64 [tiles, 9, 64] (sum r,g,b | m r,g,b | M2 r,g,b) and bounces u32 [tiles, 64]."""
    blob = bytes(blob)
    assert len(blob) >= HEADER and blob[:8] == MAGIC, "not a session blob"
    version, nx, ny, tiles, kind = struct.unpack_from("<5I", blob, 8)
    assert version == VERSION
    assert tiles == ((nx + 7) // 8) * ((ny + 7) // 8)
    out = {"nx": nx, "ny": ny, "tiles": tiles, "kind": kind}
    out.update(zip(OPTS, struct.unpack_from("<3I2f3I", blob, 28)))
    out["max_depth"], out["t_min"], out["flags"], out["seed"] = struct.unpack_from("<IfIQ", blob, 60)
    out["camera"] = np.frombuffer(blob, "<f4", 21, 80)
    out["scene_counts"] = np.frombuffer(blob, "<u4", 8, 164)
    out["last_cap"], out["last_abs_tol"], out["last_rel_tol"] = struct.unpack_from("<Idd", blob, 196)
    assert len(blob) == HEADER + tiles * (4 + 9 * 64 * 8 + 64 * 4), "wrong blob length"
    at = HEADER
    out["n"] = np.frombuffer(blob, "<u4", tiles, at).copy()
    at += 4 * tiles
    out["state"] = np.frombuffer(blob, "<f8", tiles * 9 * 64, at).reshape(tiles, 9, 64).copy()
    at += 8 * tiles * 9 * 64
    out["bounces"] = np.frombuffer(blob, "<u4", tiles * 64, at).reshape(tiles, 64).copy()
    return out


def untile(plane, nx, ny):
    """[tiles, 64, ...] (lane = ly * 8 + lx, tiles from the top-left) -> [ny, nx, ...]"""
    tx, ty = (nx + 7) // 8, (ny + 7) // 8
    rest = plane.shape[2:]
    a = plane.reshape((ty, tx, 8, 8) + rest)
    a = np.moveaxis(a, 2, 1).reshape((ty * 8, tx * 8) + rest)
    return np.ascontiguousarray(a[:ny, :nx])


def tile_pixels(samples):
    """[ny, nx, ...] -> [tiles, 64, ...], zero where a lane lies outside the image"""
    ny, nx = samples.shape[:2]
    tx, ty = (nx + 7) // 8, (ny + 7) // 8
    pad = np.zeros((ty * 8, tx * 8) + samples.shape[2:], samples.dtype)
    pad[:ny, :nx] = samples
    a = pad.reshape((ty, 8, tx, 8) + samples.shape[2:])
    return np.moveaxis(a, 1, 2).reshape((ty * tx, 64) + samples.shape[2:])


def quantise(total, n):
    """texel of a f64 sum over n samples: linear f32 and rgb8, as rtmi_render quantises (sqrt, clamp, 255.99, `as i32`)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        mm = total / np.float64(n)
        g = np.sqrt(mm)
        g = np.where(g > 0.0, np.where(g < 1.0, g, 1.0), 0.0)  # NaN -> 0
        x = 255.99 * g
    return mm.astype(np.float32), np.where(np.isnan(x), 0, x).astype(np.int32).astype(np.uint8)


def stderr_of(M2, n):
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.float64(n)
        return np.sqrt(M2 / (n * (n - 1.0)))


def readout(b):
    """rtmi_session_image of a parsed blob: dict(linear, rgb8, stderr, spp, bounces), row 0 the top row"""
    nx, ny = b["nx"], b["ny"]
    n = b["n"].astype(np.float64)[:, None, None]
    st = np.moveaxis(b["state"], 1, 2)  # [tiles, 64, 9]
    lin, rgb = quantise(st[..., 0:3], n)
    se = stderr_of(st[..., 6:9], n).astype(np.float32)
    spp = np.repeat(b["n"][:, None], 64, 1)
    return {"linear": untile(lin, nx, ny), "rgb8": untile(rgb, nx, ny), "stderr": untile(se, nx, ny),
            "spp": untile(spp, nx, ny), "bounces": untile(b["bounces"], nx, ny)}


def merge_stats(sumA, mA, M2A, nA, sumB, mB, M2B, nB):
    """the pairwise combination of rtmi_session.h, in double"""
    nA, nB = np.float64(nA), np.float64(nB)
    n = nA + nB
    d = mB - mA
    return sumA + sumB, mA + d * (nB / n), (M2A + M2B) + (d * d) * ((nA * nB) / n)


def merge(a, b):
    """rtmi_session_merge(dst = a, src = b) on parsed blobs of FIXED sessions; returns the merged parsed blob"""
    assert a["kind"] == 0 and b["kind"] == 0
    nA, nB = int(a["n"][0]), int(b["n"][0])
    assert b["first_sample"] == a["first_sample"] + nA
    out = dict(a)
    if nB == 0:
        return out
    if nA == 0:
        out["state"], out["bounces"] = b["state"].copy(), b["bounces"].copy()
    else:
        A, B = a["state"], b["state"]
        s, m, M2 = merge_stats(A[:, 0:3], A[:, 3:6], A[:, 6:9], nA, B[:, 0:3], B[:, 3:6], B[:, 6:9], nB)
        out["state"] = np.concatenate([s, m, M2], axis=1)
        out["bounces"] = a["bounces"] + b["bounces"]
    out["n"] = a["n"] + b["n"]
    return out


def accumulate(samples):
    """(sum, m, M2) in double of per-sample radiances [..., ns, 3] (fp32) in sample order, as the resolve steps them, after
    every sample: three arrays [ns + 1, ..., 3], entry k = the state after k samples"""
    x = samples.astype(np.float64)
    ns = x.shape[-2]
    shape = x.shape[:-2] + (3,)
    s, m, M2 = np.zeros((ns + 1,) + shape), np.zeros((ns + 1,) + shape), np.zeros((ns + 1,) + shape)
    for k in range(ns):
        xk = x[..., k, :]
        d = xk - m[k]
        s[k + 1] = s[k] + xk
        m[k + 1] = m[k] + d / float(k + 1)
        M2[k + 1] = M2[k] + d * (xk - m[k + 1])
    return s, m, M2


def ulps(a, b):
    """distance of two f32 arrays in units in the last place (NaN against NaN counts 0)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)

    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    d = np.abs(key(a) - key(b))
    return np.where(np.isnan(a) & np.isnan(b), 0, d)


# ---- the refine rule and the one-shot rule on per-sample radiances ------------------------------------------------------
class TileStats:
    """The prefix states of every tile of an image's per-sample radiances [ny, nx, ns, 3]: converged(tile, n, tol)."""

    def __init__(self, samples):
        self.ny, self.nx, self.ns = samples.shape[:3]
        inside = tile_pixels(np.ones((self.ny, self.nx), bool))
        self.inside = inside  # [tiles, 64]
        s, _, M2 = accumulate(tile_pixels(samples))  # [ns + 1, tiles, 64, 3]
        self.s, self.M2 = s, M2
        self.tiles = inside.shape[0]

    def stderr(self, tile, n):
        return stderr_of(self.M2[n, tile], n)

    def converged(self, tile, n, abs_tol, rel_tol):
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = self.s[n, tile] / np.float64(n)
            e = self.stderr(tile, n)
            ok = np.isfinite(e) & np.isfinite(mean) & (e <= abs_tol + rel_tol * np.abs(mean))
        return bool(np.all(ok.all(axis=-1) | ~self.inside[tile]))


def one_shot_counts(ts, min_spp, step_spp, abs_tol, rel_tol, cap):
    """rtmi_adaptive.h's steps: the count every tile retires at, and the samples traced (in tile-samples per tile)"""
    n = np.zeros(ts.tiles, np.int64)
    for t in range(ts.tiles):
        k = min_spp
        while k < cap and not ts.converged(t, k, abs_tol, rel_tol):
            k = min(k + step_spp, cap)
        n[t] = k
    return n


class RefineSim:
    """rtmi_session_refine's rule on the host: per tile a parked count; refine() advances as the header states and
    returns the tile-samples traced by the call."""

    def __init__(self, ts, min_spp, step_spp):
        self.ts, self.min_spp, self.step = ts, min_spp, step_spp
        self.n = np.zeros(ts.tiles, np.int64)
        self.last = (0, np.inf, np.inf)

    def on_lattice(self, k):
        return k >= self.min_spp and (k - self.min_spp) % self.step == 0

    def refine(self, abs_tol, rel_tol, cap):
        assert cap >= self.last[0] and abs_tol <= self.last[1] and rel_tol <= self.last[2], "a call must not loosen"
        self.last = (cap, abs_tol, rel_tol)
        parked = {}
        for t in range(self.ts.tiles):
            if self.n[t] < cap:
                parked.setdefault(int(self.n[t]), []).append(t)
        active, cur, traced, launches = [], 0, 0, []
        while True:
            if not active:
                if not parked:
                    break
                cur = min(parked)
            active += parked.pop(cur, [])
            if self.on_lattice(cur):
                active = [t for t in active if not self.ts.converged(t, cur, abs_tol, rel_tol)]
            if not active:
                continue
            nxt = self.min_spp if cur < self.min_spp else cur + self.step - (cur - self.min_spp) % self.step
            nxt = min(nxt, cap)
            if parked and min(parked) < nxt:
                nxt = min(parked)
            launches.append((cur, nxt, len(active)))
            traced += len(active) * (nxt - cur)
            for t in active:
                self.n[t] = nxt
            cur = nxt
            if cur >= cap:
                break
        self.launches = launches
        return traced
