"""Environment lighting's formulas (include/rtmi_env.h) restated in numpy, for the CPU and GPU tests.

* `tables`: the sampling tables of rtmi_env_tables in float64, each output rounded once to float32;
* `lookup` and `sample`: the device's fp32 arithmetic operation for operation (numpy float32 operations round once, as
  the device's do under -ffp-contract=off).  The contract functions rtmi_atan2f, rtmi_asinf, rtmi_sinf and rtmi_cosf come
  from a gcc build of include/rtmi_math.h (`ContractMath`), as tests/test_denoise_abi.py does for rtmi_expf;
* `sun_map`, `lat_long_dirs`: test inputs."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np

F = np.float32
PI_F = F(3.1415927410125732)
PIO2_F = F(1.5707963705062866)
TWO_PI2_F = F(19.739208802178716)
ONE_MINUS = F(0.99999994039535522)
FLT_MAX = np.finfo(np.float32).max
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")

_SRC = r"""
#include "rtmi_math.h"
#define V1(name, fn) void name(const float *x, float *y, long n) { for (long i = 0; i < n; i++) y[i] = fn(x[i]); }
V1(v_asinf, rtmi_asinf)
V1(v_sinf, rtmi_sinf)
V1(v_cosf, rtmi_cosf)
void v_atan2f(const float *y, const float *x, float *out, long n) { for (long i = 0; i < n; i++) out[i] = rtmi_atan2f(y[i], x[i]); }
"""


class ContractMath:
    """rtmi_math.h compiled by gcc (-O2 -ffp-contract=off), applied elementwise to float32 arrays."""

    def __init__(self, workdir=None):
        d = workdir or tempfile.mkdtemp(prefix="rtmi_env_ref_")
        src, so = os.path.join(d, "m.c"), os.path.join(d, "libm_contract.so")
        with open(src, "w") as f:
            f.write(_SRC)
        subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I" + INCLUDE, src, "-o", so],
                       check=True)
        self.lib = C.CDLL(so)
        for n in ("v_asinf", "v_sinf", "v_cosf"):
            getattr(self.lib, n).argtypes = [C.c_void_p, C.c_void_p, C.c_long]
        self.lib.v_atan2f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]

    def _1(self, name, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.empty_like(x)
        getattr(self.lib, name)(x.ctypes.data, y.ctypes.data, x.size)
        return y

    def asinf(self, x):
        return self._1("v_asinf", x)

    def sinf(self, x):
        return self._1("v_sinf", x)

    def cosf(self, x):
        return self._1("v_cosf", x)

    def atan2f(self, y, x):
        y = np.ascontiguousarray(y, dtype=np.float32)
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty_like(y)
        self.lib.v_atan2f(y.ctypes.data, x.ctypes.data, out.ctypes.data, y.size)
        return out


# ---- tables (host, f64) ---------------------------------------------------------------------------------------------------
def tables(rgb):
    """rtmi_env_tables of a float32 [H, W, 3] map -> dict(row_cdf, row_p, col_cdf [H, W], col_p [H, W], total)."""
    a = np.asarray(rgb, dtype=np.float32)
    h, w = a.shape[:2]
    mc = a.max(axis=2)
    mr = np.maximum(np.maximum(np.roll(mc, 1, axis=1), mc), np.roll(mc, -1, axis=1))
    rows = np.arange(h)
    m3 = np.maximum(np.maximum(mr[np.maximum(rows - 1, 0)], mr), mr[np.minimum(rows + 1, h - 1)]).astype(np.float64)
    c = np.array([math.sin((j + 0.5) * math.pi / h) for j in range(h)])
    wt = m3 * c[:, None]
    R = np.cumsum(wt, axis=1)[:, -1]
    col_p = np.zeros((h, w), np.float32)
    col_cdf = np.ones((h, w), np.float32)
    pos = R > 0
    if pos.any():
        p = wt[pos] / R[pos][:, None]
        col_p[pos] = p.astype(np.float32)
        cdf = np.cumsum(p, axis=1).astype(np.float32)
        cdf[:, -1] = 1.0
        col_cdf[pos] = cdf
    total = float(np.cumsum(R)[-1])
    row_p = np.zeros(h, np.float32)
    row_cdf = np.ones(h, np.float32)
    if total > 0:
        p = R / total
        row_p = p.astype(np.float32)
        row_cdf = np.cumsum(p).astype(np.float32)
        row_cdf[-1] = 1.0
    return {"row_cdf": row_cdf, "row_p": row_p, "col_cdf": col_cdf, "col_p": col_p, "total": total}


# ---- device arithmetic (fp32) ---------------------------------------------------------------------------------------------
def env_uv(M, d):
    """(ok, u, v, theta) of float32 directions [n, 3]."""
    d = np.asarray(d, dtype=np.float32)
    ax, ay, az = np.abs(d[:, 0]), np.abs(d[:, 1]), np.abs(d[:, 2])
    with np.errstate(invalid="ignore"):
        ok = (ax <= FLT_MAX) & (ay <= FLT_MAX) & (az <= FLT_MAX)
        m = np.maximum(np.maximum(ax, ay), az)
        ok &= m > 0
    m = np.where(ok, m, F(1))
    dd = np.where(ok[:, None], d, F(1))
    s = dd / m[:, None]
    ln = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    n = s / ln[:, None]
    phi = M.atan2f(n[:, 2], n[:, 0])
    th = M.asinf(np.minimum(np.maximum(n[:, 1], F(-1)), F(1)))
    u = F(1) - (phi + PI_F) / (F(2) * PI_F)
    v = (th + PIO2_F) / PI_F
    return ok, u, v, th


def radiance(tex, u, v):
    """env at (u, v): bilinear, wrapped in x, clamped in y.  tex float32 [H, W, 3]."""
    h, w = tex.shape[:2]
    x = u * F(w) - F(0.5)
    y = (F(1) - v) * F(h) - F(0.5)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    i0 = x0.astype(np.int64)
    i0 = np.clip(np.where(i0 < 0, i0 + w, i0), 0, w - 1)
    i1 = np.where(i0 + 1 < w, i0 + 1, 0)
    yi = y0.astype(np.int64)
    j0, j1 = np.clip(yi, 0, h - 1), np.clip(yi + 1, 0, h - 1)
    a, b, c, e = tex[j0, i0], tex[j0, i1], tex[j1, i0], tex[j1, i1]
    t0 = a + fx * (b - a)
    t1 = c + fx * (e - c)
    return t0 + fy * (t1 - t0)


def pdf_texel(T, p_env, w, h, i, j, ct):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return (((F(p_env) * T["row_p"][j]) * T["col_p"][j, i]) * F(w * h)) / (TWO_PI2_F * ct)


def lookup(M, tex, T, d, p_env=1.0):
    """The device's RTMI_ENV_PROBE_LOOKUP: float32 [n, 4] = env(d), BSDF-side pdf."""
    h, w = tex.shape[:2]
    ok, u, v, th = env_uv(M, d)
    out = np.zeros((len(ok), 4), np.float32)
    rad = radiance(tex, u, v)
    ct = M.cosf(th)
    i = np.clip(np.floor(u * F(w)).astype(np.int64), 0, w - 1)
    j = np.clip(np.floor((F(1) - v) * F(h)).astype(np.int64), 0, h - 1)
    pdf = pdf_texel(T, p_env, w, h, i, j, ct)
    pdf = np.where((ct > 0) & (F(p_env) > 0), pdf, F(0))
    out[:, :3] = np.where(ok[:, None], rad, F(0))
    out[:, 3] = np.where(ok, pdf, F(0))
    return out


def sample(M, T, w, h, u1, u2, p_env=1.0):
    """The device's RTMI_ENV_PROBE_SAMPLE: float32 [n, 4] = direction, pdf (zeros when there is no sample)."""
    u1 = np.asarray(u1, np.float32)
    u2 = np.asarray(u2, np.float32)
    row_cdf, col_cdf = T["row_cdf"], T["col_cdf"]
    j = np.minimum(np.searchsorted(row_cdf, u1, side="right"), h - 1)
    off = 2.0 * np.arange(h, dtype=np.float64)
    flat = (col_cdf.astype(np.float64) + off[:, None]).ravel()
    i = np.searchsorted(flat, u2.astype(np.float64) + off[j], side="right") - j * w
    i = np.clip(i, 0, w - 1)
    r0 = np.where(j > 0, row_cdf[np.maximum(j - 1, 0)], F(0))
    c0 = np.where(i > 0, col_cdf[j, np.maximum(i - 1, 0)], F(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        fy = np.fmin((u1 - r0) / (row_cdf[j] - r0), ONE_MINUS)
        fx = np.fmin((u2 - c0) / (col_cdf[j, i] - c0), ONE_MINUS)
    u = (i.astype(np.float32) + fx) / F(w)
    v = F(1) - (j.astype(np.float32) + fy) / F(h)
    phi = (F(1) - u) * (F(2) * PI_F) - PI_F
    th = v * PI_F - PIO2_F
    ct = M.cosf(th)
    d = np.stack([ct * M.cosf(phi), M.sinf(th), ct * M.sinf(phi)], axis=1)
    pdf = pdf_texel(T, p_env, w, h, i, j, ct)
    ok = (ct > 0) & (pdf > 0) & (pdf < FLT_MAX) & (F(p_env) > 0)
    out = np.zeros((len(u1), 4), np.float32)
    out[:, :3] = np.where(ok[:, None], d, F(0))
    out[:, 3] = np.where(ok, pdf, F(0))
    return out


# ---- test inputs ----------------------------------------------------------------------------------------------------------
def sun_map(w=256, h=128, sun=2.0e3, sky=0.05):
    """A dim uniform sky and a 2 x 2-texel sun about 35 degrees above the horizon: more than half the weight in under
    0.1 % of the solid angle."""
    m = np.full((h, w, 3), sky, np.float32)
    js, is_ = h // 5, w // 3
    m[js:js + 2, is_:is_ + 2] = np.float32([sun, sun * 0.9, sun * 0.7])
    return m


def lat_long_dirs(n, rng):
    """About n directions: random unit and unnormalised vectors, the poles, the axes, the phi = +-pi seam (z = +-0,
    x < 0), tiny and huge vectors, and a few that see nothing."""
    g = rng.standard_normal((n, 3)).astype(np.float32)
    g[: n // 4] *= rng.uniform(1e-3, 1e3, (n // 4, 1)).astype(np.float32)
    k = np.arange(-8, 9, dtype=np.float32)
    seam = np.stack([np.full_like(k, -1.0), k * F(0.1), np.zeros_like(k)], 1)
    seam_n = seam.copy()
    seam_n[:, 2] = F(-0.0)
    seam_e = seam.copy()
    seam_e[:, 2] = F(1e-7)
    seam_w = seam.copy()
    seam_w[:, 2] = F(-1e-7)
    axes = np.float32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1e-30, 1e-30, 0],
                       [1e-38, -1e-39, 1e-40], [3e38, 3e38, -3e38], [0, 0, 0], [np.inf, 0, 0], [np.nan, 1, 0],
                       [0, 1, 1e-20], [0, -1, -1e-20]])
    return np.concatenate([g, seam, seam_n, seam_e, seam_w, axes]).astype(np.float32)


def uniforms(n, rng):
    """About n pairs (u1, u2) on the 24-bit grid of rtmi_u01, with 0 and 1 - 2^-24 on both sides."""
    q = (rng.integers(0, 1 << 24, (n, 2)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    e = np.float32([0.0, 1.0 - 2.0 ** -24, 0.5, 2.0 ** -24])
    edge = np.stack(np.meshgrid(e, e), -1).reshape(-1, 2)
    return np.concatenate([q, edge]).astype(np.float32)
