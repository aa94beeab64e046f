"""numpy restatement of include/rtmi_tonemap.h, operation for operation: the metering histogram, the solve and the apply.

fp32 steps are numpy float32 operations in the header's order (each rounds once, as the device's do under
-ffp-contract=off), the f64 steps numpy float64, the integers Python ints (exact; the device's are 64-bit).  rtmi_expf is
tests/denoise_ref.expf; rtmi_logf, whose polynomial is fused, comes from a gcc build of include/rtmi_math.h (`logf`), the
way tests/env_ref.ContractMath builds its functions.  Used by tests/test_tonemap_abi.py, tests/test_tonemap_ref.py and
tests/test_gpu_tonemap.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from denoise_ref import expf

F = np.float32
D = np.float64
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
OPS = {"clamp": 0, "reinhard": 1, "aces": 2}
OETFS = {"gamma2": 0, "srgb": 1}
EXPOSURES = {"manual": 0, "auto": 1}
DEFAULTS = dict(op="aces", oetf="srgb", exposure="auto", ev=0.0, white=float("inf"), key=0.18, log2_min=-12.0, log2_max=12.0,
                p_low=0.10, p_high=0.95, speed_up=3.0, speed_down=1.0, adapt_min=None, adapt_max=None)

_SRC = r"""
#include "rtmi_math.h"
void v_logf(const float *x, float *y, long n) { for (long i = 0; i < n; i++) y[i] = rtmi_logf(x[i]); }
"""
_lib = None


def logf(x):
    """rtmi_logf on a float32 array."""
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="rtmi_tonemap_ref_")
        src, so = os.path.join(d, "m.c"), os.path.join(d, "liblogf_contract.so")
        with open(src, "w") as f:
            f.write(_SRC)
        subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I" + INCLUDE, src, "-o", so, "-lm"],
                       check=True)
        _lib = C.CDLL(so)
        _lib.v_logf.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
    x = np.ascontiguousarray(x, dtype=F)
    y = np.empty_like(x)
    _lib.v_logf(x.ctypes.data, y.ctypes.data, x.size)
    return y


def params(**kw):
    """The header's defaults with `kw` over them, every float rounded to float32 as the struct holds it."""
    p = dict(DEFAULTS)
    p.update(kw)
    if p["adapt_min"] is None:
        p["adapt_min"] = p["log2_min"]
    if p["adapt_max"] is None:
        p["adapt_max"] = p["log2_max"]
    for k, v in p.items():
        if k not in ("op", "oetf", "exposure"):
            p[k] = F(v)
    return p


def luminance(linear):
    x = np.asarray(linear, F)
    with np.errstate(all="ignore"):
        return (F(0.2126) * x[..., 0] + F(0.7152) * x[..., 1]) + F(0.0722) * x[..., 2]


def bin_index(l, p):
    """(counted, bin) of float32 luminances: step 1 of the header."""
    l = np.asarray(l, F)
    with np.errstate(all="ignore"):
        counted = np.isfinite(l) & (l > 0)
        scale = F(256.0) / (p["log2_max"] - p["log2_min"])
        e = logf(np.where(counted, l, F(1.0))) * F(1.44269504)
        t = (e - p["log2_min"]) * scale
        b = np.where(t < 0, 0, np.where(t >= 256, 255, np.where(counted, t, F(0)).astype(np.int64)))
    return counted, b


def histogram(linear, p):
    """The 256 bins (uint32) of an image."""
    counted, b = bin_index(luminance(linear).ravel(), p)
    return np.bincount(b[counted], minlength=256).astype(np.uint32)


def solve(bins, p, a, has, dt):
    """Step 2 (AUTO) -> (E, a', m, counted, kept, has'): a, has = the handle's adapted value and whether it exists (False
    on the first apply after create or reset)."""
    n = int(np.asarray(bins, np.uint64).sum())
    if n == 0:
        a2 = F(a) if has else F(0.0)
        m, K = a2, 0
    else:
        lo, hi = int(D(n) * D(p["p_low"])), int(D(n) * D(p["p_high"]))
        if hi == lo:
            if lo == n:
                lo = n - 1
            hi = lo + 1
        K = hi - lo
        S = below = 0
        for b in range(256):
            c = int(bins[b])
            S += max(0, min(below + c, hi) - max(below, lo)) * b
            below += c
        m = F(D(p["log2_min"]) + (D(S) / D(K) + D(0.5)) * ((D(p["log2_max"]) - D(p["log2_min"])) / D(256.0)))
        if not has:
            a2 = m
        else:
            a = F(a)
            s = p["speed_up"] if m > a else p["speed_down"]
            al = F(1.0) - expf(-(F(dt) * s))
            a2 = a + (m - a) * al
        a2 = np.fmin(np.fmax(F(a2), p["adapt_min"]), p["adapt_max"])
        has = True
    with np.errstate(all="ignore"):
        E = p["key"] * expf((p["ev"] - F(a2)) * F(0.69314718))
    return F(E), F(a2), F(m), n, K, has


def srgb(y):
    """The sRGB transfer function of float32 y -> (bytes uint8, display float32)."""
    y = np.asarray(y, F)
    with np.errstate(all="ignore"):
        v = np.where(y > 0, np.where(y < 1, y, F(1.0)), F(0.0)).astype(F)
        hi = np.fmin(F(1.055) * expf(logf(np.where(v > 0, v, F(1.0))) * F(0.41666667)) - F(0.055), F(1.0))
        s = np.where(v <= F(0.0031308), F(12.92) * v, hi).astype(F)
        q = (s * F(255.0) + F(0.5)).astype(np.int32).astype(np.uint8)
    return q, s


def curve(x, p):
    """The tone curve of float32 x = linear*E."""
    x = np.asarray(x, F)
    op = OPS[p["op"]]
    if op == 0:
        return x
    with np.errstate(all="ignore"):
        x = np.fmax(x, F(0.0))
        if op == 1:
            w2 = p["white"] * p["white"]
            return ((x * (F(1.0) + x / w2)) / (F(1.0) + x)).astype(F)
        return ((x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14))).astype(F)


def apply(linear, E, p):
    """Step 3 -> (rgb8 uint8, display float32) of a float32 image under the factor E."""
    with np.errstate(all="ignore"):
        y = curve(np.asarray(linear, F) * F(E), p)
        if OETFS[p["oetf"]] == 1:
            return srgb(y)
        g = np.sqrt(y.astype(D))
        g = np.where(g > 0.0, np.where(g < 1.0, g, 1.0), 0.0)
        return (255.99 * g).astype(np.int32).astype(np.uint8), g.astype(F)


class Tonemap:
    """The state a handle carries across applies.  apply() -> (rgb8, display, state) with state the eight words of
    rtmi_tonemap_state as a dict (reserved left out: they are 0)."""

    def __init__(self, **kw):
        self.p = params(**kw)
        self.reset()

    def reset(self):
        self.a, self.has, self.applies = F(0.0), False, 0

    def apply(self, linear, dt=0.0):
        p = self.p
        self.applies += 1
        if EXPOSURES[p["exposure"]] == 0:
            E = expf(p["ev"] * F(0.69314718))
            st = dict(exposure=F(E), adapted_log2=F(0.0), metered_log2=F(0.0), counted=0, kept=0, applies=self.applies)
        else:
            E, a2, m, n, K, self.has = solve(histogram(linear, p), p, self.a, self.has, dt)
            self.a = a2
            st = dict(exposure=E, adapted_log2=a2, metered_log2=m, counted=n, kept=K, applies=self.applies)
        rgb8, display = apply(linear, st["exposure"], p)
        return rgb8, display, st


def state_words(st):
    """A state dict as the eight uint32 words of rtmi_tonemap_state."""
    f = np.array([st["exposure"], st["adapted_log2"], st["metered_log2"]], F).view(np.uint32)
    return np.concatenate([f, np.array([st["counted"], st["kept"], st["applies"], 0, 0], np.uint32)])


def sample_image(ny, nx, seed, lo=-30.0, hi=30.0):
    """A float32 [ny,nx,3] image for the metering tests: luminances log-uniform over 2^lo .. 2^hi with colour casts, and
    among them zeros, negatives, NaN, +-inf, denormals and greys that lie on bin edges of the default range."""
    rng = np.random.default_rng(seed)
    n = ny * nx
    lum = np.exp2(rng.uniform(lo, hi, n)).astype(F)
    img = (lum[:, None] * rng.uniform(0.2, 1.8, (n, 3))).astype(F)
    special = [(0.0, 0.0, 0.0), (-1.0, -2.0, -0.5), (np.nan, 1.0, 1.0), (np.inf, 0.0, 0.0), (-np.inf, 1.0, 1.0),
               (1e-41, 1e-41, 1e-41), (1e-45, 0.0, 0.0), (3e38, 3e38, 3e38), (-1.0, 3.0, 0.0)]
    special += [(2.0 ** k,) * 3 for k in (-13, -12, -3, 0, 5, 12, 13)]  # on the edges of the bins and of the range
    special += [(float(np.exp2(F(-12 + 24 * b / 256))),) * 3 for b in (1, 17, 128, 255)]
    idx = rng.permutation(n)
    for k, v in enumerate(special[:max(0, n - 1)]):  # at least one ordinary pixel survives
        img[idx[k]] = v
    return img.reshape(ny, nx, 3)
