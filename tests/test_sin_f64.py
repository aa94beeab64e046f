"""The f64 render mode's sine (csrc/rtmi_sin_f64.hpp) against mpmath: the correctly rounded double of sin(x) at every argument here.

The header is plain C++ for the host and the device.  Here g++ compiles it (-ffp-contract=off, as the device build has it) and
every result must equal mpmath's sine rounded once to a double: arguments 0 and tiny, within pi/4 (no reduction), the doubles
nearest to multiples of pi/2 (the reduction cancels all but a few bits), the ranges the render evaluates (10 p of a checker,
scale p.x + 5 turb of a noise texture, tests/test_gpu_f64_mode.py), [2^32, 2^36) of tests/test_gpu_tex_contract.py's plate,
and up to the limit 2^40.  glibc's sine, which the f64 oracle calls, is counted against the same reference: it is within 0.55
ULP, so it is the rounded value except near a midpoint.  Measured here: 17 of the 25 118 arguments (0.7 in 1000).
The GPU test asks the same of the device's copy through rtmi_probe_math_f64."""
import ctypes as C
import math
import os
import subprocess

import mpmath
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "raytracing_rust_amd", "csrc")
LIMIT = 2.0 ** 40

_SRC = r"""
#include "rtmi_sin_f64.hpp"
extern "C" void v_sin_cr(const double *x, double *y, long n) { for (long i = 0; i < n; i++) y[i] = rtmi_sin64::sin_cr(x[i]); }
"""


@pytest.fixture(scope="module")
def args():
    rng = np.random.default_rng(5)
    tiny = np.finfo(np.float64).tiny
    edges = [0.0, -0.0, 5e-324, -5e-324, tiny, -tiny, tiny / 3, 1e-300, 1e-16, 2.0 ** -27, 2.0 ** -26, 0.5, 1.0, -1.0,
             math.pi / 4, math.nextafter(math.pi / 4, 1.0), math.pi / 2, math.pi, -math.pi, 1e8, LIMIT * (1 - 2.0 ** -53), -LIMIT * (1 - 2.0 ** -53)]
    with mpmath.workprec(200):
        ks = np.concatenate([np.arange(1, 1025), rng.integers(1, 2 ** 39, 3000)])
        near = np.array([float(int(k) * mpmath.pi / 2) for k in ks])
    near = np.concatenate([near, np.nextafter(near, 0.0), np.nextafter(near, np.inf), -near])
    x = np.concatenate([np.array(edges), near, rng.uniform(-0.8, 0.8, 2000), rng.uniform(-2000, 2000, 3000),
                        rng.uniform(2.0 ** 32, 2.0 ** 36, 3000) * rng.choice([-1.0, 1.0], 3000),
                        rng.uniform(-1, 1, 1000) * 2.0 ** rng.uniform(-60, 40, 1000)])
    x = x[np.abs(x) < LIMIT]
    with mpmath.workprec(400):  # |x| < 2^40 and sin(x) >= 2^-62 |x| or so for a double: 400 bits round correctly
        want = np.array([float(mpmath.sin(mpmath.mpf(float(v)))) for v in x])
    want = np.where(x == 0.0, x, want)  # the sign of -0
    return x, want


def _same(a, b):
    return a.view(np.int64) == b.view(np.int64)


def test_host_copy_is_correctly_rounded(args, tmp_path):
    x, want = args
    src, so = tmp_path / "s.cpp", tmp_path / "libsin64.so"
    src.write_text(_SRC)
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, str(src), "-o", str(so)],
                   check=True)
    lib = C.CDLL(str(so))
    lib.v_sin_cr.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
    got = np.empty_like(x)
    lib.v_sin_cr(x.ctypes.data, got.ctypes.data, len(x))
    bad = np.flatnonzero(~_same(got, want))
    libm = np.flatnonzero(~_same(np.sin(x), want))
    print("sin_cr: %d arguments, %d not correctly rounded; glibc's sine: %d not correctly rounded" % (len(x), len(bad), len(libm)))
    assert len(x) > 25000
    assert len(bad) == 0, [(float.hex(float(x[i])), float.hex(float(got[i])), float.hex(float(want[i]))) for i in bad[:8]]
    assert len(libm) * 100 < len(x)  # what "bit-identical to the oracle through a sine" can mean: all but a few in 1000


@pytest.mark.gpu
def test_device_copy_is_correctly_rounded(args):
    from raytracing_rust_amd import abi
    x, want = args
    lib = abi.load_rtmi()
    got = np.zeros_like(x)
    assert lib.rtmi_probe_math_f64(0, x.ctypes.data, x.ctypes.data, got.ctypes.data, len(x)) == 0, lib.rtmi_last_error()
    bad = np.flatnonzero(~_same(got, want))
    assert len(bad) == 0, [(float.hex(float(x[i])), float.hex(float(got[i])), float.hex(float(want[i]))) for i in bad[:8]]
    # from the limit on, infinities and NaN: the device library's sine
    y = np.array([LIMIT, -LIMIT, 1e15, 1.7e308, np.inf, -np.inf, np.nan])
    out = np.zeros_like(y)
    assert lib.rtmi_probe_math_f64(0, y.ctypes.data, y.ctypes.data, out.ctypes.data, len(y)) == 0, lib.rtmi_last_error()
    with np.errstate(invalid="ignore"):
        ref = np.sin(y)
    assert np.isnan(out[4:]).all() and np.allclose(out[:4], ref[:4], rtol=0, atol=1e-15)
