"""The denoiser's public interface (include/rtmi_denoise.h), without a GPU.

* the header compiles as C99 -pedantic; the layout of rtmi_denoise_params holds through header -> ctypes (abi.py) ->
  #[repr(C)] (bindings/rust/src/sys.rs), with the machinery of test_abi_layout.py;
* librtmi.so exports the functions the header declares, abi.py and sys.rs declare them, and no other symbol list has them;
* every bad argument is refused before any HIP call: RTMI_ERR_INVALID for NULL pointers, sizes and parameters out of
  range, RTMI_ERR_UNSUPPORTED for flag bits;
* rtmi_expf compiled from the header by gcc gives the bits of the numpy restatement (tests/denoise_ref.py), is within
  2 ulp of the correctly rounded exp on [-87.3, 0] and returns +0 below the cut-off;
* the Python wrapper refuses shapes and dtypes that do not match before it calls."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as ref
from raytracing_rust_amd import abi, denoise

import abi_kit as kit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
FIELDS = ["iterations", "normal_power", "sigma_l", "sigma_z", "eps_l", "eps_z", "albedo_min", "flags"]
# isolated=False: the frame pipeline, the upscaler and the tone mapper embed rtmi_denoise_params and say the word
FAMILY = kit.Family("rtmi_denoise.h", ["rtmi_denoise", "rtmi_probe_expf"],
                    {"rtmi_denoise_params": (abi.DenoiseParams, "RtmiDenoiseParams", 32, FIELDS)},
                    word="denoise", isolated=False, includes=["rtmi.h", "rtmi_math.h"])


def test_header_is_c99(tmp_path):
    FAMILY.c99(tmp_path, holds="rtmi_expf(0.0f) == 1.0f",
               body="rtmi_denoise_params p = {5u, 128u, 4.0f, 1.0f, 1e-10f, 1e-3f, 1e-3f, 0u}; (void)p;")


def test_header_and_stdio_together(tmp_path):
    """The colour's standard error is not called `stderr`, the macro of <stdio.h>."""
    src = tmp_path / "stdio.c"
    src.write_text('#include <stdio.h>\n#include "rtmi_denoise.h"\nint main(void) { (void)&rtmi_denoise; return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + INCLUDE, str(src), "-c", "-o",
                    str(tmp_path / "stdio.o")], check=True)


def test_layout_chain_header_ctypes_rust():
    FAMILY.layout()
    assert kit.compiled_layout("rtmi_denoise.h")["rtmi_denoise_params"][:2] == (32, 4)


def test_exports_and_declarations_agree():
    FAMILY.exports()


def test_the_header_keeps_to_itself():
    FAMILY.isolation()
    FAMILY.constants()


def _params(**kw):
    d = dict(ref.DEFAULTS, flags=0)
    d.update(kw)
    return abi.DenoiseParams(*(d[f] for f in FIELDS))


def _call(nx=8, ny=4, p="default", null=None, se=True):
    lib = abi.load_rtmi()
    buf = np.zeros(max(nx * ny, 1) * 3, np.float32)
    ptr = buf.ctypes.data
    args = {"linear": ptr, "albedo": ptr, "normal": ptr, "depth": ptr, "stderr": ptr if se else None}
    if null:
        args[null] = None
    prm = _params() if p == "default" else p
    rc = lib.rtmi_denoise(0, nx, ny, C.byref(prm) if prm is not None else None, args["linear"], args["albedo"],
                          args["normal"], args["depth"], args["stderr"], ptr, None)
    return rc, (lib.rtmi_last_error() or b"").decode()


@pytest.mark.parametrize("null", ["linear", "albedo", "normal", "depth"])
def test_null_inputs_are_invalid(null):
    rc, msg = _call(null=null)
    assert rc == 1 and "NULL" in msg, msg


def test_null_params_is_invalid():
    rc, msg = _call(p=None)
    assert rc == 1 and "NULL" in msg, msg


@pytest.mark.parametrize("nx,ny", [(0, 4), (4, 0), (32769, 1), (1, 32769)])
def test_bad_sizes_are_invalid(nx, ny):
    rc, msg = _call(nx=nx, ny=ny)
    assert rc == 1 and "nx and ny" in msg, msg


BAD = [("iterations", 11), ("normal_power", 3), ("normal_power", 2048), ("normal_power", 96),
       ("sigma_l", -1.0), ("sigma_l", float("inf")), ("sigma_l", float("nan")), ("sigma_z", -0.5), ("sigma_z", float("inf")),
       ("eps_l", 0.0), ("eps_l", -1e-10), ("eps_l", float("inf")), ("eps_z", 0.0), ("eps_z", float("nan")),
       ("albedo_min", 0.0), ("albedo_min", float("-inf"))]


@pytest.mark.parametrize("field,value", BAD)
def test_bad_parameters_are_invalid(field, value):
    rc, msg = _call(p=_params(**{field: value}))
    assert rc == 1 and field in msg, msg


@pytest.mark.parametrize("flags", [1, 2, 1 << 31])
def test_flag_bits_are_unsupported(flags):
    rc, msg = _call(p=_params(flags=flags))
    assert rc == 2 and "flags" in msg, msg
    rc, msg = _call(p=_params(flags=flags, iterations=11))  # argument errors first
    assert rc == 1, msg


@pytest.mark.skipif(abi.load_rtmi().rtmi_device_count() > 0, reason="CPU-only check")
@pytest.mark.parametrize("kw", [dict(), dict(iterations=0), dict(normal_power=0, sigma_l=0.0), dict(normal_power=1024, iterations=10),
                                dict(sigma_z=0.0)])
def test_valid_arguments_reach_the_device_check(kw):
    """Boundary values are accepted: without a GPU the call gets as far as the device check, NULL stderr_rgb included."""
    for se in (True, False):
        rc, msg = _call(p=_params(**kw), se=se)
        assert rc == 3 and "device" in msg, msg
    rc, msg = _call(nx=32768, ny=1)
    assert rc == 3, msg


def test_probe_expf_refuses_null():
    lib = abi.load_rtmi()
    assert lib.rtmi_probe_expf(0, None, None, 4) == 1


DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include "rtmi_denoise.h"
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "rb");
    long n;
    float *x, *y;
    if (!f) return 2;
    fseek(f, 0, SEEK_END); n = ftell(f) / 4; fseek(f, 0, SEEK_SET);
    x = malloc(n * 4); y = malloc(n * 4);
    if (fread(x, 4, n, f) != (size_t)n) return 3;
    fclose(f);
    for (long i = 0; i < n; i++) y[i] = rtmi_expf(x[i]);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(y, 4, n, f) != (size_t)n) return 4;
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_expf(tmp_path_factory):
    d = tmp_path_factory.mktemp("expf")
    src, exe = d / "drv.c", d / "drv"
    src.write_text(DRIVER)
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + INCLUDE, str(src), "-o",
                    str(exe)], check=True)
    x = ref.expf_sweep()
    (d / "x.bin").write_bytes(x.tobytes())
    subprocess.run([str(exe), str(d / "x.bin"), str(d / "y.bin")], check=True)
    return x, np.frombuffer((d / "y.bin").read_bytes(), np.float32)


def test_expf_c_equals_restatement(host_expf):
    x, y = host_expf
    assert x.size > 10_000_000
    want = ref.expf(x)
    assert y.view(np.uint32).tobytes() == want.view(np.uint32).tobytes()


def test_expf_special_values(host_expf):
    x = np.array([0.0, -0.0, -np.inf, np.nan, -87.33654, -87.3366, -104.0, np.inf, 88.8, 1.0], np.float32)
    y = ref.expf(x)
    assert y[0] == 1.0 and y[1] == 1.0 and y[2] == 0.0 and np.isnan(y[3])
    assert y[4] >= np.finfo(np.float32).tiny  # the cut-off's own value is a normal number
    assert y[5] == 0.0 and y[6] == 0.0 and y[7] == np.inf and y[8] == np.inf
    assert y[9] == np.float32(np.e)


def test_expf_accuracy(host_expf):
    x, y = host_expf
    inside = np.isfinite(x) & (x >= np.float32(-87.3)) & (x <= 0)
    exact = np.exp(x[inside].astype(np.float64)).astype(np.float32)
    ulp = np.abs(y[inside].view(np.int32).astype(np.int64) - exact.view(np.int32).astype(np.int64))
    assert ulp.max() <= 2, (ulp.max(), x[inside][ulp.argmax()])
    below = x < ref.EXPF_LOW
    assert below.sum() > 1000 and np.all(y[below].view(np.uint32) == 0)
    # no subnormal results anywhere
    assert not np.any((y > 0) & (y < np.finfo(np.float32).tiny))


def test_python_wrapper_checks_shapes_and_dtypes():
    f = np.zeros((4, 5, 3), np.float32)
    z = np.zeros((4, 5), np.float32)
    for args in [(f[:, :4], f, f, z), (f, f, f, z[:3]), (f, f, f[..., :2], z), (f, f, f, f)]:
        with pytest.raises(ValueError):
            denoise(*args)
    with pytest.raises(ValueError):
        denoise(f, f.astype(np.float64), f, z)
    with pytest.raises(ValueError):
        denoise(f, f, f, z.astype(np.float16))
    with pytest.raises(ValueError):
        denoise(f, f, f, z, stderr=f[:2])


def test_restatement_basics():
    """Properties of the numpy restatement itself that the device tests lean on."""
    rng = np.random.default_rng(3)
    ny, nx = 9, 11
    lin = rng.random((ny, nx, 3), dtype=np.float32)
    alb = rng.random((ny, nx, 3), dtype=np.float32)
    nrm = rng.standard_normal((ny, nx, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=2, keepdims=True)).astype(np.float32)
    dep = (1 + rng.random((ny, nx))).astype(np.float32)
    dep[2, 3] = np.inf
    out0, rgb0 = ref.denoise(lin, alb, nrm, dep, iterations=0)
    assert out0.tobytes() == lin.tobytes() and np.array_equal(rgb0, ref.quantise(lin))
    out, _ = ref.denoise(lin, alb, nrm, dep, stderr=lin * np.float32(0.1))
    assert out[2, 3].tobytes() == lin[2, 3].tobytes()  # not a surface: copied
    assert np.all(np.isfinite(out))
    # a constant image with a constant albedo stays what it is within rounding
    c = np.full((ny, nx, 3), 0.25, np.float32)
    out, _ = ref.denoise(c, np.full_like(c, 0.5), np.tile(np.float32([0, 0, 1]), (ny, nx, 1)), np.ones((ny, nx), np.float32))
    assert np.abs(out - c).max() < 1e-6
