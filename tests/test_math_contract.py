"""include/rtmi_math.h: accuracy of the fp32 transcendental contract against libm on the ranges
the path uses (CPU), and bit-equality of device and host evaluation (GPU)."""
import ctypes as C

import numpy as np
import pytest

from raytracing_rust_amd import abi


def _host_eval(orc32, name, *args):
    fn = getattr(orc32.lib, name)
    return np.array([fn(*[float(a[i]) for a in args]) for i in range(len(args[0]))], np.float32)


def test_accuracy_against_libm(orc32):
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-60000, 60000, 20000), rng.uniform(-10, 10, 20000), [0.0, -0.0, 1e-30]]).astype(np.float32)
    s = _host_eval(orc32, "orc_rtmi_sinf", x)
    # absolute error: Cody-Waite reduction loses ~ulp(x) of phase
    assert np.max(np.abs(s - np.sin(x.astype(np.float64))) / (1.0 + np.abs(x) * 6e-8 / 1e-7)) < 1e-6
    u = ((rng.integers(1, 1 << 24, 40000)).astype(np.float32) * np.float32(2.0 ** -24))
    l = _host_eval(orc32, "orc_rtmi_logf", u)
    assert np.max(np.abs(l - np.log(u.astype(np.float64))) / np.maximum(1e-3, np.abs(np.log(u.astype(np.float64))))) < 3e-7
    assert orc32.lib.orc_rtmi_logf(0.0) == -np.inf
    n = rng.normal(size=(20000, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n = n.astype(np.float32)
    a = _host_eval(orc32, "orc_rtmi_atan2f", n[:, 2], n[:, 0])
    assert np.max(np.abs(a - np.arctan2(n[:, 2].astype(np.float64), n[:, 0].astype(np.float64)))) < 1e-6
    y = _host_eval(orc32, "orc_rtmi_asinf", n[:, 1])
    assert np.max(np.abs(y - np.arcsin(n[:, 1].astype(np.float64)))) < 1e-6
    assert np.isnan(orc32.lib.orc_rtmi_asinf(1.0000001))  # like Rust's asin outside [-1,1]


def test_cos_accuracy_against_libm(orc32):
    """rtmi_cosf (NEE's cone sampler, phi = 2 pi u in [0, 2 pi)) against f64 libm: on the sampler's range, every 24-bit
    uniform's phi included at a stride, and on the sin test's wide range with the same phase allowance."""
    rng = np.random.default_rng(2)
    u = (np.arange(0, 1 << 24, 97, dtype=np.int64).astype(np.float32) * np.float32(2.0 ** -24))
    phi = np.float32(2.0) * np.float32(np.pi) * u
    x = np.concatenate([phi, rng.uniform(0.0, 2 * np.pi, 20000), [0.0, -0.0, 2 * np.pi, np.pi, np.pi / 2]]).astype(np.float32)
    c = _host_eval(orc32, "orc_rtmi_cosf", x)
    assert np.max(np.abs(c - np.cos(x.astype(np.float64)))) < 1e-6
    assert orc32.lib.orc_rtmi_cosf(0.0) == 1.0
    w = np.concatenate([rng.uniform(-60000, 60000, 20000), rng.uniform(-10, 10, 20000)]).astype(np.float32)
    cw = _host_eval(orc32, "orc_rtmi_cosf", w)
    assert np.max(np.abs(cw - np.cos(w.astype(np.float64))) / (1.0 + np.abs(w) * 6e-8 / 1e-7)) < 1e-6
    # the two share one reduction: sin^2 + cos^2 = 1 to a few ulp
    s = _host_eval(orc32, "orc_rtmi_sinf", x)
    assert np.max(np.abs(s.astype(np.float64) ** 2 + c.astype(np.float64) ** 2 - 1.0)) < 4e-7
    assert _host_eval(orc32, "orc_rtmi_cosf", np.array([np.inf, np.nan, 2.0 ** 21], np.float32)).tolist() == [0.0, 0.0, 0.0]


def test_u01_is_24_bit_exact():
    from raytracing_rust_amd.philox import Stream

    s = Stream(3)
    for _ in range(100):
        w = s.u32()
        u = (w >> 8) * 2.0 ** -24
        assert np.float32(u) == u and 0.0 <= u < 1.0


@pytest.mark.gpu
def test_device_equals_host_bit_for_bit(orc32):
    lib = abi.load_rtmi()
    rng = np.random.default_rng(1)
    n = 1 << 16
    cases = {
        0: (np.concatenate([rng.uniform(-60000, 60000, n // 2), rng.uniform(-8, 8, n // 2)]).astype(np.float32), None, "orc_rtmi_sinf"),
        1: ((rng.integers(0, 1 << 24, n)).astype(np.float32) * np.float32(2.0 ** -24), None, "orc_rtmi_logf"),
        2: (rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32), "orc_rtmi_atan2f"),
        3: (rng.uniform(-1.0, 1.0, n).astype(np.float32), None, "orc_rtmi_asinf"),
        7: (np.concatenate([np.float32(2.0 * np.pi) * rng.uniform(0.0, 1.0, n // 2), rng.uniform(-60000, 60000, n // 2)]
                           ).astype(np.float32), None, "orc_rtmi_cosf"),
    }
    for op, (x, y, name) in cases.items():
        out = np.zeros(n, np.float32)
        rc = lib.rtmi_probe_math(op, x.ctypes.data, y.ctypes.data if y is not None else None, out.ctypes.data, n)
        assert rc == 0, lib.rtmi_last_error()
        ref = _host_eval(orc32, name, *([x] if y is None else [x, y]))
        same = (out.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(out) & np.isnan(ref))
        assert same.all(), "%s: %d of %d differ" % (name, int((~same).sum()), n)
    # IEEE division and square root: device == numpy float32 (correctly rounded on both)
    a = rng.normal(size=n).astype(np.float32) * 1000
    b = rng.normal(size=n).astype(np.float32)
    out = np.zeros(n, np.float32)
    assert lib.rtmi_probe_math(4, a.ctypes.data, b.ctypes.data, out.ctypes.data, n) == 0
    assert np.array_equal(out.view(np.uint32), (a / b).view(np.uint32))
    pos = np.abs(a)
    assert lib.rtmi_probe_math(5, pos.ctypes.data, None, out.ctypes.data, n) == 0
    assert np.array_equal(out.view(np.uint32), np.sqrt(pos).view(np.uint32))


@pytest.mark.gpu
def test_device_philox_kat():
    lib = abi.load_rtmi()
    from test_philox import KAT

    ctr = np.array([k[0] for k in KAT], np.uint32)
    key = np.array([k[1] for k in KAT], np.uint32)
    out = np.zeros((len(KAT), 4), np.uint32)
    assert lib.rtmi_probe_philox(ctr.ctypes.data, key.ctypes.data, out.ctypes.data, len(KAT)) == 0
    assert out.tolist() == [k[2] for k in KAT]


@pytest.mark.gpu
def test_instance_transforms_on_device():
    """Traslate / Rotate{X,Y,Z} chains as the render kernels apply them (traslate.rs:18-24, rotate.rs:85-113),
    against the same fp32 operations in numpy: world->object for the ray, object->world for the hit record."""
    import ctypes as C

    from raytracing_rust_amd import abi

    lib = abi.load_rtmi()
    rng = np.random.default_rng(3)
    n = 4096
    a = (rng.normal(size=(n, 3)) * 4).astype(np.float32)
    b = rng.normal(size=(n, 3)).astype(np.float32)
    AB = {1: (1, 2), 2: (2, 0), 3: (0, 1)}  # Axis::X/Y/Z -> (a_axis, b_axis), rotate.rs:13-19

    def fwd(o, xf):  # Rotate::hit ray part / Traslate::hit
        o = o.copy()
        if xf.kind == 0:
            return o - np.array([xf.x, xf.y, xf.z], np.float32)
        ia, ib = AB[xf.kind]
        s, c = np.float32(xf.x), np.float32(xf.y)
        na = c * o[:, ia] + s * o[:, ib]
        nb = (-s) * o[:, ia] + c * o[:, ib]
        o[:, ia], o[:, ib] = na, nb
        return o

    def inv(p, xf, is_point):
        p = p.copy()
        if xf.kind == 0:
            return p + np.array([xf.x, xf.y, xf.z], np.float32) if is_point else p
        ia, ib = AB[xf.kind]
        s, c = np.float32(xf.x), np.float32(xf.y)
        na = c * p[:, ia] - s * p[:, ib]
        nb = s * p[:, ia] + c * p[:, ib]
        p[:, ia], p[:, ib] = na, nb
        return p

    chains = [[(1, 33.0)], [(2, 33.0)], [(3, 33.0)], [(3, 180.0)], [(0, (0.5, -1.0, 2.0))],
              [(0, (0.5, -1.0, 2.0)), (3, -40.0), (2, 20.0)], [(3, 10.0), (1, -70.0), (0, (1.0, 1.0, 1.0)), (3, 5.0)]]
    for chain in chains:
        xs = (abi.Xform * len(chain))()
        for k, (kind, arg) in enumerate(chain):
            xs[k].kind = kind
            if kind == 0:
                xs[k].x, xs[k].y, xs[k].z = arg
            else:
                xs[k].x, xs[k].y, xs[k].z = np.sin(np.radians(arg)), np.cos(np.radians(arg)), 0.0
        out = np.zeros((n, 13), np.float32)
        assert lib.rtmi_probe_xform(xs, len(chain), a.ctypes.data, b.ctypes.data, out.ctypes.data, n) == 0
        o, d, p, nn = a, b, a, b
        for xf in xs:  # outermost wrapper first
            o = fwd(o, xf)
            d = fwd(d, xf) if xf.kind != 0 else d
        for xf in reversed(list(xs)):  # innermost first on the way back
            p = inv(p, xf, True)
            nn = inv(nn, xf, False)
        assert np.array_equal(out[:, 0:3], o), chain
        assert np.array_equal(out[:, 3:6], d), chain
        assert np.array_equal(out[:, 6:9], p), chain
        assert np.array_equal(out[:, 9:12], nn), chain
        assert (out[:, 12] == (1.0 if any(k for k, _ in chain) else 0.0)).all()
