"""numpy float32 restatement of include/rtmi_denoise.h: rtmi_expf, the a-trous filter of rtmi_denoise and the quantiser.

Every operation is a float32 numpy operation in the order the header writes, so the results are the device's bits.  Sums
run tap by tap (never np.sum, whose pairwise order is not the device's), and a skipped tap leaves the sums untouched
(np.where) instead of adding a zero weight.  Used by tests/test_denoise_abi.py and tests/test_gpu_denoise.py."""
import numpy as np

F = np.float32
EXPF_LOW = F(-87.33654)
EXPF_HIGH = F(88.72283)
K3 = (F(0.25), F(0.5), F(0.25))
K5 = (F(1 / 16), F(0.25), F(0.375), F(0.25), F(1 / 16))

DEFAULTS = dict(iterations=5, normal_power=128, sigma_l=4.0, sigma_z=1.0, eps_l=1e-10, eps_z=1e-3, albedo_min=1e-3)


def expf(x):
    """rtmi_expf on a float32 array."""
    x = np.asarray(x, dtype=F)
    with np.errstate(all="ignore"):
        k = np.rint(x * F(1.44269504088896341))
        r = x - k * F(0.693359375)
        r = r - k * F(-2.12194440e-4)
        p = F(1.9875691500e-4) * r + F(1.3981999507e-3)
        p = p * r + F(8.3334519073e-3)
        p = p * r + F(4.1665795894e-2)
        p = p * r + F(1.6666665459e-1)
        p = p * r + F(5.0000001201e-1)
        e = (p * (r * r) + r) + F(1.0)
        n = np.where(np.isfinite(k), k, 0).astype(np.int64)
        big = n > 127
        e = np.where(big, e * F(2.0), e)
        n = np.where(big, n - 1, n)
        scale = (np.clip(n + 127, 1, 254).astype(np.uint32) << np.uint32(23)).view(F)
        out = e * scale
    out = np.where(x > EXPF_HIGH, F(np.inf), out)
    out = np.where(x < EXPF_LOW, F(0.0), out)
    return np.where(np.isnan(x), x, out).astype(F)


def quantise(lin):
    """rtmi_render's rgb8 of a float32 image: sqrt in f64, clamp with NaN -> 0, (int)(255.99*g)."""
    with np.errstate(all="ignore"):
        g = np.sqrt(lin.astype(np.float64))
    g = np.where(g > 0.0, np.where(g < 1.0, g, 1.0), 0.0)
    return (255.99 * g).astype(np.int32).astype(np.uint8)


def _gradient(z, surf, axis):
    """gx (axis 1) or gy (axis 0) of the prepass."""
    zf = np.moveaxis(z, axis, 0)
    sf = np.moveaxis(surf, axis, 0)
    n = zf.shape[0]
    g = np.zeros_like(zf)
    for i in range(n):
        has_p = sf[i + 1] if i + 1 < n else np.zeros_like(sf[i])
        has_m = sf[i - 1] if i > 0 else np.zeros_like(sf[i])
        zp = zf[i + 1] if i + 1 < n else zf[i]
        zm = zf[i - 1] if i > 0 else zf[i]
        central = F(0.5) * (zp - zm)
        g[i] = np.where(has_p & has_m, central, np.where(has_p, zp - zf[i], np.where(has_m, zf[i] - zm, F(0.0))))
    return np.moveaxis(g, 0, axis)


def _lum(x):
    return (F(0.2126) * x[..., 0] + F(0.7152) * x[..., 1]) + F(0.0722) * x[..., 2]


def _shift(a, dy, dx, fill):
    """a[y + dy, x + dx], `fill` outside the image."""
    ny, nx = a.shape[:2]
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, ny), slice(0, ny - dy)) if dy >= 0 else (slice(0, ny + dy), slice(-dy, ny))
    xs, xd = (slice(dx, nx), slice(0, nx - dx)) if dx >= 0 else (slice(0, nx + dx), slice(-dx, nx))
    if ys.stop > ys.start and xs.stop > xs.start:
        out[yd, xd] = a[ys, xs]
    return out


def denoise(linear, albedo, normal, depth, stderr=None, iterations=5, normal_power=128, sigma_l=4.0, sigma_z=1.0,
            eps_l=1e-10, eps_z=1e-3, albedo_min=1e-3):
    """rtmi_denoise -> (linear float32 [ny,nx,3], rgb8 uint8 [ny,nx,3])."""
    linear = np.asarray(linear, F)
    albedo = np.asarray(albedo, F)
    normal = np.asarray(normal, F)
    z = np.asarray(depth, F)
    sigma_l, sigma_z, eps_l, eps_z, albedo_min = F(sigma_l), F(sigma_z), F(eps_l), F(eps_z), F(albedo_min)
    surf = np.isfinite(z)
    if iterations == 0:
        out = linear.copy()
        return out, quantise(out)
    with np.errstate(all="ignore"):
        a = np.fmax(albedo, albedo_min)
        x = linear / a
        if stderr is not None:
            se = np.asarray(stderr, F)
            s_r = F(0.2126) * (se[..., 0] / a[..., 0])
            s_g = F(0.7152) * (se[..., 1] / a[..., 1])
            s_b = F(0.0722) * (se[..., 2] / a[..., 2])
            var = (s_r * s_r + s_g * s_g) + s_b * s_b
        else:
            var = np.zeros(z.shape, F)
        gx = _gradient(z, surf, 1)
        gy = _gradient(z, surf, 0)
        nlen = (normal[..., 0] * normal[..., 0] + normal[..., 1] * normal[..., 1]) + normal[..., 2] * normal[..., 2]
        squarings = int(normal_power).bit_length() - 1
        for it in range(iterations):
            s = 1 << it
            if stderr is not None:
                kv = np.zeros(z.shape, F)
                ks = np.zeros(z.shape, F)
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        ok = _shift(surf, dy, dx, False)
                        k = K3[dy + 1] * K3[dx + 1]
                        kv = np.where(ok, kv + k * _shift(var, dy, dx, F(0.0)), kv)
                        ks = np.where(ok, ks + k, ks)
                gv = kv / ks
                inv_l = F(1.0) / (sigma_l * np.sqrt(gv) + eps_l)
                lp = _lum(x)
            W = np.zeros(z.shape, F)
            C = np.zeros(x.shape, F)
            V = np.zeros(z.shape, F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = s * dy, s * dx
                    ok = _shift(surf, oy, ox, False)
                    h = K5[dy + 2] * K5[dx + 2]
                    xq = _shift(x, oy, ox, F(0.0))
                    vq = _shift(var, oy, ox, F(0.0))
                    if dy == 0 and dx == 0:
                        w = np.full(z.shape, h, F)
                    else:
                        if normal_power == 0:
                            wn = np.ones(z.shape, F)
                        else:
                            nq = _shift(normal, oy, ox, F(0.0))
                            d = (normal[..., 0] * nq[..., 0] + normal[..., 1] * nq[..., 1]) + normal[..., 2] * nq[..., 2]
                            wn = np.fmax(d, F(0.0))
                            for _ in range(squarings):
                                wn = wn * wn
                            flat = (nlen == F(0.0)) | (_shift(nlen, oy, ox, F(0.0)) == F(0.0))
                            wn = np.where(flat, F(1.0), wn)
                        zq = _shift(z, oy, ox, F(0.0))
                        dz = np.abs(z - zq) / (sigma_z * (np.abs(gx * F(ox)) + np.abs(gy * F(oy))) + eps_z)
                        if stderr is not None:
                            dl = np.abs(lp - _lum(xq)) * inv_l
                        else:
                            dl = np.zeros(z.shape, F)
                        w = (h * wn) * expf(-(dl + dz))
                    W = np.where(ok, W + w, W)
                    C = np.where(ok[..., None], C + w[..., None] * xq, C)
                    V = np.where(ok, V + (w * w) * vq, V)
            x = np.where(surf[..., None], C / W[..., None], x)
            var = np.where(surf, V / (W * W), var)
        out = np.where(surf[..., None], x * a, linear).astype(F)
    return out, quantise(out)


def expf_sweep():
    """The float32 inputs of the rtmi_expf tests: every 61st bit pattern over [-104, 0], every pattern within 4096 ulp of
    the cut-off and of -0, and +-0, -inf and NaN."""
    lo = int(np.array(-104.0, F).view(np.uint32))
    cut = int(EXPF_LOW.view(np.uint32))
    bits = np.concatenate([np.arange(0x80000000, lo + 1, 61, dtype=np.uint64),
                           np.arange(cut - 4096, cut + 4097, dtype=np.uint64),
                           np.arange(0x80000000, 0x80000000 + 4097, dtype=np.uint64),
                           np.array([0x00000000, 0xff800000, 0x7fc00000, 0xffc00000], np.uint64)]).astype(np.uint32)
    return bits.view(F)
