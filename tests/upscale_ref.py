"""numpy float32 restatement of include/rtmi_upscale.h: the guided reconstruction of rtmi_upscale, bit for bit, and the
synthetic inputs the CPU and GPU tests share.

Every operation is a float32 numpy operation in the order the header writes; the sums run tap by tap, and a skipped tap
leaves the sums untouched (np.where) instead of adding a zero weight.  rtmi_expf and the quantiser are
tests/denoise_ref.py's.  Used by tests/test_upscale_abi.py, tests/test_upscale_ref.py and tests/test_gpu_upscale.py."""
import numpy as np

from denoise_ref import expf, quantise

F = np.float32
DEFAULTS = dict(normal_power=32, sigma_z=0.05, eps_z=1e-3, albedo_min=1e-3, w_min=1e-3)
BACKGROUND, GUIDED, NEAREST, MISMATCH = 0, 1, 2, 3


def tap_axis(n_lo, n_full):
    """Step 1 along one axis: (x0 int64 [n_full], (w_0, w_1) float32 [n_full])."""
    s = F(n_lo) / F(n_full)
    f = (np.arange(n_full).astype(F) + F(0.5)) * s - F(0.5)
    x0 = np.floor(f)
    t = f - x0
    return x0.astype(np.int64), (F(1.0) - t, t)


def upscale(linear_lo, albedo_lo, normal_lo, depth_lo, albedo, normal, depth, normal_power=32, sigma_z=0.05, eps_z=1e-3,
            albedo_min=1e-3, w_min=1e-3, taps=None):
    """rtmi_upscale -> dict(linear float32 [ny,nx,3], rgb8 uint8 [ny,nx,3], cls uint8 [ny,nx]).  taps: a list that receives
    one dict per tap, in tap order: use (the tap is not skipped), same (it is of p's kind), qx, qy, b, e, w, x."""
    lin_lo, alb_lo, nrm_lo = (np.asarray(a, F) for a in (linear_lo, albedo_lo, normal_lo))
    z_lo, alb, nrm, z = (np.asarray(a, F) for a in (depth_lo, albedo, normal, depth))
    (ly, lx), (ny, nx) = z_lo.shape, z.shape
    sigma_z, eps_z, albedo_min, w_min = F(sigma_z), F(eps_z), F(albedo_min), F(w_min)
    squarings = int(normal_power).bit_length() - 1
    x0, wx = tap_axis(lx, nx)
    y0, wy = tap_axis(ly, ny)
    surf = np.isfinite(z)
    shape = z.shape
    with np.errstate(all="ignore"):
        lenp = (nrm[..., 0] * nrm[..., 0] + nrm[..., 1] * nrm[..., 1]) + nrm[..., 2] * nrm[..., 2]
        zden = sigma_z * z + eps_z
        B, R = np.zeros(shape, F), np.zeros(shape + (3,), F)
        W, C = np.zeros(shape, F), np.zeros(shape + (3,), F)
        best_e, best = np.zeros(shape, F), np.zeros(shape + (3,), F)
        have = np.zeros(shape, bool)
        for j in (0, 1):
            for i in (0, 1):
                qx = np.broadcast_to((x0 + i)[None, :], shape)
                qy = np.broadcast_to((y0 + j)[:, None], shape)
                b = (wy[j][:, None] * wx[i][None, :]).astype(F)
                use = (qx >= 0) & (qx < lx) & (qy >= 0) & (qy < ly) & (b != F(0.0))
                cx, cy = np.clip(qx, 0, lx - 1), np.clip(qy, 0, ly - 1)
                zq, l, aq, nq = z_lo[cy, cx], lin_lo[cy, cx], alb_lo[cy, cx], nrm_lo[cy, cx]
                B = np.where(use, B + b, B)
                R = np.where(use[..., None], R + b[..., None] * l, R)
                sq = np.isfinite(zq)
                xq = l / np.fmax(aq, albedo_min)
                if normal_power == 0:
                    wn = np.ones(shape, F)
                else:
                    lenq = (nq[..., 0] * nq[..., 0] + nq[..., 1] * nq[..., 1]) + nq[..., 2] * nq[..., 2]
                    wn = np.fmax((nrm[..., 0] * nq[..., 0] + nrm[..., 1] * nq[..., 1]) + nrm[..., 2] * nq[..., 2], F(0.0))
                    for _ in range(squarings):
                        wn = wn * wn
                    wn = np.where((lenp == F(0.0)) | (lenq == F(0.0)), F(1.0), wn)
                dz = np.abs(z - zq) / zden
                e = (wn * expf(-dz)).astype(F)
                w = b * e
                ss = use & surf & sq
                bb = use & ~surf & ~sq
                W = np.where(ss, W + w, np.where(bb, W + b, W))
                C = np.where(ss[..., None], C + w[..., None] * xq, np.where(bb[..., None], C + b[..., None] * l, C))
                take = ss & (~have | (e > best_e))
                best_e = np.where(take, e, best_e)
                best = np.where(take[..., None], xq, best)
                have = have | ss | bb
                if taps is not None:
                    taps.append(dict(use=use, same=ss | bb, qx=qx, qy=qy, b=b, e=e, w=w, x=xq))
        ap = np.fmax(alb, albedo_min)
        guided = surf & have & (W > w_min)
        cls = np.where(~have, MISMATCH, np.where(~surf, BACKGROUND, np.where(guided, GUIDED, NEAREST))).astype(np.uint8)
        out = np.where((cls == MISMATCH)[..., None], R / B[..., None],
                       np.where((cls == BACKGROUND)[..., None], C / W[..., None],
                                np.where((cls == GUIDED)[..., None], (C / W[..., None]) * ap, best * ap))).astype(F)
    return {"linear": out, "rgb8": quantise(out), "cls": cls}


def bilinear(linear_lo, ny, nx):
    """The plain bilinear mean of step 4 at every pixel: the same taps, no guide (float32 [ny,nx,3])."""
    lin_lo = np.asarray(linear_lo, F)
    ly, lx = lin_lo.shape[:2]
    x0, wx = tap_axis(lx, nx)
    y0, wy = tap_axis(ly, ny)
    B, R = np.zeros((ny, nx), F), np.zeros((ny, nx, 3), F)
    for j in (0, 1):
        for i in (0, 1):
            qx = np.broadcast_to((x0 + i)[None, :], (ny, nx))
            qy = np.broadcast_to((y0 + j)[:, None], (ny, nx))
            b = (wy[j][:, None] * wx[i][None, :]).astype(F)
            use = (qx >= 0) & (qx < lx) & (qy >= 0) & (qy < ly) & (b != F(0.0))
            l = lin_lo[np.clip(qy, 0, ly - 1), np.clip(qx, 0, lx - 1)]
            B = np.where(use, B + b, B)
            R = np.where(use[..., None], R + b[..., None] * l, R)
    return (R / B[..., None]).astype(F)


# ---- the synthetic inputs of the kernel tests ----------------------------------------------------------------------------
# (lx, ly, nx, ny) of tests/test_gpu_upscale.py's kernel test
SIZES = ((1, 1, 1, 1), (1, 1, 3, 2), (2, 3, 5, 7), (8, 8, 16, 16), (19, 12, 37, 23), (65, 34, 130, 67), (23, 37, 23, 37))
# the parameter sets of the four variants of every size: normal_power 0, 1 and 32, sigma_z and w_min 0 and the default
PARAM_SETS = ({}, dict(normal_power=0, sigma_z=0.0), dict(normal_power=1, w_min=0.0), dict(normal_power=32, sigma_z=0.0, w_min=0.0))


def _features(rng, nx, ny):
    """Colour-free planes of one image: albedo, normal, depth, with a planted depth edge along a diagonal of the unit
    square and a corner without a surface (the same at every resolution), +inf rectangles of this image's own,
    zero-length normals and albedo below albedo_min (some at random, one of each planted)."""
    u = (np.arange(nx) + 0.5) / nx
    v = (np.arange(ny) + 0.5) / ny
    uu, vv = np.meshgrid(u, v)
    depth = np.where(uu + 0.5 * vv < 0.8, 1.0 + 0.2 * uu, 50.0 + 0.2 * vv) + 0.01 * rng.random((ny, nx))
    depth = np.where((uu > 0.7) & (vv > 0.6), np.inf, depth)  # no surface in either image
    for _ in range(2):  # this image's own regions without a surface
        cx, cy, r = rng.random(), rng.random(), 0.1 + 0.2 * rng.random()
        depth = np.where((np.abs(uu - cx) < r) & (np.abs(vv - cy) < r), np.inf, depth)
    n = rng.normal(size=(ny, nx, 3))
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    n = np.where((uu < 0.5)[..., None], np.array([0.0, 0.0, 1.0]), n)  # a flat half, where the normal weight is near 1
    n[rng.random((ny, nx)) < 0.05] = 0.0
    a = rng.random((ny, nx, 3))
    a[rng.random((ny, nx)) < 0.05] = 1e-4
    a[rng.random((ny, nx)) < 0.02] = 0.0
    if nx * ny >= 16:
        k = nx * ny
        a.reshape(k, 3)[k // 2], a.reshape(k, 3)[k // 3], n.reshape(k, 3)[k // 4] = 0.0, 1e-4, 0.0
    return a.astype(F), n.astype(F), depth.astype(F)


def synthetic(size, variant):
    """The inputs of rtmi_upscale for SIZES' entry `size` and variant 0..3, and PARAM_SETS[variant]: random colours over
    2^-10 .. 2^10 and _features at both resolutions, placed independently.  The full-resolution pixel (0, 0) and the
    low-resolution pixels its taps can reach are forced so that it comes out class `variant`: so the four variants of a
    size reach every class even at 1 x 1."""
    lx, ly, nx, ny = size
    rng = np.random.default_rng([lx, ly, nx, ny, variant])
    lin_lo = (2.0 ** rng.uniform(-10, 10, (ly, lx, 3))).astype(F)
    alb_lo, nrm_lo, z_lo = _features(rng, lx, ly)
    alb, nrm, z = _features(rng, nx, ny)
    blk = (slice(0, 2), slice(0, 2))
    up = np.array([0.0, 0.0, 1.0], F)
    z[0, 0], z_lo[blk] = {BACKGROUND: (np.inf, np.inf), GUIDED: (1.0, 1.0), NEAREST: (1.0, 1000.0), MISMATCH: (1.0, np.inf)}[variant]
    nrm[0, 0], nrm_lo[blk] = up, up
    planes = dict(linear_lo=lin_lo, albedo_lo=alb_lo, normal_lo=nrm_lo, depth_lo=z_lo, albedo=alb, normal=nrm, depth=z)
    return planes, dict(PARAM_SETS[variant])
