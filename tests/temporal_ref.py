"""numpy float32 restatement of include/rtmi_temporal.h: the host's double inverse of the camera matrix and the push.

Every operation is a float32 numpy operation in the order the header writes (the inverse: float64), so the results are
the device's bits.  The four taps are added one by one, and an unused tap leaves the sums untouched (np.where) instead of
adding a zero weight.  Temporal keeps the history between pushes as rtmi_temporal does.  Used by
tests/test_temporal_ref.py and tests/test_gpu_temporal.py."""
import numpy as np

F = np.float32
D = np.float64

DEFAULTS = dict(max_history=32, alpha_min=0.0, depth_tol=0.05, normal_min=0.9, albedo_min=1e-3, demodulate=True)


def _lowered(cam):
    return cam.lower() if hasattr(cam, "lower") else cam


def _vec(c, name):
    return np.array(list(getattr(c, name)), F)


def camera_inverse(cam):
    """Step 4's M: the inverse of the matrix with columns (horizontal, vertical, llc - origin), in double, each entry
    rounded once to float32.  ValueError for a singular or non-finite matrix (rtmi_temporal_push: RTMI_ERR_INVALID)."""
    c = _lowered(cam)
    h = _vec(c, "horizontal").astype(D)
    w = _vec(c, "vertical").astype(D)
    g = _vec(c, "lower_left_corner").astype(D) - _vec(c, "origin").astype(D)

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    with np.errstate(all="ignore"):
        r = [cross(w, g), cross(g, h), cross(h, w)]
        det = (h[0] * r[0][0] + h[1] * r[0][1]) + h[2] * r[0][2]
        if not np.isfinite(det) or det == 0.0:
            raise ValueError("singular camera")
        return np.array([[F(r[j][k] / det) for k in range(3)] for j in range(3)], F)


def _len2(n):
    return (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]


class Temporal:
    """rtmi_temporal: push(cam, linear, albedo, normal, depth, stderr=None) -> dict(linear, stderr (or None), history,
    motion), float32 arrays shaped as Temporal.push of the package returns them."""

    def __init__(self, nx, ny, max_history=32, alpha_min=0.0, depth_tol=0.05, normal_min=0.9, albedo_min=1e-3,
                 demodulate=True):
        self.nx, self.ny = nx, ny
        self.max_history, self.alpha_min, self.depth_tol = F(max_history), F(alpha_min), F(depth_tol)
        self.normal_min, self.albedo_min, self.demodulate = F(normal_min), F(albedo_min), demodulate
        self.prev = None

    def reset(self):
        self.prev = None

    def push(self, cam, linear, albedo, normal, depth, stderr=None):
        c = _lowered(cam)
        nx, ny = self.nx, self.ny
        linear, albedo, normal, z = (np.asarray(a, F) for a in (linear, albedo, normal, depth))
        assert linear.shape == albedo.shape == normal.shape == (ny, nx, 3) and z.shape == (ny, nx)
        M = camera_inverse(c)
        with_se = stderr is not None
        if self.prev is not None and self.prev["with_se"] != with_se:
            raise ValueError("stderr must be supplied on every push since the reset or on none")
        org, llc, hor, ver = (_vec(c, k) for k in ("origin", "lower_left_corner", "horizontal", "vertical"))
        one, zero, half = F(1.0), F(0.0), F(0.5)
        with np.errstate(all="ignore"):
            surf = np.isfinite(z)
            # 2. demodulate
            a = np.fmax(albedo, self.albedo_min) if self.demodulate else np.ones_like(albedo)
            x = linear / a
            if with_se:
                e = np.asarray(stderr, F) / a
                v = e * e
            else:
                v = np.zeros_like(x)
            # 3, 4. where the pixel's point was in the previous frame
            ii = np.broadcast_to(np.arange(nx, dtype=F)[None, :], (ny, nx))
            rr = np.broadcast_to(np.arange(ny, dtype=F)[:, None], (ny, nx))
            fx, fr, z_exp = ii, rr, z
            mx = my = np.zeros((ny, nx), F)
            valid = np.full((ny, nx), self.prev is not None)
            if self.prev is not None and self.prev["cam_bytes"] != bytes(c):
                u = (ii + half) / F(nx)
                vv = (np.broadcast_to(np.arange(ny)[::-1].astype(F)[:, None], (ny, nx)) + half) / F(ny)
                d = [((llc[k] + hor[k] * u) + ver[k] * vv) - org[k] for k in range(3)]
                ln = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                s = z / ln
                po, m = self.prev["org"], self.prev["M"]
                q = [(org[k] + d[k] * s) - po[k] for k in range(3)]
                ca = (m[0, 0] * q[0] + m[0, 1] * q[1]) + m[0, 2] * q[2]
                cb = (m[1, 0] * q[0] + m[1, 1] * q[1]) + m[1, 2] * q[2]
                cc = (m[2, 0] * q[0] + m[2, 1] * q[1]) + m[2, 2] * q[2]
                z_exp = np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
                valid = cc > zero
                fx = np.where(valid, (ca / cc) * F(nx) - half, ii)
                fr = np.where(valid, F(ny - 1) - ((cb / cc) * F(ny) - half), rr)
                mx = np.where(valid, fx - ii, zero)
                my = np.where(valid, fr - rr, zero)
            # 5. the four bilinear taps
            ok = (surf & valid & np.isfinite(fx) & np.isfinite(fr) & (fx >= F(-1.0)) & (fx < F(nx)) & (fr >= F(-1.0))
                  & (fr < F(ny)))
            W = np.zeros((ny, nx), F)
            L = np.zeros((ny, nx), F)
            X = np.zeros((ny, nx, 3), F)
            V = np.zeros((ny, nx, 3), F)
            if self.prev is not None:
                fxs, frs = np.where(ok, fx, zero), np.where(ok, fr, zero)
                bx, by = np.floor(fxs), np.floor(frs)
                wx1, wy1 = fxs - bx, frs - by
                wx, wy = (one - wx1, wx1), (one - wy1, wy1)
                tx, ty = bx.astype(np.int64), by.astype(np.int64)
                lc = _len2(normal)
                tol = self.depth_tol * z_exp
                h = self.prev
                for k in range(4):
                    qx, qy = tx + (k & 1), ty + (k >> 1)
                    w = wy[k >> 1] * wx[k & 1]
                    inside = (qx >= 0) & (qx < nx) & (qy >= 0) & (qy < ny)
                    cx, cy = np.clip(qx, 0, nx - 1), np.clip(qy, 0, ny - 1)
                    hN, hz, hn, hx, hv = h["N"][cy, cx], h["z"][cy, cx], h["n"][cy, cx], h["x"][cy, cx], h["v"][cy, cx]
                    lt = _len2(hn)
                    dot = (normal[..., 0] * hn[..., 0] + normal[..., 1] * hn[..., 1]) + normal[..., 2] * hn[..., 2]
                    n_ok = (lc == zero) | (lt == zero) | (dot >= self.normal_min * np.sqrt(lc * lt))
                    use = ok & (w > zero) & inside & (hN > zero) & (np.abs(hz - z_exp) <= tol) & n_ok
                    W = np.where(use, W + w, W)
                    X = np.where(use[..., None], X + w[..., None] * hx, X)
                    L = np.where(use, L + w * hN, L)
                    V = np.where(use[..., None], V + (w * w)[..., None] * hv, V)
            # 6. blend
            hist = W > zero
            N = np.where(hist, np.fmin(L / W + one, self.max_history), one)
            al = np.fmax(one / N, self.alpha_min)
            be = one - al
            y = np.where(hist[..., None], be[..., None] * (X / W[..., None]) + al[..., None] * x, x)
            WW = W * W
            t = np.where(hist[..., None], (be * be)[..., None] * (V / WW[..., None]) + (al * al)[..., None] * v, v)
            # 7. store and output
            s3 = surf[..., None]
            self.prev = {"cam_bytes": bytes(c), "org": org, "M": M, "with_se": with_se,
                         "N": np.where(surf, N, zero).astype(F), "z": z.copy(), "n": normal.copy(),
                         "x": np.where(s3, y, zero).astype(F), "v": np.where(s3, t, zero).astype(F)}
            out = {"linear": np.where(s3, y * a, linear).astype(F),
                   "stderr": np.where(s3, np.sqrt(t) * a, np.asarray(stderr, F)).astype(F) if with_se else None,
                   "history": self.prev["N"].copy(),
                   "motion": np.stack([np.where(surf, mx, zero), np.where(surf, my, zero)], axis=2).astype(F)}
        return out


def mean_bound(k):
    """The relative bound of a K-frame running mean against the float64 mean of its frames: a push rounds 1/N, 1 - 1/N,
    two products and one sum, each within 2^-24 of terms no larger than the largest frame value, and carries the error
    of the push before it with a weight below one; so 4*K*2^-24 times that value."""
    return 4.0 * k * 2.0 ** -24


def pinhole(look_from, look_at, view_up=(0.0, 1.0, 0.0), vertical_fov=40.0, aspect=1.0, focus_dist=10.0):
    """An abi.Camera (lens radius 0) from the usual look-at description, computed in double and rounded to float32."""
    from raytracing_rust_amd import abi

    lf, la, vu = (np.array(t, D) for t in (look_from, look_at, view_up))
    hh = np.tan(np.radians(vertical_fov) / 2.0)
    hw = aspect * hh
    w = (lf - la) / np.linalg.norm(lf - la)
    u = np.cross(vu, w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    c = abi.Camera()
    for name, val in (("origin", lf), ("lower_left_corner", lf - hw * focus_dist * u - hh * focus_dist * v - focus_dist * w),
                      ("horizontal", 2.0 * hw * focus_dist * u), ("vertical", 2.0 * hh * focus_dist * v), ("u", u), ("v", v)):
        setattr(c, name, (abi.C.c_float * 3)(*[float(F(t)) for t in val]))
    c.time0, c.time1, c.lens_radius = 0.0, 1.0, 0.0
    return c


def plane_depth(cam, nx, ny, distance):
    """The depth plane (Euclidean distance along the pixel-centre rays, float32 [ny,nx]) of a plane that faces the
    camera at the perpendicular `distance`, in double from the camera's float32 fields."""
    org, llc, hor, ver = (_vec(cam, k).astype(D) for k in ("origin", "lower_left_corner", "horizontal", "vertical"))
    u = (np.arange(nx) + 0.5) / nx
    v = (np.arange(ny)[::-1] + 0.5) / ny
    d = (llc + hor * u[None, :, None]) + ver * v[:, None, None] - org
    fwd = np.cross(hor, ver)
    fwd /= np.linalg.norm(fwd)
    along = d @ fwd
    return (distance * np.linalg.norm(d, axis=2) / np.abs(along)).astype(F)
