"""Next-event estimation's formulas (include/rtmi_nee.h) restated in numpy float64, for the CPU and GPU
tests: the Lambertian's scatter density, the light densities, the power-heuristic weights, and the quadrature of
F = the integral of p_b over a light's solid angle, which gives the known answers a * Le * F."""
import numpy as np


def pb_lambert(w, n):
    """Density (solid angle) of direction w for the reference's Lambertian, which scatters toward n + a uniform point of
    the unit ball: (2/pi) max(0, cos)^3.  w, n: [..., 3]."""
    w = np.asarray(w, np.float64)
    n = np.asarray(n, np.float64)
    c = np.sum(w * n, -1) / np.sqrt(np.sum(w * w, -1) * np.sum(n * n, -1))
    return np.where(c > 0, (2.0 / np.pi) * np.maximum(c, 0.0) ** 3, 0.0)


PB_ISOTROPIC = 1.0 / (4.0 * np.pi)


def rect_pdf(x, q, axis, area):
    """Solid-angle density of a uniform point q on a rect (normal along `axis`) seen from x: d^2 / (|cos_l| A)."""
    w = np.asarray(q, np.float64) - np.asarray(x, np.float64)
    d2 = np.sum(w * w, -1)
    return d2 * np.sqrt(d2) / (np.abs(w[..., axis]) * area)


def one_minus_cos_max(x, c, r):
    """1 - cos(theta_max) of the cone a sphere (c, r) subtends from x, as s / (1 + sqrt(1 - s)); nan inside."""
    dc = np.asarray(c, np.float64) - np.asarray(x, np.float64)
    s = r * r / np.sum(dc * dc, -1)
    return np.where(s < 1, s / (1 + np.sqrt(np.maximum(1 - s, 0))), np.nan)


def cone_pdf(x, c, r):
    """Uniform-cone density 1 / (2 pi (1 - cos theta_max)); 0 from inside the sphere."""
    omc = one_minus_cos_max(x, c, r)
    return np.where(np.isnan(omc), 0.0, 1.0 / (2 * np.pi * np.where(np.isnan(omc), 1.0, omc)))


def mis_light(pb, pl):
    """p_b p_l / (p_b^2 + p_l^2) as ratios (the factor of a light sample)."""
    pb, pl = np.asarray(pb, np.float64), np.asarray(pl, np.float64)
    lo, hi = np.minimum(pb, pl), np.maximum(pb, pl)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(hi > 0, lo / np.where(hi > 0, hi, 1), 0.0)
    return r / (1 + r * r)


def mis_bsdf(pb, pl):
    """p_b^2 / (p_b^2 + p_l^2) as ratios (the weight of an emitter a diffuse scatter hits); 1 when p_l = 0."""
    pb, pl = np.asarray(pb, np.float64), np.asarray(pl, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r1 = pl / np.where(pb > 0, pb, 1)
        r2 = pb / np.where(pl > 0, pl, 1)
    return np.where(pl <= 0, 1.0, np.where(pb >= pl, 1 / (1 + r1 * r1), r2 * r2 / (1 + r2 * r2)))


def f_rect(x, n, corner, ea, eb, na=96, nb=96):
    """F = integral of p_b over the solid angle of the rect corner + [0,1] ea + [0,1] eb seen from x (midpoint rule in
    area measure: dw = |cos_l| dA / d^2).  Returns (F, an error bound from the halved grid)."""
    def quad(ma, mb):
        ua = (np.arange(ma) + 0.5) / ma
        ub = (np.arange(mb) + 0.5) / mb
        q = corner + ua[:, None, None] * ea + ub[None, :, None] * eb
        w = q - x
        d2 = np.sum(w * w, -1)
        nl = np.cross(ea, eb)
        area = np.linalg.norm(nl)
        cos_l = np.abs(np.sum(w * nl, -1)) / (np.sqrt(d2) * area)
        return np.sum(pb_lambert(w, n) * cos_l / d2) * area / (ma * mb)
    full = quad(na, nb)
    half = quad(na // 2, nb // 2)
    return full, abs(full - half)


def f_sphere_below(r, h):
    """F for a sphere of radius r whose centre is at height h straight above the vertex (normal pointing at it):
    integral of (2/pi) cos^3 over the cone = 1 - cos^4(theta_max) = 1 - (1 - r^2/h^2)^2."""
    return 1.0 - (1.0 - r * r / (h * h)) ** 2


def f_sphere(x, n, c, r, m=256):
    """F for a sphere (c, r) seen from x with normal n: quadrature over the cone in (cos theta, phi)."""
    x, n, c = (np.asarray(v, np.float64) for v in (x, n, c))
    dc = c - x
    dist = np.linalg.norm(dc)
    w = dc / dist
    omc = float(one_minus_cos_max(x, c, r))
    t1 = np.cross(w, [1.0, 0, 0] if abs(w[0]) < 0.9 else [0, 1.0, 0])
    t1 /= np.linalg.norm(t1)
    t2 = np.cross(w, t1)
    u = (np.arange(m) + 0.5) / m
    ct = 1 - u * omc
    st = np.sqrt(np.maximum(0, 1 - ct * ct))
    phi = 2 * np.pi * u
    d = (ct[:, None, None] * w + (st[:, None] * np.cos(phi)[None, :])[..., None] * t1 +
         (st[:, None] * np.sin(phi)[None, :])[..., None] * t2)
    return float(np.mean(pb_lambert(d, n)) * 2 * np.pi * omc)


def lambert_directions(n, count, rng):
    """normalize(n + u), u uniform in the unit ball (the reference's Lambertian scatter), by rejection."""
    out = []
    while sum(len(o) for o in out) < count:
        u = rng.uniform(-1, 1, (count, 3))
        u = u[np.sum(u * u, -1) < 1]
        d = np.asarray(n, np.float64) + u
        out.append(d / np.linalg.norm(d, axis=-1, keepdims=True))
    return np.concatenate(out)[:count]
