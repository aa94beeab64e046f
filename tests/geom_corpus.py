"""Deterministic corpus and exact reference for tests/test_geom_contract.py.

Every input is an fp32 value (held in a Python float / float64 array).  The exact reference evaluates the
reference's formulas on those inputs in real arithmetic: decisions with fractions.Fraction, square roots and
transcendentals with mpmath at 200 bits.  Where an input makes an intermediate non-finite (a zero direction component
in a rect or slab test) the real-number formula has no value; the caller then takes the f64 literal oracle's answer,
i.e. the reference's IEEE semantics.

Sources restated: sphere.rs:37-77 and :115-164 (Sphere / MovingSphere::hit), rect.rs:39-69, cube.rs:21-86 with
hittable.rs:37-47, aabb.rs:31-44, medium.rs:29-30, material.rs:9-28, sphere.rs:9-15."""
import math
from fractions import Fraction as Fr

import mpmath
import numpy as np

mpmath.mp.prec = 200
EPS = 2.0 ** -23  # fp32 machine epsilon (one ulp of 1.0)
FMAX = float(np.finfo(np.float32).max)
PLANE_AXES = {0: (0, 1, 2), 1: (1, 2, 0), 2: (2, 0, 1)}  # rect.rs:40-44: (k, a, b) for YZ, ZX, XY
GROUP = 64  # PRIM cases per primitive: the device probe's list-scan entry point needs a wave-uniform index


def f32(x):
    return float(np.float32(x))


def is_f32(q):
    """q (a Fraction) is exactly an fp32 value: then an fp32 operation that produces it is exact."""
    v = float(np.float32(float(q)))
    return math.isfinite(v) and Fr(v) == q


def mpf(q):
    return mpmath.mpf(q.numerator) / q.denominator if isinstance(q, Fr) else mpmath.mpf(q)


def norm_q(v):
    return mpmath.sqrt(mpf(sum(c * c for c in v)))


# ---------------------------------------------------------------------------------------------------------------------
# primitives: specs that build the same hittable through any backend (Host, Oracle)
# ---------------------------------------------------------------------------------------------------------------------
def make(api, spec):
    mat = api.Lambertian(api.SolidTexture(0.5, 0.5, 0.5))
    k = spec["kind"]
    if k == "sphere":
        h = api.Sphere(spec["c"], spec["r"], mat)
    elif k == "msphere":
        h = api.MovingSphere(spec["c0"], spec["c1"], spec["t0"], spec["t1"], spec["r"], mat)
    elif k == "rect":
        h = api.Rect(spec["plane"], *spec["rect"], spec["k"], mat)
    else:
        h = api.Cube(spec["lo"], spec["hi"], mat)
    for w in spec.get("wrap", ()):
        h = api.Traslate(h, w[1]) if w[0] == "T" else api.Rotate(w[1], h, w[2])
    return h


def lower_prims(host, specs):
    """planes A, B, meta and xforms of each spec's primitive as the lowering produces them (the primitive as the first
    member of a nested list, so that a wrapper chain becomes the primitive's own: an instanced primitive), and the
    indices of the specs the lowering leaves out."""
    from raytracing_rust_amd import abi

    A, B, meta, xforms, dropped = [], [], [], [], []
    for g, s in enumerate(specs):
        w = host.HittableList()
        lst = host.HittableList()
        lst.push(make(host, s))
        lst.push(host.Sphere((0.0, 0.0, 0.0), 1.0, host.Lambertian(host.SolidTexture(0.5, 0.5, 0.5))))
        w.push(lst)
        a = host.lower(w).arrays()
        if len(a["prim_meta"]) == 1:  # the lowering dropped the primitive (a rect with x0 > x1 or y0 > y1): the dummy
            dropped.append(g)       # sphere stands in, the caller skips the group
        m = a["prim_meta"][0]
        cnt = (m.flags >> abi.RTMI_PRIMFLAG_XF_COUNT_SHIFT) & 15
        first = m.flags >> abi.RTMI_PRIMFLAG_XF_FIRST_SHIFT
        mm = abi.PrimMeta()
        mm.material, mm.inv_dt, mm.type = m.material, m.inv_dt, m.type
        mm.flags = m.flags & ((1 << abi.RTMI_PRIMFLAG_XF_FIRST_SHIFT) - 1)
        if cnt:
            mm.flags |= len(xforms) << abi.RTMI_PRIMFLAG_XF_FIRST_SHIFT
            xforms.extend(a["xforms"][first:first + cnt])
        A.append(a["prim_a"][0])
        B.append(a["prim_b"][0])
        meta.append(mm)
    return np.array(A, np.float32), np.array(B, np.float32), meta, xforms, dropped


# ---------------------------------------------------------------------------------------------------------------------
# the corpus
# ---------------------------------------------------------------------------------------------------------------------
# (radius, |o - c|) pairs of the reference scenes: random_spheres (0.2 and 1 seen from 13, the radius-1000 ground),
# two_spheres / two_perlin_spheres (10, 2), final_scene (10 in the sphere box, 50, 70, 80, 100 seen from ~800, the
# radius-5000 fog), and the small far spheres of the r04 discriminant bug
SPHERE_PAIRS = [(0.2, 13.0), (0.2, 300.0), (1.0, 13.0), (1000.0, 1000.5), (1000.0, 1013.0), (2.0, 26.0), (10.0, 30.0),
                (10.0, 800.0), (50.0, 700.0), (70.0, 800.0), (70.0, 1500.0), (80.0, 900.0), (100.0, 600.0),
                (5000.0, 1200.0), (-0.45, 3.0), (-15.0, 600.0)]
FAR_SMALL = [(10.0, 800.0), (0.2, 300.0), (70.0, 1500.0)]  # the negative control's spheres


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _perp(u, rng):
    p = np.cross(u, _unit(rng))
    return p / np.linalg.norm(p)


class Corpus:
    """PRIM cases in groups of GROUP rays per primitive spec, plus the AABB / SHADE / UV cases.  `cls` labels every case
    with its edge class; test_corpus_composition asserts how many of each there are."""

    def __init__(self, seed=20261015):
        self.rng = np.random.default_rng(seed)
        self.specs, self.rays, self.cls = [], [], []
        self._spheres()
        self._moving()
        self._rects()
        self._cubes()
        self._instanced()
        self.rays = np.array(self.rays, np.float64)  # n x 9: o, d, time, t_min, t_max (fp32 values)
        self.pidx = np.repeat(np.arange(len(self.specs)), GROUP)
        self.cls = np.array(self.cls)
        self.aabb, self.aabb_cls = self._aabb()
        self.shade, self.shade_cls = self._shade()
        self.uv, self.uv_cls = self._uv()
        self.medium_groups = [g for g, s in enumerate(self.specs) if s["kind"] == "sphere" and not s.get("wrap")]

    # -- helpers --
    def _group(self, spec, rays, cls):
        assert len(rays) == GROUP and len(cls) == GROUP
        self.specs.append(spec)
        for r in rays:
            assert len(r) == 9
            self.rays.append([f32(x) for x in r])
        self.cls.extend(cls)

    def _dscale(self):
        return 10.0 ** self.rng.uniform(-3.0, 3.0)  # |d| from 1e-3 to 1e3

    def _sphere_rays(self, c, r, dist, time=0.0):
        """rays at a sphere: aimed across the disc, tangent to within a few ulp, from the fp32 hit point of a
        previous bounce, from inside"""
        rng, rays, cls = self.rng, [], []
        ar = abs(r)
        for j in range(GROUP):
            u = _unit(rng)
            o = c + dist * u
            kind = j % 8
            if kind in (0, 1, 2):  # across the disc, some misses
                tgt = c + _perp(u, rng) * ar * rng.uniform(0.0, 1.3)
                lab = "across"
            elif kind in (3, 4):  # tangent: aimed at a point at distance r (1 +- few ulp) from the centre
                tgt = c + _perp(u, rng) * ar * (1.0 + rng.choice([-1, 1]) * rng.integers(0, 6) * 2.0 ** -23)
                lab = "tangent"
            elif kind == 5:  # from inside the sphere (hollow glass, the medium's second query)
                o = c + _unit(rng) * ar * rng.uniform(0.0, 0.9)
                tgt = o + _unit(rng)
                lab = "inside"
            else:  # kinds 6, 7: filled below from the hit points of the first rays
                tgt = None
                lab = "surface"
            if tgt is None:
                rays.append(None)
            else:
                d = (tgt - o)
                d = d / np.linalg.norm(d) * self._dscale()
                rays.append([*o, *d, time, 0.001, FMAX])
            cls.append(lab)
        return rays, cls

    def _surface_fill(self, spec, rays, orc32):
        """origins on the fp32 hit point of a previous bounce (orc32 contract): the scattered ray leaves with t_min = 0.001"""
        from oracle.oracle import ARITH_DEVICE

        h = make(orc32, spec)
        src = [r for r in rays if r is not None]
        for j, r in enumerate(rays):
            if r is not None:
                continue
            for k in range(len(src)):
                s = src[(j + k) % len(src)]
                rec = orc32.hit(h, s[0:3], s[3:6], s[6], s[7], FMAX, flags=ARITH_DEVICE)
                if rec is not None:
                    break
            if rec is None:  # nothing hits (time0 == time1: a NaN centre): a point of the nominal surface instead
                n = _unit(self.rng)
                p = np.array(spec.get("c", spec.get("c0"))) + n * spec["r"]
            else:
                p, n = rec["p"], rec["normal"]
            d = _unit(self.rng)
            if j % 2 == 0 and np.dot(d, n) < 0:  # half outward (the next bounce), half any direction
                d = -d
            rays[j] = [*p, *(d * self._dscale()), s[6], 0.001, FMAX]
        return rays

    # -- groups --
    def _spheres(self):
        from oracle.oracle import Oracle

        orc32 = Oracle("f32")
        for r, dist in SPHERE_PAIRS:
            for rep in range(2):
                c = np.array([f32(x) for x in self.rng.uniform(-1.0, 1.0, 3) * (0 if rep == 0 else 400.0)])
                spec = {"kind": "sphere", "c": c, "r": f32(r), "pair": (r, dist)}
                rays, cls = self._sphere_rays(c, r, dist)
                self._group(spec, self._surface_fill(spec, rays, orc32), cls)
        orc32.free_all()

    def _moving(self):
        from oracle.oracle import Oracle

        orc32 = Oracle("f32")
        for r, dist, t0, t1 in ((0.2, 13.0, 0.0, 1.0), (50.0, 700.0, 0.0, 1.0), (2.0, 20.0, 0.5, 0.5), (1.0, 8.0, 0.25, 2.0)):
            c0 = np.array([f32(x) for x in self.rng.uniform(-300.0, 300.0, 3)])
            c1 = np.array([f32(x) for x in c0 + self.rng.uniform(-30.0, 30.0, 3)])
            spec = {"kind": "msphere", "c0": c0, "c1": c1, "t0": f32(t0), "t1": f32(t1), "r": f32(r)}
            for time in ((0.0, 1.0) if t0 != t1 else (0.5,)) + ((0.3721,) if t0 != t1 else (0.0,)):
                time = f32(time)
                f = 0.0 if t1 == t0 else (time - t0) / (t1 - t0)
                rays, cls = self._sphere_rays(c0 + (c1 - c0) * f, r, dist, time)
                cls = ["moving_t0t1_equal" if t0 == t1 else "moving"] * GROUP
                self._group(spec, self._surface_fill(spec, rays, orc32), cls)
        orc32.free_all()

    def _rects(self):
        rng = self.rng
        for plane in (0, 1, 2):
            for scale in (1.0, 300.0):
                x0, y0 = f32(rng.integers(-4, 0) * scale), f32(rng.integers(-4, 0) * scale)
                x1, y1 = f32(rng.integers(1, 5) * scale), f32(rng.integers(1, 5) * scale)
                kk = f32(rng.integers(-3, 4) * scale)
                spec = {"kind": "rect", "plane": plane, "rect": (x0, y0, x1, y1), "k": kk}
                self._group(spec, *self._plane_rays(plane, (x0, y0, x1, y1), kk, scale))
        # final_scene's light: x0 > x1 (rect.rs never accepts it)
        spec = {"kind": "rect", "plane": 1, "rect": (423.0, 147.0, 123.0, 412.0), "k": 554.0}
        rays, cls = self._plane_rays(1, (123.0, 147.0, 423.0, 412.0), 554.0, 100.0)
        self._group(spec, rays, ["degenerate_x0_gt_x1"] * GROUP)
        # denormal differences: a ray parallel to an edge one denormal step outside (or on) it; x1 = 2^-125
        e = 2.0 ** -125
        spec = {"kind": "rect", "plane": 2, "rect": (-1.0, -1.0, e, 1.0), "k": 0.0}
        rays, cls = [], []
        for j in range(GROUP):
            x = float(np.nextafter(np.float32(e), np.float32(1.0) if j % 3 == 0 else np.float32(-1.0))) if j % 3 < 2 else e
            rays.append([x, f32(rng.uniform(-0.9, 0.9)), 1.0, 0.0, 0.0, -f32(2.0 ** rng.integers(-3, 4)), 0.0, 0.001, FMAX])
            cls.append("denormal_edge")
        self._group(spec, rays, cls)

    def _plane_rays(self, plane, rect, kk, scale):
        """rays at a rect: random, exactly at its closed edges and corners (small dyadic values: the fp32 test is
        exact there), parallel to the plane (+-0 direction components), t exactly at t_max"""
        rng, rays, cls = self.rng, [], []
        K, A, B = PLANE_AXES[plane]
        x0, y0, x1, y1 = rect
        for j in range(GROUP):
            kind = j % 8
            o, d = np.zeros(3), np.zeros(3)
            tmin, tmax = 0.001, FMAX
            if kind <= 2:  # random through the plane, some outside the rect
                o = rng.uniform(-6, 6, 3) * scale
                tgt = np.zeros(3)
                tgt[K], tgt[A], tgt[B] = kk, rng.uniform(x0 - 0.3 * scale, x1 + 0.3 * scale), rng.uniform(y0 - 0.3 * scale, y1 + 0.3 * scale)
                d = (tgt - o) / np.linalg.norm(tgt - o) * self._dscale()
                lab = "random"
            elif kind <= 4:  # exactly on an edge or a corner, power-of-two direction along k
                o[K] = kk + 2.0 * scale
                o[A] = rng.choice([x0, x1, (x0 + x1) / 2])
                o[B] = rng.choice([y0, y1]) if kind == 3 else rng.choice([y0, y1, (y0 + y1) / 2])
                d[K] = -(2.0 ** rng.integers(-2, 3))
                lab = "edge"
            elif kind == 5:  # t exactly at t_max (closed interval: rect.rs:48 rejects only t > t_max)
                o[K], o[A], o[B] = kk - 4.0, (x0 + x1) / 2, (y0 + y1) / 2
                d[K] = 2.0
                tmax = 2.0 if rng.random() < 0.5 else float(np.nextafter(np.float32(2.0), np.float32(0.0)))
                lab = "t_at_t_max"
            else:  # parallel to the plane: the k component +0 or -0, origin in or off the plane
                o[K] = kk if kind == 6 else kk + scale
                o[A], o[B] = rng.uniform(x0, x1), rng.uniform(y0, y1)
                d[A], d[B] = rng.normal(size=2)
                d[K] = -0.0 if rng.random() < 0.5 else 0.0
                lab = "parallel"
            rays.append([*o, *d, 0.0, tmin, tmax])
            cls.append(lab)
        return rays, cls

    def _cubes(self):
        rng = self.rng
        for scale, off in ((1.0, 0.0), (1.0, 0.0), (100.0, 200.0), (0.25, -3.0)):
            lo = np.array([f32(x) for x in off + rng.integers(-3, 0, 3) * scale])
            hi = np.array([f32(x) for x in lo + rng.integers(1, 4, 3) * scale])
            spec = {"kind": "cube", "lo": lo, "hi": hi}
            rays, cls = [], []
            for j in range(GROUP):
                kind = j % 4
                if kind == 0:  # random
                    o = (lo + hi) / 2 + _unit(rng) * 4 * scale * rng.uniform(1.0, 3.0)
                    tgt = rng.uniform(lo - 0.2 * scale, hi + 0.2 * scale)
                    d = (tgt - o) / np.linalg.norm(tgt - o) * self._dscale()
                    lab = "random"
                else:  # through an edge or a corner: faces tie (the later face of the scan wins, hittable.rs:41-44)
                    p = np.array([rng.choice([lo[i], hi[i], (lo[i] + hi[i]) / 2]) for i in range(3)])
                    ax = rng.permutation(3)[: 2 if kind < 3 else 3]
                    for i in ax:
                        p[i] = rng.choice([lo[i], hi[i]])
                    d = np.array([float(rng.choice([-1, 1])) * 2.0 ** int(rng.integers(-1, 2)) for _ in range(3)])
                    if kind == 2:
                        d[rng.integers(0, 3)] = 0.0  # along a face: +-0 components, NaN slabs
                    o = p - 2.0 * d
                    lab = "edge_or_corner"
                rays.append([*o, *d, 0.0, 0.001, FMAX])
                cls.append(lab)
            self._group(spec, rays, cls)

    def _instanced(self):
        """primitives under Traslate / Rotate: bit parity only (the exact reference of a rotation would need the
        reference's f64 sin / cos; the chain itself is tested by test_xform_*)"""
        rng = self.rng
        bases = [{"kind": "sphere", "c": np.array([1.0, 2.0, -1.0]), "r": 0.75},
                 {"kind": "cube", "lo": np.array([-1.0, -1.0, -1.0]), "hi": np.array([1.0, 0.5, 2.0])},
                 {"kind": "rect", "plane": 2, "rect": (-1.0, -2.0, 1.5, 1.0), "k": 0.5},
                 {"kind": "msphere", "c0": np.array([0.0, 0.0, 0.0]), "c1": np.array([0.5, 0.25, 0.0]), "t0": 0.0, "t1": 1.0, "r": 0.5}]
        for i, b in enumerate(bases):
            spec = dict(b)
            spec["wrap"] = [("R", int(i % 3), 15.0 + 20 * i), ("T", (f32(700.0 * (i % 2)), 3.0, f32(-700.0 * (i % 2))))]
            centre = np.array(spec["wrap"][1][1])
            rays, cls = [], []
            for j in range(GROUP):
                o = centre + _unit(rng) * rng.uniform(3.0, 30.0)
                tgt = centre + rng.uniform(-2.0, 2.0, 3)
                d = (tgt - o) / np.linalg.norm(tgt - o) * self._dscale()
                rays.append([*o, *d, f32(rng.uniform(0.0, 1.0)), 0.001, FMAX])
                cls.append("instanced")
            self._group(spec, rays, cls)

    def _aabb(self):
        rng, rows, cls = self.rng, [], []
        for j in range(2048):
            scale = [1.0, 0.25, 300.0, 1000.0][j % 4]
            lo = np.array([f32(x) for x in rng.integers(-4, 0, 3) * scale])
            hi = np.array([f32(x) for x in lo + rng.integers(1, 4, 3) * scale])
            kind = (j // 4) % 4
            tmin, tmax = 0.001, FMAX
            if kind == 0:  # random
                o = (lo + hi) / 2 + _unit(rng) * 6 * scale
                tgt = rng.uniform(lo - scale, hi + scale)
                d = (tgt - o) * (10.0 ** rng.uniform(-3, 3) / np.linalg.norm(tgt - o))
                lab = "random"
            else:  # only touching an edge (kind 1) or a corner (2), or grazing along a face with +-0 components (3)
                p = np.array([rng.choice([lo[i], hi[i]]) for i in range(3)])
                d = np.array([float(rng.choice([-1, 1])) * 2.0 ** int(rng.integers(-1, 2)) for _ in range(3)])
                if kind == 1:  # a direction that leaves the box through the edge only: outward on two axes
                    ax = rng.permutation(3)
                    i0, i1, i2 = ax
                    p[i2] = (lo[i2] + hi[i2]) / 2
                    d[i2] = 0.0 if rng.random() < 0.5 else -0.0
                    # inward on i0, outward on i1: the slabs touch at exactly one t
                    d[i0] = abs(d[i0]) if p[i0] == lo[i0] else -abs(d[i0])
                    d[i1] = -abs(d[i1]) if p[i1] == lo[i1] else abs(d[i1])
                elif kind == 2:  # through the corner, inward on one axis, outward on the others
                    sgn = [(1 if p[i] == lo[i] else -1) for i in range(3)]
                    d = np.array([sgn[i] * abs(d[i]) * (1 if i == 0 else -1) for i in range(3)])
                else:
                    d[rng.integers(0, 3)] = 0.0 if rng.random() < 0.5 else -0.0
                o = p - 2.0 * d
                if rng.random() < 0.25:
                    tmin, tmax = -FMAX, FMAX
                lab = ["random", "touch_edge", "touch_corner", "grazing_face"][kind]
            rows.append([*o, *d, 0.0, tmin, tmax, *lo, *hi])
            cls.append(lab)
        return np.array([[f32(x) for x in r] for r in rows]), np.array(cls)

    def _shade(self):
        rng, rows, cls = self.rng, [], []
        for j in range(2048):
            n = _unit(rng)
            n = np.array([f32(x) for x in n])
            eta = float(rng.choice([1.5, 1 / 1.5, 2.4, 1 / 2.4, 1.3, 0.7, 1.0]))
            kind = j % 4
            if kind == 0:  # random incidence, unnormalised direction
                v = _unit(rng) * 10.0 ** rng.uniform(-3, 3)
                lab = "random"
            elif kind == 1:  # near total internal reflection: sin(theta_t) = eta sin(theta_i) ~ 1
                eta = float(rng.choice([1.5, 2.4, 1.3]))
                s = (1.0 / eta) * (1.0 + rng.uniform(-1e-5, 1e-5))
                cth = math.sqrt(max(0.0, 1.0 - s * s))
                v = (-cth * n + s * _perp(n, rng)) * 10.0 ** rng.uniform(-2, 2)
                lab = "near_tir"
            elif kind == 2:  # near-zero scatter direction (Lambertian n + random_in_unit_sphere close to -n)
                v = (n + (-n + _unit(rng) * 10.0 ** rng.uniform(-6, -3))) * 1.0
                lab = "near_zero"
            else:  # grazing
                v = _perp(n, rng) + n * rng.uniform(-1e-3, 1e-3)
                lab = "grazing"
            cosine = f32(rng.uniform(0.0, 1.0)) if kind != 3 else f32(rng.choice([0.0, 1.0, 1e-4, 0.9999]))
            rows.append([*v, *n, f32(eta), cosine, f32(rng.choice([1.5, 2.4, 1.0, 0.7]))])
            cls.append(lab)
        return np.array([[f32(x) for x in r] for r in rows]), np.array(cls)

    def _uv(self):
        rng, rows, cls = self.rng, [], []
        for j in range(1024):
            kind = j % 4
            if kind == 0:
                n = _unit(rng)
                lab = "random"
            elif kind == 1:  # the poles
                n = np.array([rng.choice([0.0, -0.0, 1e-30]), rng.choice([1.0, -1.0]), rng.choice([0.0, -0.0])])
                lab = "pole"
            else:  # the atan2 seam: z = +-0 (or one ulp off it) with x < 0
                y = rng.uniform(-0.99, 0.99)
                x = -math.sqrt(1 - y * y)
                z = rng.choice([0.0, -0.0, 1e-38, -1e-38, 1e-7, -1e-7])
                n = np.array([x, y, z])
                lab = "seam"
            n = np.array([f32(c) for c in n])
            n[1] = max(-1.0, min(1.0, n[1]))
            rows.append(list(n))
            cls.append(lab)
        return np.array(rows), np.array(cls)


# ---------------------------------------------------------------------------------------------------------------------
# exact reference
# ---------------------------------------------------------------------------------------------------------------------
class Ex:
    """result of an exact evaluation: hit, t (mpf or None), face, in_band (the decision is within the stated
    uncertainty of the fp32 contract), scale S of the error bound (length units), centre (spheres)"""

    def __init__(self, hit, t=None, face=0, band=False, S=0.0, c=None, r=None, dt=0.0, tq=None):
        self.hit, self.t, self.face, self.band, self.S, self.c, self.r, self.dt = hit, t, face, band, S, c, r, dt
        self.tq = tq  # t as a Fraction (rects)


def sphere_centre(spec, time):
    if spec["kind"] == "sphere":
        return [Fr(x) for x in spec["c"]]
    t0, t1 = Fr(spec["t0"]), Fr(spec["t1"])
    f = (Fr(time) - t0) / (t1 - t0)  # sphere.rs:115-118 (t0 == t1: the caller takes the f64 literal oracle's answer)
    return [Fr(a) + f * (Fr(b) - Fr(a)) for a, b in zip(spec["c0"], spec["c1"])]


def sphere_exact(spec, ray, K_TAN, K_T):
    """Sphere::hit on the exact inputs.  Bands (derivation in tests/test_geom_contract.py):
    tangent |r^2 - l^2| <= K_TAN eps |r| S, root t within dt of t_min / t_max, with S = |o - c| + |r| (+ |c0| + |c1 - c0|
    for a moving centre, which the contract rounds) and dt = (K_T eps S + K_TAN eps |r| S / (2 h)) / |d|, h the half chord."""
    o, d = [Fr(x) for x in ray[0:3]], [Fr(x) for x in ray[3:6]]
    tmin, tmax = Fr(ray[7]), Fr(ray[8])
    c, r = sphere_centre(spec, ray[6]), Fr(spec["r"])
    oc = [a - b for a, b in zip(o, c)]
    a = sum(x * x for x in d)
    b = sum(x * y for x, y in zip(oc, d))
    l2 = sum(x * x for x in oc) - b * b / a
    S = float(norm_q(oc)) + abs(float(r))
    if spec["kind"] == "msphere":
        S += float(norm_q([Fr(x) for x in spec["c0"]])) + float(norm_q([Fr(y) - Fr(x) for x, y in zip(spec["c0"], spec["c1"])]))
    h2 = r * r - l2
    band = abs(float(h2)) <= K_TAN * EPS * abs(float(r)) * S
    dn = float(norm_q(d))
    hh = math.sqrt(max(float(h2), K_TAN * EPS * abs(float(r)) * S))
    dt = (K_T * EPS * S + K_TAN * EPS * abs(float(r)) * S / (2 * hh)) / dn
    if h2 <= 0:
        return Ex(False, band=band, S=S, c=c, r=r, dt=dt)
    sq = mpmath.sqrt(mpf(a * h2))
    t1, t2 = (mpf(-b) - sq) / mpf(a), (mpf(-b) + sq) / mpf(a)
    for t in (t1, t2):
        if abs(float(t) - float(tmin)) <= dt or abs(float(t) - float(tmax)) <= dt:
            band = True
    for t in (t1, t2):
        if mpf(tmin) < t < mpf(tmax):
            return Ex(True, t, band=band, S=S, c=c, r=r, dt=dt)
    return Ex(False, band=band, S=S, c=c, r=r, dt=dt)


def radial_error(ray, t, c, r):
    """| |o + t d - c| - |r| | of the returned t, exactly"""
    tt = Fr(float(t))
    p = [Fr(ray[i]) + tt * Fr(ray[3 + i]) - c[i] for i in range(3)]
    return abs(float(norm_q(p) - abs(mpf(r))))


def rect_exact(plane, rect, kk, ray, tmin, tmax, K_R):
    """Rect::hit (rect.rs:39-69) on the exact inputs; None when the k component of d is +-0 (non-finite t: the f64
    literal oracle decides).  Band: every compared pair within K_R eps of its magnitude, unless every intermediate of the
    fp32 evaluation is an fp32 value (then the fp32 test is exact and the band is empty)."""
    K, A, B = PLANE_AXES[plane]
    o, d = [Fr(x) for x in ray[0:3]], [Fr(x) for x in ray[3:6]]
    if d[K] == 0:
        return None
    x0, y0, x1, y1 = (Fr(v) for v in rect)
    kk = Fr(kk)
    t = (kk - o[K]) / d[K]
    x, y = o[A] + t * d[A], o[B] + t * d[B]
    reject = t < tmin or t > tmax or x < x0 or x > x1 or y < y0 or y > y1
    exact = all(is_f32(q) for q in (kk - o[K], 1 / d[K], t, t * d[A], x, t * d[B], y))
    band = False
    if not exact:
        et = K_R * EPS * abs(float(t))
        ex = K_R * EPS * (abs(float(o[A])) + abs(float(t * d[A])))
        ey = K_R * EPS * (abs(float(o[B])) + abs(float(t * d[B])))
        band = (abs(float(t - tmin)) <= et or abs(float(t - tmax)) <= et or abs(float(x - x0)) <= ex
                or abs(float(x - x1)) <= ex or abs(float(y - y0)) <= ey or abs(float(y - y1)) <= ey)
    return Ex(not reject, mpf(t), band=band, dt=K_R * EPS * abs(float(t)) if not exact else 0.0, tq=t)


def cube_faces(lo, hi):
    """cube.rs:21-74: the six rects in construction order: (plane, (x0, y0, x1, y1), k)"""
    ax, ay, az = lo
    bx, by, bz = hi
    return [(2, (ax, ay, bx, by), bz), (2, (ax, ay, bx, by), az), (1, (az, ax, bz, bx), by), (1, (az, ax, bz, bx), ay),
            (0, (ay, az, by, bz), bx), (0, (ay, az, by, bz), ax)]


def prim_exact(spec, ray, K):
    """exact hit / t / face of one PRIM case, or None where the f64 literal oracle decides"""
    if spec.get("wrap"):
        return None
    kind = spec["kind"]
    if kind in ("sphere", "msphere"):
        if kind == "msphere" and spec["t0"] == spec["t1"]:
            return None
        return sphere_exact(spec, ray, K["tan"], K["t"])
    tmin, tmax = Fr(ray[7]), Fr(ray[8])
    if kind == "rect":
        return rect_exact(spec["plane"], spec["rect"], spec["k"], ray, tmin, tmax, K["rect"])
    closest, hit, face, band = tmax, False, 0, False  # hittable.rs:37-47 over the six sides
    t_hit, dt = None, 0.0
    for f, (pl, rc, kk) in enumerate(cube_faces(spec["lo"], spec["hi"])):
        e = rect_exact(pl, rc, kk, ray, tmin, closest, K["rect"])
        if e is None:
            return None
        band = band or e.band
        if e.hit:
            closest, hit, face, t_hit, dt = e.tq, True, f, e.t, e.dt
    return Ex(hit, t_hit, face, band, dt=dt)


def aabb_exact(row, K_A):
    """AABB::hit (aabb.rs:31-44) on the exact inputs: (hit, t_enter, band).  A zero direction component gives inv_d =
    +-inf and slab distances +-inf or NaN (0 * inf), exactly as in f64, ignored by max / min like f64::max / min."""
    o, d, tmin, tmax, lo, hi = row[0:3], row[3:6], row[7], row[8], row[9:12], row[12:15]
    tmin = -math.inf if tmin <= -FMAX else Fr(tmin)
    tmax = math.inf if tmax >= FMAX else Fr(tmax)
    exact = True

    def fmax(a, b):
        if isinstance(a, float) and math.isnan(a):
            return b
        if isinstance(b, float) and math.isnan(b):
            return a
        return a if a >= b else b

    def fmin(a, b):
        if isinstance(a, float) and math.isnan(a):
            return b
        if isinstance(b, float) and math.isnan(b):
            return a
        return a if a <= b else b

    for i in range(3):
        if d[i] == 0:
            inv = math.copysign(math.inf, d[i])
            t0 = (lo[i] - o[i]) * inv if lo[i] != o[i] else math.nan
            t1 = (hi[i] - o[i]) * inv if hi[i] != o[i] else math.nan
            neg = inv < 0
        else:
            t0, t1 = (Fr(lo[i]) - Fr(o[i])) / Fr(d[i]), (Fr(hi[i]) - Fr(o[i])) / Fr(d[i])
            exact = exact and all(is_f32(q) for q in (Fr(lo[i]) - Fr(o[i]), Fr(hi[i]) - Fr(o[i]), 1 / Fr(d[i]), t0, t1))
            neg = d[i] < 0
        if neg:
            t0, t1 = t1, t0
        tmin, tmax = fmax(tmin, t0), fmin(tmax, t1)
    hit = not (tmax <= tmin)
    band = False
    if not exact and not (math.isinf(float(tmin)) or math.isinf(float(tmax))):
        band = abs(float(tmax - tmin)) <= K_A * EPS * (abs(float(tmin)) + abs(float(tmax)))
    return hit, tmin, band, exact


def shade_exact(row):
    """material.rs:9-28: reflect(v, n), refract (ok, vector, disc), schlick(cosine, ref_idx) in real arithmetic"""
    v, n = [Fr(x) for x in row[0:3]], [Fr(x) for x in row[3:6]]
    eta, cosine, ri = Fr(row[6]), Fr(row[7]), Fr(row[8])
    vn = sum(a * b for a, b in zip(v, n))
    refl = [a - 2 * vn * b for a, b in zip(v, n)]
    vl = norm_q(v)
    uv = [mpf(a) / vl for a in v]
    dt = sum(a * mpf(b) for a, b in zip(uv, n))
    disc = 1 - mpf(eta) ** 2 * (1 - dt * dt)
    ok = disc > 0
    refr = [(a - mpf(b) * dt) * mpf(eta) - mpf(b) * mpmath.sqrt(disc) for a, b in zip(uv, n)] if ok else None
    r0 = ((1 - ri) / (1 + ri)) ** 2
    x = 1 - cosine
    sch = r0 + (1 - r0) * x ** 5
    return [mpf(q) for q in refl], ok, refr, disc, mpf(sch), float(abs(vn)), float(vl)


def uv_exact(n, book, zero_as_plus=False):
    """get_sphere_uv (sphere.rs:9-15): u = 1 - (atan2(z, x) + pi) / (2 pi), v = (asin(y) + FRAC_2_PI) / pi (the book:
    pi / 2).  atan2 of a zero z is 0 or +-pi exactly as in IEEE, by the signs of the zeros (mpmath has no signed zero);
    zero_as_plus: the contract's documented rule instead (include/rtmi_math.h rtmi_atan2f: -0 is +0, atan2(0, 0) = 0)."""
    x, y, z = n
    if z == 0.0 and zero_as_plus:
        phi = mpmath.pi if x < 0 else mpmath.mpf(0)
    elif z == 0.0:
        phi = mpmath.mpf(math.atan2(z, x))
    else:
        phi = mpmath.atan2(mpmath.mpf(z), mpmath.mpf(x))
    theta = mpmath.asin(mpmath.mpf(y))
    u = 1 - (phi + mpmath.pi) / (2 * mpmath.pi)
    v = (theta + (mpmath.pi / 2 if book else 2 / mpmath.pi)) / mpmath.pi
    return u, v
