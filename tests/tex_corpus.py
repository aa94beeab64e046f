"""Texture evaluation: the corpus of tests/test_tex_contract.py and tests/test_gpu_tex_contract.py, and an exact reference.

Reference (src/texture.rs, src/perlin.rs) evaluated on the given binary floating-point inputs (u, v, p): the lattice work
(floor, p - floor(p), p * 2^o, the `as usize` cast with its 64-bit saturation and wrapping `+ 1`, the permutation index,
the texel index) in Python integers and fractions, exact; the smoothstep, the corner sums, the sines and the final value in
mpmath at PREC bits, which is exact for every purpose here (the inputs have 24 or 53 bits).

Every case is a point of an axis-aligned plate z = k lit by a DiffuseLight of one texture, so that the GPU tier can reach
it through the public entries: an axis-aligned ray places p exactly, and (u, v) are rect.rs:52-56 on the plate's extents.
The cases of one FAMILY ("noise", "checker", "image") make one scene; within it a plate is known by its z."""
import math
from fractions import Fraction as Fr

import mpmath
import numpy as np

f32 = np.float32
PREC = 200
U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}  # unit roundoff
BIG = 3e20  # half the side of the large plates
SIN_LIMIT = 2 ** 20  # rtmi_sinf's domain (include/rtmi_math.h): beyond it the contract's sine is 0
K_TURB = 200.0  # error of the contract's turb(p, 7) in units of the unit roundoff (derived in test_tex_contract.py)
USIZE_MAX = 2 ** 64 - 1
MUTATIONS = ("octaves6", "cell_before_floor", "v_not_flipped", "checker_le", "cast32", "no_sin_rule")
THRESHOLDS = {"256": 256, "2p24": 2 ** 24, "2p31": 2 ** 31, "2p32": 2 ** 32, "2p63": 2 ** 63, "2p64": 2 ** 64}

IMAGES = {"i1x1": (1, 1), "i2x2": (2, 2), "i3x5": (3, 5), "i7x2": (7, 2), "i16x8": (16, 8)}


def image_data(nx, ny):
    """every texel a distinct value: the red channel is the texel's index"""
    idx = np.arange(nx * ny)
    return np.stack([idx, 255 - idx, (7 * idx + 3) % 256], axis=1).astype(np.uint8).reshape(-1)


def _chain(depth, side, leaf):
    """`depth` checkers nested along one side: the other side of level n is a solid of its own colour"""
    node = leaf
    for n in range(depth):
        solid = ("solid", (n + 1) / 32.0, 0.5, 1.0 - (n + 1) / 32.0)
        node = ("checker", node, solid) if side == "odd" else ("checker", solid, node)
    return node


# name -> spec, in construction order (a NoiseTexture takes its tables from the scene RNG when it is made)
SPECS = [
    ("NA", ("noise", 4.0)),
    ("NB", ("noise", 0.37)),
    ("S0", ("solid", 0.25, 0.5, 0.75)),
    ("S1", ("solid", 0.875, 0.125, 0.0625)),
] + [(k, ("image", k)) for k in IMAGES] + [
    ("CK1", ("checker", ("solid", 0.125, 0.25, 0.5), ("solid", 0.875, 0.75, 0.625))),
    ("CK2", ("checker", ("checker", ("noise", 2.0), ("image", "i3x5")), ("checker", ("solid", 0.5, 0.25, 0.125), ("noise", 1.5)))),
    ("CK16O", _chain(15, "odd", ("checker", ("noise", 3.0), ("solid", 1.0, 0.0, 0.5)))),  # 16 checkers, the innermost over noise
    ("CK16E", _chain(15, "even", ("checker", ("solid", 0.0, 1.0, 0.5), ("image", "i7x2")))),
    ("CKN", ("checker", ("noise", 5.0), ("noise", 0.5))),
]
FAMILY = {"NA": "noise", "NB": "noise", "S0": "noise", "S1": "noise", "CKN": "noise", "CK1": "checker", "CK2": "checker",
          "CK16O": "checker", "CK16E": "checker"}
FAMILY.update({k: "image" for k in IMAGES})
SCENE_SEED = 11


def depth_of(spec):
    return 1 + max(depth_of(spec[1]), depth_of(spec[2])) if spec[0] == "checker" else 0


def build(api, prec="f32"):
    """name -> (the api's texture object, the resolved tree the exact reference walks).  The scene RNG is seeded first, so
    every api builds the same tables.  prec: the precision in which the api holds colours, scales and tables."""
    api.seed_scene_rng(SCENE_SEED)
    cast = (lambda x: float(f32(x))) if prec == "f32" else float

    def make(spec):
        if spec[0] == "solid":
            return api.SolidTexture(*spec[1:]), ("solid", [Fr(cast(c)) for c in spec[1:]])
        if spec[0] == "noise":
            obj = api.NoiseTexture(spec[1])
            rv, pm = api.perlin_tables(obj)
            rv = [[mpmath.mpf(cast(c)) for c in row] for row in np.asarray(rv, np.float64)]
            return obj, ("noise", Fr(cast(spec[1])), rv, [[int(x) for x in row] for row in np.asarray(pm)])
        if spec[0] == "image":
            nx, ny = IMAGES[spec[1]]
            data = image_data(nx, ny)
            return api.ImageTexture(data, nx, ny), ("image", nx, ny, [int(x) for x in data])
        (odd, todd), (even, teven) = make(spec[1]), make(spec[2])
        return api.CheckerTexture(odd, even), ("checker", todd, teven)

    return {name: make(spec) for name, spec in SPECS}


# ---------------------------------------------------------------------------------------------------------------------
# the exact reference
# ---------------------------------------------------------------------------------------------------------------------
def as_usize(n, mut=None):
    """Rust's `as usize` of an integer-valued float: saturating (perlin.rs:83-85)"""
    if n <= 0:
        return 0
    if mut == "cast32":  # the device's rule before this test existed: 0 for everything from 2^32 on
        return 0 if n >= 2 ** 32 else n
    return min(n, USIZE_MAX)


def sin_err(x, prec):
    """|contract sine - sin| at argument x: the bound tests/test_math_contract.py asserts for rtmi_sinf; libm's 1 ulp"""
    return 1e-6 * (1.0 + 0.6 * abs(x)) if prec == "f32" else 2.0 ** -52


class Ex:
    """value: 3 mpf; bound: absolute error allowed to the contract; band: a decision is within rounding of flipping (the value
    is then held to the fp32 oracle only); rule: decided by rtmi_sinf's domain rule, not by real arithmetic; leaf: the
    kind of the leaf reached; path: the checker branches taken; texel: (i, j) of an image leaf; cells: the lattice cells
    and permutation indices of a noise leaf, octave by octave"""
    __slots__ = ("value", "bound", "band", "rule", "leaf", "path", "texel", "cells", "arg")

    def __init__(self):
        self.value, self.bound, self.band, self.rule, self.leaf, self.path, self.texel, self.cells, self.arg = None, 0.0, False, False, None, (), None, None, None


def _checker_branch(p, prec, mut):
    """('odd' | 'even', band, rule) of texture.rs:39-48 at p"""
    band = rule = False
    sines = []
    for c in p:
        x = 10 * Fr(c)
        if prec == "f32" and abs(x) > SIN_LIMIT and mut != "no_sin_rule":  # that mutation: the true sine everywhere
            if abs(x) > SIN_LIMIT * (1 + Fr(1, 2 ** 23)):  # the fp32 product 10 * p_k is beyond the limit too
                rule = True
                sines.append(mpmath.mpf(0))
                continue
            band = True  # the product may round to the limit itself
        s = mpmath.sin(mpmath.mpf(x.numerator) / x.denominator)
        if x != 0 and abs(s) <= U[prec] * abs(float(x)) + sin_err(float(x), prec):
            band = True
        sines.append(s)
    prod = sines[0] * sines[1] * sines[2]
    odd = prod <= 0 if mut == "checker_le" else prod < 0
    return ("odd" if odd else "even"), band, rule


def _noise_octave(rv, pm, tp, mut):
    """Perlin::noise (perlin.rs:76-97, 38-56) at the exact point tp (3 fractions) -> (mpf, (cell, permutation indices))"""
    fl = [math.floor(c) for c in tp]
    if mut == "cell_before_floor":  # the cell taken by casting the coordinate itself, the fraction relative to that cell
        fl = [as_usize(int(c)) for c in tp]
    uvw = [mpmath.mpf((c - f).numerator) / (c - f).denominator for c, f in zip(tp, fl)]
    cell = [as_usize(f, mut) for f in fl]
    sm = [x * x * (3 - 2 * x) for x in uvw]
    acc = mpmath.mpf(0)
    hs = []
    for di in range(2):
        for dj in range(2):
            for dk in range(2):
                h = pm[0][((cell[0] + di) & USIZE_MAX) & 255] ^ pm[1][((cell[1] + dj) & USIZE_MAX) & 255] ^ \
                    pm[2][((cell[2] + dk) & USIZE_MAX) & 255]
                hs.append(h)
                c = rv[h]
                w = [uvw[0] - di, uvw[1] - dj, uvw[2] - dk]
                acc += (di * sm[0] + (1 - di) * (1 - sm[0])) * (dj * sm[1] + (1 - dj) * (1 - sm[1])) * \
                       (dk * sm[2] + (1 - dk) * (1 - sm[2])) * (c[0] * w[0] + c[1] * w[1] + c[2] * w[2])
    return acc, (tuple(cell), tuple(hs))


def turb_exact(node, p, mut=None):
    """Perlin::turb(p, 7) (perlin.rs:99-109) -> (mpf, the cells of the octaves)"""
    _, _, rv, pm = node
    acc, cells = mpmath.mpf(0), []
    tp = [Fr(c) for c in p]
    for o in range(6 if mut == "octaves6" else 7):
        n, cell = _noise_octave(rv, pm, tp, mut)
        acc += n / 2 ** o
        cells.append(cell)
        tp = [2 * c for c in tp]
    return abs(acc), cells


def tex_exact(node, u, v, p, prec="f32", mut=None):
    """Texture::value at (u, v, p): Python floats holding the fp32 (or f64) inputs exactly"""
    with mpmath.workprec(PREC):
        ex = Ex()
        ur = U[prec]
        if node[0] == "checker":
            side, ex.band, ex.rule = _checker_branch(p, prec, mut)
            while node[0] == "checker":
                ex.path += (side,)
                node = node[1] if side == "odd" else node[2]
        ex.leaf = node[0]
        if node[0] == "solid":
            ex.value = [mpmath.mpf(c.numerator) / c.denominator for c in node[1]]
        elif node[0] == "image":
            _, nx, ny, data = node
            X = Fr(u) * nx
            V1 = Fr(v) if mut == "v_not_flipped" else 1 - Fr(v)
            Y = V1 * ny
            rep = (lambda q: Fr(float(f32(float(q)))) == q) if prec == "f32" else (lambda q: Fr(float(q)) == q)
            idx = lambda q, n: min(as_usize(math.floor(q)), n - 1)  # noqa: E731
            i, j = idx(X, nx), idx(Y, ny)
            if not rep(X) and idx(X * (1 - Fr(ur)), nx) != idx(X * (1 + Fr(ur)), nx):
                ex.band = True  # one rounding of u * nx
            if not (rep(V1) and rep(Y)) and idx(Y * (1 - 2 * Fr(ur)), ny) != idx(Y * (1 + 2 * Fr(ur)), ny):
                ex.band = True  # two roundings of (1 - v) * ny
            ex.texel = (i, j)
            at = 3 * i + 3 * nx * j
            ex.value = [mpmath.mpf(data[at + c]) / 255 for c in range(3)]
            ex.bound = ur * 1.0  # one division by 255 of a value <= 1
        else:
            _, scale, rv, pm = node
            turb, ex.cells = turb_exact(node, p, mut)
            sx = scale * Fr(p[0])
            sxf = mpmath.mpf(sx.numerator) / sx.denominator
            arg = sxf + 5 * turb
            ex.arg = float(arg)
            darg = K_TURB * 5 * ur + ur * (abs(float(sxf)) + 5 * float(turb) + abs(float(arg)))
            g = (1 + mpmath.sin(arg)) / 2
            ex.bound = 0.5 * (darg + sin_err(float(arg), prec) + 2 * ur)
            if prec == "f32" and abs(arg) > SIN_LIMIT - darg and mut != "no_sin_rule":
                if abs(arg) > SIN_LIMIT + darg:
                    ex.rule = True
                    g = mpmath.mpf(0.5)
                    ex.bound = 0.0  # held to the rule: 0.5 (1 + 0) is exact
                else:
                    ex.band = True
            ex.value = [g, g, g]
        return ex


# ---------------------------------------------------------------------------------------------------------------------
# the corpus
# ---------------------------------------------------------------------------------------------------------------------
def plate_of(tex):
    if tex in IMAGES:
        nx, ny = IMAGES[tex]
        return (0.0, 0.0, float(nx), float(ny))
    return (-BIG, -BIG, BIG, BIG)


def plate_uv(x, y, plate):
    """rect.rs:52-56 in fp32"""
    x0, y0, x1, y1 = (f32(c) for c in plate)
    return (f32(x) - x0) / (x1 - x0), (f32(y) - y0) / (y1 - y0)


def _nx(c, up):
    return f32(np.nextafter(f32(c), f32(np.inf if up else -np.inf)))


class Corpus:
    """cases: parallel arrays tex (names), cls (labels), xyz float32 [n, 3], aux (per-case data of the class's property)"""

    def __init__(self):
        self.tex, self.cls, self.xyz, self.aux = [], [], [], []
        rng = np.random.default_rng(2026)
        self._noise(rng)
        self._checker(rng)
        self._image(rng)
        self.xyz = np.array(self.xyz, f32)
        self.tex, self.cls = np.array(self.tex), np.array(self.cls)
        self.family = np.array([FAMILY[t] for t in self.tex])
        uv = [plate_uv(p[0], p[1], plate_of(t)) for t, p in zip(self.tex, self.xyz)]
        self.uv = np.array(uv, f32)
        for fam in ("noise", "checker", "image"):  # within a scene a plate is known by its z
            pl = {(t, float(z)) for t, z in zip(self.tex[self.family == fam], self.xyz[self.family == fam, 2])}
            zs = sorted(z for _, z in pl)
            assert all(np.nextafter(f32(a), f32(np.inf)) < f32(b) for a, b in zip(zs, zs[1:])), fam  # an fp32 value lies between

    def add(self, tex, cls, x, y, z, aux=None):
        self.tex.append(tex)
        self.cls.append(cls)
        self.xyz.append((f32(x), f32(y), f32(z)))
        self.aux.append(aux)

    def plates(self, fam):
        """[(tex, z)] of a family's scene, in a fixed order"""
        m = self.family == fam
        return sorted({(t, float(z)) for t, z in zip(self.tex[m], self.xyz[m, 2])}, key=lambda a: (a[1], a[0]))

    # ---- noise -------------------------------------------------------------------------------------------------------
    def _noise(self, rng):
        un = lambda lo, hi: f32(rng.uniform(lo, hi))  # noqa: E731
        for t, tex in enumerate(("NA", "NB")):
            n = 1 if t == 0 else 2  # the second table gets half the random cases
            za, zb = 0.37 + 0.25 * t, 5.73 + 0.25 * t
            for z in (za, zb):
                for _ in range(100 // n):
                    self.add(tex, "interior", un(0.01, 9), un(0.01, 9), z)
            for _ in range(40 // n):
                self.add(tex, "lattice_z", un(0.01, 9), un(0.01, 9), 3.0 + 4 * t, (2,))
                self.add(tex, "lattice_x", float(rng.integers(0, 8)), un(0.01, 9), za, (0,))
                self.add(tex, "lattice_y", un(0.01, 9), float(rng.integers(0, 8)), za, (1,))
            for _ in range(16 // n):
                self.add(tex, "lattice_xyz", float(rng.integers(0, 300)), float(rng.integers(0, 300)), 3.0 + 4 * t, (0, 1, 2))
            for up in (False, True):
                zn = _nx(2.0 + 2 * t, up)
                for m in range(1, 7):
                    self.add(tex, "nextafter", _nx(m, up), un(0.01, 9), za, (0,))
                    self.add(tex, "nextafter", un(0.01, 9), _nx(m, not up), zb, (1,))
                    self.add(tex, "nextafter", un(0.01, 9), un(0.01, 9), zn, (2,))
                    self.add(tex, "nextafter", _nx(m, up), _nx(m + 1, up), zn, (0, 1, 2))
            tiny = -(2.0 ** -(30 - t))  # p - floor(p) rounds to 1
            for z in (-0.6 - 0.25 * t, tiny, -3.0 - t):
                for _ in range(24 // n):
                    self.add(tex, "negative", un(-9, -0.01), un(-9, -0.01), z)
                self.add(tex, "negative", tiny, -1.0, z)
                self.add(tex, "negative", -0.5, tiny, z)
                self.add(tex, "negative", tiny, tiny, z)
            for _ in range(16 // n):
                self.add(tex, "negative", un(-9, -0.01), un(0.01, 9), za)
                self.add(tex, "negative_tiny", tiny, un(0.01, 9), za, (0,))
                self.add(tex, "negative_tiny", un(0.01, 9), un(-9, 9), tiny, (2,))
            for name, T in THRESHOLDS.items():
                c = f32(T / 8 * (0.9 - 0.05 * t))  # octaves 0..2 below T, 3 (t = 0: 0.9 * 8 = 7.2 > ... ) .. 6 at or above it
                below, at = _nx(T, False), f32(T)
                for _ in range(4):
                    a, b = un(0.01, 0.99), un(0.01, 0.99)
                    for cc, kind in ((c, "straddle"), (below, "straddle"), (at, "at")):
                        self.add(tex, "%s_%s" % (kind, name), cc, a, za, (T, (0,)))
                        self.add(tex, "%s_%s" % (kind, name), a, cc, zb, (T, (1,)))
                    self.add(tex, "straddle_%s" % name, a, b, c, (T, (2,)))
                    self.add(tex, "straddle_%s" % name, -a, -b, c, (T, (2,)))
                self.add(tex, "straddle_%s" % name, c, c, c, (T, (0, 1, 2)))
                self.add(tex, "straddle_%s" % name, below, c, c, (T, (0, 1, 2)))
            # |scale * p.x + 5 * turb| on both sides of rtmi_sinf's limit
            for k in range(96):
                x = 2.0 ** 18 - 4.0 + k / 16.0 if t == 0 else 2833989.0 - 20.0 + k / 4.0
                self.add(tex, "sin_limit", x, un(0.01, 9), za)
                if k % 8 == 0:
                    self.add(tex, "sin_limit", -x, un(0.01, 9), zb)
        self.add("NA", "beyond_2p64", 0.3, 2e20, 0.7, (2 ** 64, (1,)))  # the case the disagreement was first seen at
        self.add("NA", "lattice_z", 0.3, 1.7, 0.0, (2,))
        for _ in range(20):
            self.add("NA", "lattice_z", un(-9, 9), un(-9, 9), 0.0, (2,))
        # the plates the GPU tier's independence batches use beside these: solids, a second table, a checker over noise
        for tex, z in (("S0", 20.0), ("S1", 21.0), ("CKN", 22.0)):
            for _ in range(64):
                self.add(tex, "beside", un(-3, 3), un(-3, 3), z)

    # ---- checker -----------------------------------------------------------------------------------------------------
    def _checker(self, rng):
        un = lambda lo, hi: f32(rng.uniform(lo, hi))  # noqa: E731
        z0 = 0.05  # sin(0.5): no zero near
        for _ in range(100):
            self.add("CK1", "interior", un(-3, 3), un(-3, 3), z0)
        # a sine within the band of a zero: 10 p_k near m pi, m small, and m large enough that the reduction matters
        for m in (1, 2, 3, 7, 1000, 19000):
            c0 = f32(m * math.pi / 10)
            for sgn in (1.0, -1.0):
                c = f32(sgn * c0)
                for step in (-16, -2, -1, 0, 1, 2, 16):  # +-16 ulp: just outside the band
                    cc = c
                    for _ in range(abs(step)):
                        cc = _nx(cc, step > 0)
                    self.add("CK1", "near_zero", cc, un(0.02, 0.29), z0, (0,))
                    self.add("CK1", "near_zero", un(0.02, 0.29), cc, z0, (1,))
        for zz in (f32(3 * math.pi / 10), f32(-1000 * math.pi / 10), _nx(f32(19000 * math.pi / 10), True)):
            for _ in range(12):
                self.add("CK1", "near_zero", un(0.02, 0.29), un(-0.29, -0.02), zz, (2,))
        # p_k = +-0
        for a in (0.0, -0.0):
            for b in (0.1, -0.1, 0.0, -0.0):
                self.add("CK1", "zero", a, b, z0, (0,))
                self.add("CK1", "zero", b, a, z0, (1,))
                self.add("CK1", "zero", a, b, 0.0, (2,))
                self.add("CK1", "zero", b, a, -z0, (1,))
        # |10 p_k| on both sides of 2^20
        lim = f32(104857.6)
        vals = [104857.5, lim, _nx(lim, False), _nx(lim, True), 104857.7, 104858.0, 104850.0, 2.0e5, 1.0e7, 3.0e20]
        for c in vals:
            for sgn in (1.0, -1.0):
                self.add("CK1", "limit", sgn * c, un(0.02, 0.29), z0, (0,))
                self.add("CK1", "limit", un(0.02, 0.29), sgn * c, z0, (1,))
        for zz in (104857.0, 104858.0, -104859.0):
            for _ in range(8):
                self.add("CK1", "limit", un(0.02, 0.29), un(0.02, 0.29), zz, (2,))
        # nests of 2 and 16 with noise, image and solid leaves; both parities (z of either sign)
        for k, tex in enumerate(("CK2", "CK16O", "CK16E")):
            for zz in (0.15 + 0.1 * k, -0.15 - 0.1 * k):
                for _ in range(40):
                    self.add(tex, "nested", un(-3, 3), un(-3, 3), zz)
                self.add(tex, "nested_zero", 0.0, un(-3, 3), zz, (0,))
                self.add(tex, "nested_limit", 2.0e5, un(-3, 3), zz, (0,))

    # ---- image -------------------------------------------------------------------------------------------------------
    def _image(self, rng):
        for k, (tex, (nx, ny)) in enumerate(IMAGES.items()):
            z = 1.0 + k

            def marks(n):
                out = [(float(m), "integer") for m in range(0, n + 1)]
                out += [(_nx(m, True), "nextafter") for m in range(0, n)] + [(_nx(m, False), "nextafter") for m in range(1, n + 1)]
                out += [(f32(rng.uniform(0, n)), "interior") for _ in range(6)]
                return out

            xs, ys = marks(nx), marks(ny)
            ys += [(f32(ny * 2.0 ** -30), "round_up"), (f32(ny * 2.0 ** -26), "round_up"), (f32(ny * 3e-9), "round_up")]
            pairs = set()
            for ix in range(len(xs)):
                for iy in rng.choice(len(ys), min(len(ys), 5), replace=False):
                    pairs.add((ix, int(iy)))
            for iy in range(len(ys)):
                for ix in rng.choice(len(xs), min(len(xs), 5), replace=False):
                    pairs.add((int(ix), iy))
            for ix, iy in sorted(pairs):
                (x, cx), (y, cy) = xs[ix], ys[iy]
                edge = x in (0.0, float(nx)) or y in (0.0, float(ny))
                cls = "edge" if edge else cy if cy == "round_up" else cx if cx != "interior" else cy
                self.add(tex, cls, x, y, z, (cx, cy))


def walk(spec, p):
    """(the number of checkers passed, the kind of the leaf reached) from p by the exact branch: every level of a nest
    takes the same side, texture.rs:39-48"""
    side = _checker_branch(p, "f32", None)[0]
    depth = 0
    while spec[0] == "checker":
        spec = spec[1] if side == "odd" else spec[2]
        depth += 1
    return depth, spec[0]


def has_property(cls, aux, tex, u, v, p):
    """whether the (u, v, p) actually evaluated has the property its class is named after"""
    p = [float(c) for c in p]
    ints = [c == math.floor(c) for c in p]
    if tex in IMAGES:
        nx, ny = IMAGES[tex]
        X, Y = Fr(float(u)) * nx, (1 - Fr(float(v))) * ny
        near = lambda q: abs(q - round(q)) < Fr(1, 10 ** 5)  # noqa: E731  (on it, or within a rounding of it)
        if cls == "edge":
            return float(u) in (0.0, 1.0) or float(v) in (0.0, 1.0)
        if cls in ("integer", "nextafter"):
            return near(X) or near(Y)
        if cls == "round_up":
            return float(v) > 0 and float(f32(1) - f32(v)) * ny == ny
        return 0 < X < nx and 0 < Y < ny
    if cls == "beside":  # the plates the independence batches put beside the noise ray: solids, a checker over noise
        return tex in ("S0", "S1", "CKN") and max(abs(c) for c in p[:2]) <= 3 and p[2] in (20.0, 21.0, 22.0)
    if cls == "nested":  # a nest of at least two checkers, walked by real arithmetic to one of its own leaves
        depth, leaf = walk(dict(SPECS)[tex], p)
        return depth_of(dict(SPECS)[tex]) >= 2 and 1 <= depth and leaf in ("noise", "image", "solid") and \
            all(abs(10.0 * c) < SIN_LIMIT for c in p)
    if cls == "interior" and FAMILY[tex] == "checker":  # no sine within the band of a zero, none beyond the limit
        return _checker_branch(p, "f32", None)[1:] == (False, False)
    if cls == "interior":
        return min(p) > 0 and not any(ints)
    if cls.startswith("lattice"):
        return all(ints[k] for k in aux)
    if cls == "nextafter":
        return all(not ints[k] and float(np.nextafter(f32(p[k]), f32(round(p[k])))) == round(p[k]) for k in aux)
    if cls == "negative":
        return min(p) < 0
    if cls == "negative_tiny":
        return all(p[k] < 0 and float(f32(p[k]) - f32(math.floor(p[k]))) == 1.0 for k in aux)
    if cls.startswith("straddle"):
        T, axes = aux
        return all(abs(p[k]) < T <= 64 * abs(p[k]) for k in axes)
    if cls.startswith("beyond"):
        T, axes = aux
        return all(abs(p[k]) >= T for k in axes)
    if cls.startswith("at_"):
        T, axes = aux
        return all(abs(p[k]) == T for k in axes)
    if cls == "sin_limit":
        scale = 4.0 if tex == "NA" else float(f32(0.37))
        return abs(abs(scale * p[0]) - SIN_LIMIT) <= 32
    if cls == "near_zero":
        return all(abs(math.sin(10.0 * p[k])) <= 0.1 for k in aux)
    if cls in ("zero", "nested_zero"):
        return all(p[k] == 0.0 for k in aux)
    if cls in ("limit", "nested_limit"):
        return all(abs(10.0 * p[k]) >= SIN_LIMIT - 80 for k in aux)
    raise KeyError(cls)
