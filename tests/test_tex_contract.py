"""Texture evaluation (texture.rs, perlin.rs), one value at a time, against an exact reference (tests/tex_corpus.py).

Device and fp32 oracle share the arithmetic contract and include/rtmi_math.h, so a common-mode error in the texture code
passes every bit-exact test of the suite.  Here the contract itself (orc32 with ARITH_DEVICE) and the f64 literal oracle
(orc64) are held against the reference's formulas evaluated exactly on the same inputs.  tests/test_gpu_tex_contract.py
holds the device to the fp32 oracle bit for bit and to the same bands and bounds.

Decisions.  The lattice cell and the permutation indices are integer work on exact values (p * 2^o is exact, floor is
exact): their band is empty, a wrong one shows as a wrong value.  The texel index is floor(u * nx), floor((1 - v) * ny),
clamped: uncertain where one rounding of u * nx, or two of (1 - v) * ny, can cross an integer (never where the products are
exact, as for power-of-two sizes on texel edges).  The checker branch is the sign of a product of three sines of 10 p_k:
uncertain where some |sin(10 p_k)| <= u |10 p_k| + E_sin(10 p_k), the rounding of the product 10 p_k plus the sine's own
error, E_sin(x) = 1e-6 (1 + 0.6 |x|) for rtmi_sinf (asserted by tests/test_math_contract.py up to |x| = 6e4; the corpus
places its near-zero cases below that) and 1 ulp for libm's.  Cases inside a band are counted and held to the fp32 oracle
only (by the GPU tier).  Outside the bands an image or solid value names its decision: every texel and every solid has a
colour of its own.

Rule.  rtmi_sinf returns 0 beyond 2^20 (include/rtmi_math.h).  A checker with some |10 p_k| beyond it takes the `even`
child (0 < 0 is false), a noise texture whose argument is beyond it has the value 0.5: counted as `rule`, held to the rule
with the bound 0 (0.5 (1 + 0) is exact).
An argument within its own error of 2^20 is in the band.

Value of a NoiseTexture, 0.5 (1 + sin(s p.x + 5 turb(p, 7))), in units of the unit roundoff u (2^-24, or 2^-53 for doubles):
  * an octave's point p 2^o is exact; u_k = p_k - floor(p_k) is one rounding of a value in [0, 1]: <= u;
  * the smoothstep u_k^2 (3 - 2 u_k) has slope <= 1.5 and three roundings of values <= 3 relative to a result <= 1:
    <= 1.5 u + 3 u = 4.5 u, and 1 - that one more: each interpolation factor is within 5.5 u;
  * the 8 weights f_i f_j f_k sum to 1 and each factor's error meets the other two factors' sums (1 each): the sum of the
    weights' errors is <= 2 * 3 * 5.5 u + 2 u (two products) = 35 u, times |c . w| <= sqrt 3: 61 u;
  * c . w with |c| = 1 and w = (u_k - d) within 1.5 u per component: 1.5 u sqrt 3 + 3 u sqrt 3 (three products, two
    sums) = 8 u, weighted by weights that sum to 1;
  * the product weight times c . w: sqrt 3 u in all; the 8 additions of partial sums <= sqrt 3: 14 u;
  * an octave is within 61 + 8 + 1.7 + 14 = 85 u; the octave weights 2^-o are exact and sum to < 2: 170 u; the 7
    additions of partial sums <= 2 sqrt 3: 24 u.  turb(p, 7) is within 194 u: K_TURB = 200.
  * the argument a = s p.x + 5 turb: 5 K_TURB u, and one rounding each of s p.x, 5 turb and the sum:
    d_a = 5 K_TURB u + u (|s p.x| + 5 turb + |a|);
  * the value: 0.5 (d_a + E_sin(a) + 2 u) (the sine's argument error, its own error, the rounding of 1 + sin; 0.5 is exact).
For fp32 and ordinary arguments E_sin dominates: 0.5e-6 (1 + 0.6 |a|) against 1000 u / 2 = 3e-5 from turb.
Image and solid values: the texel over 255 is one correctly rounded division (<= u relative), a solid is exact.

Measured maxima (printed by every test) are quoted next to the constants below."""
import collections

import mpmath
import numpy as np

import tex_corpus as tc
from oracle.oracle import ARITH_DEVICE

f32 = np.float32
K_TURB = tc.K_TURB  # = 200 u, derived above.  Measured on the corpus (CPU, fp32 contract; the device on the MI355X: the same
#                     bits): the whole value's error is at most 0.095 of its bound, and 13.8 u where |argument| <= 64; f64
#                     literal oracle: 0.66 of its bound (at arguments near 2^20, where u |argument| is the bound), 15.2 u
ROUND_TRIP = 1.0  # image values: one division, <= 1 u; measured 0.498 u (fp32) and 0.498 u (f64)

_CORPUS = []


def corpus():
    if not _CORPUS:
        _CORPUS.append(tc.Corpus())
    return _CORPUS[0]


def oracle_values(orc, trees, C, idx, flags):
    return [orc.tex_value(trees[C.tex[i]][0], float(C.uv[i][0]), float(C.uv[i][1]), C.xyz[i].astype(np.float64), flags=flags)
            for i in idx]


def check(C, idx, uvp, got, trees, prec, label, mut=None, quiet=False):
    """got[n]: the 3 channels of case idx[n] evaluated at uvp[n] = (u, v, p).  Asserts nothing; returns (statistics, the
    cases that break a decision or a bound)."""
    st = collections.Counter()
    mx = {"noise/bound": 0.0, "noise_u": 0.0, "image_u": 0.0}
    bad = []
    ur = tc.U[prec]
    for n, i in enumerate(idx):
        u, v, p = uvp[n]
        ex = tc.tex_exact(trees[C.tex[i]][1], float(u), float(v), [float(c) for c in p], prec, mut)
        if mut is not None:  # a mutated reference is held to the bands and bounds of the true one
            ex0 = tc.tex_exact(trees[C.tex[i]][1], float(u), float(v), [float(c) for c in p], prec)
            ex.band, ex.bound = ex0.band, ex0.bound
        st["checked"] += 1
        if ex.band:
            st["band"] += 1
            st["band/" + str(C.cls[i])] += 1
            continue
        st["rule"] += int(ex.rule)
        st[ex.leaf] += 1
        g = [float(c) for c in got[n]]
        with mpmath.workprec(tc.PREC):
            err = max(abs(float(ex.value[c] - mpmath.mpf(g[c]))) for c in range(3))
        if ex.leaf == "image":  # the decision, read back from the colour: the red channel is the texel's number
            _, nx, ny, _ = _leaf(trees[C.tex[i]][1], ex.path)
            if round(g[0] * 255.0) != ex.texel[0] + nx * ex.texel[1]:
                bad.append((int(i), C.tex[i], C.cls[i], "texel", round(g[0] * 255.0), ex.texel))
                continue
            mx["image_u"] = max(mx["image_u"], err / ur)
        elif ex.leaf == "noise" and not ex.rule and ex.bound > 0.0:
            mx["noise/bound"] = max(mx["noise/bound"], err / ex.bound)
            if abs(ex.arg) <= 64.0 and mut is None:
                mx["noise_u"] = max(mx["noise_u"], err / ur)
        if err > ex.bound or not np.isfinite(err):
            bad.append((int(i), C.tex[i], C.cls[i], ex.leaf, "rule" if ex.rule else "value", err, ex.bound, g[0]))
    if not quiet:
        print("%s: %s maxima %s" % (label, dict(st), {k: round(x, 4) for k, x in mx.items()}))
    return st, mx, bad


def _leaf(node, path):
    for side in path:
        node = node[1] if side == "odd" else node[2]
    return node


def _inputs(C, idx):
    return [(C.uv[i][0], C.uv[i][1], C.xyz[i]) for i in idx]


# ---------------------------------------------------------------------------------------------------------------------
def test_corpus_composition():
    C = corpus()
    n = collections.Counter(C.cls)
    print("classes:", dict(sorted(n.items())))
    print("families:", dict(collections.Counter(C.family)), "plates:", {f: len(C.plates(f)) for f in ("noise", "checker", "image")})
    assert 2000 <= len(C.tex) <= 4096
    for i in range(len(C.tex)):
        assert tc.has_property(C.cls[i], C.aux[i], C.tex[i], C.uv[i][0], C.uv[i][1], C.xyz[i]), (i, C.tex[i], C.cls[i], C.xyz[i])
    for lab, lo in (("interior", 300), ("lattice_x", 40), ("lattice_y", 40), ("lattice_z", 60), ("lattice_xyz", 20),
                    ("nextafter", 90), ("negative", 100), ("negative_tiny", 40), ("sin_limit", 200), ("beyond_2p64", 1),
                    ("near_zero", 120), ("zero", 30), ("limit", 60), ("nested", 240), ("edge", 100), ("integer", 100),
                    ("round_up", 100)):
        assert n[lab] >= lo, lab
    for name in tc.THRESHOLDS:
        assert n["straddle_" + name] >= 40 and n["at_" + name] >= 16, name
        for axes in ((0,), (1,), (2,), (0, 1, 2)):  # each coordinate in turn, and all three together
            assert any(c == "straddle_" + name and a[1] == axes for c, a in zip(C.cls, C.aux)), (name, axes)
    noise = C.family == "noise"
    assert {"NA", "NB"} <= set(C.tex[noise]) and (C.tex == "NB").sum() >= 400  # two tables, two scales
    assert sorted(tc.depth_of(s) for k, s in tc.SPECS if k in ("CK1", "CK2", "CK16O", "CK16E")) == [1, 2, 16, 16]
    # the nests are walked to both ends and to every kind of leaf: the innermost of 16 levels, the first level's solid
    walked = collections.Counter((t, ) + tc.walk(dict(tc.SPECS)[t], [float(c) for c in p])
                                 for t, c, p in zip(C.tex, C.cls, C.xyz) if c == "nested")
    print("nested walks (texture, depth, leaf):", dict(walked))
    for t in ("CK16O", "CK16E"):
        assert {d for (tt, d, _) in walked if tt == t} == {1, 16}, (t, walked)
    assert {d for (tt, d, _) in walked if tt == "CK2"} == {2} and {leaf for (_, _, leaf) in walked} == {"noise", "image", "solid"}
    assert min(walked.values()) >= 5, walked
    z = C.xyz[C.cls == "zero"]
    assert ((z == 0) & np.signbit(z)).any() and ((z == 0) & ~np.signbit(z)).any()
    # power-of-two sizes: u * nx is exactly an integer on the texel edges; the others round
    exact = sum(1 for t, c, uv in zip(C.tex, C.cls, C.uv) if t in ("i2x2", "i16x8") and c == "integer"
                and (float(uv[0]) * tc.IMAGES[t][0]).is_integer())
    assert exact >= 30, exact
    assert {t for t in C.tex[C.family == "image"]} == set(tc.IMAGES)


def test_tables_agree_between_the_apis(host, orc32, orc64):
    """the three constructors draw the same tables from the seeded scene RNG; the fp32 side holds them rounded once"""
    t64, t32, th = tc.build(orc64, "f64"), tc.build(orc32, "f32"), tc.build(host, "f64")
    for name in ("NA", "NB"):
        assert t64[name][1][3] == t32[name][1][3] == th[name][1][3]
        assert t64[name][1][2] == th[name][1][2]
        r64, r32 = orc64.perlin_tables(t64[name][0])[0], orc32.perlin_tables(t32[name][0])[0]
        assert np.array_equal(r64.astype(f32), r32.astype(f32)) and np.array_equal(r32, r32.astype(f32).astype(np.float64))
    assert t64["NA"][1][3] != t64["NB"][1][3]


def test_contract_against_exact_reference(orc32):
    C = corpus()
    idx = range(len(C.tex))
    trees = tc.build(orc32, "f32")
    got = oracle_values(orc32, trees, C, idx, ARITH_DEVICE)
    st, mx, bad = check(C, idx, _inputs(C, idx), got, trees, "f32", "fp32 contract")
    assert not bad, bad[:10]
    # the bands are narrow: only the classes aimed into them have cases there; the rule is reached by both kinds
    aimed = ("near_zero", "limit", "nested_limit", "sin_limit", "nextafter", "integer", "edge", "round_up", "nested")
    assert {k[5:] for k in st if k.startswith("band/")} <= set(aimed) and st["band/nested"] <= 5, st
    assert st["band"] <= 0.2 * st["checked"], st
    assert st["rule"] >= 100 and st["noise"] >= 1200 and st["image"] >= 800 and st["solid"] >= 300, st
    assert mx["noise/bound"] <= 1.0 and mx["image_u"] <= ROUND_TRIP
    # the case the disagreement between device and oracle was first seen at
    i = int(np.flatnonzero(C.cls == "beyond_2p64")[0])
    assert abs(got[i][0] - 0.8832566) < 1e-6, got[i]


def test_f64_literal_oracle_against_exact_reference(orc64):
    C = corpus()
    idx = range(len(C.tex))
    trees = tc.build(orc64, "f64")
    got = oracle_values(orc64, trees, C, idx, 0)
    st, mx, bad = check(C, idx, _inputs(C, idx), got, trees, "f64", "f64 literal oracle")
    assert not bad, bad[:10]
    assert st["band"] <= 0.02 * st["checked"] and st["rule"] == 0, st
    assert mx["noise/bound"] <= 1.0 and mx["image_u"] <= ROUND_TRIP


MUTATION_CLASSES = {  # where a mutation of the reference has to show (it may show elsewhere too)
    "octaves6": ("interior",),
    "cell_before_floor": ("negative", "negative_tiny"),
    "v_not_flipped": ("interior", "integer", "edge"),
    "checker_le": ("zero", "limit", "nested_zero", "nested_limit"),
    "cast32": ("straddle_2p64", "at_2p64", "beyond_2p64"),
    "no_sin_rule": ("sin_limit", "limit", "nested_limit"),
}


def test_negative_controls(orc32):
    """Each mutation of the reference makes the contract fail on the corpus.  cell_before_floor: the cell is the cast of the
    coordinate itself and the fraction is taken relative to it (for a positive coordinate the cast IS the floor; the two
    part at negative ones and from 2^64 on); cast32: the 32-bit cast's former rule, 0 for everything from 2^32 on;
    no_sin_rule: the true sine beyond 2^20, where the contract's is 0 (the rule cases are held to 0.5 and to the `even`
    child exactly, so a contract without the rule fails them one by one)."""
    C = corpus()
    trees = tc.build(orc32, "f32")
    assert set(MUTATION_CLASSES) == set(tc.MUTATIONS)
    for mut, classes in MUTATION_CLASSES.items():
        idx = [i for i in range(len(C.tex)) if C.cls[i] in classes]
        got = oracle_values(orc32, trees, C, idx, ARITH_DEVICE)
        _, _, clean = check(C, idx, _inputs(C, idx), got, trees, "f32", mut, quiet=True)
        _, _, bad = check(C, idx, _inputs(C, idx), got, trees, "f32", mut, mut=mut, quiet=True)
        caught = collections.Counter(b[2] for b in bad)
        print("mutation %s: caught in %d of %d cases %s" % (mut, len(bad), len(idx), dict(caught)))
        assert not clean and len(bad) >= 5, (mut, clean[:3], len(bad))
        if mut == "no_sin_rule":  # every noise case decided by the rule is caught: its bound is 0 and no true sine is 0
            ruled = {i for i in idx if C.family[i] == "noise" and tc.tex_exact(
                trees[C.tex[i]][1], float(C.uv[i][0]), float(C.uv[i][1]), [float(c) for c in C.xyz[i]], "f32").rule}
            assert len(ruled) >= 50 and ruled <= {b[0] for b in bad}, (len(ruled), len(bad))
        if mut == "cast32":
            # the cases whose y or z alone reaches 2^64 are caught, but for one or two at a crest of the final sine, where the
            # changed turbulence moves the value by less than its bound.  (x there puts the sine's argument beyond 2^20: the
            # value is 0.5 by the rule whatever the cell; all three there make every fraction 0 and the noise 0.)
            want = {i for i in idx if C.aux[i][1] in ((1,), (2,))}
            assert len(want) >= 30 and len(want - {b[0] for b in bad}) <= 2, (len(want), len(bad))


def test_the_32_bit_cast_rule_keeps_the_low_bits():
    """the device's 32-bit restatement of `as usize` (csrc/rtmi_shade.hpp as_usize_u32), restated once
    more here, gives the low 8 bits of the 64-bit cast and of its wrapping + 1 for every fp32 value"""
    def rule32(x):
        if not x > 0.0:
            return 0
        if x >= 2.0 ** 64:
            return 0xFFFFFFFF
        return int(min(x, 2.0 ** 32 - 256))  # the clamp's end: low 8 bits 0, as a multiple of 512 has

    xs = [0.0, -0.0, -1.0, float("nan"), float("inf"), 0.5, 255.0, 256.0, 2.0 ** 24, 2.0 ** 31, 2.0 ** 32 - 256, 2.0 ** 32,
          2.0 ** 32 + 512, 2.0 ** 63, float(np.nextafter(f32(2.0 ** 64), f32(0))), 2.0 ** 64, 2e20, 3.4e38]
    xs += [float(f32(x)) for x in np.random.default_rng(5).uniform(0, 1, 500) * 2.0 ** np.random.default_rng(6).integers(0, 70, 500)]
    for x in xs:
        x = float(np.floor(f32(x)))
        want = 0 if not x > 0 else tc.USIZE_MAX if x == float("inf") else tc.as_usize(int(x))
        for d in (0, 1):
            assert ((rule32(x) + d) & 0xFFFFFFFF) & 255 == ((want + d) & tc.USIZE_MAX) & 255, (x, d)
