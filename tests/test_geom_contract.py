"""The ray-primitive and shading arithmetic, one operation at a time, against an exact reference (tests/geom_corpus.py).

Device and fp32 oracle share the arithmetic contract: a common-mode error in an intersector passes every
bit-exact test of the suite.  Here the contract itself (orc32 with ARITH_DEVICE) is held against the reference's
formulas evaluated in real arithmetic on the same fp32 inputs (CPU tier), and the device's production inline functions,
reached through rtmi_probe_geom, are held bit for bit against the oracle and against the same bounds (GPU tier).

Error analysis (u = eps / 2 = 2^-24 the unit roundoff, S = |o - c| + |r|, plus |c0| + |c1 - c0| for a moving centre,
whose A + B f the contract rounds):
  * sphere, radial error of the returned hit point | |o + t d - c| - |r| |.  oc carries one rounding per component
    (u |oc|); l = oc - (b/a) d takes the rounding of q = b/a times |q d| <= |oc| and one fma rounding (u |l|); the
    discriminant a (r^2 - |l|^2) is then off by about a (2 |l| |dl| + 3 u (r^2 + |l|^2)) ~ a (4 u |oc| r + 6 u r^2) near
    the surface, which moves the root by dD / (2 sqrt(D)) and, after the sqrt, the -b, the product with 1/a and the final
    o + t d, the point by a few u S.  The worst-case sum is ~ 6 u S = 3 eps S; the terms do
    not peak together and the measured maximum is 1.59 eps S, so K_RAD = 2 (the derivation's 3 would be 1.9x slack).  Near
    the tangent the radial error stays of that size (the point slides along the surface, it does not leave it).
  * sphere decisions: the tangent decision is uncertain where |r^2 - l^2| <= K_TAN eps |r| S (the discriminant's error
    divided by a), the choice of root where a root lies within dt = (K_T eps S + K_TAN eps |r| S / (2 h)) / |d| of t_min or
    t_max (h the half chord; the second term is the tangent error carried through the square root).
  * rect: t = (k - o_k) (1/d_k) is three roundings (<= 1.5 eps |t|), x = o_a + t d_a two more on top of t's error
    (<= eps (|o_a| + 2.5 |t d_a|)); band K_RECT = 3 covers both.  Where every intermediate is an fp32 value the fp32 test
    is exact and the band is empty: edges, corners, t == t_max and the denormal edge are asserted exactly.
  * AABB: each slab distance is three roundings, <= 1.5 eps |t|; the decision t_max <= t_min is uncertain within
    K_AABB eps (|t_min| + |t_max|), K_AABB = 1.5; exact (band empty) where every slab value is an fp32 value.
  * reflect: v - 2 (v.n) n, four roundings in the dot product and two in the update: <= K_REFL eps (|v| + 2 |v.n|).
  * refract: normalisation, dot, disc = 1 - eta^2 (1 - dt^2) a few eps (1 + eta^2); the vector a few eps (eta (1 + |dt|) +
    1) plus the disc error through the sqrt, eps (1 + eta^2) / sqrt(disc); ok-flag band |disc| <= K_DISC eps (1 + eta^2).
  * schlick: every value in [0, 1], about ten roundings: <= K_SCH eps absolute.
  * sphere_uv: atan2 / asin are within 3 ulp (tests/test_math_tables.py), i.e. <= 3e-7 absolute, then + pi, / 2 pi:
    u, v within K_UV eps absolute.  On the atan2 seam a zero z follows the contract's documented rule (rtmi_math.h:
    -0 is taken as +0, atan2(0, 0) = 0) where IEEE's signed zeros would give u = 1 or 0.5 instead of 0: those cases
    are counted ("zero_rule") and held to the rule.
Measured maxima of the contract (and, on the GPU box, of the device: bit-identical) are printed by every test and
quoted next to each constant."""
import math

import mpmath
import numpy as np
import pytest

import geom_corpus as gc
from oracle.oracle import ARITH_DEVICE, UV_BOOK
from raytracing_rust_amd import abi

EPS = gc.EPS
K = {"tan": 8.0, "t": 8.0, "rect": 3.0}  # decision bands (see the docstring)
K_RAD = 2.0  # radial error of a sphere hit point / (eps S); measured 1.59 (contract; also the medium queries)
K_RECT_T = 1.5  # rect / cube t relative error / eps; measured 0.79 (the derivation's three roundings: 1.5)
K_AABB = 1.5  # decision band; no case of the corpus falls inside it (the touching rays are exact)
K_TENTER = 1.5  # aabb_hit_t's t_enter relative error / eps (device only); three roundings, measured 0.86
K_REFL = 1.5  # measured 0.75
K_REFR = 1.25  # measured 0.61
K_DISC = 4.0  # refract's ok-flag band; 108 of 2048 cases inside it (the near-TIR class is aimed there)
K_SCH = 3.0  # measured 1.60
K_UV = 1.5  # measured 0.79
NEG_CONTROL_FACTOR = 10.0

_CORPUS = []


def corpus():
    if not _CORPUS:
        _CORPUS.append(gc.Corpus())
    return _CORPUS[0]


def _axis_of_face(f):
    return (2, 2, 1, 1, 0, 0)[f]


# ---------------------------------------------------------------------------------------------------------------------
# the oracle on the corpus
# ---------------------------------------------------------------------------------------------------------------------
def orc_prim(orc, flags):
    """(hit, t, normal axis) of every PRIM case through orc.hit"""
    C = corpus()
    objs = [gc.make(orc, s) for s in C.specs]
    out = []
    for i, ray in enumerate(C.rays):
        rec = orc.hit(objs[C.pidx[i]], ray[0:3], ray[3:6], ray[6], ray[7], ray[8], flags=flags)
        if rec is None:
            out.append((False, math.nan, -1))
        else:
            out.append((True, rec["t"], int(np.argmax(np.abs(rec["normal"])))))
    return out


def check_prims(got, orc64_got, label, faces=None):
    """got: (hit, t, normal axis) per case (faces: the device's face numbers).  Returns the measured statistics and
    asserts: decisions outside the bands equal the exact reference; t / radial error within the bounds."""
    C = corpus()
    st = {"checked": 0, "band": 0, "band_disagree": 0, "ieee": 0, "rad_k": 0.0, "rect_k": 0.0}
    bad = []
    for i, ray in enumerate(C.rays):
        spec = C.specs[C.pidx[i]]
        if spec.get("wrap"):
            continue
        hit, t, ax = got[i]
        ex = gc.prim_exact(spec, ray, K)
        if ex is None:  # non-finite intermediates: the reference's IEEE semantics (f64 literal oracle)
            st["ieee"] += 1
            h64, t64, _ = orc64_got[i]
            if hit != h64 or (hit and math.isnan(t) != math.isnan(t64)):
                bad.append((i, C.cls[i], "ieee", hit, t, h64, t64))
            continue
        st["checked"] += 1
        if ex.band:
            st["band"] += 1
            st["band_disagree"] += int(hit != ex.hit)
            continue
        if hit != ex.hit:
            bad.append((i, C.cls[i], spec["kind"], "hit", hit, ex.hit, float(ex.t) if ex.t is not None else None))
            continue
        if not hit:
            continue
        if spec["kind"] in ("sphere", "msphere"):
            k = gc.radial_error(ray, t, ex.c, ex.r) / (EPS * ex.S)
            st["rad_k"] = max(st["rad_k"], k)
            if k > K_RAD or abs(t - float(ex.t)) > ex.dt:
                bad.append((i, C.cls[i], spec["kind"], "t", t, float(ex.t), k))
        else:
            err = abs(t - float(ex.t))
            k = err / (EPS * abs(float(ex.t))) if ex.t != 0 else (0.0 if err == 0 else math.inf)
            st["rect_k"] = max(st["rect_k"], k)
            exact = ex.dt == 0.0
            if (exact and err != 0.0) or k > K_RECT_T:
                bad.append((i, C.cls[i], spec["kind"], "t", t, float(ex.t), k))
            if spec["kind"] == "cube":
                if faces is not None and faces[i] != ex.face:
                    bad.append((i, C.cls[i], "cube", "face", faces[i], ex.face))
                if ax != _axis_of_face(ex.face):
                    bad.append((i, C.cls[i], "cube", "normal axis", ax, ex.face))
    print("%s: %s" % (label, st))
    return st, bad


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------------------------------------------------
def test_corpus_composition():
    C = corpus()
    n = lambda arr, lab: int((arr == lab).sum())  # noqa: E731
    kinds = [s["kind"] for s in C.specs]
    assert len(C.rays) == gc.GROUP * len(C.specs) and len(C.rays) >= 3000
    assert all((C.pidx[g * gc.GROUP:(g + 1) * gc.GROUP] == g).all() for g in range(len(C.specs)))
    assert kinds.count("sphere") >= 2 * len(gc.SPHERE_PAIRS) and kinds.count("msphere") >= 4
    assert kinds.count("rect") >= 8 and kinds.count("cube") >= 4 and sum(bool(s.get("wrap")) for s in C.specs) >= 4
    radii = {abs(s["pair"][0]) for s in C.specs if s.get("pair")}
    assert {0.2, 10.0, 70.0, 1000.0} <= radii and any(s["kind"] == "sphere" and s["r"] < 0 for s in C.specs)
    for lab, lo in (("across", 700), ("tangent", 400), ("surface", 400), ("inside", 200), ("moving", 500),
                    ("moving_t0t1_equal", 64), ("edge", 90), ("parallel", 90), ("t_at_t_max", 40),
                    ("degenerate_x0_gt_x1", 64), ("denormal_edge", 64), ("edge_or_corner", 150), ("instanced", 256)):
        assert n(C.cls, lab) >= lo, lab
    d = np.linalg.norm(C.rays[:, 3:6], axis=1)
    assert d[C.cls == "across"].min() < 2e-3 and d[C.cls == "across"].max() > 500.0  # |d| from 1e-3 to 1e3
    assert (np.signbit(C.rays[:, 3:6]) & (C.rays[:, 3:6] == 0)).any()  # -0 direction components
    for lab in ("random", "touch_edge", "touch_corner", "grazing_face"):
        assert n(C.aabb_cls, lab) == 512, lab
    assert (C.aabb[:, 7] <= -gc.FMAX).sum() >= 100 and (C.aabb[:, 8] >= gc.FMAX).all()
    for lab in ("random", "near_tir", "near_zero", "grazing"):
        assert n(C.shade_cls, lab) == 512, lab
    assert n(C.uv_cls, "pole") == 256 and n(C.uv_cls, "seam") == 512
    z = C.uv[C.uv_cls == "seam"][:, 2]
    assert ((z == 0) & np.signbit(z)).any() and ((z == 0) & ~np.signbit(z)).any()
    times = {C.rays[g * gc.GROUP, 6] for g, s in enumerate(C.specs) if s["kind"] == "msphere" and s["t0"] != s["t1"]}
    assert {0.0, 1.0} <= times and any(0.0 < t < 1.0 for t in times)


def test_contract_prims_against_exact_reference(orc32, orc64):
    got = orc_prim(orc32, ARITH_DEVICE)
    ref64 = orc_prim(orc64, 0)
    st, bad = check_prims(got, ref64, "fp32 contract")
    assert not bad, bad[:10]
    assert st["checked"] >= 3000 and st["ieee"] >= 100
    # the bands are narrow: most cases are asserted (the tangent rays, 1/8 of the sphere rays, are aimed into the band)
    assert st["band"] <= 0.12 * st["checked"], st
    orc32.free_all()
    orc64.free_all()


def test_negative_control_literal_fp32_violates_the_sphere_bound(orc32):
    """flags 0: the literal b*b - a*c in fp32, as before substitution 5 (r04).  At the small far spheres its hit points
    lie NEG_CONTROL_FACTOR times farther off the surface than K_RAD allows: this test file would have caught that bug."""
    C = corpus()
    got = orc_prim(orc32, 0)
    worst = 0.0
    for i, ray in enumerate(C.rays):
        s = C.specs[C.pidx[i]]
        if s.get("pair") not in gc.FAR_SMALL or not got[i][0]:
            continue
        ex = gc.sphere_exact(s, ray, K["tan"], K["t"])
        if ex.hit and not ex.band:
            worst = max(worst, gc.radial_error(ray, got[i][1], ex.c, ex.r) / (EPS * ex.S))
    print("literal fp32 at the small far spheres: radial error up to %.1f eps S (bound %.1f)" % (worst, K_RAD))
    assert worst >= NEG_CONTROL_FACTOR * K_RAD
    orc32.free_all()


def orc_aabb(orc):
    C = corpus()
    return [orc.aabb_hit(r[0:3], r[3:6], r[9:15], r[7], r[8], flags=ARITH_DEVICE) for r in C.aabb]


def check_aabb(hits, t_enter=None, label=""):
    C = corpus()
    st = {"checked": 0, "band": 0, "band_disagree": 0, "exact": 0, "tenter_k": 0.0}
    bad = []
    for i, row in enumerate(C.aabb):
        h, te, band, exact = gc.aabb_exact(row, K_AABB)
        st["checked"] += 1
        st["exact"] += int(exact)
        if band:
            st["band"] += 1
            st["band_disagree"] += int(h != hits[i])
            continue
        if h != hits[i]:
            bad.append((i, C.aabb_cls[i], "hit", hits[i], h))
        if t_enter is not None and h and hits[i]:
            ref = float(te) if not isinstance(te, float) else te
            if math.isfinite(ref):
                err = abs(t_enter[i] - ref)
                k = err / (EPS * abs(ref)) if ref != 0 else (0.0 if err == 0 else math.inf)
                st["tenter_k"] = max(st["tenter_k"], k)
                if (exact and err != 0) or k > K_TENTER:
                    bad.append((i, C.aabb_cls[i], "t_enter", t_enter[i], ref))
            elif t_enter[i] != ref:
                bad.append((i, C.aabb_cls[i], "t_enter", t_enter[i], ref))
    print("%s aabb: %s" % (label, st))
    return st, bad


def test_contract_aabb_against_exact_reference(orc32):
    st, bad = check_aabb(orc_aabb(orc32), label="fp32 contract")
    assert not bad, bad[:10]
    assert st["exact"] >= 1000  # the touching rays are decided exactly: aabb.rs rejects t_max <= t_min


def orc_medium(orc, flags):
    C = corpus()
    out = {}
    for g in C.medium_groups:
        obj = gc.make(orc, C.specs[g])
        for i in range(g * gc.GROUP, (g + 1) * gc.GROUP):
            r = C.rays[i]
            out[i] = orc.medium_queries(obj, r[0:3], r[3:6], r[6], flags=flags)
    return out


def check_medium(res, label):
    """medium.rs:29-30: t1 = the first root in (-MAX, MAX), t2 = the first root beyond t1 + 0.0001"""
    C = corpus()
    st = {"checked": 0, "band": 0, "rad_k": 0.0}
    bad = []
    for i, (h1, t1, h2, t2) in res.items():
        ray = list(C.rays[i])
        ray[7], ray[8] = -gc.FMAX, gc.FMAX
        spec = C.specs[C.pidx[i]]
        ex = gc.sphere_exact(spec, ray, K["tan"], K["t"])
        st["checked"] += 1
        if ex.band:
            st["band"] += 1
            continue
        if h1 != ex.hit:
            bad.append((i, "h1", h1, ex.hit))
            continue
        if not h1:
            continue
        ta = ex.t
        tb = 2 * mpmath.mpf(-sum(gc.mpf(gc.Fr(a) - c) * b for a, c, b in zip(ray[0:3], ex.c, ray[3:6]))) / \
            mpmath.mpf(sum(b * b for b in ray[3:6])) - ta
        for t in (t1,) + ((t2,) if h2 else ()):
            k = gc.radial_error(ray, t, ex.c, ex.r) / (EPS * ex.S)
            st["rad_k"] = max(st["rad_k"], k)
            if k > K_RAD:
                bad.append((i, "radial", t, k))
        if abs(t1 - float(ta)) > ex.dt:
            bad.append((i, "t1", t1, float(ta)))
        gap = float(tb - ta) - 1e-4
        if abs(gap) <= 2 * ex.dt + EPS * abs(float(ta)):
            st["band"] += 1
            continue
        if h2 != (gap > 0) or (h2 and abs(t2 - float(tb)) > ex.dt):
            bad.append((i, "h2/t2", h2, t2, gap, float(tb)))
    print("%s medium: %s" % (label, st))
    return st, bad


def test_contract_medium_boundary_against_exact_reference(orc32):
    st, bad = check_medium(orc_medium(orc32, ARITH_DEVICE), "fp32 contract")
    assert not bad, bad[:10]
    assert st["checked"] >= 1500


def check_shade(res, label):
    """res[i] = (reflect (3), ok, refract (3), schlick)"""
    C = corpus()
    st = {"checked": 0, "band": 0, "refl_k": 0.0, "refr_k": 0.0, "sch_k": 0.0}
    bad = []
    for i, row in enumerate(C.shade):
        refl, ok, refr, disc, sch, vn, vl = gc.shade_exact(row)
        eta = row[6]
        st["checked"] += 1
        e = max(abs(float(refl[j]) - res[i][0][j]) for j in range(3)) / (EPS * (vl + 2 * vn))
        st["refl_k"] = max(st["refl_k"], e)
        if e > K_REFL:
            bad.append((i, C.shade_cls[i], "reflect", e))
        e = abs(float(sch) - res[i][3]) / EPS
        st["sch_k"] = max(st["sch_k"], e)
        if e > K_SCH:
            bad.append((i, "schlick", e))
        if abs(float(disc)) <= K_DISC * EPS * (1 + eta * eta):
            st["band"] += 1
            continue
        if res[i][1] != ok:
            bad.append((i, C.shade_cls[i], "refract ok", res[i][1], ok, float(disc)))
            continue
        if ok:
            scale = eta * 2 + 1 + (1 + eta * eta) / math.sqrt(float(disc))
            e = max(abs(float(refr[j]) - res[i][2][j]) for j in range(3)) / (EPS * scale)
            st["refr_k"] = max(st["refr_k"], e)
            if e > K_REFR:
                bad.append((i, C.shade_cls[i], "refract", e))
    print("%s shade: %s" % (label, st))
    return st, bad


def test_contract_shading_against_exact_reference(orc32):
    C = corpus()
    res = [orc32.shade(r[0:3], r[3:6], r[6], r[7], r[8]) for r in C.shade]
    st, bad = check_shade(res, "fp32 contract")
    assert not bad, bad[:10]
    assert sum(1 for r in res if not r[1]) >= 100  # total internal reflection is reached


def check_uv(res, label):
    C = corpus()
    st = {"checked": 0, "uv_k": 0.0, "zero_rule": 0}
    bad = []
    for i, n in enumerate(C.uv):
        # a zero z where IEEE atan2 and the contract's documented rule part (-0, or x = +-0 as well): the rule's value
        rule = n[2] == 0.0 and (np.signbit(n[2]) or n[0] == 0.0)
        st["zero_rule"] += int(rule)
        for b, book in enumerate((False, True)):
            u, v = gc.uv_exact(n, book, zero_as_plus=rule)
            e = max(abs(float(u) - res[i][2 * b]), abs(float(v) - res[i][2 * b + 1])) / EPS
            st["uv_k"] = max(st["uv_k"], e)
            st["checked"] += 1
            if e > K_UV:
                bad.append((i, C.uv_cls[i], book, e, list(n)))
    print("%s uv: %s" % (label, st))
    return st, bad


def test_contract_sphere_uv_against_exact_reference(orc32):
    C = corpus()
    res = [orc32.sphere_uv(n, flags=ARITH_DEVICE) + orc32.sphere_uv(n, flags=ARITH_DEVICE | UV_BOOK) for n in C.uv]
    st, bad = check_uv(res, "fp32 contract")
    assert not bad, bad[:10]


# ---------------------------------------------------------------------------------------------------------------------
# the device probe
# ---------------------------------------------------------------------------------------------------------------------
def _probe(op, rows, pidx, specs_lowered):
    A, B, meta, xforms = specs_lowered[:4]
    n = len(rows)
    inp = np.zeros((n, abi.PROBE_GEOM_IN), np.float32)
    inp[:, :min(rows.shape[1], 9)] = rows[:, :9]
    if rows.shape[1] > 9:
        inp[:, 10:10 + rows.shape[1] - 9] = rows[:, 9:]
    inp[:, 9] = np.asarray(pidx, np.int32).view(np.float32)
    out = np.zeros((n, abi.PROBE_GEOM_OUT), np.float32)
    M = (abi.PrimMeta * max(1, len(meta)))(*meta)
    X = (abi.Xform * max(1, len(xforms)))(*xforms)
    rc = abi.load_rtmi().rtmi_probe_geom(op, A.ctypes.data, B.ctypes.data, M, len(meta), X, len(xforms),
                                         inp.ctypes.data, out.ctypes.data, n)
    assert rc == 0, abi.load_rtmi().rtmi_last_error()
    return out


def test_probe_geom_without_device_or_with_bad_indices(host):
    """host side of rtmi_probe_geom: without a GPU it reports RTMI_ERR_DEVICE (like rtmi_probe_math, test_abi.py); with
    one, out-of-range primitive or transform indices and a divergent PRIM group are RTMI_ERR_INVALID before any launch"""
    lib = abi.load_rtmi()
    A, B, meta, xf, _ = gc.lower_prims(host, corpus().specs[:2])
    inp = np.zeros((64, abi.PROBE_GEOM_IN), np.float32)
    out = np.zeros((64, abi.PROBE_GEOM_OUT), np.float32)
    M = (abi.PrimMeta * 2)(*meta)
    X = (abi.Xform * 1)()
    call = lambda op, nprim, inp: lib.rtmi_probe_geom(op, A.ctypes.data, B.ctypes.data, M, nprim, X, 0,  # noqa: E731
                                                      inp.ctypes.data, out.ctypes.data, len(inp))
    if lib.rtmi_device_count() < 1:
        assert call(abi.PROBE_GEOM_PRIM, 2, inp) == abi.RTMI_ERR_DEVICE
        return
    bad = inp.copy()
    bad[:, 9] = np.int32(2).view(np.float32)
    assert call(abi.PROBE_GEOM_PRIM, 2, bad) == 1  # index == n_prims
    bad[:, 9] = np.int32(-1).view(np.float32)
    assert call(abi.PROBE_GEOM_MEDIUM, 2, bad) == 1
    mixed = inp.copy()
    mixed[5, 9] = np.int32(1).view(np.float32)
    assert call(abi.PROBE_GEOM_PRIM, 2, mixed) == 1  # two primitives in one group of 64
    assert call(abi.PROBE_GEOM_MEDIUM, 2, mixed) == 0  # MEDIUM reads its sphere per lane
    assert call(7, 2, inp) == 1
    meta2 = (abi.PrimMeta * 2)(*meta)
    meta2[0].flags |= 1 << abi.RTMI_PRIMFLAG_XF_COUNT_SHIFT  # a chain of one transform, xforms empty
    assert lib.rtmi_probe_geom(0, A.ctypes.data, B.ctypes.data, meta2, 2, X, 0, inp.ctypes.data, out.ctypes.data, 64) == 1


@pytest.mark.gpu
def test_device_prims_bit_identical_and_within_bounds(host, orc32, orc64):
    C = corpus()
    low = gc.lower_prims(host, C.specs)
    out = _probe(abi.PROBE_GEOM_PRIM, C.rays, C.pidx, low)
    # the three entry points of the traversals agree bit for bit and keep the primitive index
    assert np.array_equal(out[:, 0:3].view(np.uint32), out[:, 3:6].view(np.uint32)), "prim_test vs prim_test_vals"
    assert np.array_equal(out[:, 0:3].view(np.uint32), out[:, 6:9].view(np.uint32)), "prim_test vs prim_test_uniform"
    assert (out[:, 9] == 0).all()
    # the lowering leaves out rects that can only be met with a NaN t (x0 > x1: final_scene's light; rect.rs accepts a
    # ray lying in their plane with t = NaN): exactly those groups are not the probe's to compare
    dropped = low[4]
    assert [C.specs[g]["kind"] == "rect" and C.specs[g]["rect"][0] > C.specs[g]["rect"][2] for g in dropped] == [True] * len(dropped)
    assert len(dropped) == 1
    keep = ~np.isin(C.pidx, dropped)
    ref = orc_prim(orc32, ARITH_DEVICE)
    dev = [(bool(o[0]), float(o[1]) if o[0] else math.nan, _axis_of_face(int(o[2])) if C.specs[C.pidx[i]]["kind"] == "cube"
            else ref[i][2]) for i, o in enumerate(out)]
    for i, (a, b) in enumerate(zip(dev, ref)):
        if not keep[i]:
            dev[i] = ref[i]
            continue
        same_t = (not a[0]) or np.float32(a[1]).view(np.uint32) == np.float32(b[1]).view(np.uint32)
        assert a[0] == b[0] and same_t and (not a[0] or a[2] == b[2]), (i, C.cls[i], C.specs[C.pidx[i]]["kind"], a, b)
    st, bad = check_prims(dev, orc_prim(orc64, 0), "device", faces=[int(o[2]) for o in out])
    assert not bad, bad[:10]
    orc32.free_all()
    orc64.free_all()


@pytest.mark.gpu
def test_device_aabb_bit_identical_and_within_bounds(orc32):
    C = corpus()
    out = _probe(abi.PROBE_GEOM_AABB, C.aabb, np.zeros(len(C.aabb)), (np.zeros((1, 4), np.float32),) * 2 + ([], [], []))
    ref = orc_aabb(orc32)
    assert (out[:, 0] == out[:, 1]).all(), "aabb_hit vs aabb_hit_t"
    assert [bool(x) for x in out[:, 0]] == ref
    st, bad = check_aabb([bool(x) for x in out[:, 0]], [float(x) for x in out[:, 2]], "device")
    assert not bad, bad[:10]


@pytest.mark.gpu
def test_device_medium_boundary_bit_identical_and_within_bounds(host, orc32):
    C = corpus()
    low = gc.lower_prims(host, C.specs)
    rows = np.concatenate([C.rays[g * gc.GROUP:(g + 1) * gc.GROUP] for g in C.medium_groups])
    idx = np.concatenate([C.pidx[g * gc.GROUP:(g + 1) * gc.GROUP] for g in C.medium_groups])
    out = _probe(abi.PROBE_GEOM_MEDIUM, rows, idx, low)
    ref = orc_medium(orc32, ARITH_DEVICE)
    keys = sorted(ref)
    dev = {}
    for j, i in enumerate(keys):
        h1, t1, h2, t2 = ref[i]
        o = out[j]
        assert bool(o[0]) == h1 and bool(o[2]) == h2, (i, o, ref[i])
        assert (not h1 or np.float32(o[1]) == np.float32(t1)) and (not h2 or np.float32(o[3]) == np.float32(t2)), (i, o, ref[i])
        dev[i] = (bool(o[0]), float(o[1]), bool(o[2]), float(o[3]))
    st, bad = check_medium(dev, "device")
    assert not bad, bad[:10]
    orc32.free_all()


@pytest.mark.gpu
def test_device_shading_bit_identical_and_within_bounds(orc32):
    C = corpus()
    rows = np.zeros((len(C.shade), 15))
    rows[:, 3:6] = C.shade[:, 0:3]
    rows[:, 9:15] = C.shade[:, 3:9]
    out = _probe(abi.PROBE_GEOM_SHADE, rows, np.zeros(len(rows)), (np.zeros((1, 4), np.float32),) * 2 + ([], [], []))
    res = []
    for i, r in enumerate(C.shade):
        refl, ok, refr, sch = orc32.shade(r[0:3], r[3:6], r[6], r[7], r[8])
        o = out[i]
        assert np.array_equal(o[0:3], refl.astype(np.float32)) and bool(o[3]) == ok and np.float32(o[7]) == np.float32(sch), (i, o)
        assert not ok or np.array_equal(o[4:7], refr.astype(np.float32)), (i, o, refr)
        res.append((o[0:3].astype(np.float64), bool(o[3]), o[4:7].astype(np.float64), float(o[7])))
    st, bad = check_shade(res, "device")
    assert not bad, bad[:10]


@pytest.mark.gpu
def test_device_sphere_uv_bit_identical_and_within_bounds(orc32):
    C = corpus()
    rows = np.zeros((len(C.uv), 14))
    rows[:, 9:12] = C.uv
    rows[:, 13] = 1.0  # book flags: 0 (the reference's FRAC_2_PI), then 1 (RTMI_FLAG_UV_BOOK)
    out = _probe(abi.PROBE_GEOM_UV, rows, np.zeros(len(rows)), (np.zeros((1, 4), np.float32),) * 2 + ([], [], []))
    for i, n in enumerate(C.uv):
        ref = np.array(orc32.sphere_uv(n, flags=ARITH_DEVICE) + orc32.sphere_uv(n, flags=ARITH_DEVICE | UV_BOOK), np.float32)
        assert np.array_equal(out[i, 0:4], ref), (i, C.uv_cls[i], out[i, 0:4], ref)
    st, bad = check_uv([tuple(float(x) for x in o[0:4]) for o in out], "device")
    assert not bad, bad[:10]
