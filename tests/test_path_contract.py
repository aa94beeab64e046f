"""Camera rays, the rejection samplers, the medium's sample step, the transform chains and the material rules of one bounce,
one operation at a time, against exact references (tests/path_corpus.py).  CPU tier; tests/test_gpu_path_contract.py holds the device to the same checks.

Device and fp32 oracle share the arithmetic contract, so a common-mode error between a hit and the next
ray passes every bit-exact test of the suite.  Here the contract itself (orc32 with ARITH_DEVICE) is held against the
reference's formulas in real arithmetic on the same fp32 inputs and the same SCRIPTED words (oracle: orc_script; device:
RngScript of rtmi_probe_path), and the count of words each operation draws against the reference's draw order.

Error analysis (u = eps / 2 = 2^-24 the unit roundoff; second-order terms are covered by a factor 1 + 8 eps):
  * sampler components: 2 (k 2^-24) - 1 is a multiple of 2^-23 in [-1, 1): exact, asserted bit for bit.
  * sampler acceptance, sphere: x^2, y^2, z^2 carry one rounding each (absolute u x^2 ...: together u S with S = |p|^2),
    x^2 + y^2 one more (u (x^2 + y^2) <= u S) and the last sum one (u S): |fl(S) - S| <= 3 u S = 1.5 eps S.  Near the surface
    S = 1: fp32 `S < 1` can differ from the exact decision only where | |p|^2 - 1 | <= K_SPHERE eps, K_SPHERE = 1.5.  The
    disk has two squares and one sum: 2 u S, K_DISK = 1.0.  Where every square and partial sum is an fp32 value the test is
    exact and the band is EMPTY: the points with |p|^2 = 1 exactly (a component of -1; +1 is not on the lattice) are asserted rejected.  Measured on the corpus
    (contract): the farthest disagreement lies at 0.74 eps (sphere) and 0.53 eps (disk); the derivation's worst case needs
    all five roundings to fall the same way, so it is kept as it is (2x slack).
  * camera direction llc + u h + v vert - origin, componentwise.  u = (px + w) / nx is two roundings (relative 2 u), u h a
    third: B = u h is off by 3 u |B|, likewise C = v vert; the three sums add u (|A| + |B|), u (|A| + |B| + |C|) and
    u (|A| + |B| + |C| + |D|) (A = llc, D = origin).  With a lens D = O + (U x' + V y') carries 4 u (|O| + |a| + |b|) of its
    own (x' = x lens_radius one rounding, the product one, the two sums one each), which enters the last difference.
    Sum: u (3 |A| + 6 |B| + 5 |C| + 5 |D|) <= 6 u M = K_CAM eps M, M = |llc| + |u h| + |v vert| + |O| + |a| + |b|, K_CAM = 3;
    the origin alone K_RO = 2.  Measured (contract): direction 1.03, origin 0.49.  The pixel's last column under the top
    word, where (float)px + w rounds to the next pixel's edge and u is exactly 1.0, is inside that bound like any other case.
  * shutter time t0 + w (t1 - t0): the difference, the product and the sum, u (|t0| + 3 |w (t1 - t0)|) <=
    K_TIME eps (|t0| + |w (t1 - t0)|), K_TIME = 1.5; exactly t0 when the shutter is closed.  Measured 0.73.
  * medium_sample: dist_inside = (t2 - t1) dn is two roundings (relative eps); hit_distance = nid ln(w) is rtmi_logf's
    1 ulp (tests/test_math_tables.py: <= eps relative) and the product's u: relative 1.5 eps.  The decision can differ from
    the exact one only where |hd - dist| <= K_MED eps (|hd| + |dist|), K_MED = 1.5.  t_out = t1 + hd / dn adds the quotient's
    u (relative 2 eps on hd / dn) and the sum's u: <= K_TOUT eps (|t1| + |hd / dn|), K_TOUT = 2.5.  Measured 1.07.  All of it
    needs normal fp32 intermediates, which the corpus asserts.
  * transform chains, 2-norm of the error of the returned point.  A rotation computes c a + s b: two products and a sum,
    <= 2 u (|c a| + |s b|) <= eps |(a, b)| per component (Cauchy-Schwarz, c^2 + s^2 = 1 + O(eps)), sqrt(2) eps |(a, b)| for
    the pair; a translation u (|o| + |offset|); the point o' + t d' one product and one sum, <= eps (|o'| + |t d'|).  Later
    steps are isometries, so the errors add: <= K_XF eps sum over the steps of the magnitude each handles (|o| + |t| |d|
    going down, |p| coming back, plus |offset| at a translation), K_XF = 1.5 >= sqrt(2).  Measured 0.38 (point), 0.54 (normal).  The reference is the
    same chain in real arithmetic with the STORED sines and cosines (c^2 + s^2 differs from 1 by up to eps: the exact
    round trip scales by it, and the test reports that drift from o + t d separately).  The normal likewise, per rotation.
The material rules (one bounce: world.hit, then Material::scatter) have their derivations next to their constants, below.
No constant is taken from the device: its obligation is bit-identity with the oracle and the same bounds."""
import ctypes as C
import math
from fractions import Fraction as Fr

import mpmath
import numpy as np
import pytest

import geom_corpus as gc
import path_corpus as pc
from oracle.oracle import ARITH_DEVICE
from raytracing_rust_amd import abi

EPS = pc.EPS
SLACK = 1.0 + 8.0 * EPS  # second-order terms of every derivation above
K_SPHERE = 1.5  # acceptance band / eps; farthest disagreement of the contract 0.74 (device: bit-identical, so the same)
K_DISK = 1.0  # 0.53
K_CAM = 3.0  # direction error / (eps M); measured 1.03 (the worst case adds six roundings of one sign: 3x slack)
K_RO = 2.0  # origin error / (eps (|O| + |a| + |b|)); measured 0.49
K_TIME = 1.5  # measured 0.73
K_MED = 1.5  # decision band of medium_sample
K_TOUT = 2.5  # measured 1.07
K_XF = 1.5  # measured 0.38 (point), 0.54 (normal)
NEG_CONTROL_FACTOR = 10.0

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def bits(x):
    return np.float32(x).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# samplers
# ---------------------------------------------------------------------------------------------------------------------
def sampler_corpus(dim):
    return cached(("sampler", dim), lambda: pc.sampler_cases(dim, 1000 + dim))


def orc_sampler(orc, dim, wrong=None):
    words, _ = sampler_corpus(dim)
    return [orc.sample_unit(3 - dim, w, wrong=wrong) for w in words]


def check_sampler(got, dim, label):
    """got: (p, consumed, exhausted) per case.  Asserts: no script ran out; the words consumed are dim per trial; the
    point is the accepted trial's exact rationals bit for bit; every trial's decision equals the exact one outside the band.
    Returns the statistics per class."""
    words, cls = sampler_corpus(dim)
    k_band = K_SPHERE if dim == 3 else K_DISK
    st, bad = {}, []
    for i, (p, used, exhausted) in enumerate(got):
        s = st.setdefault(cls[i], {"n": 0, "accept_clear": 0, "reject_clear": 0, "band": 0, "band_differs": 0, "far": 0.0, "trials": set()})
        s["n"] += 1
        if exhausted or used % dim or used == 0:
            bad.append((i, cls[i], "script", used, exhausted))
            continue
        trials = used // dim
        s["trials"].add(trials)
        ex = pc.sampler_exact(words[i], dim, k_band)
        for t in range(trials):
            q, inside, band, s2 = ex[t]
            accepted = t == trials - 1
            if band:
                s["band"] += 1
                if accepted != inside:
                    s["band_differs"] += 1
                    s["far"] = max(s["far"], float(abs(s2 - 1)) / EPS)
            else:
                s["accept_clear" if inside else "reject_clear"] += 1
                if accepted != inside:
                    bad.append((i, cls[i], "decision", t, float(s2 - 1) / EPS))
        want = [float(c) for c in ex[trials - 1][0]] + [0.0] * (3 - dim)
        if [bits(c) for c in p] != [bits(c) for c in want]:
            bad.append((i, cls[i], "point", list(p), want))
    for name, s in sorted(st.items()):
        print("%s %s %-9s: %d cases, clear accept / reject %d / %d, in band %d (fp32 differs in %d, farthest %.2f eps), trials %s" % (
            label, "sphere" if dim == 3 else "disk", name, s["n"], s["accept_clear"], s["reject_clear"], s["band"],
            s["band_differs"], s["far"], sorted(s["trials"])))
    return st, bad


def assert_sampler_composition(st, dim):
    aimed = st["surface"]
    assert aimed["n"] == 1600 and aimed["accept_clear"] >= 20 and aimed["reject_clear"] >= 20 and aimed["band"] >= 20, aimed
    # fp32 rejects where the reference accepts inside the band (what the band exists for), nowhere beyond it
    assert 0 < aimed["band_differs"] and aimed["far"] <= (K_SPHERE if dim == 3 else K_DISK)
    assert st["shell"]["n"] == 96 and st["shell"]["band"] == 0 and st["shell"]["accept_clear"] >= 20 <= st["shell"]["reject_clear"]
    assert st["unit_axis"]["n"] == 2 * dim and st["unit_axis"]["band"] == 0  # exact: k = 0 rejected, k = 2^24 - 1 accepted
    assert st["unit_axis"]["reject_clear"] == dim and st["unit_axis"]["accept_clear"] == 2 * dim
    assert st["corner"]["n"] == 1 << dim and st["corner"]["reject_clear"] == 1 << dim and st["corner"]["trials"] == {2}
    assert st["origin"]["trials"] == {1}
    assert st["trials"]["trials"] == set(range(1, 10)) and st["trials"]["band"] == 0
    rnd = st["random"]  # not aimed: at most 1 % of its trials in the band
    assert rnd["band"] <= 0.01 * (rnd["band"] + rnd["accept_clear"] + rnd["reject_clear"]), rnd
    assert sum(s["n"] for s in st.values()) <= 4096


@pytest.mark.parametrize("dim", [3, 2], ids=["sphere", "disk"])
def test_sampler_contract_against_exact_reference(orc32, dim):
    st, bad = check_sampler(orc_sampler(orc32, dim), dim, "fp32 contract")
    assert not bad, bad[:10]
    assert_sampler_composition(st, dim)


@pytest.mark.parametrize("dim", [3, 2], ids=["sphere", "disk"])
def test_sampler_f64_reference_decides_exactly(orc64, dim):
    """the literal f64 oracle squares 24-bit components exactly: no band at all, the same checks with the band ignored"""
    words, cls = sampler_corpus(dim)
    for i, (p, used, exhausted) in enumerate(orc_sampler(orc64, dim)):
        ex = pc.sampler_exact(words[i], dim, 0)
        trials = used // dim
        assert not exhausted and used == dim * trials
        assert [e[1] for e in ex[:trials]] == [False] * (trials - 1) + [True], (i, cls[i])
        assert [float(c) for c in ex[trials - 1][0]] == list(p[:dim])


@pytest.mark.parametrize("dim", [3, 2], ids=["sphere", "disk"])
def test_sampler_negative_controls_are_caught(orc32, dim):
    """`<= 1` accepts the points with |p|^2 = 1 exactly, where the band is empty; a comparison `<= 1 + 1e-4` accepts
    points that lie 1e-4 / (K eps) > NEG_CONTROL_FACTOR band widths outside the sphere"""
    _, bad = check_sampler(orc_sampler(orc32, dim, wrong=1.0), dim, "control <= 1")
    assert {b[1] for b in bad if b[2] == "decision"} == {"unit_axis"} and len([b for b in bad if b[2] == "decision"]) == dim
    _, bad = check_sampler(orc_sampler(orc32, dim, wrong=1.0 + 1e-4), dim, "control <= 1 + 1e-4")
    worst = max(abs(b[4]) for b in bad if b[2] == "decision")
    assert worst >= NEG_CONTROL_FACTOR * (K_SPHERE if dim == 3 else K_DISK), worst
    print("controls caught: `<= 1` at the %d exact points; `<= 1 + 1e-4` up to %.0f eps outside" % (dim, worst))


# ---------------------------------------------------------------------------------------------------------------------
# camera
# ---------------------------------------------------------------------------------------------------------------------
def camera_corpus(host):
    """the lowered cameras (abi.Camera) per (spec, aspect) are built per case: Camera::new takes the aspect nx / ny"""
    def make():
        specs = pc.camera_specs()
        cases, rows, cls = pc.camera_cases(len(specs))
        rng = np.random.default_rng(31337)
        cams, index, cam_of = [], {}, []
        for c, nx, ny, px, j in cases:
            key = (int(c), int(nx), int(ny))
            if key not in index:
                index[key] = len(cams)
                cams.append(key)
            cam_of.append(index[key])
        states = []
        for c, nx, ny in cams:
            frm, at, up, vfov, aperture, focus, t0, t1 = specs[c][1]
            low = host.Camera(frm, at, up, vfov, float(nx) / float(ny), aperture, focus, t0, t1).lower()
            states.append(np.frombuffer(low, np.float32).copy())
        states = np.array(states, np.float32)
        words = np.array([pc.camera_script(rows[i], states[cam_of[i]][20] != 0.0, rng) for i in range(len(cases))], np.uint32)
        cases = cases.copy()
        cases[:, 0] = cam_of
        return specs, cams, states, cases, words, cls
    return cached("camera", make)


def orc_camera(orc, host):
    specs, cams, states, cases, words, _ = camera_corpus(host)
    # the oracle's cameras from exactly the lowered fp32 state the device gets and the exact reference reads (that this
    # state is Camera::new's, rounded once, is test_lowered_camera_fields_are_the_correctly_rounded_camera_new's business)
    objs = [orc.CameraFromState(state) for state in states]
    for obj, state in zip(objs, states):
        assert np.array_equal(orc.camera_state(obj).astype(np.float32).view(np.uint32), state.view(np.uint32))
    out = []
    for i, (c, nx, ny, px, j) in enumerate(cases):
        ray, used, exhausted = orc.pixel_ray(objs[c], int(px), int(j), int(nx), int(ny), words[i])
        out.append((ray, used, exhausted))
    return out


def check_camera(got, host, label):
    """got: ((ro, rd, time), consumed, exhausted) per case"""
    specs, cams, states, cases, words, cls = camera_corpus(host)
    st = {"rd_k": 0.0, "ro_k": 0.0, "time_k": 0.0, "top_edge": 0, "lens": 0, "pinhole": 0, "closed": 0, "pixels": {}}
    bad = []
    for i, (ray, used, exhausted) in enumerate(got):
        state = states[cases[i][0]]
        ro, rd, time, m_ro, m_rd, m_time, draws = pc.camera_exact(state, cases[i], words[i])
        if exhausted or used != draws:  # u, v; two words per disk trial with a lens only; then the time
            bad.append((i, "draws", used, draws, exhausted))
            continue
        st["lens" if state[20] != 0.0 else "pinhole"] += 1
        st["top_edge"] += cls[i] == "top_edge"
        name = specs[cams[cases[i][0]][0]][0]
        nx = int(cases[i][1])
        h_len = math.sqrt(sum(float(x) ** 2 for x in state[6:9]))
        for a in range(3):
            e_rd = abs(Fr(float(ray[3 + a])) - rd[a])
            e_ro = abs(Fr(float(ray[a])) - ro[a])
            if m_rd[a]:
                st["rd_k"] = max(st["rd_k"], float(e_rd / m_rd[a]) / EPS)
            if m_ro[a]:
                st["ro_k"] = max(st["ro_k"], float(e_ro / m_ro[a]) / EPS)
            if e_rd > Fr(K_CAM * EPS * SLACK) * m_rd[a] or e_ro > Fr(K_RO * EPS * SLACK) * m_ro[a]:
                bad.append((i, name, "ray", a, float(e_rd), float(e_ro)))
            if name in pc.REFERENCE_CAMERAS:  # the direction's error in pixels of this image: |horizontal| / nx each, which
                ny = int(cases[i][2])         # is |vertical| / ny (aspect = nx / ny): the figure goes by the image's height
                st["pixels"][(name, ny)] = max(st["pixels"].get((name, ny), 0.0), float(e_rd) / (h_len / nx))
        e_t = abs(Fr(float(ray[6])) - time)
        if state[18] == state[19]:
            st["closed"] += 1
            if bits(ray[6]) != bits(state[18]):
                bad.append((i, name, "closed shutter", ray[6]))
        if m_time:
            st["time_k"] = max(st["time_k"], float(e_t / m_time) / EPS)
        if e_t > Fr(K_TIME * EPS * SLACK) * m_time:
            bad.append((i, name, "time", float(e_t)))
    print("%s camera: %d cases (%d lens, %d pinhole, %d closed shutter, %d top-word edge); direction %.2f eps M (K %.1f), origin "
          "%.2f (K %.1f), time %.2f (K %.1f)" % (label, len(got), st["lens"], st["pinhole"], st["closed"], st["top_edge"],
                                                 st["rd_k"], K_CAM, st["ro_k"], K_RO, st["time_k"], K_TIME))
    print("%s camera: worst direction error in pixels (|horizontal| / nx = |vertical| / ny), by ny: %s" % (label, "; ".join(
        "%s %s" % (name, ", ".join("%d: %.1e" % (nx, v) for (n2, nx), v in sorted(st["pixels"].items()) if n2 == name))
        for name in sorted(pc.REFERENCE_CAMERAS))))
    return st, bad


def test_camera_contract_against_exact_reference(orc32, host):
    orc32.lib.orc_set_flags(ARITH_DEVICE)
    st, bad = check_camera(orc_camera(orc32, host), host, "fp32 contract")
    orc32.free_all()
    assert not bad, bad[:10]
    specs, cams, states, cases, words, cls = camera_corpus(host)
    assert len(cases) <= 4096 and st["lens"] >= 1000 and st["pinhole"] >= 1000 and st["closed"] >= 500
    assert st["top_edge"] >= 8 * len(specs)  # px = nx - 1 under the top word, for nx in {2, 400, 1920, 32768}, twice per camera
    assert set(int(x) for x in cases[:, 1]) == set(pc.SIZES) == set(int(x) for x in cases[:, 2])
    far = [np.abs(states[c][0:3]).max() for c in range(len(cams)) if specs[cams[c][0]][0] in ("cornell_box", "final_scene")]
    assert far and min(far) >= 600.0  # look_from far from the origin


def test_lowered_camera_fields_are_the_correctly_rounded_camera_new(orc64, host):
    """Camera::new (camera.rs:21-51) in mpmath against orc64's f64 state and the lowered fp32 fields.

    f64 bound (u64 = 2^-53).  theta and tan(theta / 2): the pi literal, a product, a quotient, a halving (exact) and libm's
    tan (1 ulp): 5 u64 relative, amplified by at most theta / sin(theta) <= 2.3 for vfov <= 90 -> half_height within 13 u64,
    half_width one more.  w = (from - at) / |from - at|: the difference u64 (of components up to the operands, not the
    result: cancellation is the inputs' own, both sides see the same fp32-valued inputs, exact in f64 for these
    corpus values), the norm 2.5 u64, the quotient 1: 4 u64.  u = unit(up x w): each component a difference of two
    products, 3 u64 (|a b| + |c d|) — relative to the products, not to the difference; with |up| = O(1) that is an absolute
    3 u64 |up| on a vector of length |up| sin(angle), then normalised: (4 + 3 / sin) u64.  v = w x u the same again.  The
    corner is from - hw u - hh v - f w: each term (14 + 4 + 3 / sin) u64 of its size, three sums.  Altogether below
    K_NEW64 u64 times (|from| + hw + hh + focus) / sin, K_NEW64 = 64, sin the sine between up and w (>= 0.2 in the corpus,
    asserted).  The fp32 field is then that f64 value rounded once: within 0.5 ulp32 (1 + 2^-20) of the exact value."""
    K_NEW64 = 64.0
    U64 = 2.0 ** -53
    worst64, worst32 = 0.0, 0.0
    for name, (frm, at, up, vfov, aperture, focus, t0, t1) in pc.camera_specs():
        for aspect in (1.0, 400.0 / 225.0):
            F, A, UP = (mpmath.matrix([mpmath.mpf(float(x)) for x in v]) for v in (frm, at, up))
            hh = mpmath.mpf(focus) * mpmath.tan(mpmath.mpf(vfov) * mpmath.pi / 180 / 2)
            hw = mpmath.mpf(aspect) * hh
            w = (F - A) / mpmath.norm(F - A)
            cross = lambda a, b: mpmath.matrix([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])  # noqa: E731
            cu = cross(UP, w)
            sin = mpmath.norm(cu) / mpmath.norm(UP)
            assert sin >= 0.2
            u = cu / mpmath.norm(cu)
            v = cross(w, u)
            exact = list(F) + list(F - hw * u - hh * v - mpmath.mpf(focus) * w) + list(2 * hw * u) + list(2 * hh * v) + list(u) + list(v) + [
                mpmath.mpf(t0), mpmath.mpf(t1), mpmath.mpf(aperture) / 2]
            size = [mpmath.norm(F)] * 3 + [mpmath.norm(F) + hw + hh + focus] * 3 + [2 * hw] * 3 + [2 * hh] * 3 + [1] * 6 + [1, 1, 1]
            got64 = orc64.camera_state(orc64.Camera(frm, at, up, vfov, aspect, aperture, focus, t0, t1))
            low = np.frombuffer(host.Camera(frm, at, up, vfov, aspect, aperture, focus, t0, t1).lower(), np.float32)
            for k in range(21):
                e64 = abs(mpmath.mpf(float(got64[k])) - exact[k]) / (U64 * size[k] / sin)
                worst64 = max(worst64, float(e64))
                assert e64 <= K_NEW64, (name, k, float(e64))
                assert bits(low[k]) == bits(got64[k]), (name, k)  # the lowering rounds the f64 state once
                half_ulp = float(np.spacing(np.abs(low[k]))) / 2 if low[k] != 0 else 2.0 ** -150
                e32 = abs(mpmath.mpf(float(low[k])) - exact[k])
                if abs(exact[k]) > K_NEW64 * U64 * size[k] / sin * 2 ** 24:  # components that are not a rounded zero
                    worst32 = max(worst32, float(e32 / half_ulp))
                    assert e32 <= half_ulp * (1 + 2.0 ** -20), (name, k, float(e32 / half_ulp))
                else:
                    assert e32 <= K_NEW64 * U64 * size[k] / sin, (name, k)
    orc64.free_all()
    print("Camera::new: f64 state within %.1f u64 (size / sin) of mpmath (K %.0f); fp32 fields within %.3f half-ulps" % (worst64, K_NEW64, worst32))


# ---------------------------------------------------------------------------------------------------------------------
# medium_sample
# ---------------------------------------------------------------------------------------------------------------------
def medium_corpus():
    return cached("medium", pc.medium_cases)


def orc_medium(orc):
    rows, dens, words, _ = medium_corpus()
    return [orc.medium_sample(*(float(x) for x in r[:5]), float(d), w, flags=ARITH_DEVICE) for r, d, w in zip(rows, dens, words)]


def check_medium(got, label):
    """got: (taken, t_out, consumed, exhausted) per case"""
    rows, dens, words, cls = medium_corpus()
    st, bad, worst = {}, [], 0.0
    for i, (taken, t_out, used, exhausted) in enumerate(got):
        s = st.setdefault(cls[i], {"n": 0, "draw": 0, "taken_clear": 0, "not_clear": 0, "band": 0, "band_differs": 0})
        s["n"] += 1
        draws, ex_taken, band, t_ex, mag = pc.medium_exact(rows[i], words[i][0], K_MED)
        if exhausted or used != int(draws):  # the draw happens iff t1 < t2 after the clamps
            bad.append((i, cls[i], "draws", used, draws))
            continue
        s["draw"] += draws
        if band:
            s["band"] += 1
            s["band_differs"] += taken != ex_taken
        else:
            s["taken_clear" if ex_taken else "not_clear"] += 1
            if taken != ex_taken:
                bad.append((i, cls[i], "decision", taken, ex_taken))
        if taken and t_ex is not None:
            k = float(abs(mpmath.mpf(float(t_out)) - t_ex) / mag) / EPS
            worst = max(worst, k)
            if k > K_TOUT * SLACK:
                bad.append((i, cls[i], "t_out", k))
    for name, s in sorted(st.items()):
        print("%s medium %-12s: %d cases, %d draw, taken / not outside the band %d / %d, in band %d (fp32 differs in %d)" % (
            label, name, s["n"], s["draw"], s["taken_clear"], s["not_clear"], s["band"], s["band_differs"]))
    print("%s medium: t_out within %.2f eps (|t1| + |hd / dn|) (K %.1f)" % (label, worst, K_TOUT))
    return st, bad


def assert_medium_composition(st):
    assert sum(s["n"] for s in st.values()) <= 4096
    for name in ("empty_equal", "empty_behind", "empty_beyond"):
        assert st[name]["n"] == 32 and st[name]["draw"] == 0
    for name in ("clamp_lohi", "clamp_lo-", "clamp_-hi", "clamp_--"):
        assert st[name]["n"] == 64 and st[name]["draw"] == 64
    assert st["word_zero"]["not_clear"] == st["word_zero"]["n"] == 64  # ln 0: never taken
    assert st["word_top"]["taken_clear"] >= 60  # the shortest distance there is
    assert st["flt_max"]["draw"] == 64 and st["flt_max"]["taken_clear"] >= 20 <= st["flt_max"]["not_clear"]
    for name in ("aimed", "scaled"):  # aimed at the decision: both sides well populated outside the band
        assert st[name]["taken_clear"] >= 20 and st[name]["not_clear"] >= 20, (name, st[name])
    assert st["aimed"]["band"] >= 20
    for name in ("scene", "clamp_lohi", "clamp_lo-", "clamp_-hi", "clamp_--", "flt_max", "word_top"):  # not aimed: <= 1 % in the band
        assert st[name]["band"] <= 0.01 * st[name]["n"], (name, st[name])
    assert st["scene"]["taken_clear"] >= 20 and st["scene"]["not_clear"] >= 20


def test_medium_sample_contract_against_exact_reference(orc32):
    st, bad = check_medium(orc_medium(orc32), "fp32 contract")
    assert not bad, bad[:10]
    assert_medium_composition(st)


# ---------------------------------------------------------------------------------------------------------------------
# transform chains
# ---------------------------------------------------------------------------------------------------------------------
def chain_corpus(host):
    def make():
        specs = pc.chain_specs()
        low = gc.lower_prims(host, [{"kind": "sphere", "c": (0.0, 0.0, 0.0), "r": 1.0, "wrap": w} for _, w, _ in specs])
        xforms, meta = [abi.Xform(x.kind, x.x, x.y, x.z) for x in low[3]], low[2]  # copies: the lowered scenes are freed
        first, count = [], []
        for m, (_, wraps, _) in zip(meta, specs):
            count.append((m.flags >> abi.RTMI_PRIMFLAG_XF_COUNT_SHIFT) & 15)
            first.append(m.flags >> abi.RTMI_PRIMFLAG_XF_FIRST_SHIFT)
            assert count[-1] == len(wraps)  # the lowering keeps every wrapper, a rotation by 0 included
        rows, idx = pc.chain_rows(specs)
        return specs, xforms, first, count, rows, idx
    return cached("chain", make)


def orc_chain(orc, host):
    specs, _, _, _, rows, idx = chain_corpus(host)
    out = []
    for r, s in zip(rows, idx):
        h = orc.ProbePoint(float(r[6]), r[7:10])
        for w in specs[s][1]:
            h = orc.Traslate(h, w[1]) if w[0] == "T" else orc.Rotate(w[1], h, w[2])
        rec = orc.hit(h, r[0:3], r[3:6], 0.0, 0.0, float("inf"), flags=ARITH_DEVICE)
        out.append((rec["p"], rec["normal"]))
    orc.free_all()
    return out


def check_chain(got, host, label):
    """got: (p, n) per case"""
    specs, xforms, first, count, rows, idx = chain_corpus(host)
    bad, st = [], {"p_k": 0.0, "n_k": 0.0, "tmin": {}}
    for i, (p, n) in enumerate(got):
        s = idx[i]
        recs = [(x.kind, float(x.x), float(x.y), float(x.z)) for x in xforms[first[s]:first[s] + count[s]]]
        pe, ne, straight, mag_p, mag_n = pc.chain_exact(recs, rows[i])
        e_p = mpmath.sqrt(sum((mpmath.mpf(float(p[a])) - gc.mpf(pe[a])) ** 2 for a in range(3)))
        e_n = mpmath.sqrt(sum((mpmath.mpf(float(n[a])) - gc.mpf(ne[a])) ** 2 for a in range(3)))
        st["p_k"] = max(st["p_k"], float(e_p / mag_p) / EPS)
        if e_p > K_XF * EPS * SLACK * mag_p:
            bad.append((i, specs[s][0], "point", float(e_p / mag_p) / EPS))
        if mag_n:
            st["n_k"] = max(st["n_k"], float(e_n / mag_n) / EPS)
            # |n| - 1 after the chain: what the exact chain makes of the input's own length, plus the same bound
            len_got = mpmath.sqrt(sum(mpmath.mpf(float(c)) ** 2 for c in n))
            len_ex = mpmath.sqrt(gc.mpf(sum(c * c for c in ne)))
            if e_n > K_XF * EPS * SLACK * mag_n or abs(len_got - len_ex) > K_XF * EPS * SLACK * mag_n:
                bad.append((i, specs[s][0], "normal", float(e_n / mag_n) / EPS))
        elif [bits(c) for c in n] != [bits(c) for c in rows[i][7:10]]:
            bad.append((i, specs[s][0], "normal untouched by translations"))
        # distance of the returned point from the exact o + t d, as a fraction of t_min = 0.001
        group = specs[s][0] if specs[s][0].startswith("cornell") else ("len15/1e4" if specs[s][0].startswith("len15/10000") else None)
        if group:
            d = mpmath.sqrt(sum((mpmath.mpf(float(p[a])) - gc.mpf(straight[a])) ** 2 for a in range(3)))
            st["tmin"][group] = max(st["tmin"].get(group, 0.0), float(d) / 0.001)
    print("%s chains: %d cases; point within %.2f eps sum|.| of the exact chain (K %.1f), normal %.2f" % (label, len(got), st["p_k"], K_XF, st["n_k"]))
    print("%s chains: worst |p - (o + t d)| / t_min: %s" % (label, ", ".join("%s %.3f" % kv for kv in sorted(st["tmin"].items()))))
    return st, bad


def test_chain_round_trip_contract_against_exact_reference(orc32, host):
    st, bad = check_chain(orc_chain(orc32, host), host, "fp32 contract")
    assert not bad, bad[:10]
    specs, xforms, first, count, rows, idx = chain_corpus(host)
    assert sorted(set(count)) == [1, 2, 3, 4, 15] and len(rows) <= 4096
    assert set(st["tmin"]) == {"cornell_box/box1", "cornell_box/box2", "len15/1e4"}


def test_stored_sines_and_cosines_are_the_correctly_rounded_ones(host):
    """rotate.rs:31-33 takes sin and cos of (pi / 180) angle in f64; the lowering stores them rounded to fp32.  Against
    mpmath's sine of the angle GIVEN IN DEGREES: the f64 radians carry the constant's, the product's and libm's rounding,
    <= 4 u64 |radians| + u64 <= 2e-15 absolute for |angle| <= 180, then half an fp32 ulp of the stored value (2^-150 for the
    stored denormal-free zero).  cos 90 is therefore 6.1e-17, not 0: the reference's own value."""
    specs, xforms, first, count, _, _ = chain_corpus(host)
    seen = set()
    for s, (_, wraps, _) in enumerate(specs):
        recs = xforms[first[s]:first[s] + count[s]]
        for x, w in zip(recs, reversed(wraps)):  # outermost first
            if w[0] == "T":
                assert x.kind == abi.XF_TRANSLATE and (x.x, x.y, x.z) == tuple(gc.f32(c) for c in w[1])
                continue
            assert x.kind == abi.XF_ROTATE_X + w[1]
            seen.add(w[2])
            rad = mpmath.mpf(w[2]) * mpmath.pi / 180
            for stored, exact in ((x.x, mpmath.sin(rad)), (x.y, mpmath.cos(rad))):
                half_ulp = float(np.spacing(np.abs(np.float32(stored)))) / 2
                assert abs(mpmath.mpf(float(stored)) - exact) <= half_ulp + 2e-15, (w, stored)
    assert seen == set(pc.ANGLES)


# ---------------------------------------------------------------------------------------------------------------------
# one bounce: the material rules of shade_hit / Material::scatter
# ---------------------------------------------------------------------------------------------------------------------
# Bounds of the scattered direction (u = eps / 2):
#   * Lambertian hn + rs: one rounding per component, so the correctly rounded sum, asserted EXACTLY (rs is exact, hn the
#     record's fp32 normal); T the texture value.
#   * Metal: v / |v| carries the dot product (2.5 u relative), the root and the quotient (u each): each component within
#     2.25 eps |v^|; reflect (K_REFL = 1.5 of tests/test_geom_contract.py, on |v^| + 2 |v^ . n| <= 3) amplifies that by at
#     most 3 and adds 4.5 eps; fuzz rs one product and one sum.  Together below K_METAL eps (1 + fuzz |rs|), K_METAL = 12
#     (loose: the terms do not peak together, measured 0.91); the decision refl . n > 0 is exact outside |refl . n| <= K_METAL eps (1 + fuzz |rs|).
#   * Dielectric: one word is drawn iff refract succeeded: disc = 1 - eta^2 (1 - (v^ . n)^2) > 0, exact outside test_geom_contract's
#     band |disc| <= K_DISC eps (1 + eta^2), K_DISC = 4; the choice u >= schlick is exact outside |u - schlick| <= K_SCH eps
#     (K_SCH = 3 there) plus the cosine's own 3 eps through schlick's slope (<= 5): K_CHOICE = 18 eps.
#   * Isotropic: rd = rs exactly; ro = o + t d, one product and one sum: <= eps (|o| + |t d|) per component.
K_METAL = 12.0
K_DISC = 4.0
K_CHOICE = 18.0
K_POINT = 1.0


def bounce_corpus():
    return cached("bounce", pc.bounce_cases)


def orc_bounce(orc, flags):
    rows, words, cls, obj, scale = bounce_corpus()
    world = pc.bounce_world(orc)
    out = [orc.bounce(world, r[0:3], r[3:6], float(r[6]), float(r[7]), float(r[8]), int(r[9]), pc.BOUNCE_MAX_DEPTH, w, flags=flags)
           for r, w in zip(rows, words)]
    orc.free_all()
    return out


def _first_accepted(words, start):
    """the sampler's accepted point from word `start` on (exact rationals) and the words it took; no band in this corpus"""
    at = start
    while True:
        p = [pc.comp(int(w) >> 8) for w in words[at:at + 3]]
        at += 3
        if sum(c * c for c in p) < 1:
            return p, at - start


def round_f32(q):
    """the fp32 value nearest to the rational q, ties to even: ONE rounding (through float64 there would be two)"""
    x = np.float32(float(q))
    best = None
    for c in (np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))):
        key = (abs(Fr(float(c)) - q), int(c.view(np.uint32)) & 1)
        if best is None or key < best[0]:
            best = (key, c)
    return float(best[1])


BOUNCE_STAT = ("n", "hit", "miss", "metal_scattered", "metal_absorbed", "metal_band", "refracted", "reflected", "choice_band", "tir",
               "drew", "disc_band", "glass")


def check_bounce(got, face_forward, label):
    """got: per case None (no hit) or dict(t, normal (the record's, before FACE_FORWARD), mat_kind, scattered, o, d, T, L,
    consumed, exhausted).  The material rules against real arithmetic on the fp32 record.  Returns the statistics, overall
    and per class (st["cls"]): refracted / reflected count the choices OUTSIDE the choice's band, metal_scattered /
    metal_absorbed the decisions outside Metal's."""
    rows, words, cls, obj, scale = bounce_corpus()
    st = {"metal_k": 0.0, "iso_k": 0.0, "kinds": {}, "cls": {}}
    bad = []
    for i, b in enumerate(got):
        c = st["cls"].setdefault(cls[i], dict.fromkeys(BOUNCE_STAT, 0))
        c["n"] += 1
        aimed_at = pc.BOUNCE_OBJECTS[obj[i]][0]
        name = aimed_at
        if b is not None and np.isfinite(b["t"]):  # the object that was hit, by where: it need not be the one aimed at
            x = float(rows[i][0]) + float(np.float32(b["t"])) * float(rows[i][3])
            name = pc.BOUNCE_OBJECTS[min(max(int(round(x / pc.BOUNCE_SPACING)), 0), len(pc.BOUNCE_OBJECTS) - 1)][0]
        if cls[i] in ("miss", "short_interval"):
            c["miss"] += b is None
            if b is not None:
                bad.append((i, cls[i], "hit"))
            continue
        if b is None:  # only the fog may let a ray through: every other ray of these classes is aimed at a surface
            c["miss"] += 1
            if aimed_at != "fog":
                bad.append((i, cls[i], aimed_at, "missed"))
            continue
        c["hit"] += 1
        if scale[i] < -60 or scale[i] > 63:  # out of range: held to the oracle only (the pinning test)
            continue
        if b["exhausted"]:
            bad.append((i, cls[i], "script"))
            continue
        kind = b["mat_kind"]
        st["kinds"][kind] = st["kinds"].get(kind, 0) + 1
        v = [Fr(float(x)) for x in rows[i][3:6]]
        n = [Fr(float(x)) for x in b["normal"]]
        medium_words = 1 if kind == abi.MAT_ISOTROPIC else 0  # the fog's one draw; plates in front of it draw none
        if name == "fog" and kind != abi.MAT_ISOTROPIC:
            medium_words = b["consumed"] - (b["consumed"] // 3) * 3 if b["scattered"] else b["consumed"]
        if face_forward and kind != abi.MAT_DIELECTRIC and sum(p * q for p, q in zip(v, n)) > 0:
            n = [-x for x in n]
        if int(rows[i][9]) >= pc.BOUNCE_MAX_DEPTH:  # color.rs:9: nothing scatters, the sampler draws nothing
            if b["scattered"] or b["consumed"] != medium_words:
                bad.append((i, cls[i], "depth", b["scattered"], b["consumed"]))
            continue
        if kind == abi.MAT_DIFFUSE_LIGHT:
            if b["scattered"] or b["consumed"] != 0 or [bits(x) for x in b["L"]] != [bits(x) for x in pc.LIGHT_RGB]:
                bad.append((i, cls[i], "light", b))
            continue
        if any(float(x) != 0.0 for x in b["L"]):
            bad.append((i, cls[i], "emission of a non-emitter"))
        if kind in (abi.MAT_LAMBERTIAN, abi.MAT_ISOTROPIC):
            rs, took = _first_accepted(words[i], medium_words)
            want = [round_f32(n[a] + rs[a]) if kind == abi.MAT_LAMBERTIAN else float(rs[a]) for a in range(3)]
            if not b["scattered"] or b["consumed"] != medium_words + took or [bits(x) for x in b["d"]] != [bits(x) for x in want]:
                bad.append((i, cls[i], name, "diffuse direction", list(b["d"]), want, b["consumed"]))
            if name in ("lambert", "lambert_moved", "lambert_flipped", "lambert_ball") and [bits(x) for x in b["T"]] != [bits(x) for x in pc.LAMBERT_RGB]:
                bad.append((i, cls[i], name, "T", list(b["T"])))
            if kind == abi.MAT_ISOTROPIC:
                if [bits(x) for x in b["T"]] != [bits(x) for x in pc.FOG_RGB]:
                    bad.append((i, cls[i], "fog T"))
                t = Fr(float(np.float32(b["t"])))
                for a in range(3):
                    o = Fr(float(rows[i][a]))
                    mag = abs(o) + abs(t * v[a])
                    k = float(abs(Fr(float(b["o"][a])) - (o + t * v[a])) / mag) / EPS if mag else 0.0
                    st["iso_k"] = max(st["iso_k"], k)
                    if k > K_POINT * SLACK:
                        bad.append((i, cls[i], "fog point", k))
            continue
        vn = gc.norm_q(v)
        vh = [gc.mpf(x) / vn for x in v]
        dt = sum(vh[a] * gc.mpf(n[a]) for a in range(3))
        if kind == abi.MAT_METAL:
            fuzz = min(pc.METAL[name.split("_")[0]], 1.0)  # material.rs:70
            rs, took = ([Fr(0)] * 3, 0) if fuzz == 0.0 else _first_accepted(words[i], 0)
            refl = [vh[a] - 2 * dt * gc.mpf(n[a]) + gc.mpf(Fr(float(np.float32(fuzz))) * rs[a]) for a in range(3)]
            size = 1 + fuzz * float(gc.norm_q(rs))
            dec = sum(refl[a] * gc.mpf(n[a]) for a in range(3))
            if b["consumed"] != took:
                bad.append((i, cls[i], name, "metal draws", b["consumed"], took))
            if abs(dec) <= K_METAL * EPS * size:
                c["metal_band"] += 1
            else:
                c["metal_scattered" if dec > 0 else "metal_absorbed"] += 1
                if b["scattered"] != bool(dec > 0):
                    bad.append((i, cls[i], name, "metal decision", float(dec)))
            if b["scattered"]:
                k = max(float(abs(mpmath.mpf(float(b["d"][a])) - refl[a])) for a in range(3)) / (EPS * size)
                st["metal_k"] = max(st["metal_k"], k)
                if k > K_METAL or [bits(x) for x in b["T"]] != [bits(x) for x in pc.LAMBERT_RGB]:
                    bad.append((i, cls[i], name, "metal vector", k))
            continue
        # Dielectric
        c["glass"] += 1
        ref = Fr(float(np.float32(pc.GLASS[name.split("_")[0]])))
        if not b["scattered"] or [bits(x) for x in b["T"]] != [bits(1.0)] * 3:
            bad.append((i, cls[i], name, "glass always scatters with attenuation 1"))
        if cls[i] == "ddn_zero":
            # dot(rd, hn) = +-0 is not > 0: entering, ni_over_nt = 1 / ref_idx, cosine 0, schlick 1.  Every fp32 intermediate is
            # exact here (rd = (-1, 0, +-0), hn = (0, 0, 1)): no band.  refract succeeds iff 1 - (1 / ref_idx)^2 > 0; then one
            # word is drawn and u >= 1 never holds: the reflected ray, rd - 2 (+-0) hn = rd.  The record's t and p are NaN.
            draws = int(ref > 1)
            c["drew"] += draws
            c["tir"] += 1 - draws
            c["reflected"] += draws
            if b["consumed"] != draws or not np.isnan(b["t"]) or not np.isnan(np.asarray(b["o"], np.float64)).all() or \
                    [float(x) for x in b["d"]] != [float(x) for x in rows[i][3:6]]:
                bad.append((i, cls[i], name, "ddn = 0", b["consumed"], list(b["d"]), list(b["o"])))
            continue
        ddn = sum(p * q for p, q in zip(v, n))
        eta = gc.mpf(ref) if ddn > 0 else 1 / gc.mpf(ref)
        cosine = (gc.mpf(ref) * gc.mpf(ddn) if ddn > 0 else -gc.mpf(ddn)) / vn
        disc = 1 - eta * eta * (1 - dt * dt)
        if abs(disc) <= K_DISC * EPS * (1 + eta * eta):
            c["disc_band"] += 1
            continue
        if b["consumed"] != int(disc > 0):  # exactly one word iff refract succeeded
            bad.append((i, cls[i], name, "glass draws", b["consumed"], float(disc)))
            continue
        outward = [(-x if ddn > 0 else x) for x in n]
        dto = -abs(dt)
        refr = [eta * (vh[a] - gc.mpf(outward[a]) * dto) - gc.mpf(outward[a]) * mpmath.sqrt(max(disc, 0)) for a in range(3)]
        refl = [gc.mpf(v[a]) - 2 * gc.mpf(ddn) * gc.mpf(n[a]) for a in range(3)]
        d_refr = max(abs(mpmath.mpf(float(b["d"][a])) - refr[a]) for a in range(3))
        d_refl = max(abs(mpmath.mpf(float(b["d"][a])) - refl[a]) for a in range(3)) / vn
        took_refr = d_refr < d_refl
        if min(d_refr, d_refl) > 1e-5:  # a structural check of the assembly (which vector, which normal, which ratio); the
            bad.append((i, cls[i], name, "glass vector", float(d_refr), float(d_refl)))  # vectors' own bounds: test_geom_contract
        if disc <= 0:
            c["tir"] += 1
            if took_refr and d_refl > 1e-5:
                bad.append((i, cls[i], name, "refraction under total internal reflection"))
            continue
        c["drew"] += 1
        r0 = ((1 - gc.mpf(ref)) / (1 + gc.mpf(ref))) ** 2
        prob = r0 + (1 - r0) * (1 - cosine) ** 5
        u = mpmath.mpf(int(words[i][0]) >> 8) / (1 << 24)
        # normal incidence on ref_idx 1: cosine = 1, x = 0 and r0 = 0 are exact in fp32, schlick is 0 exactly: no band, and
        # the word 0 equals it: `>=` refracts
        exact = cls[i] == "schlick_equal" and ref == 1
        if not exact and abs(u - prob) <= K_CHOICE * EPS:
            c["choice_band"] += 1
            continue
        if abs(d_refr - d_refl) < 1e-5:  # refraction and reflection coincide: nothing to tell apart
            bad.append((i, cls[i], name, "glass choice cannot be read", float(d_refr)))
            continue
        c["refracted" if u >= prob else "reflected"] += 1
        if took_refr != bool(u >= prob):
            bad.append((i, cls[i], name, "glass choice", float(u), float(prob)))
    tot = {k: sum(c[k] for c in st["cls"].values()) for k in BOUNCE_STAT}
    st.update(tot)
    print("%s bounce (face_forward %d): hits by material %s; metal vector %.2f eps (K %.0f); fog point %.2f eps (K %.0f)" % (
        label, face_forward, sorted(st["kinds"].items()), st["metal_k"], K_METAL, st["iso_k"], K_POINT))
    for name, c in sorted(st["cls"].items()):
        print("%s bounce %-14s: %4d cases, %4d hit; metal scattered / absorbed / band %d / %d / %d; glass %d: drew %d, no refraction %d "
              "(disc band %d), refracted / reflected / choice band %d / %d / %d" % (
                  label, name, c["n"], c["hit"], c["metal_scattered"], c["metal_absorbed"], c["metal_band"], c["glass"], c["drew"], c["tir"],
                  c["disc_band"], c["refracted"], c["reflected"], c["choice_band"]))
    return st, bad


def assert_bounce_composition(st, face_forward):
    """each class's own composition (asserted on whatever results are handed in: the oracle's on the CPU)"""
    C = st["cls"]
    assert set(st["kinds"]) == {0, 1, 2, 3, 4} and min(st["kinds"].values()) >= 8
    assert sum(c["n"] for c in C.values()) == len(bounce_corpus()[0]) <= 4096
    n_obj, n_glass = len(pc.BOUNCE_OBJECTS), len(pc.GLASS)
    for name in ("miss", "short_interval"):
        assert C[name]["n"] == C[name]["miss"] == n_obj
    # not aimed at a decision: every ray hits (the fog may let its own through), at most 1 % of a class in a band
    assert C["plain"]["n"] == 24 * n_obj and C["plain"]["hit"] >= 24 * (n_obj - 1) + 8
    assert C["plain"]["metal_band"] + C["plain"]["disc_band"] + C["plain"]["choice_band"] <= 0.01 * C["plain"]["n"]
    assert C["plain"]["metal_scattered"] >= 20 and C["plain"]["refracted"] >= 20
    assert C["depth_limit"]["n"] == n_obj and C["depth_limit"]["hit"] >= n_obj - 1
    assert C["lambert_cancel"]["hit"] == C["lambert_cancel"]["n"] == 4
    # aimed at Metal's decision: grazing rays on both sides, fuzz vectors that tip it
    g = C["graze"]
    assert g["hit"] == g["n"] == 18 * (len(pc.METAL) + n_glass)
    assert g["metal_scattered"] >= 20 and g["metal_band"] + g["metal_scattered"] + g["metal_absorbed"] == 18 * len(pc.METAL)
    assert face_forward or g["metal_absorbed"] >= 20
    # aimed at total internal reflection: both sides of refract's band
    g = C["glass_leaving"]
    assert g["hit"] == g["n"] == g["glass"] == 24 * n_glass and g["tir"] >= 20 and g["drew"] >= 20
    assert g["disc_band"] + g["choice_band"] <= 0.01 * g["n"]
    # aimed at the choice: SCHLICK_DELTAS word-ulps about the exact probability
    g = C["schlick"]
    assert g["hit"] == g["n"] == g["glass"] == 12 * len(pc.SCHLICK_DELTAS) * n_glass
    assert g["refracted"] >= 20 and g["reflected"] >= 20 and g["choice_band"] >= 20
    g = C["schlick_equal"]
    assert g["hit"] == g["n"] == 2 * n_glass and g["choice_band"] == 0 and g["refracted"] >= 2 and g["reflected"] >= 4
    g = C["ddn_zero"]
    assert g["hit"] == g["n"] == 6 * n_glass and g["drew"] == 12 and g["tir"] == 12
    g = C["scaled"]
    assert g["hit"] == g["n"] == 64 * (len(pc.METAL) + n_glass)


@pytest.mark.parametrize("face_forward", [0, 1])
def test_material_rules_contract_against_exact_reference(orc32, face_forward):
    from oracle.oracle import FACE_FORWARD
    st, bad = check_bounce(orc_bounce(orc32, ARITH_DEVICE | (FACE_FORWARD if face_forward else 0)), face_forward, "fp32 contract")
    assert not bad, bad[:10]
    assert_bounce_composition(st, face_forward)


def test_metal_fuzz_is_clamped_by_the_lowering(host):
    """Metal::new clamps fuzz to 1 (material.rs:70): Metal(fuzz = 5) is lowered with parameter 1"""
    mats = host.lower(pc.bounce_world(host)).arrays()["materials"]
    metal = [m.param for m in mats if m.kind == abi.MAT_METAL]
    assert sorted(set(metal)) == [0.0, float(np.float32(0.3)), 1.0], metal


def test_direction_magnitude_in_range_is_scale_free(orc32):
    """rd scaled by 2^k with d.d a normal fp32 number (k = -60, 60, 63): the same decision, the same words and, a power of
    two being exact, the same scattered vector as k = 0 (a reflection of the un-normalised ray scales with it)"""
    rows, words, cls, obj, scale = bounce_corpus()
    got = orc_bounce(orc32, ARITH_DEVICE)
    idx = [i for i in range(len(rows)) if cls[i] == "scaled"]
    n = len(pc.DIRECTION_SCALES)
    seen = 0
    for g in range(0, len(idx), n):
        group = {int(scale[i]): got[i] for i in idx[g:g + n]}
        base = group[0]
        for k in (-60, 60, 63):
            b = group[k]
            assert b["scattered"] == base["scattered"] and b["consumed"] == base["consumed"], (g, k)
            same = [bits(c) for c in b["d"]] == [bits(c) for c in base["d"]]
            scaled = [bits(c) for c in b["d"]] == [bits(np.float32(c) * np.float32(2.0) ** k) for c in base["d"]]
            assert (same or scaled) if base["scattered"] else True, (g, k, b["d"], base["d"])
            assert bits(b["t"]) == bits(np.float32(base["t"]) * np.float32(2.0) ** -k)
            seen += 1
    assert seen == 3 * 64


def test_out_of_range_direction_magnitude_pins_documented_difference_from_the_reference(orc32, orc64):
    """include/rtmi_query.h and include/rtmi_radiance.h state the supported range of a caller's |d|: d.d must be a normal fp32
    number (2^-63 < |d| < 2^64).  Outside it the fp32 contract differs from the reference, whose f64 scatters as at any
    scale; what it does instead is pinned here (and the device to it, bit for bit, in the GPU tier): when d.d overflows
    (k = 64, 66) normalize(rd) is rd / inf = 0, so Metal's reflected vector is the fuzz term alone or 0, and the
    Dielectric's cosine is NaN or its refract fails; when d.d is a denormal (k = -64, -70: 2^-128 and 2^-140 times |d|^2,
    denormals are kept) the decisions and draws hold but d.d has 21 and 9 bits left, and the normalised ray with it: the
    scattered vectors drift from their k = 0 values (five roundings at 9 bits, halved by the root, times reflect's 3: below 2^-6; measured 5e-3, and 1.4e-6 at 21 bits).  The f64 oracle gives the k = 0 decision at every k."""
    rows, words, cls, obj, scale = bounce_corpus()
    g32, g64 = orc_bounce(orc32, ARITH_DEVICE), orc_bounce(orc64, 0)
    differ = {k: 0 for k in (-70, -64, 64, 66)}
    absorbed = scatters64 = 0
    drift = {-70: 0.0, -64: 0.0}
    n_cases = {k: 0 for k in differ}
    idx = [i for i in range(len(rows)) if cls[i] == "scaled"]
    n = len(pc.DIRECTION_SCALES)
    base_of = {}
    for g in range(0, len(idx), n):  # the eight scales of one ray are consecutive; the k = 0 member is the reference point
        zero = [i for i in idx[g:g + n] if scale[i] == 0][0]
        for i in idx[g:g + n]:
            base_of[i] = zero
    for i in idx:
        k = int(scale[i])
        if k not in differ:
            continue
        ref = g64[base_of[i]]
        assert g64[i] is not None and g64[i]["scattered"] == ref["scattered"] and g64[i]["consumed"] == ref["consumed"], (i, k)  # the reference: scale-free
        n_cases[k] += 1
        b = g32[i]
        assert b is not None  # the plate is still hit: the rect test needs no d.d
        nonfinite = not np.isfinite(np.asarray(b["d"], np.float64)).all()
        differ[k] += int(b["scattered"] != ref["scattered"] or b["consumed"] != ref["consumed"] or nonfinite)
        name = pc.BOUNCE_OBJECTS[obj[i]][0]
        if k < 0 and b["scattered"] and g32[base_of[i]]["scattered"] and b["consumed"] == g32[base_of[i]]["consumed"] and not nonfinite:
            drift[k] = max(drift[k], float(np.abs(np.asarray(b["d"]) * (2.0 ** -k if np.abs(b["d"]).max() < 1e-6 else 1.0) - g32[base_of[i]]["d"]).max()))
        with np.errstate(over="ignore"):
            dd = rows[i][3] * rows[i][3] + rows[i][4] * rows[i][4] + rows[i][5] * rows[i][5]  # fp32, as ray_derive
        if np.isinf(dd) and name == "metal0":  # the documented case: rd / inf = 0, the reflection is 0, `dot > 0` fails
            assert not b["scattered"], (i, k)
            absorbed += 1
            scatters64 += int(ref["scattered"])
    print("out of range: cases / differing from the reference's decision, draws or finiteness: %s" % {k: (n_cases[k], differ[k]) for k in sorted(differ)})
    print("Metal(fuzz 0) rays whose d.d overflows: %d, all absorbed; the reference scatters %d of them" % (absorbed, scatters64))
    print("denormal d.d: largest drift of a scattered vector from its k = 0 value: %s" % drift)
    assert all(n_cases[k] == 64 for k in differ) and differ[64] > 0 and differ[66] > 0 and absorbed >= 8 and scatters64 >= 4
    assert differ[-64] == 0 and differ[-70] == 0 and 1e-5 < drift[-70] < 2.0 ** -6 and drift[-64] < 2.0 ** -6 * 2.0 ** -12


# ---------------------------------------------------------------------------------------------------------------------
# the device probe's host side
# ---------------------------------------------------------------------------------------------------------------------
def probe(op, inp, words, cams=None, xforms=None, scene=None):
    """rtmi_probe_path on n cases: inp [n, <= PROBE_PATH_IN] float32 (bit patterns), words [n, PROBE_PATH_WORDS] uint32"""
    n = len(inp)
    a = np.zeros((n, abi.PROBE_PATH_IN), np.float32)
    a[:, :inp.shape[1]] = inp
    w = np.ascontiguousarray(words, np.uint32)
    assert w.shape == (n, abi.PROBE_PATH_WORDS)
    out = np.zeros((n, abi.PROBE_PATH_OUT), np.float32)
    cams = np.ascontiguousarray(cams if cams is not None else np.zeros((0, 21)), np.float32)
    X = (abi.Xform * max(1, len(xforms or [])))(*(xforms or []))
    rc = abi.load_rtmi().rtmi_probe_path(scene, op, cams.ctypes.data if len(cams) else None, len(cams), X, len(xforms or []), a.ctypes.data,
                                         w.ctypes.data, out.ctypes.data, n)
    return rc, out


def test_probe_stream_without_device_or_with_bad_arguments():
    """host side of rtmi_probe_stream, and the script corpus's own shape (checked here, where no GPU is needed).  The entry
    point checks for a device first, as rtmi_probe_geom does: without one every call is RTMI_ERR_DEVICE and the
    RTMI_ERR_INVALID cases below run only where a GPU exists (they need none: nothing is launched before they return)."""
    lib = abi.load_rtmi()
    scripts = pc.stream_scripts(100)
    assert sorted(scripts) == ["render", "seven_ahead"] and all(s.shape == (100, pc.STREAM_STEPS) and s.max() <= 4 for s in scripts.values())
    want = pc.stream_expected(scripts["seven_ahead"][:8], 42, 0)
    assert not np.array_equal(want[5, 3], want[4, 3])  # lane 5 reads other words than its neighbour: other pixel, other place
    script = np.ascontiguousarray(scripts["render"])
    out = np.zeros(script.shape + (3,), np.uint32)
    call = lambda kind, s, steps, o, n: lib.rtmi_probe_stream(kind, 42, s.ctypes.data if s is not None else None, steps,  # noqa: E731
                                                              o.ctypes.data if o is not None else None, n)
    if lib.rtmi_device_count() < 1:
        assert call(0, script, pc.STREAM_STEPS, out, 100) == abi.RTMI_ERR_DEVICE
        return
    assert call(0, script, pc.STREAM_STEPS, out, 100) == 0
    assert call(-1, script, pc.STREAM_STEPS, out, 100) == 1 and call(3, script, pc.STREAM_STEPS, out, 100) == 1
    assert call(0, script, 0, out, 100) == 1 and call(0, script, 257, out, 100) == 1
    assert call(0, None, pc.STREAM_STEPS, out, 100) == 1 and call(0, script, pc.STREAM_STEPS, None, 100) == 1
    assert call(0, None, pc.STREAM_STEPS, None, 0) == 0
    high = script.copy()
    high[99, 199] = 5
    assert call(0, high, pc.STREAM_STEPS, out, 100) == 1


def test_probe_path_without_device_or_with_bad_arguments():
    """host side of rtmi_probe_path: without a GPU it reports RTMI_ERR_DEVICE; with one, an unknown op, NULL arrays and
    out-of-range camera, pixel and chain indices are RTMI_ERR_INVALID before any launch.  The device check comes first, as
    in rtmi_probe_geom, so on a machine without a GPU only RTMI_ERR_DEVICE can be observed; the RTMI_ERR_INVALID cases run
    wherever a device exists, in the non-GPU suite too (this test carries no gpu mark)."""
    lib = abi.load_rtmi()
    words = np.zeros((64, abi.PROBE_PATH_WORDS), np.uint32)
    inp = np.zeros((64, abi.PROBE_PATH_IN), np.float32)
    cam = np.zeros((1, 21), np.float32)
    case = np.array([[0, 4, 4, 3, 3]] * 64, np.uint32)
    if lib.rtmi_device_count() < 1:
        for op in range(6):
            assert probe(op, case.view(np.float32), words, cams=cam)[0] == abi.RTMI_ERR_DEVICE
        return
    assert probe(abi.PROBE_PATH_CAMERA, case.view(np.float32), words, cams=cam)[0] == 0
    for col, value in ((0, 1), (1, 0), (2, 0), (3, 4), (4, 4)):  # camera index, nx, ny, px, j
        wrong = case.copy()
        wrong[5, col] = value
        assert probe(abi.PROBE_PATH_CAMERA, wrong.view(np.float32), words, cams=cam)[0] == 1
    assert probe(abi.PROBE_PATH_CAMERA, case.view(np.float32), words)[0] == 1  # no cameras at all
    assert probe(-1, inp, words)[0] == 1 and probe(6, inp, words)[0] == 1
    assert probe(abi.PROBE_PATH_BOUNCE, inp, words)[0] == 1  # BOUNCE without a scene
    out = np.zeros((64, abi.PROBE_PATH_OUT), np.float32)
    X = (abi.Xform * 1)()
    for a, w, o in ((None, words, out), (inp, None, out), (inp, words, None)):
        assert lib.rtmi_probe_path(None, abi.PROBE_PATH_SPHERE, None, 0, X, 0, a.ctypes.data if a is not None else None,
                                   w.ctypes.data if w is not None else None, o.ctypes.data if o is not None else None, 64) == 1
    assert lib.rtmi_probe_path(None, abi.PROBE_PATH_SPHERE, None, 1, X, 0, inp.ctypes.data, words.ctypes.data, out.ctypes.data, 64) == 1
    chain = np.zeros((64, abi.PROBE_PATH_IN), np.float32)
    xf = [abi.Xform(abi.XF_TRANSLATE, 1.0, 2.0, 3.0)] * 2
    for first, count, rc in ((0, 2, 0), (1, 1, 0), (1, 2, 1), (-1, 1, 1), (0, -1, 1), (0, 16, 1), (2, 0, 0), (3, 0, 1)):
        chain[7, 7:9] = np.array([first, count], np.int32).view(np.float32)
        assert probe(abi.PROBE_PATH_XFORM_ROUNDTRIP, chain, words, xforms=xf)[0] == rc, (first, count)
    chain[7, 7:9] = 0.0
    assert probe(abi.PROBE_PATH_XFORM_ROUNDTRIP, chain, words, xforms=[abi.Xform(abi.XF_GATE_MIN, 0.0, 0.0, 0.0)])[0] == 1
    assert lib.rtmi_probe_path(None, abi.PROBE_PATH_SPHERE, None, 0, X, 0, None, None, None, 0) == 0  # n = 0: nothing to do
    assert isinstance(C.c_char_p(lib.rtmi_last_error()).value, bytes)
