"""Deterministic corpus and exact references for tests/test_path_contract.py and tests/test_gpu_path_contract.py.

What a path does between a hit and its next ray: the rejection samplers (util.rs:4-24), Camera::get_ray under the pixel's
u, v (camera.rs:53-67, tests/test.rs:66-68), ConstantMedium::hit after its boundary queries (medium.rs:33-53) and the
round trip of a hit through a chain of Traslate / Rotate wrappers (traslate.rs:18-24, rotate.rs:85-113), and one bounce
(world.hit, then Material::scatter, material.rs:49-168) over a small hand-built world.  Every input is
an fp32 value or a 32-bit word of a SCRIPT: the words the operation draws, in order, in place of a Philox stream.  The
exact references evaluate the reference's formulas in real arithmetic (fractions.Fraction; mpmath at 200 bits for ln and
the norms) on those inputs.  Seeds are fixed; every class is named and the tests assert each class's composition."""
import math
from fractions import Fraction as Fr

import mpmath
import numpy as np

from geom_corpus import EPS, FMAX, f32, is_f32, mpf

mpmath.mp.prec = 200
WORDS = 32  # RTMI_PROBE_PATH_WORDS: the length of every script
ORIGIN_K = 1 << 23  # the word whose component is 0: p = (0, 0, 0) is accepted
TOP_K = (1 << 24) - 1
EXHAUSTED_WORD = 0x80000000  # what a draw beyond the script delivers: k = 2^23


def word(k, rng):
    """a 32-bit word whose upper 24 bits are k; the lower 8 are noise, which rtmi_u01 drops"""
    return ((int(k) << 8) | int(rng.integers(0, 256))) & 0xFFFFFFFF


def comp(k):
    """the sampler's component 2 (k 2^-24) - 1 as a rational"""
    return Fr(int(k), 1 << 23) - 1


def script(ks, rng, fill=ORIGIN_K):
    ks = list(ks) + [fill] * (WORDS - len(ks))
    assert len(ks) == WORDS
    return [word(k, rng) for k in ks]


# ---------------------------------------------------------------------------------------------------------------------
# samplers
# ---------------------------------------------------------------------------------------------------------------------
def sampler_cases(dim, seed):
    """(words [n, WORDS] uint32, class names) for random_in_unit_sphere (dim 3) / random_in_unit_disk (dim 2)"""
    rng = np.random.default_rng(seed)
    rows, cls = [], []

    def add(name, ks):
        rows.append(script(ks, rng))
        cls.append(name)

    def inside():
        while True:
            k = rng.integers(0, 1 << 24, dim)
            if sum(comp(x) ** 2 for x in k) < Fr(9, 10):
                return [int(x) for x in k]

    def outside():
        while True:
            k = rng.integers(0, 1 << 24, dim)
            if sum(comp(x) ** 2 for x in k) > Fr(11, 10):
                return [int(x) for x in k]

    # aimed at the surface: the leading components chosen, the last solved to within +-2 lattice steps of |p|^2 = 1
    for _ in range(320):
        while True:
            lead = [int(x) for x in rng.integers(0, 1 << 24, dim - 1)]
            rest = 1 - sum(comp(x) ** 2 for x in lead)
            if rest > Fr(1, 100):
                break
        z = math.sqrt(float(rest)) * (1.0 if rng.integers(0, 2) else -1.0)
        k0 = int(round((z + 1.0) * (1 << 23)))
        for delta in (-2, -1, 0, 1, 2):
            k = min(max(k0 + delta, 0), TOP_K)
            add("surface", lead + [k])
    # clear of the band on either side: |p|^2 = 1 +- 2^-20, 2^-16, 2^-14 (a comparison against 1 + 1e-4 decides these wrongly)
    for n in range(96):
        r = (1.0 if n & 1 else -1.0) * 2.0 ** (-20, -16, -14)[n % 3]
        while True:
            lead = [int(x) for x in rng.integers(0, 1 << 24, dim - 1)]
            rest = 1 + Fr(r) - sum(comp(x) ** 2 for x in lead)
            if rest > Fr(1, 100):
                break
        z = math.sqrt(float(rest)) * (1.0 if rng.integers(0, 2) else -1.0)
        add("shell", lead + [min(max(int(round((z + 1.0) * (1 << 23))), 0), TOP_K)])
    # |p|^2 = 1 exactly: one component -1 (k = 0), the others 0; and +1 is not on the lattice (k = 2^24 - 1: 1 - 2^-23)
    for axis in range(dim):
        for k in (0, TOP_K):
            ks = [ORIGIN_K] * dim
            ks[axis] = k
            add("unit_axis", ks)
    for m in range(1 << dim):
        add("corner", [TOP_K if (m >> a) & 1 else 0 for a in range(dim)])
    add("origin", [ORIGIN_K] * dim)
    # 0 to 8 rejected trials before the accepted one; neighbouring lanes leave the loop at different trials
    for rep in range(64):
        for r in range(9):
            ks = []
            for _ in range(r):
                ks += outside()
            add("trials", ks + inside())
    # plain random words; the tenth trial is the origin so that the script cannot run out
    for _ in range(1024):
        ks = [int(x) for x in rng.integers(0, 1 << 24, dim * 9)]
        add("random", ks)
    return np.array(rows, np.uint32), cls


def sampler_exact(words, dim, k_band):
    """per trial of the script: (p as rationals, |p|^2 < 1, in the band).  The band is empty where the fp32 evaluation is
    exact: every square and every partial sum an fp32 value."""
    out = []
    for t in range(WORDS // dim):
        p = [comp(int(w) >> 8) for w in words[dim * t:dim * t + dim]]
        sq = [c * c for c in p]
        s = sum(sq)
        partial, exact = Fr(0), True
        for q in sq:
            partial += q
            exact = exact and is_f32(q) and is_f32(partial)
        band = (not exact) and abs(s - 1) <= Fr(k_band) * Fr(EPS) * (1 + 8 * Fr(EPS))
        out.append((p, s < 1, band, s))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# camera
# ---------------------------------------------------------------------------------------------------------------------
# (look_from, look_at, view_up, vfov, aperture, focus_dist, time0, time1); aspect = nx / ny of the case
REFERENCE_CAMERAS = {  # tests/test.rs: the eight drivers use four cameras
    "random_spheres": ((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, 0.1, 10.0, 0.0, 1.0),
    "simple_light": ((13.0, 3.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 50.0, 0.1, 10.0, 0.0, 1.0),
    "cornell_box": ((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), (0.0, 1.0, 0.0), 40.0, 0.1, 10.0, 0.0, 1.0),
    "final_scene": ((478.0, 278.0, -600.0), (278.0, 278.0, 0.0), (0.0, 1.0, 0.0), 40.0, 0.1, 10.0, 0.0, 1.0),
}
SIZES = (1, 2, 400, 1920, 32768)
CAM_WORD_KS = (0, 1, 1 << 23, TOP_K)


def camera_specs():
    """(name, spec) of every camera of the corpus: the reference's four, each also with a pinhole lens and with a closed
    shutter, and random ones"""
    rng = np.random.default_rng(20240611)
    specs = []
    for name, s in REFERENCE_CAMERAS.items():
        specs.append((name, s))
        specs.append((name + "/pinhole", s[:4] + (0.0,) + s[5:]))
        specs.append((name + "/closed_shutter", s[:6] + (0.25, 0.25)))
    for i in range(6):
        frm = tuple(f32(x) for x in rng.uniform(-1000.0, 1000.0, 3))
        at = tuple(f32(x) for x in rng.uniform(-100.0, 100.0, 3))
        up = tuple(f32(x) for x in rng.normal(0.0, 1.0, 3))
        specs.append(("random%d" % i, (frm, at, up, f32(rng.uniform(10.0, 90.0)), f32(rng.uniform(0.0, 2.0)) if i % 2 else 0.0,
                                       f32(rng.uniform(0.5, 900.0)), f32(rng.uniform(-1.0, 1.0)), f32(rng.uniform(1.0, 3.0)))))
    return specs


def camera_cases(n_cams, seed=77):
    """(cases [n, 5] uint32 = camera, nx, ny, px, j; words [n, WORDS]; classes).  The script of a case: u, v, then disk
    trials (read only by a camera with a lens: 0 to 2 points far outside, then one far inside), then the time."""
    rng = np.random.default_rng(seed)
    full = []
    for nx in SIZES:
        for ny in SIZES:
            for px in sorted({0, min(1, nx - 1), nx - 1}):
                for j in sorted({0, min(1, ny - 1), ny - 1}):
                    for ku in CAM_WORD_KS:
                        for kv in CAM_WORD_KS:
                            full.append((nx, ny, px, j, ku, kv))
    cases, rows, cls = [], [], []
    per_cam = 4000 // n_cams
    for c in range(n_cams):
        pick = rng.permutation(len(full))[:per_cam]
        for n, idx in enumerate(pick):
            nx, ny, px, j, ku, kv = full[idx]
            if n < 2 * len(SIZES):  # always there: the last pixel of a row under the top word, where u is exactly 1.0
                nx = SIZES[n % len(SIZES)]
                px, ku = nx - 1, TOP_K
            rejected = int(rng.integers(0, 3))
            disk = []
            for _ in range(rejected):
                disk += [int(rng.choice([0, TOP_K])), int(rng.choice([0, TOP_K]))]  # a corner: |p|^2 ~ 2
            while True:
                k = [int(x) for x in rng.integers(0, 1 << 24, 2)]
                if sum(comp(x) ** 2 for x in k) < Fr(9, 10):
                    break
            kt = int(rng.choice(CAM_WORD_KS))
            cases.append((c, nx, ny, px, j))
            # both layouts of the script: with a lens the time follows the disk trials, without it follows v directly
            rows.append((ku, kv, disk + k, kt))
            cls.append("top_edge" if (ku == TOP_K and px >= 1) else "plain")
    return np.array(cases, np.uint32), rows, cls


def camera_script(row, has_lens, rng):
    ku, kv, disk, kt = row
    return script([ku, kv] + (disk if has_lens else []) + [kt], rng)


def camera_exact(state, case, words):
    """state: the camera's 21 fp32 fields.  Returns (ro, rd, time) as rationals, the magnitudes of the two bounds
    (componentwise for ro and rd, a scalar for the time) and the words the reference draws."""
    F = [Fr(float(x)) for x in state]
    O, LLC, H, V, U, W = (F[3 * i:3 * i + 3] for i in range(6))
    t0, t1, lens = F[18], F[19], F[20]
    _, nx, ny, px, j = (int(x) for x in case)
    ks = [int(w) >> 8 for w in words]
    u = (px + Fr(ks[0], 1 << 24)) / nx
    v = (j + Fr(ks[1], 1 << 24)) / ny
    at = 2
    off_a, off_b = [Fr(0)] * 3, [Fr(0)] * 3
    if lens != 0:
        while True:
            x, y = comp(ks[at]), comp(ks[at + 1])
            at += 2
            if x * x + y * y < 1:
                break
        off_a = [c * (x * lens) for c in U]
        off_b = [c * (y * lens) for c in W]
    ro = [O[i] + off_a[i] + off_b[i] for i in range(3)]
    rd = [LLC[i] + u * H[i] + v * V[i] - ro[i] for i in range(3)]
    w = Fr(ks[at], 1 << 24)
    at += 1
    time = t0 + w * (t1 - t0)
    m_ro = [abs(O[i]) + abs(off_a[i]) + abs(off_b[i]) for i in range(3)]
    m_rd = [abs(LLC[i]) + abs(u * H[i]) + abs(v * V[i]) + m_ro[i] for i in range(3)]
    m_time = abs(t0) + abs(w * (t1 - t0))
    return ro, rd, time, m_ro, m_rd, m_time, at


# ---------------------------------------------------------------------------------------------------------------------
# medium_sample
# ---------------------------------------------------------------------------------------------------------------------
def medium_cases(seed=4242):
    """(rows [n, 6] float32 = t1, t2, t_min, closest, dn, neg_inv_density; densities [n] float32; words [n, WORDS];
    classes).  neg_inv_density = -(1 / density) in fp32, as the lowering stores it."""
    rng = np.random.default_rng(seed)
    rows, dens, words, cls = [], [], [], []

    def add(name, t1, t2, t_min, closest, dn, density, k):
        density = np.float32(density)
        nid = -(np.float32(1.0) / density)
        rows.append([t1, t2, t_min, closest, dn, nid])
        dens.append(density)
        words.append(script([k], rng))
        cls.append(name)

    def aimed_t2(t1, dn, density, k, rel):
        """t2 such that dist_inside = (t2 - t1) dn is (1 + rel) times the exact hit distance of word k"""
        nid = -(np.float32(1.0) / np.float32(density))
        hd = float(nid) * math.log(k * 2.0 ** -24)
        return f32(float(np.float32(t1)) + hd * (1.0 + rel) / float(np.float32(dn)))

    scene_density = (0.01, 0.0001, 0.5, 2.0)  # cornell_smoke's, final_scene's two, and denser ones
    for _ in range(512):  # scene ranges, decision wherever it falls
        t1 = f32(rng.uniform(0.0, 800.0))
        add("scene", t1, f32(t1 + rng.uniform(0.01, 400.0)), 0.001, f32(rng.choice([FMAX, t1 + rng.uniform(0.0, 800.0)])),
            f32(rng.uniform(0.5, 30.0)), rng.choice(scene_density), int(rng.integers(1, 1 << 24)))
    for n in range(256):  # the two clamps, either side
        t1 = f32(rng.uniform(-5.0, 5.0))
        t2 = f32(t1 + rng.uniform(0.5, 50.0))
        t_min = f32(t1 + (1 if n & 1 else -1) * rng.uniform(0.001, 0.4))
        closest = f32(t2 + (1 if n & 2 else -1) * rng.uniform(0.001, 0.4))
        add("clamp_%s%s" % ("lo" if n & 1 else "-", "hi" if not n & 2 else "-"), t1, t2, t_min, closest, f32(rng.uniform(0.5, 2.0)),
            rng.choice([0.05, 0.5]), int(rng.integers(1, 1 << 24)))
    for n in range(96):  # t1 >= t2 after the clamps: no draw
        t1 = f32(rng.uniform(0.0, 10.0))
        kind = n % 3
        if kind == 0:
            add("empty_equal", t1, t1, 0.001, FMAX, 1.0, 0.5, int(rng.integers(1, 1 << 24)))
        elif kind == 1:  # the whole interval behind t_min
            add("empty_behind", f32(t1 - 20.0), f32(t1 - 15.0), t1, FMAX, 1.0, 0.5, int(rng.integers(1, 1 << 24)))
        else:  # the closest hit so far lies before the entry
            add("empty_beyond", f32(t1 + 1.0), f32(t1 + 2.0), 0.001, t1, 1.0, 0.5, int(rng.integers(1, 1 << 24)))
    for _ in range(64):
        t1 = f32(rng.uniform(0.0, 10.0))
        add("word_zero", t1, f32(t1 + rng.uniform(1.0, 1e6)), 0.001, FMAX, 1.0, rng.choice([1e-4, 0.5, 100.0]), 0)
        add("word_top", t1, f32(t1 + rng.uniform(1e-3, 10.0)), 0.001, FMAX, 1.0, rng.choice([0.01, 0.5]), TOP_K)
    for _ in range(64):  # nothing hit yet: closest = FLT_MAX and an exit far away
        t1 = f32(rng.uniform(0.0, 10.0))
        add("flt_max", t1, f32(10.0 ** rng.uniform(28.0, 30.5) if _ % 4 else rng.uniform(1e30, 5e37)), 0.001, FMAX, f32(rng.uniform(0.5, 2.0)), 1e-30, int(rng.integers(1, 1 << 24)))
    for n in range(512):  # |d| and the density across 2^+-40, the interval scaled to match, decision aimed within 2^-6
        e, g = int(rng.integers(-40, 41)), int(rng.integers(-40, 41))
        dn = f32(rng.uniform(1.0, 2.0) * 2.0 ** e)
        density = f32(rng.uniform(1.0, 2.0) * 2.0 ** g)
        k = int(rng.integers(1, 1 << 24))
        t1 = f32(rng.uniform(0.0, 2.0) * 2.0 ** (-g - e))
        add("scaled", t1, aimed_t2(t1, dn, density, k, rng.uniform(-2.0 ** -6, 2.0 ** -6)), 0.0, FMAX, dn, density, k)
    for n in range(768):  # aimed at the decision: dist_inside within a few eps of the hit distance, and clear of it
        dn = f32(rng.uniform(0.5, 30.0))
        density = rng.choice(scene_density)
        k = int(rng.integers(1, 1 << 24))
        t1 = f32(rng.uniform(0.001, 3.0))
        rel = (rng.choice([-1.0, 1.0]) * EPS * rng.choice([0.25, 1.0, 4.0, 16.0, 64.0, 1024.0]))
        add("aimed", t1, aimed_t2(t1, dn, density, k, rel), 0.001, FMAX, dn, density, k)
    return np.array(rows, np.float32), np.array(dens, np.float32), np.array(words, np.uint32), cls


def medium_exact(row, w0, k_band):
    """(draws, taken, in the band, t_out (mpf) or None, |t1| + |hd / dn| the magnitude of t_out's bound)"""
    t1, t2, t_min, closest, dn, nid = (Fr(float(x)) for x in row)
    t1 = max(t1, t_min)
    t2 = min(t2, closest)
    if not t1 < t2:
        return False, False, False, None, None
    k = int(w0) >> 8
    if k == 0:  # ln 0 = -inf: the hit distance is +inf, never below dist_inside
        return True, False, False, None, None
    dist = mpf((t2 - t1) * dn)
    hd = mpf(nid) * mpmath.log(mpmath.mpf(k) / (1 << 24))
    for q in (dist, hd, hd / mpf(dn)):  # the derivation needs normal fp32 intermediates
        assert mpmath.mpf(2) ** -120 < abs(q) < mpmath.mpf(2) ** 127, (row, q)
    band = abs(hd - dist) <= k_band * EPS * (abs(hd) + abs(dist))
    return True, bool(hd < dist), bool(band), mpf(t1) + hd / mpf(dn), abs(mpf(t1)) + abs(hd / mpf(dn))


# ---------------------------------------------------------------------------------------------------------------------
# word delivery under divergence (rtmi_probe_stream)
# ---------------------------------------------------------------------------------------------------------------------
STREAM_STEPS = 200
# what a render draws, as script bytes (1 uniform, 2 take2, 3 take3, 4 re-init, 0 idle)
_CAMERA = ([4, 2, 1], [4, 2, 2, 1], [4, 2, 2, 2, 1])  # a new path: u and v, disk trials with a lens, the time
_BOUNCE = ([3], [3, 3], [3, 3, 3], [1], [1, 3], [1, 1, 3, 3], [1, 1], [0], [0, 0, 0], [0] * 7)  # Lambertian / Metal trials, Schlick, fog


def stream_scripts(lanes, seed=2718):
    """{name: [lanes, STREAM_STEPS] uint8}.  render: every lane starts at its own phase (lane % 4 single draws), then runs
    camera samples and bounces of its own, with idle stretches and re-inits mid-way.  seven_ahead: lane 5 draws 3 + 3 + 1
    words while its neighbours idle, then all lanes draw in step."""
    rng = np.random.default_rng(seed)
    render = np.zeros((lanes, STREAM_STEPS), np.uint8)
    for lane in range(lanes):
        ops = [1] * (lane % 4)
        while len(ops) < STREAM_STEPS:
            ops += _CAMERA[int(rng.integers(0, len(_CAMERA)))] if rng.random() < 0.15 else _BOUNCE[int(rng.integers(0, len(_BOUNCE)))]
        render[lane] = ops[:STREAM_STEPS]
    ahead = np.zeros((lanes, STREAM_STEPS), np.uint8)
    ahead[5, 0:3] = (3, 3, 1)
    common = []
    while len(common) < STREAM_STEPS - 3:
        common += [3, 1, 2, 3, 3, 1, 1, 2]
    ahead[:, 3:] = common[:STREAM_STEPS - 3]
    return {"render": render, "seven_ahead": ahead}


def stream_expected(script, seed, stream_id):
    """what rtmi_probe_stream delivers for the script: [lanes, steps, 3] uint32 from raytracing_rust_amd.philox.Stream"""
    from raytracing_rust_amd.philox import Stream

    lanes, steps = script.shape
    out = np.zeros((lanes, steps, 3), np.uint32)
    for lane in range(lanes):
        sample = 0
        st = Stream(seed, sample, lane, stream_id)
        for s in range(steps):
            op = int(script[lane, s])
            if op == 1:
                out[lane, s, 0] = (st.u32() >> 8) << 8
            elif op in (2, 3):
                out[lane, s, :op] = [st.u32() for _ in range(op)]
            elif op == 4:
                sample += 1
                st = Stream(seed, sample, lane, stream_id)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# transform chains
# ---------------------------------------------------------------------------------------------------------------------
ANGLES = (15.0, -18.0, 0.0, 90.0, 180.0, 33.0)


def chain_specs(seed=99):
    """(name, wraps, scale): wraps innermost first, as geom_corpus.make applies them — ('T', offset) or ('R', axis, angle)"""
    rng = np.random.default_rng(seed)
    specs = [("cornell_box/box1", [("R", 1, -18.0), ("T", (130.0, 0.0, 65.0))], 555.0),
             ("cornell_box/box2", [("R", 1, 15.0), ("T", (265.0, 0.0, 295.0))], 555.0)]
    for scale in (1.0, 555.0, 1e4):
        for length in (1, 2, 3, 4, 15):
            for rep in range(3):
                wraps = []
                for n in range(length):
                    if (n + rep) % 2 == 0:
                        wraps.append(("R", int(rng.integers(0, 3)), float(ANGLES[int(rng.integers(0, len(ANGLES)))])))
                    else:
                        wraps.append(("T", tuple(f32(x) for x in rng.uniform(-scale, scale, 3))))
                specs.append(("len%d/%g/%d" % (length, scale, rep), wraps, scale))
    return specs


def chain_rows(specs, per=48, seed=5):
    """rows [n, 10] float32: world origin, direction, t, unit normal; the spec index of each"""
    rng = np.random.default_rng(seed)
    rows, idx = [], []
    for s, (_, _, scale) in enumerate(specs):
        for _ in range(per):
            o = rng.uniform(-scale, scale, 3)
            d = rng.normal(0.0, 1.0, 3)
            d *= rng.uniform(0.5, 2.0) / np.linalg.norm(d)
            n = rng.normal(0.0, 1.0, 3)
            n /= np.linalg.norm(n)
            rows.append(list(o) + list(d) + [rng.uniform(0.001, 2.0) * scale] + list(n))
            idx.append(s)
    return np.array(rows, np.float32), np.array(idx)


def chain_exact(xforms, row):
    """the round trip of include/rtmi.h's XFORM_ROUNDTRIP in real arithmetic over the lowered records (kind, x, y, z), outermost
    first: (p, n, o + t d, the sum of the magnitudes each step handled for p, and for n)"""
    AX = {1: (1, 2), 2: (2, 0), 3: (0, 1)}  # RTMI_XF_ROTATE_X / Y / Z: the (a, b) components
    v = [Fr(float(x)) for x in row]
    o, d, t, n = v[0:3], v[3:6], v[6], v[7:10]
    straight = [o[i] + t * d[i] for i in range(3)]
    nrm = lambda q: mpmath.sqrt(mpf(sum(c * c for c in q)))  # noqa: E731
    mag_p, mag_n = mpmath.mpf(0), mpmath.mpf(0)
    for kind, x, y, z in xforms:
        if kind == 0:
            off = [Fr(x), Fr(y), Fr(z)]
            mag_p += nrm(o) + nrm(off)
            o = [o[i] - off[i] for i in range(3)]
        else:
            a, b = AX[kind]
            s, c = Fr(x), Fr(y)
            mag_p += nrm(o) + abs(mpf(t)) * nrm(d)
            o[a], o[b] = c * o[a] + s * o[b], -s * o[a] + c * o[b]
            d[a], d[b] = c * d[a] + s * d[b], -s * d[a] + c * d[b]
    mag_p += nrm(o) + abs(mpf(t)) * nrm(d)
    p = [o[i] + t * d[i] for i in range(3)]
    for kind, x, y, z in reversed(xforms):
        if kind == 0:
            off = [Fr(x), Fr(y), Fr(z)]
            mag_p += nrm(p) + nrm(off)
            p = [p[i] + off[i] for i in range(3)]
        else:
            a, b = AX[kind]
            s, c = Fr(x), Fr(y)
            mag_p += nrm(p)
            mag_n += nrm(n)
            p[a], p[b] = c * p[a] - s * p[b], s * p[a] + c * p[b]
            n[a], n[b] = c * n[a] - s * n[b], s * n[a] + c * n[b]
    return p, n, straight, mag_p, mag_n


# ---------------------------------------------------------------------------------------------------------------------
# one bounce: world.hit, then Material::scatter (rtmi_probe_path's BOUNCE, the oracle's orc_bounce)
# ---------------------------------------------------------------------------------------------------------------------
BOUNCE_MAX_DEPTH = 50
BOUNCE_SPACING = 10.0
DIRECTION_SCALES = (-70, -64, -60, 0, 60, 63, 64, 66)  # rd scaled by 2^k; d.d is a normal fp32 number for -60 .. 63
# name -> (kind, parameter): XY plates [cx - 2, cx + 2] x [-2, 2] at z = 0 and unit spheres, centres BOUNCE_SPACING apart along x
BOUNCE_OBJECTS = [
    ("lambert", "plate"), ("metal0", "plate"), ("metal0.3", "plate"), ("metal1", "plate"), ("metal5", "plate"),
    ("glass1.5", "plate"), ("glass2.4", "plate"), ("glass1.0", "plate"), ("glass1/1.5", "plate"), ("light", "plate"),
    ("checker", "plate"), ("noise", "plate"), ("fog", "medium"), ("lambert_moved", "moved"), ("lambert_flipped", "flipped"),
    ("lambert_ball", "sphere"), ("metal0.3_ball", "sphere"), ("glass1.5_ball", "sphere"),
]
GLASS = {"glass1.5": 1.5, "glass2.4": 2.4, "glass1.0": 1.0, "glass1/1.5": 1.0 / 1.5}
METAL = {"metal0": 0.0, "metal0.3": 0.3, "metal1": 1.0, "metal5": 5.0}
LAMBERT_RGB, LIGHT_RGB, FOG_RGB = (0.5, 0.625, 0.75), (4.0, 3.0, 2.0), (0.25, 0.5, 0.75)


def bounce_world(api):
    """the hand-built world through any backend (Host, Oracle): a plain HittableList, one material per object"""
    api.seed_scene_rng(7)
    world = api.HittableList()
    solid = api.SolidTexture(*LAMBERT_RGB)
    for n, (name, shape) in enumerate(BOUNCE_OBJECTS):
        cx = n * BOUNCE_SPACING
        base = name.split("_")[0]
        if base in METAL:
            mat = api.Metal(solid, METAL[base])
        elif base in GLASS:
            mat = api.Dielectric(GLASS[base])
        elif base == "light":
            mat = api.DiffuseLight(api.SolidTexture(*LIGHT_RGB))
        elif base == "checker":
            mat = api.Lambertian(api.CheckerTexture(api.SolidTexture(0.25, 0.25, 0.25), api.SolidTexture(0.75, 0.75, 0.75)))
        elif base == "noise":
            mat = api.Lambertian(api.NoiseTexture(4.0))
        else:
            mat = api.Lambertian(solid)
        if shape == "plate":
            world.push(api.Rect(api.PLANE_XY, cx - 2.0, -2.0, cx + 2.0, 2.0, plate_z(name), mat))
        elif shape == "flipped":
            world.push(api.FlipNormals(api.Rect(api.PLANE_XY, cx - 2.0, -2.0, cx + 2.0, 2.0, 0.0, mat)))
        elif shape == "moved":  # the plate at the origin, turned by 15 degrees about y, then moved to its place
            world.push(api.Traslate(api.Rotate(api.AXIS_Y, api.Rect(api.PLANE_XY, -2.0, -2.0, 2.0, 2.0, 0.0, mat), 15.0), (cx, 0.0, 0.0)))
        elif shape == "sphere":
            world.push(api.Sphere((cx, 0.0, 0.0), 1.0, mat))
        else:
            world.push(api.ConstantMedium(api.Sphere((cx, 0.0, 0.0), 2.0, api.Lambertian(solid)), 0.5, api.SolidTexture(*FOG_RGB)))
    return world


def plate_z(name):
    """the plane of an object's plate: z = 0, but each glass plate in a plane of its own, so that a ray lying IN the plane
    of one (the `ddn` = 0 class) is parallel to every other rect of the world and in the plane of none"""
    return {"glass1.5": 0.25, "glass2.4": 0.5, "glass1.0": 0.75, "glass1/1.5": 1.0}.get(name, 0.0)


SCHLICK_DELTAS = (-400, -80, -40, -1, 0, 1, 2, 40, 80, 400)  # word-ulps about schlick; the choice's band is 36 wide


def bounce_cases(seed=606):
    """(rows [n, 10] float32 = origin, direction, time, t_min, t_max, depth; words [n, WORDS]; class; object index; k of 2^k)"""
    rng = np.random.default_rng(seed)
    rows, words, cls, obj, scale = [], [], [], [], []

    def add(name, n, o, d, ks, depth=0, k2=0, t_max=float("inf")):
        d = [f32(c) * 2.0 ** k2 for c in d]
        rows.append([f32(c) for c in o] + d + [0.0, 0.001 * 2.0 ** -k2, t_max, depth])
        words.append(script(ks, rng))
        cls.append(name)
        obj.append(n)
        scale.append(k2)

    def rnd_words():
        return [int(x) for x in rng.integers(0, 1 << 24, 27)]

    for n, (name, shape) in enumerate(BOUNCE_OBJECTS):
        cx = n * BOUNCE_SPACING
        pz = plate_z(name)
        for rep in range(24):  # either side of the object, aimed at a random point of it
            side = 1.0 if rep % 2 == 0 else -1.0
            o = (cx + rng.uniform(-3.0, 3.0), rng.uniform(-3.0, 3.0), pz + side * rng.uniform(4.0, 6.0))
            target = (cx + rng.uniform(-0.6, 0.6), rng.uniform(-0.6, 0.6), pz)
            stretch = rng.uniform(0.2, 3.0)
            add("plain", n, o, [(target[a] - o[a]) * stretch for a in range(3)], rnd_words())
        add("depth_limit", n, (cx, 0.0, 5.0), (0.01, 0.02, -1.0), rnd_words(), depth=BOUNCE_MAX_DEPTH)
        add("miss", n, (cx, 0.0, 5.0), (0.0, 0.0, 1.0), rnd_words())
        add("short_interval", n, (cx, 0.0, 5.0), (0.0, 0.0, -1.0), rnd_words(), t_max=2.0)
        base = name.split("_")[0]
        if base == "lambert" and shape == "plate":  # rs within a few lattice steps of -hn: hn + rs = (0, 0, k 2^-23) exactly
            for k in (1, 2, 3, 5):
                add("lambert_cancel", n, (cx, 0.0, 5.0), (0.0, 0.0, -1.0), [ORIGIN_K, ORIGIN_K, k])
        if shape == "plate" and (base in METAL or base in GLASS):
            for h in (1e-3, 1e-5, 1e-7):  # grazing incidence on either side of the plate; fuzz vectors that tip refl . n
                for side in (1.0, -1.0):
                    for kz in (ORIGIN_K, ORIGIN_K + (1 << 22), ORIGIN_K - (1 << 22)):
                        add("graze", n, (cx - 1.0, 0.0, f32(pz + side * h)), (1.0, 0.0, -side * h), [ORIGIN_K, ORIGIN_K, kz])
            for rep in range(8):  # the direction-magnitude class: the same rays under eight scales
                o = (cx + rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0), (1.0 if rep % 2 == 0 else -1.0) * 5.0)
                d = (rng.uniform(-0.15, 0.15), rng.uniform(-0.15, 0.15), -o[2] / 5.0 * rng.uniform(0.7, 1.3))
                ks = rnd_words()
                for k2 in DIRECTION_SCALES:
                    add("scaled", n, o, d, ks, k2=k2)
        if base in GLASS and shape == "plate":
            # aimed at the choice `u >= schlick`: the word SCHLICK_DELTAS word-ulps from the exact reflect probability of the
            # ray (real arithmetic on the fp32 inputs): clear of the band on either side, and on the edge
            for rep in range(12):
                land = (cx + rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0), pz)  # steep to grazing, always onto the plate
                o = [f32(c) for c in (land[0] + rng.uniform(-3.0, 3.0), land[1] + rng.uniform(-3.0, 3.0), pz + rng.uniform(0.1, 5.0))]
                stretch = rng.uniform(0.3, 3.0)
                d = [f32((land[a] - o[a]) * stretch) for a in range(3)]
                cosine = -mpf(Fr(d[2])) / mpmath.sqrt(mpf(sum(Fr(c) * Fr(c) for c in d)))
                ref = mpf(Fr(f32(GLASS[base])))
                r0 = ((1 - ref) / (1 + ref)) ** 2
                k0 = int(mpmath.floor((r0 + (1 - r0) * (1 - cosine) ** 5) * (1 << 24)))
                for delta in SCHLICK_DELTAS:
                    add("schlick", n, o, d, [min(max(k0 + delta, 0), TOP_K)])
            # normal incidence: every fp32 intermediate is exact (cosine = 1, x = 0), so schlick is r0 exactly; for ref_idx 1
            # that is 0 and the word 0 EQUALS it: `>=` refracts.  The word 1 for comparison.
            for k in (0, 1):
                add("schlick_equal", n, (cx, 0.0, 5.0), (0.0, 0.0, -2.0), [k])
            # ddn exactly 0: a ray lying in the plate's plane with d_z = +-0 is accepted by Rect::hit with t = NaN
            # (include/rtmi_query.h, "In-plane rays"); dot(rd, hn) is +-0, not > 0: the entering branch, cosine 0, schlick 1
            for dz in (0.0, -0.0):
                for k in (0, ORIGIN_K, TOP_K):
                    add("ddn_zero", n, (cx + 1.0, 0.0, pz), (-1.0, 0.0, dz), [k])
            for rep in range(24):  # leaving the glass steeply and flatly: total internal reflection on both sides
                ang = rng.uniform(0.05, 1.5)
                add("glass_leaving", n, (cx - 2.0 * math.sin(ang), 0.0, pz - 2.0 * math.cos(ang)), (math.sin(ang), 0.0, math.cos(ang)), rnd_words())
    return np.array(rows, np.float32), np.array(words, np.uint32), cls, np.array(obj), np.array(scale)
