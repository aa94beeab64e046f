"""Texture evaluation on the device (csrc/rtmi_shade.hpp as_usize_u32, as_image_index, perlin_noise, perlin_turb,
perlin_turb7_wave, tex_value_wave; csrc/rtmi_f64_kernels.hpp tex_value_d, perlin_noise_d) through the public entries.

A textured DiffuseLight shows a texture value bit for bit: the first hit of a PLAIN radiance query (spp = 1, samples) is
emitted = tex_value(u, v, p), rtmi_trace of the same ray returns the (u, v, p) and the material the kernel used, and an
ns = 1 render gives the same value per pixel.  The scenes are XY plates at different z, one texture each (tests/tex_corpus.py);
a ray along z with its first segment's interval closed around the plate places p exactly.

 1. the corpus on the per-lane radiance kernel: every sample equals the fp32 oracle's tex_value at the traced (u, v, p)
    bit for bit, and satisfies the bands and bounds of tests/test_tex_contract.py against the exact reference;
 2. independence of the other lanes: a batch of at most 64 items at spp = 1 is one chunk (batch_chunks: at least 64 items
    a chunk) and so one wavefront; all 64 lanes take their item in one batch_take, every ray hits its plate in the first
    scan, so 64 lanes >= shade_threshold hold a hit and phase B shades them together (csrc/rtmi_radiance.hip, the body of
    rtmi_kernel_perlane.inc with the batch take): __ballot(noise) in tex_value_wave counts exactly the noise rays of the
    batch.  1, 10 (the cooperative turbulence), 11 and 64 (every lane its own) are reached; a batch of 1; and in a batch
    of 65 the last ray is alone in the second chunk;
 3. both again on the cooperative batch kernel, which test_gpu_batch_coop._kernel shows to have run;
 4. whole 20 x 12 images (partial tiles), ns = 1: features albedo, render on the default kernel and under RTMI_FLAG_SYNC
    against the oracle at the hit record; the f64 mode against the exact reference at the bound for doubles, and against
    orc64 bit for bit (its sine is the correctly rounded one, csrc/rtmi_sin_f64.hpp, and so is glibc's on this plate).

Measured on the MI355X: no sample differs from the fp32 oracle (3290 axis-aligned and 1098 oblique rays, both kernels); the
device's maxima against the exact reference are the contract's own (value error at most 0.095 of its bound, 13.8 u).  On the
parent commit's kernels 81 noise cases differed, all of them with a y or z whose octaves reach 2^64 (as_usize_u32 returned
0 there; the point (0.3, 2e20, 0.7) gave 0.333 where the oracle has 0.8832566)."""
import collections
import math

import mpmath
import numpy as np
import pytest

import tex_corpus as tc
import test_gpu_batch_coop as bc
import test_tex_contract as cpu
from oracle.oracle import ARITH_DEVICE, THROUGHPUT_FORM
from raytracing_rust_amd import abi
from raytracing_rust_amd.philox import Stream
from test_gpu_features import _primary_rays

f32 = np.float32
FC = abi.RTMI_FLAG_FAST_CULL
SEED = 42
INF = f32(np.inf)


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _plates_world(api, trees, plates):
    world = api.HittableList()
    for tex, z in plates:
        x0, y0, x1, y1 = tc.plate_of(tex)
        world.push(api.Rect(api.PLANE_XY, x0, y0, x1, y1, z, api.DiffuseLight(trees[tex][0])))
    return world


def axis_rays(xyz, oblique=None):
    """rays along z that meet the plate z = xyz[:, 2] at exactly (x, y): origin (x, y, 0) (a plate at z = 0: from -2^-20),
    direction (+-0, +-0, +-1) with the zeros signed like x and y (-0 + t * -0 stays -0), the first segment closed on the
    two neighbours of t = |z|.  oblique [n, 2]: the direction's x and y; the origin is moved back so that p lands near."""
    xyz = np.asarray(xyz, f32)
    n = len(xyz)
    z = xyz[:, 2]
    o, d = np.zeros((n, 3), f32), np.zeros((n, 3), f32)
    at0 = z == 0
    o[:, 2] = np.where(at0, f32(-2.0 ** -20), f32(0))
    t = np.where(at0, f32(2.0 ** -20), np.abs(z)).astype(f32)
    d[:, 2] = np.where(z < 0, f32(-1), f32(1))
    if oblique is None:
        o[:, 0:2] = xyz[:, 0:2]
        d[:, 0:2] = np.where((xyz[:, 0:2] == 0) & np.signbit(xyz[:, 0:2]), f32(-0.0), f32(0.0))
    else:
        d[:, 0:2] = oblique
        o[:, 0:2] = xyz[:, 0:2] - t[:, None] * d[:, 0:2]
    return o, d, np.nextafter(t, f32(0)), np.nextafter(t, INF)


class _Family:
    """one family's scene on the device, its rays traced once, and the fp32 oracle's value at every traced record"""

    def __init__(self, host, orc32, fam, oblique):
        C = cpu.corpus()
        self.C, self.fam = C, fam
        self.idx = np.flatnonzero(C.family == fam)
        self.trees = tc.build(orc32, "f32")
        plates = C.plates(fam)
        self.sc = host.lower(_plates_world(host, tc.build(host, "f64"), plates)).upload(0)
        xyz = C.xyz[self.idx]
        if oblique:
            rng = np.random.default_rng(7)
            self.idx = self.idx[::3]
            xyz = C.xyz[self.idx]
            self.rays = axis_rays(xyz, rng.uniform(-0.5, 0.5, (len(xyz), 2)).astype(f32))
        else:
            self.rays = axis_rays(xyz)
        o, d, t0, t1 = self.rays
        assert len(o) <= 4096
        self.tr = self.sc.trace(o, d, t_min=t0, t_max=t1, flags=FC)
        tr = self.tr
        self.hit = tr["hit"]
        if oblique:
            assert self.hit.mean() >= (0.5 if fam == "image" else 1.0), (fam, self.hit.mean())  # small plates can be missed
        else:
            assert self.hit.all(), (fam, np.flatnonzero(~self.hit)[:8])
            assert np.array_equal(_bits(tr["p"]), _bits(xyz)), fam  # p is placed exactly, signed zeros included
        assert np.array_equal(_bits(tr["p"][self.hit, 2]), _bits(xyz[self.hit, 2]))
        # one material per plate: the texture the kernel used is the plate's
        by_plate = collections.defaultdict(set)
        for n in np.flatnonzero(self.hit):
            by_plate[(C.tex[self.idx[n]], float(xyz[n, 2]))].add(int(tr["material"][n]))
        assert all(len(m) == 1 for m in by_plate.values()) and len({next(iter(m)) for m in by_plate.values()}) == len(by_plate)
        assert oblique or len(by_plate) == len(plates)
        self.want = np.zeros((len(o), 3), f32)
        for n in np.flatnonzero(self.hit):
            w = orc32.tex_value(self.trees[C.tex[self.idx[n]]][0], float(tr["u"][n]), float(tr["v"][n]), tr["p"][n].astype(np.float64),
                                flags=ARITH_DEVICE)
            self.want[n] = (0.0 + w).astype(f32)

    def radiance(self, **kw):
        o, d, t0, t1 = self.rays
        return self.sc.radiance(o, d, t_min=t0, t_max=t1, spp=1, estimator="plain", seed=SEED, samples=True, **kw)

    def check(self, got, label):
        C, hit = self.C, self.hit
        bad = np.flatnonzero(np.any(_bits(got[:, 0]) != _bits(self.want), axis=1) & hit)
        # what the device gave where it parts from the oracle, class by class (printed before the assertion)
        parts = collections.Counter(str(C.cls[self.idx[n]]) for n in bad)
        print("%s %s: %d rays, %d hit, %d differ from the fp32 oracle %s" % (label, self.fam, len(hit), int(hit.sum()), len(bad), dict(parts)))
        first = {}
        for n in bad:
            first.setdefault(str(C.cls[self.idx[n]]), n)
        for n in first.values():  # one example of every class
            print("   case %d %s %s p=%s device %s oracle %s" % (self.idx[n], C.tex[self.idx[n]], C.cls[self.idx[n]], self.tr["p"][n],
                                                                got[n, 0], self.want[n]))
        assert len(bad) == 0, (label, self.fam, len(bad), dict(parts))
        assert not np.any(got[~hit])
        at = np.flatnonzero(hit)
        uvp = [(self.tr["u"][n], self.tr["v"][n], self.tr["p"][n]) for n in at]
        st, mx, broken = cpu.check(C, self.idx[at], uvp, got[at, 0], self.trees, "f32", "%s %s, device" % (label, self.fam))
        assert not broken, broken[:10]
        return st


_FAMILIES = {}


def _family(host, orc32, fam, oblique=False):
    """the traced family, shared by the tests of this module (the scene is uploaded again if the host released it)"""
    key = (fam, oblique)
    if key not in _FAMILIES:
        _FAMILIES[key] = _Family(host, orc32, fam, oblique)
    else:
        f = _FAMILIES[key]
        f.trees = tc.build(orc32, "f32")
        f.sc = host.lower(_plates_world(host, tc.build(host, "f64"), f.C.plates(fam))).upload(0)
    return _FAMILIES[key]


# ---- 1. the corpus, per-lane kernel ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["noise", "checker", "image"])
def test_perlane_radiance_equals_oracle_and_reference(host, orc32, fam):
    F = _family(host, orc32, fam)
    C = F.C
    for n, i in enumerate(F.idx):  # no class is vacuous: the record the kernel used has the class's property
        assert tc.has_property(C.cls[i], C.aux[i], C.tex[i], F.tr["u"][n], F.tr["v"][n], F.tr["p"][n]), (i, C.cls[i], F.tr["p"][n])
    got = F.radiance(flags=FC)["samples"]
    st = F.check(got, "per-lane, axis-aligned")
    if fam == "noise":
        assert st["rule"] >= 100 and st["noise"] >= 1200, st
    got0 = F.radiance(flags=0)["samples"]  # the reference-topology traversal shades with the same code
    assert np.array_equal(_bits(got0), _bits(got))


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["noise", "checker", "image"])
def test_oblique_rays_on_both_kernels(host, orc32, fam):
    F = _family(host, orc32, fam, oblique=True)
    moved = np.any(_bits(F.tr["p"][F.hit, 0:2]) != _bits(F.C.xyz[F.idx][F.hit, 0:2]), axis=1)
    assert moved.sum() >= 30  # p = o + t d rounds: these are other points than the corpus's own
    got = F.radiance(flags=FC)["samples"]
    F.check(got, "per-lane, oblique")
    assert bc._kernel(lambda **kw: F.radiance(**kw)) == bc.COOP
    coop = F.radiance(flags=FC, coop=True)["samples"]
    F.check(coop, "cooperative, oblique")


# ---- 2. / 3. independence of the batch ------------------------------------------------------------------------------------------
def _pick(C, tex, cls, k, skip=0):
    at = np.flatnonzero((C.tex == tex) & (C.cls == cls))[skip:skip + k]
    assert len(at) == k, (tex, cls, k)
    return at


@pytest.mark.gpu
@pytest.mark.parametrize("coop", [False, True])
def test_noise_value_does_not_depend_on_the_batch(host, orc32, coop):
    C = cpu.corpus()
    F = _family(host, orc32, "noise")
    sc = F.sc
    row = {int(i): n for n, i in enumerate(F.idx)}
    bases = [int(_pick(C, "NA", "interior", 1)[0]), int(_pick(C, "NA", "beyond_2p64", 1)[0]), int(_pick(C, "NA", "negative_tiny", 1)[0]),
             int(_pick(C, "NA", "sin_limit", 1, skip=40)[0])]
    noise = list(_pick(C, "NA", "interior", 64, skip=1))
    solid = list(_pick(C, "S0", "beside", 32)) + list(_pick(C, "S1", "beside", 32))
    second = list(_pick(C, "NB", "interior", 64))
    checker = list(_pick(C, "CKN", "beside", 64))

    def run(cases):
        o, d, t0, t1 = axis_rays(C.xyz[cases])
        call = lambda **kw: sc.radiance(o, d, t_min=t0, t_max=t1, spp=1, estimator="plain", seed=SEED, samples=True, **kw)  # noqa: E731
        if coop:
            assert bc._kernel(call) == bc.COOP
        return call(flags=FC, coop=coop)["samples"][:, 0]

    for base in bases:
        want = F.want[row[base]]
        batches = {"alone": [base], "last of 65": noise[:64] + [base]}
        for k in (0, 9, 10, 63):  # 1, 10, 11 and 64 noise lanes of the wavefront
            front = solid[:min(5, 63 - k)]
            batches["%d other noise rays" % k] = front + [base] + noise[:k] + solid[len(front):63 - k]
        batches["among the second table"] = second[:20] + [base] + second[20:63]
        batches["among checker-over-noise"] = checker[:40] + [base] + checker[40:63]
        batches["3 noise rays of three tables"] = solid[:30] + [base] + second[:1] + checker[:1] + solid[30:61]
        for label, cases in batches.items():
            assert len(cases) in (1, 64, 65), (label, len(cases))
            got = run(cases)
            at = cases.index(base)
            assert np.array_equal(_bits(got[at]), _bits(want)), (C.cls[base], label, got[at], want)
            others = np.array([F.want[row[int(i)]] for i in cases])
            assert np.array_equal(_bits(got), _bits(others)), (C.cls[base], label)  # and nobody else's changed either


# ---- 4. whole images ------------------------------------------------------------------------------------------------------------
NX, NY = 20, 12


def _image_scene(api, trees, noise_left):
    """in front (z = 0) a noise plate over the columns up to the middle of column 8 (counted from the noise side); behind it
    a 16-deep checker over image and solids on the lower half (z = 0.9) and an image (z = 1) over the rest"""
    world = api.HittableList()
    x0, x1 = (-tc.BIG, -0.45) if noise_left else (0.45, tc.BIG)
    world.push(api.Rect(api.PLANE_XY, x0, -tc.BIG, x1, tc.BIG, 0.0, api.DiffuseLight(trees["NA"][0])))
    world.push(api.Rect(api.PLANE_XY, -8.0, -6.0, 8.0, 0.0, 0.9, api.DiffuseLight(trees["CK16E"][0])))
    world.push(api.Rect(api.PLANE_XY, -8.0, -6.0, 8.0, 6.0, 1.0, api.DiffuseLight(trees["i16x8"][0])))
    cam = api.Camera((0.0, 0.0, -10.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 27.0, NX / NY, 0.0, 10.0, 0.0, 1.0)
    return cam, world


@pytest.mark.gpu
def test_whole_images_equal_the_oracle_at_the_hit_record(host, orc32):
    th, t32 = tc.build(host, "f64"), tc.build(orc32, "f32")
    cam0, _ = _image_scene(host, th, True)
    org, dirs = _primary_rays(cam0.lower(), NX, NY, SEED)
    noise_left = bool(dirs[0, 0, 0] < 0)  # the side of the image's column 0
    cam, world = _image_scene(host, th, noise_left)
    _, oworld = _image_scene(orc32, t32, noise_left)
    sc = host.lower(world).upload(0)
    texs = {0.0: "NA", 0.9: "CK16E", 1.0: "i16x8"}
    want = np.zeros((NY, NX, 3), f32)
    kinds = collections.Counter()
    C = cpu.corpus()
    uvp, trees_of = [], []
    for r in range(NY):
        for i in range(NX):
            h = orc32.hit(oworld, org.astype(np.float64), dirs[r, i].astype(np.float64), flags=ARITH_DEVICE)
            assert h is not None, (r, i)
            tex = texs[round(float(h["p"][2]), 1)]
            kinds[tex] += 1
            w = orc32.tex_value(t32[tex][0], h["u"], h["v"], h["p"], flags=ARITH_DEVICE).astype(f32)
            want[r, i] = ((0.0 + w.astype(np.float64)) / 1.0).astype(f32)
            uvp.append((h["u"], h["v"], h["p"]))
            trees_of.append(tex)
    assert min(kinds.values()) >= 20, kinds
    # the tiles (8 x 8, j = 0 the bottom row) by the traced materials: one with 1..10 noise pixels, one with more
    tr = sc.trace(np.broadcast_to(org, (NX * NY, 3)), dirs[::-1].reshape(-1, 3), flags=FC)
    mat = tr["material"].reshape(NY, NX)
    noise_mat = mat[NY - 1, 0]  # the noise plate is on the side of column 0, over the whole height
    per_tile = [int((mat[j:j + 8, i:i + 8] == noise_mat).sum()) for j in range(0, NY, 8) for i in range(0, NX, 8)]
    print("noise pixels per tile", per_tile, kinds)
    assert int((mat == noise_mat).sum()) == kinds["NA"]
    assert any(1 <= n <= 10 for n in per_tile) and any(n > 10 for n in per_tile), per_tile
    f = sc.render_features(cam, NX, NY, 1, seed=SEED)
    assert (f["hits"] == 1).all()
    for label, got in (("features albedo", f["albedo"]), ("render", sc.render(cam, NX, NY, 1, seed=SEED)["linear"]),
                       ("render, FAST_CULL", sc.render(cam, NX, NY, 1, seed=SEED, flags=FC)["linear"]),
                       ("render, SYNC", sc.render(cam, NX, NY, 1, seed=SEED, flags=abi.RTMI_FLAG_SYNC)["linear"])):
        bad = np.argwhere(np.any(_bits(got) != _bits(want), axis=2))
        assert len(bad) == 0, (label, len(bad), bad[:8].tolist())
    # and the exact reference at those records
    fake = type("Cases", (), {"tex": np.array(trees_of), "cls": np.array(["image_pixel"] * len(trees_of))})
    st, mx, broken = cpu.check(fake, range(len(trees_of)), uvp, want.reshape(-1, 3), t32, "f32", "whole image")
    assert not broken, broken[:10]


B33 = 2.0 ** 33


def _f64_scene(api, trees):
    """a noise plate at z = 2^33 + 10 seen from (2^33 + 0.3, 2^33 + 0.7, 2^33): every coordinate of a hit is in [2^32, 2^34),
    where a double's cell index is no multiple of 256 (an fp32 value's would be) and the 64-bit cast is past 32 bits"""
    world = api.HittableList()
    world.push(api.Rect(api.PLANE_XY, 0.0, 0.0, 4.0 * B33, 4.0 * B33, B33 + 10.0, api.DiffuseLight(trees["NA"][0])))
    cam = api.Camera((B33 + 0.3, B33 + 0.7, B33), (B33 + 0.3, B33 + 0.7, B33 + 10.0), (0.0, 1.0, 0.0), 27.0, NX / NY, 0.0, 10.0, 0.0, 1.0)
    return cam, world


def _f64_records(orc64, ocam, oworld):
    """the hit record of every pixel's one sample, restated as the oracle's render loop draws it (rt_oracle.c: u, v from the
    first two words of stream (seed, 0, j nx + i)), row 0 the top row"""
    out = []
    for r in range(NY):
        for i in range(NX):
            j = NY - 1 - r
            st = Stream(SEED, 0, j * NX + i)
            wu, wv = st.u32(), st.u32()
            ray = orc64.get_ray(ocam, (i + (wu >> 8) * 2.0 ** -24) / NX, (j + (wv >> 8) * 2.0 ** -24) / NY)
            h = orc64.hit(oworld, ray[0:3], ray[3:6])
            assert h is not None and (h["p"] >= 2.0 ** 32).all() and (h["p"] < 2.0 ** 34).all()
            out.append((h["u"], h["v"], h["p"]))
    return out


@pytest.mark.gpu
def test_f64_image_within_the_double_bound_of_the_exact_reference(host, orc64):
    th, t64 = tc.build(host, "f64"), tc.build(orc64, "f64")
    cam, world = _f64_scene(host, th)
    ocam, oworld = _f64_scene(orc64, t64)
    got = host.lower(world).upload(0, f64=True).render(cam, NX, NY, 1, seed=SEED, precision="f64")["linear"]
    assert got.dtype == np.float64
    uvp = _f64_records(orc64, ocam, oworld)
    ref = orc64.render(ocam, oworld, NX, NY, 1, seed=SEED, flags=THROUGHPUT_FORM)["mean"].reshape(-1, 3)
    for n, (u, v, p) in enumerate(uvp):  # the records are the oracle render's own
        assert np.array_equal(orc64.tex_value(t64["NA"][0], u, v, p), ref[n]), n
    cells = {(int(p[0]) & 255, int(p[1]) & 255) for _, _, p in uvp}
    assert len(cells) >= 20 and any(c[0] != 0 for c in cells), cells
    fake = type("Cases", (), {"tex": np.array(["NA"] * len(uvp)), "cls": np.array(["f64_pixel"] * len(uvp))})
    st, mx, broken = cpu.check(fake, range(len(uvp)), uvp, got.reshape(-1, 3), t64, "f64", "f64 image, device")
    assert not broken, broken[:10]
    assert st["noise"] == NX * NY


def _noise_d(rv, pm, p):
    """Perlin::noise (perlin.rs:76-97) in doubles, operation by operation as oracle/rt_oracle.c has it"""
    fl = [math.floor(c) for c in p]
    u, v, w = (c - f for c, f in zip(p, fl))
    i, j, k = (int(f) for f in fl)
    uu, vv, ww = u * u * (3.0 - 2.0 * u), v * v * (3.0 - 2.0 * v), w * w * (3.0 - 2.0 * w)
    acc = 0.0
    for di in range(2):
        for dj in range(2):
            for dk in range(2):
                c = rv[pm[0][(i + di) & 255] ^ pm[1][(j + dj) & 255] ^ pm[2][(k + dk) & 255]]
                acc += (di * uu + (1 - di) * (1.0 - uu)) * (dj * vv + (1 - dj) * (1.0 - vv)) * (dk * ww + (1 - dk) * (1.0 - ww)) * \
                    (c[0] * (u - di) + c[1] * (v - dj) + c[2] * (w - dk))
    return acc


def _f64_sine_arguments(orc64, t64, uvp):
    """the double that each record's NoiseTexture::value passes to sin (texture.rs:68), restated in Python floats; checked
    against orc64.tex_value, which is 0.5 (1 + glibc's sine of it)"""
    obj, node = t64["NA"]
    rv, pm = orc64.perlin_tables(obj)
    rv, pm = np.asarray(rv, np.float64).tolist(), np.asarray(pm).astype(int).tolist()
    out = []
    for u, v, p in uvp:
        tp, acc, wgt = [float(c) for c in p], 0.0, 1.0
        for _ in range(7):
            acc += wgt * _noise_d(rv, pm, tp)
            wgt *= 0.5
            tp = [c * 2.0 for c in tp]
        arg = float(node[1]) * float(p[0]) + 5.0 * abs(acc)
        assert 0.5 * (1.0 + math.sin(arg)) == float(orc64.tex_value(obj, u, v, p)[0])
        out.append(arg)
    return out


def _sin_rounded(x):
    with mpmath.workprec(300):
        return float(mpmath.sin(mpmath.mpf(x)))


def test_f64_plate_has_sines_that_glibc_rounds_correctly(orc64):
    """The premise of the bit-for-bit test below, on the CPU.  The reference's f64::sin is the platform's libm; the oracle
    calls glibc's, which is within 0.55 ULP: the correctly rounded double except near a midpoint, 1 argument in 1000
    (tests/test_sin_f64.py).  The device's sine is the correctly rounded one at every argument tested, so the two sides are equal where glibc's is.
    It is at all 240 arguments of this plate (near 3.4e10); were it not, the pixels would be named here.
    This test and the one below therefore depend on the C library of the machine they run on: glibc 2.35 rounds
    these arguments correctly (measured); a libm that rounds one of them the other way fails here, on the CPU, naming the pixel, and
    that failure says nothing about the project's code."""
    t64 = tc.build(orc64, "f64")
    ocam, oworld = _f64_scene(orc64, t64)
    args = _f64_sine_arguments(orc64, t64, _f64_records(orc64, ocam, oworld))
    off = [(divmod(n, NX), x) for n, x in enumerate(args) if math.sin(x) != _sin_rounded(x)]
    print("f64 plate: sine arguments in [%.6g, %.6g], glibc's sine not the rounded one at %d of %d" % (min(args), max(args), len(off), len(args)))
    assert len(args) == NX * NY and min(args) >= 2.0 ** 32 and max(args) < 2.0 ** 40
    assert not off, off


@pytest.mark.gpu
def test_f64_image_equals_orc64_bit_for_bit(host, orc64):
    """The device's value at every pixel is 0.5 (1 + the correctly rounded sine of the oracle's argument): the lattice work is
    + - * and floor, equal on both sides, and csrc/rtmi_sin_f64.hpp rounds the sine once.  That is orc64's value wherever
    glibc's sine is the rounded one, which the test above shows for the whole plate.  With the device library's sine (the
    parent commit) 4 of the 240 pixels were off by 6e-17 in the value, one ULP of the sine (measured on the MI355X)."""
    th, t64 = tc.build(host, "f64"), tc.build(orc64, "f64")
    cam, world = _f64_scene(host, th)
    ocam, oworld = _f64_scene(orc64, t64)
    got = host.lower(world).upload(0, f64=True).render(cam, NX, NY, 1, seed=SEED, precision="f64")["linear"]
    ref = orc64.render(ocam, oworld, NX, NY, 1, seed=SEED, flags=THROUGHPUT_FORM)["mean"]
    uvp = _f64_records(orc64, ocam, oworld)
    args = _f64_sine_arguments(orc64, t64, uvp)
    rounded = np.array([0.5 * (1.0 + _sin_rounded(x)) for x in args]).reshape(NY, NX)
    bad = np.argwhere(got[:, :, 0] != ref[:, :, 0])
    print("f64 image: %d of %d pixels differ from orc64, %d from the rounded sine" % (len(bad), NX * NY, int((got[:, :, 0] != rounded).sum())))
    for r, i in bad:
        ulp = abs(int(np.float64(got[r, i, 0]).view(np.int64)) - int(np.float64(ref[r, i, 0]).view(np.int64)))
        print("   pixel (%d, %d): device %.17g orc64 %.17g, %d ulp apart; rounded sine %.17g, sine's argument %.17g" %
              (r, i, got[r, i, 0], ref[r, i, 0], ulp, rounded[r, i], args[r * NX + i]))
    assert np.array_equal(got[:, :, 0], rounded)
    assert np.array_equal(got, ref), len(bad)
