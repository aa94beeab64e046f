"""The numpy restatement of windowed adaptive sampling (tests/window_ref.py) on the fp32 oracle's samples and on crafted
planes: no GPU.

The samples are the oracle's render_samples (ARITH_DEVICE | THROUGHPUT_FORM, seed 0) of the two plain inputs of
window_ref.PLAIN_INPUTS; the tolerance is computed from them as stated there.  Recorded on the CPU, not asserted: lit_smoke
16x16 traces 4892 / 6924 / 7940 samples for r = 0 / 1 / 2 against 9216 for the fixed render, cornell_box 13x13 15424 / 21760 /
23904 against 24336."""
import numpy as np
import pytest

import pixelwise_ref
import scenes_extra
import window_ref as ref
from oracle.oracle import ARITH_DEVICE, THROUGHPUT_FORM
from raytracing_rust_amd import scenes

RADII = (0, 1, 2, 3)


@pytest.fixture(scope="module", params=sorted(ref.PLAIN_INPUTS))
def case(request, orc32):
    name, nx, ny, (lo, step, cap), factor = ref.PLAIN_INPUTS[request.param]
    _, world = scenes_extra.build(orc32, name, nx, ny, seed=1)
    cam = scenes.set_camera(orc32, nx, ny, ref.VIEW[0], ref.VIEW[1], vertical_fov=ref.VIEW[2])
    x = orc32.render_samples(cam, world, nx, ny, cap, seed=0, flags=ARITH_DEVICE | THROUGHPUT_FORM)["samples"].reshape(nx * ny, cap, 3)
    orc32.free_all()
    x.setflags(write=False)
    tol = ref.tolerance(x, lo, factor)
    outs = {r: ref.render(x, nx, ny, lo, step, abs_tol=tol, r=r) for r in RADII + (15,)}
    print("%s: abs_tol %.6g, samples %r of %d" % (request.param, tol, {r: int(o["spp"].sum()) for r, o in outs.items()}, nx * ny * cap))
    return dict(x=x, nx=nx, ny=ny, lo=lo, step=step, cap=cap, tol=tol, outs=outs)


def test_radius_0_is_the_per_pixel_restatement(case):
    want = pixelwise_ref.render(case["x"], case["lo"], case["step"], abs_tol=case["tol"])
    for k, v in want.items():
        assert case["outs"][0][k].tobytes() == v.tobytes(), k


def test_the_inputs_say_something(case):
    assert case["tol"] > 0.0
    for r in (0, 1, 2):
        spp = case["outs"][r]["spp"]
        assert len(np.unique(spp)) >= 3 and (spp == case["lo"]).any() and (spp == case["cap"]).any(), (r, np.unique(spp))


def test_monotone_in_the_radius(case):
    for small, large in zip(RADII, RADII[1:]):
        a, b = case["outs"][small]["spp"], case["outs"][large]["spp"]
        assert (b >= a).all(), (small, large)
        if large <= 2:
            assert (b > a).any(), (small, large)
        print("r %d -> %d: %d pixels rise" % (small, large, int((b > a).sum())))
    assert (case["outs"][15]["spp"] >= case["outs"][3]["spp"]).all()


def test_the_global_rule(case):
    """r = 15 >= max(nx, ny) - 1: every pixel stops at the first count at which all pass, or at the cap."""
    out = case["outs"][15]
    lat = pixelwise_ref.lattice(case["cap"], case["lo"], case["step"])
    state = tuple(np.zeros((case["nx"] * case["ny"], 3)) for _ in range(3))
    x = case["x"].astype(np.float64)
    stop, done = case["cap"], 0
    for n in lat:
        for s in range(done, n):
            pixelwise_ref.fold(state, x[:, s], s + 1)
        done = n
        if pixelwise_ref.decide(state, n, case["tol"], 0.0)[2].all():
            stop = n
            break
    assert (out["spp"] == stop).all()
    n_px = case["nx"] * case["ny"]
    assert out["counts"][:, 0].tolist() == [n_px if n <= stop else 0 for n in lat]


def test_a_retired_pixel_is_never_traced_again_and_the_counts_sum(case):
    lat = pixelwise_ref.lattice(case["cap"], case["lo"], case["step"])
    per_step = np.diff([0] + lat)
    for r, out in case["outs"].items():
        c = out["counts"][:, 0].astype(np.int64)
        assert (np.diff(c) <= 0).all() and c[0] == case["nx"] * case["ny"], r  # the live set only shrinks
        assert (out["counts"][:, 0] == out["counts"][:, 1]).all()
        assert int((c * per_step).sum()) == int(out["spp"].sum()), r
        assert set(out["spp"].tolist()) <= set(lat)
        # traced at step k <=> spp >= lattice[k]: a pixel's steps are a prefix of the lattice
        assert [int((out["spp"] >= n).sum()) for n in lat] == c.tolist(), r
        fixed = ref.render(case["x"][:, :lat[1]], case["nx"], case["ny"], lat[1], 1, r=r)  # every pixel at one later count
        at = out["spp"] == lat[1]
        for k in ("linear", "stderr", "rgb8"):
            assert out[k][at].tobytes() == fixed[k][at].tobytes(), (r, k)


# ---- spread on crafted planes ---------------------------------------------------------------------------------------------------
def _brute(active, fail, nx, ny, r):
    a, f = np.asarray(active).reshape(ny, nx), np.asarray(fail).reshape(ny, nx)
    out = np.zeros((ny, nx), np.uint8)
    for y in range(ny):
        for x in range(nx):
            out[y, x] = a[y, x] != 0 and f[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1].any()
    return out.reshape(-1)


def test_spread_of_a_single_fail():
    nx, ny = 9, 7
    ones = np.ones(nx * ny, np.uint8)
    for (x, y) in ((0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1), (4, 0), (0, 3), (nx - 1, 3), (4, ny - 1), (4, 3)):
        f = np.zeros((ny, nx), np.uint8)
        f[y, x] = 1
        for r in (0, 1, 2, 3):
            got = ref.spread(ones, f, nx, ny, r).reshape(ny, nx)
            yy, xx = np.mgrid[:ny, :nx]
            want = (np.abs(yy - y) <= r) & (np.abs(xx - x) <= r)
            assert (got == want).all(), (x, y, r)
            assert got.sum() == (min(x + r, nx - 1) - max(x - r, 0) + 1) * (min(y + r, ny - 1) - max(y - r, 0) + 1)


def test_spread_does_not_wrap_between_rows():
    nx, ny = 6, 4
    ones = np.ones(nx * ny, np.uint8)
    f = np.zeros((ny, nx), np.uint8)
    f[1, nx - 1] = 1  # the last pixel of row 1: pixel (0, 2) follows it in memory
    got = ref.spread(ones, f, nx, ny, 1).reshape(ny, nx)
    assert got[:, 0].sum() == 0 and got[0:3, nx - 2:].all() and got.sum() == 6
    f[:] = 0
    f[2, 0] = 1  # the first pixel of row 2: pixel (nx - 1, 1) precedes it in memory
    got = ref.spread(ones, f, nx, ny, 1).reshape(ny, nx)
    assert got[:, nx - 1].sum() == 0 and got[1:4, 0:2].all() and got.sum() == 6


def test_spread_on_thin_images_large_radii_and_any_bytes():
    rng = np.random.default_rng(0)
    for nx, ny in ((1, 1), (1, 9), (9, 1), (5, 3), (8, 8)):
        for r in (0, 1, 2, 8, 16):  # 8 and 16 exceed every one of these images
            f = (rng.random(nx * ny) < 0.2) * rng.integers(1, 256, nx * ny)
            a = (rng.random(nx * ny) < 0.7) * rng.integers(1, 256, nx * ny)
            got = ref.spread(a.astype(np.uint8), f.astype(np.uint8), nx, ny, r)
            assert got.dtype == np.uint8 and set(got.tolist()) <= {0, 1}
            assert (got == _brute(a, f, nx, ny, r)).all(), (nx, ny, r)
            if r >= max(nx, ny) - 1:
                assert (got == ((a != 0) & f.any())).all()
            if r == 0:
                assert (got == ((a != 0) & (f != 0))).all()
    assert not ref.spread(np.ones(12, np.uint8), np.zeros(12, np.uint8), 4, 3, 2).any()
    assert not ref.spread(np.zeros(12, np.uint8), np.ones(12, np.uint8), 4, 3, 2).any()
