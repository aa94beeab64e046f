"""Properties of the numpy restatement of include/rtmi_upscale.h (tests/upscale_ref.py), without a GPU: what the
reconstruction promises, checked on the arithmetic the device tests hold the kernel to (tests/test_gpu_upscale.py)."""
import numpy as np
import pytest

import upscale_ref as ref

F = np.float32
EPS = 2.0 ** -24  # half an ulp, relative: the bound of one correctly rounded fp32 operation


def _flat(ny, nx, z=1.0, colour=1.0, albedo=0.5):
    """One image's planes: constant colour, albedo and depth, the normal +z."""
    n = np.zeros((ny, nx, 3), F)
    n[..., 2] = 1.0
    return dict(linear=np.full((ny, nx, 3), colour, F), albedo=np.full((ny, nx, 3), albedo, F), normal=n, depth=np.full((ny, nx), z, F))


def _run(lo, hi, taps=None, **params):
    return ref.upscale(lo["linear"], lo["albedo"], lo["normal"], lo["depth"], hi["albedo"], hi["normal"], hi["depth"], taps=taps,
                       **params)


def _ulps(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_ratio_one_is_the_identity_up_to_the_demodulation():
    rng = np.random.default_rng(1)
    ny, nx = 9, 13
    axes = np.eye(3, dtype=F)
    img = dict(linear=(2.0 ** rng.uniform(-10, 10, (ny, nx, 3))).astype(F), albedo=rng.uniform(0.0, 1.0, (ny, nx, 3)).astype(F),
               normal=axes[rng.integers(0, 3, (ny, nx))], depth=rng.uniform(1.0, 9.0, (ny, nx)).astype(F))
    img["normal"][2, 3] = 0.0  # a zero-length normal: the weight is 1
    img["albedo"][4, 5] = 1e-5  # below albedo_min
    img["depth"][6:, :4] = np.inf
    taps = []
    out = _run(img, img, taps=taps)
    x0, (w0, w1) = ref.tap_axis(nx, nx)
    assert (x0 == np.arange(nx)).all() and (w1 == 0).all() and (w0 == 1).all()  # tx = 0 exactly
    assert (sum(t["use"].astype(int) for t in taps) == 1).all() and taps[0]["use"].all()  # one contributing tap: itself
    surf = np.isfinite(img["depth"])
    assert (out["cls"][surf] == ref.GUIDED).all() and (out["cls"][~surf] == ref.BACKGROUND).all()
    a = np.fmax(img["albedo"], F(1e-3))
    assert np.array_equal(out["linear"][surf], ((img["linear"] / a) * a)[surf])
    assert np.array_equal(out["linear"][~surf], img["linear"][~surf])
    ok = surf[..., None] & (img["albedo"] >= F(1e-3))
    assert _ulps(out["linear"], img["linear"])[ok].max() <= 2
    assert np.array_equal(out["rgb8"], ref.quantise(out["linear"]))


@pytest.mark.parametrize("size", [s for s in ref.SIZES if s[2] > 1])
def test_outputs_lie_within_their_taps(size):
    """A class-1 output is a weighted mean of its surface taps' x_c and a class-2 output is one of them, times a'_c(p).  The
    mean's error: one rounding in each product w*x, three in the additions of C, three in those of W (every term is >= 0,
    so the sums do not cancel), one in the division and one in the product with a': nine roundings, each at most 2^-24
    relative; the bound below allows ten.  A rounding is that accurate only above the subnormal range: with w_min = 0 a
    pixel can be class 1 on subnormal weights (the repeated squaring of the normal weight reaches them), where a product
    w*x keeps a few bits only.  The bound is asserted where every weight is 0 or at least 2^-100 (x is at least 2^-10 here,
    so no product is subnormal); on the other pixels a product can round to 0 or up by a factor below two, and they are
    held to lie between 0 and twice their taps' greatest value."""
    tol = 10 * EPS
    for variant in range(4):
        planes, params = ref.synthetic(size, variant)
        taps = []
        out = ref.upscale(**planes, **params, taps=taps)
        lo = np.full(out["linear"].shape, np.inf)
        hi = np.full(out["linear"].shape, -np.inf)
        tiny = np.zeros(out["cls"].shape, bool)
        for t in taps:
            tiny |= t["use"] & t["same"] & (t["w"] > 0) & (t["w"] < F(2.0 ** -100))
            ss = (t["use"] & t["same"])[..., None]
            lo = np.where(ss, np.minimum(lo, t["x"].astype(np.float64)), lo)
            hi = np.where(ss, np.maximum(hi, t["x"].astype(np.float64)), hi)
        ap = np.fmax(planes["albedo"], F(params.get("albedo_min", 1e-3))).astype(np.float64)
        for cls in (ref.GUIDED, ref.NEAREST):
            m = (out["cls"] == cls) & ~tiny
            v = out["linear"].astype(np.float64)[m]
            assert (v >= (lo * ap)[m] * (1 - tol)).all() and (v <= (hi * ap)[m] * (1 + tol)).all(), (variant, cls)
            m = (out["cls"] == cls) & tiny
            v = out["linear"].astype(np.float64)[m]
            assert (v >= 0.0).all() and (v <= (hi * ap)[m] * 2.0).all(), (variant, cls)
        near = out["cls"] == ref.NEAREST
        exact = np.zeros(out["linear"].shape, bool)
        for t in taps:  # class 2 is exactly one tap's x times a'
            exact |= (t["use"] & t["same"])[..., None] & (out["linear"] == t["x"] * np.fmax(planes["albedo"], F(params.get("albedo_min", 1e-3))))
        assert exact[near].all()


@pytest.mark.parametrize("lx,nx", [(16, 32), (20, 30)])
def test_a_depth_step_keeps_the_two_sides_apart(lx, nx):
    """The near side at depth 1, the far side at 1.5: for a near-side pixel dz = 0.5 / (0.05*1 + 1e-3) = 9.8 and exp(-dz) =
    5.5e-5 < w_min / 4 = 2.5e-4, so all far-side taps together weigh less than w_min."""
    ly, ny = 6, 9
    lo, hi = _flat(ly, lx), _flat(ny, nx)
    lo["depth"][:, lx // 2:] = 1.5
    hi["depth"][:, nx // 2:] = 1.5
    lo["linear"][:, lx // 2:] = 100.0
    assert np.exp(-0.5 / (0.05 * 1.0 + 1e-3)) < 1e-3 / 4
    taps = []
    out = _run(lo, hi, taps=taps)
    assert (out["cls"] == ref.GUIDED).all()
    near = np.broadcast_to((np.arange(nx) < nx // 2)[None, :], (ny, nx))
    far_weight = sum(np.where(t["use"] & (t["qx"] >= lx // 2), t["w"], F(0.0)) for t in taps)
    straddles = sum((t["use"] & (t["qx"] >= lx // 2)).astype(int) for t in taps)
    assert (straddles[near] > 0).any()  # some near-side pixels do have far-side taps
    assert (far_weight[near] <= F(1e-3)).all()
    assert (out["linear"][near] < 1.05).all() and (out["linear"][near] >= 1.0 - 1e-6).all()
    assert (out["linear"][~near] > 99.0).all()
    blind = ref.bilinear(lo["linear"], ny, nx)
    assert blind[near].max() > 10.0  # what the guide prevents


def test_features_the_low_image_lacks():
    lx, ly, nx, ny = 8, 8, 16, 16
    lo, hi = _flat(ly, lx, z=np.inf, colour=3.0), _flat(ny, nx, z=np.inf)
    hi["depth"][:, 9] = 2.0  # a thin surface the low image does not see at all
    out = _run(lo, hi)
    assert (out["cls"][:, 9] == ref.MISMATCH).all() and (np.delete(out["cls"], 9, axis=1) == ref.BACKGROUND).all()
    assert np.allclose(out["linear"], 3.0, rtol=1e-6)  # class 3: the plain bilinear mean
    assert np.array_equal(out["linear"][:, 9], ref.bilinear(lo["linear"], ny, nx)[:, 9])
    # a lone surface tap behind an edge: far in depth, so it has no weight, yet it is all there is
    lo["depth"][4, 4] = 1000.0
    lo["linear"][4, 4] = 0.25
    lo["albedo"][4, 4] = 0.125
    hi["albedo"][:, 9] = 0.75
    out = _run(lo, hi)
    lone = (out["cls"] == ref.NEAREST)
    assert lone[7:11, 9].all() and lone.sum() == 4  # the four pixels of the column whose taps reach (4, 4)
    assert (out["linear"][lone] == F(0.25) / F(0.125) * F(0.75)).all()
    assert (out["cls"][:, 9][[k for k in range(ny) if k not in (7, 8, 9, 10)]] == ref.MISMATCH).all()


def test_background_pixels_ignore_surface_taps():
    lx, ly, nx, ny = 8, 8, 16, 16
    lo, hi = _flat(ly, lx, z=np.inf, colour=7.0), _flat(ny, nx, z=np.inf)
    lo["depth"][:, 4:] = 1.0
    lo["linear"][:, 4:] = 1000.0
    out = _run(lo, hi)
    has_bg_tap = np.arange(nx) <= 8  # fx < 4: the column x0 <= 3 is among the taps
    assert (out["cls"][:, has_bg_tap] == ref.BACKGROUND).all() and (out["cls"][:, ~has_bg_tap] == ref.MISMATCH).all()
    assert np.allclose(out["linear"][:, has_bg_tap], 7.0, rtol=1e-6)
    assert np.allclose(out["linear"][:, ~has_bg_tap], 1000.0, rtol=1e-6)
    assert ref.bilinear(lo["linear"], ny, nx)[:, 8].max() > 100.0


@pytest.mark.parametrize("z", [1.0, np.inf])
def test_the_borders_renormalise_over_the_taps_that_exist(z):
    lx, ly, nx, ny = 5, 4, 10, 8
    lo, hi = _flat(ly, lx, z=z, colour=0.3), _flat(ny, nx, z=z)
    taps = []
    out = _run(lo, hi, taps=taps)
    x0, _ = ref.tap_axis(lx, nx)
    y0, _ = ref.tap_axis(ly, ny)
    assert x0[0] == -1 and x0[-1] + 1 == lx and y0[0] == -1 and y0[-1] + 1 == ly
    used = sum(t["use"].astype(int) for t in taps)
    assert used[0, 0] == 1 and used[0, 3] == 2 and used[3, 0] == 2 and used[3, 3] == 4 and used[-1, -1] == 1
    total = sum(np.where(t["use"], t["b"], F(0.0)) for t in taps)
    assert total[0, 0] < 0.6 and total[3, 3] == 1.0  # the corner has a quarter of the weight, and still the full value:
    assert _ulps(out["linear"], np.full((ny, nx, 3), F(0.3) / F(0.5) * F(0.5) if z == 1.0 else 0.3, F)).max() <= 4
    assert (out["cls"] == (ref.GUIDED if z == 1.0 else ref.BACKGROUND)).all()


@pytest.mark.parametrize("size", ref.SIZES)
def test_the_synthetic_inputs_reach_every_class_at_every_size(size):
    """tests/test_gpu_upscale.py compares the kernel with the restatement on these inputs: it cannot pass by never reaching
    a branch."""
    seen = set()
    for variant in range(4):
        planes, params = ref.synthetic(size, variant)
        lx, ly, nx, ny = size
        assert planes["depth_lo"].shape == (ly, lx) and planes["depth"].shape == (ny, nx)
        assert all(a.dtype == F for a in planes.values())
        out = ref.upscale(**planes, **params)
        assert out["cls"][0, 0] == variant
        seen |= set(np.unique(out["cls"]).tolist())
        lin = planes["linear_lo"]
        assert lin.min() >= 2.0 ** -10 and lin.max() <= 2.0 ** 10
        if nx * ny >= 256:  # the larger sizes hold every ingredient in every variant
            assert set(np.unique(out["cls"]).tolist()) == {0, 1, 2, 3}, variant
            for a in (planes["albedo"], planes["albedo_lo"]):
                assert (a < 1e-3).any() and (a == 0).any()
            for n in (planes["normal"], planes["normal_lo"]):
                assert (np.abs(n).sum(axis=2) == 0).any()
            for z in (planes["depth"], planes["depth_lo"]):
                assert np.isinf(z).any() and np.isfinite(z).any()
    assert seen == {ref.BACKGROUND, ref.GUIDED, ref.NEAREST, ref.MISMATCH}
    assert {p.get("normal_power", 32) for p in ref.PARAM_SETS} == {0, 1, 32}
    assert {p.get("sigma_z", 0.05) for p in ref.PARAM_SETS} == {0.0, 0.05} and {p.get("w_min", 1e-3) for p in ref.PARAM_SETS} == {0.0, 1e-3}
