"""The numpy restatement of include/rtmi_tonemap.h (tests/tonemap_ref.py) against the oracle and against what the header
promises, without a GPU.  tests/test_gpu_tonemap.py holds the device to this restatement bit for bit; these tests hold the
restatement to the contract."""
import numpy as np
import pytest

import denoise_ref
import tonemap_ref as ref

F = np.float32


def test_restated_logf_is_the_oracles(orc32):
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.integers(1, 0x7f800000, 1 << 16, dtype=np.uint32).view(F),  # 2^16 random positive floats
                        rng.integers(1, 0x00800000, 4096, dtype=np.uint32).view(F),  # denormals
                        np.array([1, 2, 0x007fffff, 0x00800000, 0x7f7fffff], np.uint32).view(F),
                        np.exp2(np.arange(-149, 128)).astype(F)])  # every power of two
    assert (x > 0).all() and np.isfinite(x).all()
    got = ref.logf(x)
    fn = orc32.lib.orc_rtmi_logf
    want = np.array([fn(float(v)) for v in x], F)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    assert ref.logf(np.array([1.0], F))[0] == 0.0


def _grey(L, ny=9, nx=7):
    return np.full((ny, nx, 3), L, F)


@pytest.mark.parametrize("lo, hi", [(-12.0, 12.0), (-3.0, 5.0), (-20.0, -19.0)])
def test_a_constant_image_meters_to_its_log2_within_half_a_bin(lo, hi):
    """The bin b of a value e holds [lo + b*w, lo + (b+1)*w) with w = (hi - lo)/256, and the metered value of a bin is its
    centre, lo + (b + 0.5)*w: at most w/2 = (hi - lo)/512 from any value in the bin.  The exposure adds rtmi_expf's error
    and two fp32 roundings, which 2^-20 covers."""
    w = (hi - lo) / 256.0
    bound = (hi - lo) / 512.0
    for frac in (0.003, 0.25, 0.5, 0.77, 0.996):
        for b in (0, 1, 100, 255):
            e = lo + (b + frac) * w
            L = F(2.0 ** e)
            tm = ref.Tonemap(log2_min=lo, log2_max=hi, adapt_min=-64.0, adapt_max=64.0)
            _, _, st = tm.apply(_grey(L))
            assert st["counted"] == 63 == int(ref.histogram(_grey(L), tm.p).sum())
            assert 1 <= st["kept"] <= 63
            log2L = np.log2(float(L) * float(F(0.2126) + F(0.7152) + F(0.0722)))
            assert abs(float(st["metered_log2"]) - log2L) <= bound, (lo, hi, b, frac)
            assert st["adapted_log2"] == st["metered_log2"]  # a first apply adopts
            lum = float(ref.luminance(_grey(L))[0, 0])
            assert abs(np.log2(float(st["exposure"]) * lum / float(tm.p["key"]))) <= bound + 2.0 ** -20


def test_the_whole_range_of_percentiles_is_the_mean_of_the_bins():
    img = ref.sample_image(37, 23, 3)
    tm = ref.Tonemap(p_low=0.0, p_high=1.0)
    bins = ref.histogram(img, tm.p)
    counted, b = ref.bin_index(ref.luminance(img).ravel(), tm.p)
    assert bins.sum() == counted.sum() and 0 < counted.sum() < counted.size  # some pixels are not counted
    assert bins[0] > 0 and bins[255] > 0  # beyond both ends of the range
    _, _, st = tm.apply(img)
    assert st["counted"] == st["kept"] == int(bins.sum())
    mean = b[counted].astype(np.float64).mean()
    assert st["metered_log2"] == F(-12.0 + (mean + 0.5) * (24.0 / 256.0))


def test_percentiles_cut_the_tails():
    img = _grey(1.0, 10, 10)  # 100 pixels in the middle
    img[0, :5] = 2.0 ** -11.5  # 5 % dark
    img[1, :3] = 2.0 ** 11.5  # 3 % bright
    full = ref.Tonemap(p_low=0.0, p_high=1.0).apply(img)[2]
    cut = ref.Tonemap(p_low=0.05, p_high=0.97).apply(img)[2]
    assert cut["kept"] == 92 and full["kept"] == 100
    only = ref.Tonemap().apply(_grey(1.0, 10, 10))[2]
    assert cut["metered_log2"] == only["metered_log2"] != full["metered_log2"]
    # a degenerate interval keeps one sample: the last one when p_low reaches the end
    one = ref.Tonemap(p_low=0.999, p_high=1.0).apply(_grey(1.0, 2, 2))[2]
    assert one["kept"] == 1 and one["metered_log2"] == only["metered_log2"]


def test_adaptation_moves_toward_the_metered_value_and_never_past_it():
    for first, then in ((1.0, 16.0), (16.0, 1.0)):
        tm = ref.Tonemap(speed_up=3.0, speed_down=1.0)
        a0 = tm.apply(_grey(first))[2]["adapted_log2"]
        m = ref.Tonemap().apply(_grey(then))[2]["metered_log2"]
        prev = a0
        for k in range(200):
            st = tm.apply(_grey(then), dt=1 / 60)[2]
            a = st["adapted_log2"]
            assert st["metered_log2"] == m and st["applies"] == k + 2
            assert (prev <= a <= m) if m > a0 else (m <= a <= prev), (k, prev, a, m)
            prev = a
        # the brightening adapts three times as fast as the darkening
        gone = abs(float(prev) - float(a0)) / abs(float(m) - float(a0))
        want = 1 - np.exp(-(200 / 60) * (3.0 if m > a0 else 1.0))
        assert abs(gone - want) < 1e-3
        for _ in range(3):  # a long step lands on m and stays
            a = tm.apply(_grey(then), dt=1000.0)[2]["adapted_log2"]
        assert a == m


def test_dt_zero_leaves_the_adapted_value():
    tm = ref.Tonemap()
    a0 = tm.apply(_grey(1.0))[2]["adapted_log2"]
    for L in (16.0, 1 / 16.0, 100.0):
        st = tm.apply(_grey(L), dt=0.0)[2]
        assert st["adapted_log2"] == a0 and st["metered_log2"] != a0
    frozen = ref.Tonemap(speed_up=0.0, speed_down=0.0)
    a0 = frozen.apply(_grey(1.0))[2]["adapted_log2"]
    assert frozen.apply(_grey(64.0), dt=10.0)[2]["adapted_log2"] == a0


def test_the_adaptation_bounds_bind():
    tm = ref.Tonemap(adapt_min=-1.0, adapt_max=2.0)
    st = tm.apply(_grey(2.0 ** 8))[2]
    assert st["adapted_log2"] == F(2.0) and st["metered_log2"] > 7.9
    assert st["exposure"] == F(0.18) * denoise_ref.expf(F(-2.0) * F(0.69314718))
    st = tm.apply(_grey(2.0 ** -8), dt=1000.0)[2]
    assert st["adapted_log2"] == F(-1.0) and st["metered_log2"] < -7.9


def test_black_frames():
    black = np.zeros((5, 5, 3), F)
    for ev in (0.0, 1.5, -3.0):
        tm = ref.Tonemap(ev=ev)
        rgb8, display, st = tm.apply(black)
        # E = key * 2^ev, to rtmi_expf's 2 ulp
        assert abs(float(st["exposure"]) / (0.18 * 2.0 ** ev) - 1) < 4 * 2.0 ** -23
        assert st["exposure"] == F(0.18) * denoise_ref.expf(F(ev) * F(0.69314718))
        assert (st["adapted_log2"], st["metered_log2"], st["counted"], st["kept"], st["applies"]) == (0, 0, 0, 0, 1)
        assert not rgb8.any() and not display.any()
        # the next metered frame adopts m whatever dt is: there is no adapted value yet
        st = tm.apply(_grey(8.0), dt=1 / 60)[2]
        assert st["adapted_log2"] == st["metered_log2"] == ref.Tonemap().apply(_grey(8.0))[2]["metered_log2"]
        # a black frame later keeps the adapted value
        a = st["adapted_log2"]
        st = tm.apply(black, dt=10.0)[2]
        assert st["adapted_log2"] == st["metered_log2"] == a and st["counted"] == 0 and st["applies"] == 3
    # pixels that are not counted make a frame black to the meter: negative, NaN, inf
    odd = np.zeros((2, 2, 3), F)
    odd[0, 0], odd[0, 1], odd[1, 0] = (-1, -1, -1), (np.nan, 1, 1), (np.inf, 1, 1)
    assert ref.Tonemap().apply(odd)[2]["counted"] == 0


def test_the_identity_setting_is_the_projects_quantiser():
    rng = np.random.default_rng(11)
    img = np.concatenate([rng.uniform(-0.2, 1.4, 3000), np.exp2(rng.uniform(-40, 40, 2982)),
                          [0.0, -0.0, 1.0, np.nan, np.inf, -np.inf, 1e-45, 0.99999994, 1.0000001, 0.25, 3e38, -3e38,
                           (255 / 255.99) ** 2, (128 / 255.99) ** 2, (1 / 255.99) ** 2, 0.5, 2.0, 4.0]]).astype(F).reshape(40, 50, 3)
    tm = ref.Tonemap(exposure="manual", ev=0.0, op="clamp", oetf="gamma2")
    rgb8, display, st = tm.apply(img)
    assert st["exposure"] == F(1.0) and (st["counted"], st["kept"], st["adapted_log2"], st["metered_log2"]) == (0, 0, 0, 0)
    assert (rgb8 == denoise_ref.quantise(img)).all()
    assert len(np.unique(rgb8)) == 256
    with np.errstate(all="ignore"):
        ok = np.isfinite(img) & (img >= 0) & (img <= 1)
        assert (display[ok] == np.sqrt(img[ok].astype(np.float64)).astype(F)).all()
    assert display.min() == 0 and display.max() == 1 and not np.isnan(display).any()
    for ev in (1.0, -2.0, 64.0, -64.0):
        E = ref.Tonemap(exposure="manual", ev=ev).apply(img)[2]["exposure"]
        assert abs(float(E) / 2.0 ** ev - 1) < 4 * 2.0 ** -23


def test_the_srgb_curve():
    rng = np.random.default_rng(5)
    y = np.sort(np.concatenate([rng.uniform(0, 1, (1 << 16) - 8), [0.0, 1.0, 0.0031308, 0.00313081, 0.0031307, 1e-45, 0.5,
                                                                  0.99999994]]).astype(F))
    q, s = ref.srgb(y)
    assert (np.diff(s) >= 0).all() and (np.diff(q.astype(int)) >= 0).all()
    # 0 -> 0 and 1 -> 255; the display value of 1 is 1.055f - 0.055f, one ulp below 1 in fp32
    assert q[0] == 0 and s[0] == 0 and q[-1] == 255 and s[-1] == F(1.055) - F(0.055) >= F(0.99999994)
    assert len(np.unique(q)) == 256
    exact = np.where(y <= 0.0031308, 12.92 * y.astype(np.float64), 1.055 * y.astype(np.float64) ** (1 / 2.4) - 0.055)
    assert np.abs(s - exact).max() < 2e-6
    q2, s2 = ref.srgb(np.array([-1.0, np.nan, 2.0, np.inf, -np.inf, -0.0], F))
    assert q2.tolist() == [0, 0, 255, 255, 0, 0] and s2.tolist() == [0, 0, s[-1], s[-1], 0, 0]


def test_the_curves():
    x = np.concatenate([[0.0, 1e-30, 0.18, 1.0, 4.0, 1e6, 1e30], np.exp2(np.linspace(-20, 20, 400))]).astype(F)
    r = ref.curve(x, ref.params(op="reinhard"))  # white = inf: x/(1 + x)
    assert (r == x / (F(1.0) + x)).all() and (r <= 1).all() and (r[:5] < 1).all()
    w = ref.curve(x, ref.params(op="reinhard", white=4.0))
    assert w[4] == 1.0 and (w >= r).all()  # the white point maps to 1
    a = ref.curve(x, ref.params(op="aces"))
    # rising up to its limit 2.51/2.43, to the rounding of its five operations (each half an ulp of a value below 1.04)
    assert a[0] == 0 and (np.diff(a[7:]) >= -5 * 2.0 ** -24 * 1.04).all() and (np.delete(a, 6) <= F(2.51 / 2.43) + F(2e-7)).all()
    assert np.isnan(a[6])  # x*x overflows above about 1.8e19: inf/inf, which the transfer function maps to 0
    assert abs(float(a[2]) - 0.18 * (2.51 * 0.18 + 0.03) / (0.18 * (2.43 * 0.18 + 0.59) + 0.14)) < 1e-6
    neg = np.array([-1.0, np.nan, -np.inf], F)
    for op in ("reinhard", "aces"):
        assert not ref.curve(neg, ref.params(op=op)).any()
    assert ref.curve(neg, ref.params(op="clamp"))[0] == -1.0


def test_the_handle_counts_and_resets():
    tm = ref.Tonemap()
    imgs = [ref.sample_image(6, 5, k) for k in range(3)]
    first = [tm.apply(i, dt=0.5) for i in imgs]
    assert [s["applies"] for _, _, s in first] == [1, 2, 3]
    tm.reset()
    again = [tm.apply(i, dt=0.5) for i in imgs]
    for (r0, d0, s0), (r1, d1, s1) in zip(first, again):
        assert (r0 == r1).all() and (d0.view(np.uint32) == d1.view(np.uint32)).all()
        assert (ref.state_words(s0) == ref.state_words(s1)).all()
