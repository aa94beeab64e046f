"""The numpy restatement of per-pixel adaptive sampling (tests/pixelwise_ref.py) on crafted samples: no GPU."""
import numpy as np

import pixelwise_ref as ref


def _noise(n, cap, seed=0, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.random((n, cap, 3)) * scale).astype(np.float32)


def test_lattice_ends_on_the_cap_with_a_shortened_step():
    assert ref.lattice(24, 4, 4) == [4, 8, 12, 16, 20, 24]
    assert ref.lattice(22, 4, 4) == [4, 8, 12, 16, 20, 22]
    assert ref.lattice(4, 4, 9) == [4]
    assert ref.lattice(5, 4, 9) == [4, 5]


def test_zero_variance_retires_at_min_spp_with_abs_tol_zero():
    x = np.full((5, 24, 3), 0.375, np.float32)
    out = ref.render(x, 4, 4, abs_tol=0.0, rel_tol=0.0)
    assert (out["spp"] == 4).all()
    assert (out["linear"] == np.float32(0.375)).all() and (out["stderr"] == 0).all()
    assert out["counts"][:, 0].tolist() == [5, 0, 0, 0, 0, 0]


def test_a_non_finite_sample_never_converges():
    x = np.full((3, 22, 3), 0.5, np.float32)
    x[1, 2, 0] = np.nan
    x[2, 0, 1] = np.inf
    out = ref.render(x, 4, 4, abs_tol=1e30, rel_tol=1e30)
    assert out["spp"].tolist() == [4, 22, 22]
    assert np.isnan(out["linear"][1, 0]) and np.isnan(out["stderr"][1, 0]) and out["rgb8"][1, 0] == 0
    assert np.isposinf(out["linear"][2, 1]) and out["rgb8"][2, 1] == 255


def test_the_cap_is_reached_with_a_shortened_last_step():
    x = _noise(7, 22)
    out = ref.render(x, 4, 4)  # tolerances 0: every noisy pixel runs to the cap
    assert (out["spp"] == 22).all()
    assert out["counts"][:, 0].tolist() == [7] * 6
    want = x.astype(np.float64).sum(axis=1) / 22.0
    assert np.allclose(out["linear"], want, rtol=1e-6)
    se = x.astype(np.float64).std(axis=1, ddof=1) / np.sqrt(22.0)
    assert np.allclose(out["stderr"], se, rtol=1e-5)


def test_a_retired_pixel_stays_retired():
    # four equal samples pass any tolerance; the outlier that follows would fail it at the next count
    x = np.full((2, 12, 3), 0.25, np.float32)
    x[0, 5] = 100.0
    x[1] = _noise(1, 12, seed=3)[0]
    out = ref.render(x, 4, 4, abs_tol=1e-3)
    assert out["spp"].tolist() == [4, 12]
    assert (out["linear"][0] == np.float32(0.25)).all() and (out["stderr"][0] == 0).all()
    late = ref.render(x[:1, :8], 8, 1, abs_tol=1e-3)  # the same pixel tested at 8 only: it does fail there
    assert late["stderr"][0, 0] > 1e-3


def test_the_counts_sum_to_the_samples():
    x = _noise(200, 24, seed=1)
    x[:50] *= 0.01
    se4 = x[:, :4].astype(np.float64).std(axis=1, ddof=1).max(axis=1) / 2.0
    out = ref.render(x, 4, 4, abs_tol=float(np.median(se4)) / 2)
    lat = ref.lattice(24, 4, 4)
    per_step = np.diff([0] + lat)
    assert int((out["counts"][:, 0] * per_step).sum()) == int(out["spp"].sum())
    assert len(set(out["spp"].tolist())) >= 3 and set(out["spp"].tolist()) <= set(lat)
    assert (np.diff(out["counts"][:, 0].astype(np.int64)) <= 0).all() and out["counts"][0, 0] == 200
    assert (out["counts"][:, 0] == out["counts"][:, 1]).all()


def test_step_composes_to_render():
    x = _noise(70, 11, seed=2)
    want = ref.render(x, 4, 3, abs_tol=0.15)
    n = 70
    state = np.full((9, n), -7.0)
    planes = {"active": np.ones(n, np.uint8), "linear": np.zeros((n, 3), np.float32), "rgb8": np.zeros((n, 3), np.uint8),
              "stderr": np.zeros((n, 3), np.float32), "spp": np.zeros(n, np.uint32)}
    done, counts = 0, []
    for upto in ref.lattice(11, 4, 3):
        lst = np.flatnonzero(planes["active"]).astype(np.uint32)
        counts.append(lst.size)
        for a, b in [(done, done + 1), (done + 1, upto)]:  # two sub-passes; only the second decides
            if b > a and lst.size:
                state, planes = ref.step(lst, None, x[lst, a:b], state, n, a, b == upto, 11, 0.15, 0.0, planes)
        done = upto
    assert counts == want["counts"][:, 0].tolist()
    for k in ("spp", "linear", "stderr", "rgb8"):
        assert planes[k].tobytes() == want[k].tobytes(), k
