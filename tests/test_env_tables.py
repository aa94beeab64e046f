"""The sampling tables of environment lighting (rtmi_env_tables, include/rtmi_env.h) on the CPU, and the numpy
restatement of the sampler and the lookup (tests/env_ref.py) on its own.

* rtmi_env_tables equals a numpy f64 restatement bit for bit on 1x1, 3x2 and 64x32 maps, a "sun" map, an all-zero map
  and the decoded earthmap; the last CDF entries are exactly 1; sum pdf dw over the sphere is 1 within 1e-6;
* the restatement's sampler has the density it claims, and a constant map looks up its constant exactly."""
import math

import numpy as np
import pytest

import env_ref as ref
from raytracing_rust_amd import env_from_sky, env_tables, scenes


def _maps():
    rng = np.random.default_rng(11)
    data, w, h = scenes.earthmap_rgb8()
    earth = (np.asarray(data, np.float32).reshape(h, w, 3) / np.float32(255.0)).astype(np.float32)
    return {"1x1": np.float32([[[0.25, 2.0, 0.5]]]), "3x2": rng.random((2, 3, 3)).astype(np.float32),
            "64x32": (rng.random((32, 64, 3)) ** 4 * 10).astype(np.float32), "sun": ref.sun_map(),
            "zero": np.zeros((8, 16, 3), np.float32), "earth": earth, "sky": env_from_sky(64, 32)}


MAPS = _maps()


@pytest.mark.parametrize("name", sorted(MAPS))
def test_tables_equal_restatement(name):
    m = MAPS[name]
    got, want = env_tables(m), ref.tables(m)
    for k in ("row_cdf", "row_p", "col_cdf", "col_p"):
        assert got[k].dtype == np.float32 and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), (name, k, int((got[k] != want[k]).sum()))
    assert got["total"] == want["total"]
    assert got["row_cdf"][-1] == 1.0 and np.all(got["col_cdf"][:, -1] == 1.0)
    assert np.all(np.diff(got["row_cdf"]) >= 0) and np.all(np.diff(got["col_cdf"], axis=1) >= 0)
    if name == "zero":
        assert got["total"] == 0.0 and not got["row_p"].any() and not got["col_p"].any()
        assert np.all(got["row_cdf"] == 1.0) and np.all(got["col_cdf"] == 1.0)
    else:
        assert got["total"] > 0 and np.all(got["col_p"][got["row_p"] > 0].sum(1) > 0)
        # sum of pdf * dw over the texels: p_row p_col W H / (2 pi^2 cos) times the texel's 2 pi^2 cos du dv
        s = float(np.sum(got["row_p"].astype(np.float64)[:, None] * got["col_p"].astype(np.float64)))
        assert abs(s - 1.0) < 1e-6, s


def test_sun_map_is_concentrated():
    m = MAPS["sun"]
    h, w = m.shape[:2]
    t = env_tables(m)
    p = t["row_p"].astype(np.float64)[:, None] * t["col_p"]
    j = np.arange(h)
    dw = (2 * math.pi / w) * (np.cos((j + 0.5) / h * math.pi - math.pi / 2) * math.pi / h)  # solid angle per texel
    order = np.argsort(-p.ravel())
    cum = np.cumsum(p.ravel()[order])
    k = int(np.searchsorted(cum, 0.5)) + 1  # the fewest texels that hold half the weight
    omega = float(np.sum(np.broadcast_to(dw[:, None], (h, w)).ravel()[order[:k]]))
    assert omega < 1e-3 * 4 * math.pi, omega


def test_constant_map_looks_up_its_constant():
    M = ref.ContractMath()
    c = np.float32([0.3, 1.7, 5.0])
    tex = np.broadcast_to(c, (5, 9, 3)).astype(np.float32)
    d = ref.lat_long_dirs(4000, np.random.default_rng(2))
    T = ref.tables(tex)
    out = ref.lookup(M, tex, T, d)
    ok = ref.env_uv(M, d)[0]
    assert np.all(out[ok, :3] == c) and not out[~ok].any()


def test_sampler_density_is_what_it_claims():
    """A histogram of the restatement's samples over the texels matches p_row * p_col, and pdf equals the lookup's pdf
    of the sampled direction away from texel edges."""
    M = ref.ContractMath()
    tex = MAPS["64x32"]
    h, w = tex.shape[:2]
    T = ref.tables(tex)
    rng = np.random.default_rng(4)
    u = ref.uniforms(400000, rng)
    s = ref.sample(M, T, w, h, u[:, 0], u[:, 1])
    good = s[:, 3] > 0  # none only at the poles (theta = +-pi/2 in float has cos <= 0): u1 = 0 among the edge pairs
    assert (~good).sum() <= 8, int((~good).sum())
    s = s[good]
    ok, uu, vv, _ = ref.env_uv(M, s[:, :3])
    assert ok.all()
    i = np.clip(np.floor(uu * w).astype(int), 0, w - 1)
    j = np.clip(np.floor((1 - vv) * h).astype(int), 0, h - 1)
    hist = np.bincount(j * w + i, minlength=w * h).reshape(h, w) / len(s)
    p = T["row_p"].astype(np.float64)[:, None] * T["col_p"]
    big = p > 1e-4  # at least 40 expected samples
    z = (hist[big] - p[big]) / np.sqrt(p[big] / len(s))
    assert np.abs(z).max() < 6, np.abs(z).max()
    lk = ref.lookup(M, tex, T, s[:, :3])
    rel = np.abs(lk[:, 3] / s[:, 3] - 1)
    assert np.median(rel) < 1e-5
