"""The directions and the basis of the hemisphere gathers (include/rtmi_gather.h), without a GPU.

rtmi_gather_directions is compiled from the inline functions the kernels compile, so these tests pin the device's
arithmetic:
* it equals tests/gather_ref.py bit for bit, both modes, on 4096 normals: random ones, the six axes, n.z = -0.0, lengths
  1e-3 and 1e3;
* |d| is within 4 ulp of 1; COSINE draws lie in the normal's hemisphere and have mean cosine 2/3; SPHERE draws make the
  nine harmonics orthonormal;
* splitting (first_point, first_sample) reproduces the unsplit array;
* sh_irradiance of an analytic probe."""
import numpy as np
import pytest

import gather_ref as G
from raytracing_rust_amd import gather_directions, sh_irradiance
from raytracing_rust_amd.host import sh_basis

SEED = 0x1234567890ABCDEF
ULP = 2.0 ** -23


def _normals():
    rng = np.random.default_rng(11)
    n = rng.standard_normal((4096, 3)).astype(np.float32)
    n[:6] = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    n[6] = [0.6, 0.8, -0.0]
    n[7] = [1.0, 0.0, -0.0]
    n[8] = [0.0, 0.0, 1e-3]
    n[9] = [0.0, 0.0, -1e3]
    n[10:1024] *= np.float32(1e-3) / np.linalg.norm(n[10:1024], axis=1, keepdims=True).astype(np.float32)
    n[1024:2048] *= np.float32(1e3) / np.linalg.norm(n[1024:2048], axis=1, keepdims=True).astype(np.float32)
    assert np.signbit(n[6, 2]) and np.signbit(n[7, 2])
    return n


@pytest.fixture(scope="module")
def cosine():
    nrm = _normals()
    return nrm, gather_directions(nrm, 5, seed=SEED, mode="cosine", first_point=3, first_sample=2)


@pytest.fixture(scope="module")
def sphere():
    return gather_directions(None, 16, seed=SEED, mode="sphere", n=4096)


def test_cosine_directions_equal_the_restatement(cosine):
    nrm, d = cosine
    ref = G.directions(nrm, 5, seed=SEED, mode="cosine", first_point=3, first_sample=2)
    assert d.shape == ref.shape == (4096, 5, 3) and d.dtype == np.float32
    assert d.tobytes() == ref.tobytes(), "%d components differ" % int(np.sum(d.view(np.uint32) != ref.view(np.uint32)))


def test_sphere_directions_equal_the_restatement(sphere):
    ref = G.directions(None, 16, seed=SEED, mode="sphere", n=4096)
    assert sphere.shape == ref.shape == (4096, 16, 3)
    assert sphere.tobytes() == ref.tobytes(), "%d components differ" % int(np.sum(sphere.view(np.uint32) != ref.view(np.uint32)))


def test_directions_are_unit_length(cosine, sphere):
    for name, d in (("cosine", cosine[1]), ("sphere", sphere)):
        err = np.abs(np.linalg.norm(d.astype(np.float64), axis=2) - 1.0) / ULP
        print("%s: |d| is within %.2f ulp of 1" % (name, err.max()))
        assert err.max() <= 4.0, (name, err.max())


def test_cosine_draws_lie_in_the_hemisphere_with_mean_cosine_two_thirds():
    nrm = _normals()[:64]
    d = gather_directions(nrm, 4096, seed=SEED, mode="cosine").astype(np.float64)
    unit = nrm.astype(np.float64) / np.linalg.norm(nrm.astype(np.float64), axis=1, keepdims=True)
    cos = np.einsum("nkc,nc->nk", d, unit)
    print("least cosine %.3e" % cos.min())
    assert cos.min() > 0.0
    se = cos.std(axis=1, ddof=1) / np.sqrt(cos.shape[1])
    z = (cos.mean(axis=1) - 2.0 / 3.0) / se
    print("mean cosine: largest |z| of 64 normals %.2f" % np.abs(z).max())
    # 3 standard errors for the pooled mean; the 64 normals share no draw, so their largest |z| is held to 4.5
    # (P(|z| > 4.5) = 7e-6 each)
    pooled = cos.reshape(-1)
    assert abs(pooled.mean() - 2.0 / 3.0) <= 3.0 * pooled.std(ddof=1) / np.sqrt(pooled.size)
    assert np.abs(z).max() <= 4.5


def test_sphere_draws_make_the_basis_orthonormal(sphere):
    d = sphere.reshape(-1, 3)
    assert d.shape[0] == 2 ** 16
    Y = G.sh9(d).astype(np.float64)
    assert np.abs(Y - sh_basis(d)).max() < 1e-6  # the float32 basis is the float64 one of sh_irradiance
    prod = 4.0 * np.pi * Y[:, :, None] * Y[:, None, :]  # [N, 9, 9]
    mean = prod.mean(axis=0)
    se = prod.std(axis=0, ddof=1) / np.sqrt(prod.shape[0])
    # Y0 * Y0 * 4 pi is the constant 1: its sample variance is rounding noise, so the error is held absolutely there
    assert abs(mean[0, 0] - 1.0) < 1e-6
    se[0, 0] = 1.0
    z = (mean - np.eye(9)) / se
    print("largest |z| of the 81 products %.2f" % np.abs(z).max())
    assert np.abs(z).max() <= 5.0


def test_splitting_reproduces_the_unsplit_array(cosine, sphere):
    nrm, whole = cosine
    for k in (1, 63, 4095):
        a = gather_directions(nrm[:k], 5, seed=SEED, first_point=3, first_sample=2)
        b = gather_directions(nrm[k:], 5, seed=SEED, first_point=3 + k, first_sample=2)
        assert np.concatenate([a, b]).tobytes() == whole.tobytes(), k
    a = gather_directions(nrm, 2, seed=SEED, first_point=3, first_sample=2)
    b = gather_directions(nrm, 3, seed=SEED, first_point=3, first_sample=4)
    assert np.concatenate([a, b], axis=1).tobytes() == whole.tobytes()
    a = gather_directions(None, 7, seed=SEED, mode="sphere", n=100, first_point=50)
    b = gather_directions(None, 9, seed=SEED, mode="sphere", n=100, first_point=50, first_sample=7)
    assert np.concatenate([a, b], axis=1).tobytes() == np.ascontiguousarray(sphere[50:150]).tobytes()
    # the last indices that fit
    gather_directions(nrm[:2], 2, seed=1, first_point=2 ** 32 - 2, first_sample=2 ** 32 - 2)
    with pytest.raises(ValueError, match="first_point"):
        gather_directions(nrm[:3], 2, seed=1, first_point=2 ** 32 - 2)
    assert not np.array_equal(whole, gather_directions(nrm, 5, seed=SEED + 1, first_point=3, first_sample=2))


def test_reduction_restatement_on_known_samples():
    x = np.array([[[1.0, 2.0, 4.0], [3.0, 2.0, 0.0]]], np.float32)
    r = G.reduce(x, "cosine")
    assert np.allclose(r["value"], np.pi * np.array([2.0, 2.0, 2.0]))
    assert np.allclose(r["stderr"], np.pi * np.array([1.0, 0.0, 2.0]))  # sqrt(sum (x - mean)^2 / (2 * 1))
    d = gather_directions(None, 2, seed=3, mode="sphere", n=1)
    r = G.reduce(x, "sphere", d)
    assert np.allclose(r["value"], [2.0, 2.0, 2.0]) and np.allclose(r["stderr"], [1.0, 0.0, 2.0])
    assert np.allclose(r["sh"][0, 0], 4.0 * np.pi * 0.28209479 * np.array([2.0, 2.0, 2.0]), rtol=1e-6)
    assert np.all(np.isposinf(G.reduce(x[:, :1], "sphere")["stderr"]))


def test_sh_irradiance_of_analytic_probes():
    rng = np.random.default_rng(2)
    nrm = rng.standard_normal((32, 3))
    # constant radiance L: only sh[0] = L * sqrt(4 pi); E = pi * L for every normal
    sh = np.zeros((32, 9, 3))
    sh[:, 0] = np.sqrt(4.0 * np.pi) * np.array([1.0, 2.0, 3.0])
    assert np.allclose(sh_irradiance(sh, nrm), np.pi * np.array([1.0, 2.0, 3.0]))
    # L(w) = max(w.a, 0)... is not band-limited; L(w) = 1 + w.a is: E(n) = pi + (2 pi / 3) n.a
    a = np.array([0.3, -0.5, 0.2])
    w = rng.standard_normal((200000, 3))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    L = 1.0 + w @ a
    coef = 4.0 * np.pi * (L[:, None] * sh_basis(w)).mean(axis=0)  # Monte-Carlo projection
    sh = np.repeat(coef[None, :, None], 3, axis=2).repeat(32, axis=0)
    unit = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    want = np.pi + (2.0 * np.pi / 3.0) * (unit @ a)
    assert np.abs(sh_irradiance(sh, nrm)[:, 0] - want).max() < 0.05
