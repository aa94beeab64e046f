"""The numpy restatement of NEE's formulas (tests/nee_ref.py), checked on the CPU: densities integrate to 1, the cone's
1 - cos(theta_max) does not cancel, the MIS weights sum to 1, the known answers' quadrature matches the closed form, and
the reference's Lambertian direction has the density (2/pi) cos^3 — the cos/pi lobe is rejected by the same test."""
import numpy as np

import nee_ref


def test_lambert_density_integrates_to_one():
    m = 4000
    ct = (np.arange(m) + 0.5) / m  # cos theta over the upper hemisphere, dw = 2 pi d(cos theta)
    total = np.sum(nee_ref.pb_lambert(np.stack([np.sqrt(1 - ct * ct), np.zeros(m), ct], -1), [0, 0, 1.0])) * 2 * np.pi / m
    assert abs(total - 1.0) < 1e-6
    assert nee_ref.pb_lambert([0, 0, -1.0], [0, 0, 1.0]) == 0.0
    assert np.isclose(nee_ref.pb_lambert([0, 0, 5.0], [0, 0, 2.0]), 2 / np.pi)  # lengths do not enter


def _chi2_cos(dirs, bins, density_of_cos):
    c = dirs[:, 2]
    edges = np.linspace(0, 1, bins + 1)
    hist, _ = np.histogram(c, edges)
    # expected mass of a bin: integral of density over the band, dw = 2 pi dc
    fine = np.linspace(0, 1, bins * 200 + 1)
    mid = 0.5 * (fine[1:] + fine[:-1])
    mass = np.add.reduceat(density_of_cos(mid) * 2 * np.pi / (bins * 200), np.arange(0, bins * 200, 200))
    exp = mass / mass.sum() * len(c)
    return np.sum((hist - exp) ** 2 / exp)


def test_reference_lambertian_is_cos_cubed_not_cos_over_pi():
    rng = np.random.default_rng(5)
    d = nee_ref.lambert_directions([0.0, 0.0, 1.0], 400000, rng)
    bins = 20
    chi_cube = _chi2_cos(d, bins, lambda c: 2 / np.pi * c ** 3)
    chi_cos = _chi2_cos(d, bins, lambda c: c / np.pi)
    # 19 degrees of freedom: the 1e-6 quantile is about 62
    assert chi_cube < 62, chi_cube
    assert chi_cos > 1000, chi_cos


def test_rect_pdf_and_cone_pdf_integrate_to_one():
    # a rect straight above: the integral of p_L over its solid angle is 1 (midpoint rule in area measure)
    x = np.zeros(3)
    m = 400
    u = (np.arange(m) + 0.5) / m
    q = np.stack(list(np.meshgrid(-1 + 2 * u, -1 + 2 * u, indexing="ij")) + [np.full((m, m), 3.0)], -1)
    w = q - x
    d2 = np.sum(w * w, -1)
    dw = np.abs(w[..., 2]) / np.sqrt(d2) / d2 * (4.0 / (m * m))
    assert abs(np.sum(nee_ref.rect_pdf(x, q, 2, 4.0) * dw) - 1.0) < 1e-9
    # the cone: 2 pi (1 - cos max) * pdf == 1; from inside: 0
    assert np.isclose(nee_ref.cone_pdf(x, [0, 0, 10.0], 2.0) * 2 * np.pi * nee_ref.one_minus_cos_max(x, [0, 0, 10.0], 2.0), 1.0)
    assert nee_ref.cone_pdf(x, [0, 0, 1.0], 2.0) == 0.0


def test_one_minus_cos_max_does_not_cancel():
    # a small far light: 1 - sqrt(1 - s) in float32 loses everything, s / (1 + sqrt(1 - s)) does not
    r, h = 0.2, 2.0e3
    s = (r / h) ** 2
    exact = s / 2 + s * s / 8 + s ** 3 / 16
    got = nee_ref.one_minus_cos_max(np.zeros(3), [0, 0, h], r)
    assert abs(got / exact - 1) < 1e-12
    s32 = np.float32(s)
    assert np.float32(1) - np.sqrt(np.float32(1) - s32) == 0  # the cancelling form
    assert abs(float(s32 / (np.float32(1) + np.sqrt(np.float32(1) - s32))) / exact - 1) < 1e-6


def test_mis_weights():
    pb = np.array([0.0, 1e-30, 0.3, 2.0, 1e30, 5.0])
    pl = np.array([1.0, 1e30, 0.3, 0.5, 1e-30, 0.0])
    wb = nee_ref.mis_bsdf(pb, pl)
    assert np.all(np.isfinite(wb)) and np.all((wb >= 0) & (wb <= 1))
    # the two power-heuristic weights sum to 1 (where both strategies exist)
    ok = (pb > 0) & (pl > 0)
    wl = pl[ok] ** 2 / (pb[ok] ** 2 + pl[ok] ** 2)
    assert np.allclose(wb[ok] + wl, 1.0)
    # the light-sample factor p_b p_l / (p_b^2 + p_l^2) = w_l * p_b / p_l, without overflow
    ml = nee_ref.mis_light(pb, pl)
    assert np.all(np.isfinite(ml))
    assert np.allclose(ml[ok], wl * pb[ok] / pl[ok])
    assert nee_ref.mis_bsdf(1.0, 0.0) == 1.0 and nee_ref.mis_light(0.0, 1.0) == 0.0


def test_sphere_quadrature_matches_closed_form():
    for r, h in ((2.0, 7.0), (0.2, 30.0), (1.0, 1.5)):
        got = nee_ref.f_sphere(np.zeros(3), [0, 1.0, 0], [0, h, 0], r)
        assert abs(got - nee_ref.f_sphere_below(r, h)) < 1e-4 * nee_ref.f_sphere_below(r, h), (r, h)


def test_rect_quadrature_against_sphere_free_check():
    # a rect of half-width a at height h against the disk of the same area (closed form 1 - (h^2 / (h^2 + R^2))^2),
    # which it must bracket with the inscribed and circumscribed disks
    a, h = 1.0, 2.0
    f, err = nee_ref.f_rect(np.zeros(3), np.array([0, 1.0, 0]), np.array([-a, h, -a]), np.array([2 * a, 0, 0]),
                            np.array([0, 0, 2 * a]), 256, 256)
    disk = lambda R: 1 - (h * h / (h * h + R * R)) ** 2
    assert disk(a) < f < disk(a * np.sqrt(2)) and err < 1e-4
    # F of a small far rect ~ (2/pi) * solid angle
    f, err = nee_ref.f_rect(np.zeros(3), np.array([0, 1.0, 0]), np.array([-0.5, 100.0, -0.5]), np.array([1.0, 0, 0]),
                            np.array([0, 0, 1.0]))
    assert abs(f - 2 / np.pi * 1e-4) < 1e-8
