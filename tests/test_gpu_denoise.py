"""The a-trous denoiser (include/rtmi_denoise.h) on the device.

* bit for bit the numpy restatement (tests/denoise_ref.py), in linear and rgb8, on synthetic planes (odd sizes,
  non-finite depths, zero normals and albedos, every switch of the parameters) and on render outputs, media included;
* rtmi_probe_expf is the restatement's rtmi_expf on the CPU test's sweep;
* iterations = 0 copies, non-surface pixels come through unchanged, repeated calls agree, render_denoised is its three
  calls, and a denoise leaves the renders it sits between alone;
* on cornell_box the denoised 16-spp image is measurably closer to a 4096-spp render than the noisy one."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as ref
import scenes_extra
from raytracing_rust_amd import abi, denoise, scenes

FC = abi.RTMI_FLAG_FAST_CULL
SEED = 42


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _synthetic(nx, ny, seed=0):
    """Planes with the cases the spec names: smooth depth with steps, non-finite depths (inf, -inf, NaN), unit and zero
    normals, zero and tiny albedos, HDR colour, standard errors of render-like size."""
    rng = np.random.default_rng(seed + 1000 * nx + ny)
    yy, xx = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    depth = (2.0 + 0.01 * xx + 0.02 * yy + 0.5 * (xx > nx // 2) + 0.05 * rng.random((ny, nx))).astype(np.float32)
    holes = rng.random((ny, nx))
    depth[holes < 0.06] = np.inf
    depth[(holes >= 0.06) & (holes < 0.08)] = -np.inf
    depth[(holes >= 0.08) & (holes < 0.10)] = np.nan
    n = rng.standard_normal((ny, nx, 3)) + np.array([0.0, 0.0, 3.0])
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    n[rng.random((ny, nx)) < 0.1] = 0.0  # medium events and misses
    alb = rng.random((ny, nx, 3))
    alb[rng.random((ny, nx)) < 0.1] = 0.0
    alb[rng.random((ny, nx)) < 0.05] = 1e-5
    lin = rng.random((ny, nx, 3)) * 0.8 + 0.3
    lin[rng.random((ny, nx)) < 0.02] *= 40.0  # fireflies
    se = lin * (0.05 + 0.3 * rng.random((ny, nx, 1)))
    f = np.float32
    return lin.astype(f), alb.astype(f), n.astype(f), depth, se.astype(f)


def _check(lin, alb, nrm, dep, se, **kw):
    got = denoise(lin, alb, nrm, dep, stderr=se, **kw)
    want_lin, want_rgb = ref.denoise(lin, alb, nrm, dep, stderr=se, **kw)
    assert np.all(np.isfinite(want_lin)), "the restatement produced non-finite values: the case is not comparable"
    diff = got["linear"].view(np.uint32) != want_lin.view(np.uint32)
    assert not diff.any(), "%d of %d values differ, e.g. at %s: %r vs %r" % (
        diff.sum(), diff.size, np.argwhere(diff)[0], got["linear"][diff][:4], want_lin[diff][:4])
    assert _same(got["rgb8"], want_rgb)
    return got


SIZES = [(1, 1), (1, 17), (37, 23), (130, 67)]


# ---- 1. bit for bit the restatement ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny", SIZES)
@pytest.mark.parametrize("with_se", [True, False])
@pytest.mark.parametrize("iterations", [0, 1, 3, 5, 10])
def test_synthetic_parity(nx, ny, with_se, iterations):
    lin, alb, nrm, dep, se = _synthetic(nx, ny)
    for npow in (0, 1, 128):
        _check(lin, alb, nrm, dep, se if with_se else None, iterations=iterations, normal_power=npow)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(sigma_l=0.0), dict(sigma_l=0.0, normal_power=1024), dict(sigma_z=0.0, eps_z=1e-6),
                                dict(albedo_min=0.5, eps_l=1e-3, sigma_l=1.0), dict(normal_power=2, sigma_z=7.5)])
def test_synthetic_parity_parameters(kw):
    lin, alb, nrm, dep, se = _synthetic(37, 23, seed=5)
    _check(lin, alb, nrm, dep, se, **kw)
    _check(lin, alb, nrm, dep, None, **kw)


def _render_planes(host, name, nx=96, ny=72, ns=16, flags=FC):
    if name == "lit_final_scene":
        cam, world = scenes_extra.build(host, name, nx, ny, seed=1)
    else:
        cam, world = scenes.build(host, name, nx, ny, seed=1)
    sc = host.lower(world).upload(0)
    noisy = sc.render_adaptive(cam, nx, ny, ns, min_spp=ns, step_spp=1, seed=SEED, flags=flags)
    ft = sc.render_features(cam, nx, ny, ns, seed=SEED, flags=flags)
    return sc, cam, noisy, ft


# cornell_smoke as the reference builds it shows the outside of its front wall; the corrected variant (the wall at the
# back) puts the two media in view
RENDERED = [("cornell_box", FC), ("cornell_smoke", FC), ("cornell_smoke_corrected", FC),
            ("random_spheres", FC | abi.RTMI_FLAG_SKY), ("lit_final_scene", FC)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,flags", RENDERED)
def test_render_output_parity(host, name, flags):
    _, _, noisy, ft = _render_planes(host, name, flags=flags)
    args = (noisy["linear"], ft["albedo"], ft["normal"], ft["depth"])
    _check(*args, noisy["stderr"])
    _check(*args, None, iterations=3)


@pytest.mark.gpu
def test_probe_expf_equals_restatement():
    x = ref.expf_sweep()
    out = np.empty_like(x)
    assert abi.load_rtmi().rtmi_probe_expf(0, x.ctypes.data, out.ctypes.data, x.size) == 0
    assert out.view(np.uint32).tobytes() == ref.expf(x).view(np.uint32).tobytes()


# ---- 2. properties ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_zero_iterations_copy_the_input():
    lin, alb, nrm, dep, se = _synthetic(37, 23, seed=2)
    got = denoise(lin, alb, nrm, dep, stderr=se, iterations=0)
    assert _same(got["linear"], lin) and _same(got["rgb8"], ref.quantise(lin))


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [1, 2, 5, 10])
def test_non_surface_pixels_come_through(iterations):
    lin, alb, nrm, dep, se = _synthetic(130, 67, seed=3)
    hole = ~np.isfinite(dep)
    got = denoise(lin, alb, nrm, dep, stderr=se, iterations=iterations)
    assert hole.sum() > 100
    assert got["linear"][hole].tobytes() == lin[hole].tobytes()
    assert not np.array_equal(got["linear"][~hole], lin[~hole])


@pytest.mark.gpu
def test_repeated_calls_agree():
    lin, alb, nrm, dep, se = _synthetic(130, 67, seed=4)
    a = denoise(lin, alb, nrm, dep, stderr=se)
    b = denoise(lin, alb, nrm, dep, stderr=se)
    assert _same(a["linear"], b["linear"]) and _same(a["rgb8"], b["rgb8"])


@pytest.mark.gpu
def test_render_denoised_is_its_three_calls(host):
    cam, world = scenes.build(host, "cornell_box", 64, 48, seed=1)
    sc = host.lower(world).upload(0)
    got = sc.render_denoised(cam, 64, 48, 8, denoise=dict(iterations=4, sigma_l=2.0), seed=SEED, flags=FC)
    noisy = sc.render_adaptive(cam, 64, 48, 8, min_spp=8, step_spp=1, seed=SEED, flags=FC)
    ft = sc.render_features(cam, 64, 48, 8, seed=SEED, flags=FC)
    want = denoise(noisy["linear"], ft["albedo"], ft["normal"], ft["depth"], stderr=noisy["stderr"], iterations=4,
                   sigma_l=2.0)
    assert _same(got["linear"], want["linear"]) and _same(got["rgb8"], want["rgb8"])
    assert _same(got["noisy"]["linear"], sc.render(cam, 64, 48, 8, seed=SEED, flags=FC)["linear"])
    assert _same(got["features"]["normal"], ft["normal"])
    with pytest.raises(ValueError):
        sc.render_denoised(cam, 64, 48, 1)


@pytest.mark.gpu
def test_render_is_unchanged_by_a_denoise(host):
    cam, world = scenes.build(host, "cornell_smoke", 64, 48, seed=1)
    sc = host.lower(world).upload(0)
    before = sc.render(cam, 64, 48, 8, seed=SEED, flags=FC)
    lin, alb, nrm, dep, se = _synthetic(130, 67, seed=6)
    denoise(lin, alb, nrm, dep, stderr=se)
    after = sc.render(cam, 64, 48, 8, seed=SEED, flags=FC)
    assert _same(before["linear"], after["linear"]) and _same(before["rgb8"], after["rgb8"])


@pytest.mark.gpu
def test_device_errors():
    lin, alb, nrm, dep, se = _synthetic(4, 3)
    p = abi.DenoiseParams(5, 128, 4.0, 1.0, 1e-10, 1e-3, 1e-3, 0)
    lib = abi.load_rtmi()
    out = np.empty_like(lin)
    rc = lib.rtmi_denoise(lib.rtmi_device_count(), 4, 3, C.byref(p), lin.ctypes.data, alb.ctypes.data, nrm.ctypes.data,
                          dep.ctypes.data, None, out.ctypes.data, None)
    assert rc == 3 and b"device" in lib.rtmi_last_error()


# ---- 3. quality ---------------------------------------------------------------------------------------------------------
def display_rmse(a, b):
    da = np.clip(np.sqrt(np.maximum(a.astype(np.float64), 0.0)), 0.0, 1.0)
    db = np.clip(np.sqrt(np.maximum(b.astype(np.float64), 0.0)), 0.0, 1.0)
    return float(np.sqrt(np.mean((da - db) ** 2)))


# measured on an MI355X: 0.459 (noisy 0.2598, denoised 0.1192).  Fixed seeds and a bit-exact filter make
# the ratio deterministic; the margin of 0.04 leaves room for changes to the renderer's noise, not to the filter.
QUALITY_BOUND = 0.5


@pytest.mark.gpu
def test_denoised_cornell_box_is_closer_to_the_converged_image(host):
    nx = ny = 128
    cam, world = scenes.build(host, "cornell_box", nx, ny, seed=1)
    sc = host.lower(world).upload(0)
    truth = sc.render(cam, nx, ny, 4096, seed=7, flags=FC)["linear"]
    got = sc.render_denoised(cam, nx, ny, 16, seed=SEED, flags=FC)
    noisy_rmse = display_rmse(got["noisy"]["linear"], truth)
    den_rmse = display_rmse(got["linear"], truth)
    print("cornell_box 128x128 16 spp: noisy RMSE %.5f, denoised %.5f, ratio %.3f" % (noisy_rmse, den_rmse,
                                                                                    den_rmse / noisy_rmse))
    assert den_rmse <= QUALITY_BOUND * noisy_rmse, (noisy_rmse, den_rmse)
