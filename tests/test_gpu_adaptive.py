"""Adaptive sampling (include/rtmi_adaptive.h) on the device.

The whole test story rests on one property: a pixel's samples come from Philox streams keyed by (seed, sample, pixel)
and are summed in sample order, so a tile that retires with n samples is bit for bit the same tile of an ordinary
render with ns = n, in linear and in rgb8.  The decisions are pinned through the API itself: a tile that stopped at k
is converged at k (an adaptive run starting at k stops it there), one that went on from k - step was not."""
import numpy as np
import pytest

import scenes_extra
from raytracing_rust_amd import abi, scenes
from raytracing_rust_amd.host import HostError

NX, NY, NS, MIN, STEP = 160, 120, 128, 16, 16
FC = abi.RTMI_FLAG_FAST_CULL


def _scene(host, name, nx=NX, ny=NY):
    flags = FC
    if name == "lit_final_scene":
        cam, world = scenes_extra.build(host, name, nx, ny, seed=1)
    else:
        cam, world = scenes.build(host, name, nx, ny, seed=1)
        if name == "random_spheres":
            flags |= abi.RTMI_FLAG_SKY
    return cam, host.lower(world).upload(0), flags


def _tile_max(a, nx, ny):
    """per 8x8 tile, the maximum of a [ny,nx,3] plane over its pixels and channels (row 0 = top row, as the outputs)"""
    ty, tx = (ny + 7) // 8, (nx + 7) // 8
    pad = np.full((ty * 8, tx * 8, 3), -np.inf)
    pad[:ny, :nx] = a
    return pad.reshape(ty, 8, tx, 8, 3).max(axis=(1, 3, 4))


def _mixed_tolerance(sc, cam, flags):
    """abs_tol at half the median tile noise after MIN samples: some tiles stop early, some run to the cap"""
    st = sc.render_adaptive(cam, NX, NY, MIN, MIN, STEP, seed=42, flags=flags)
    return 0.5 * float(np.median(_tile_max(st["stderr"].astype(np.float64), NX, NY)))


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_box", "lit_final_scene", "random_spheres"])
def test_tiles_equal_fixed_renders_and_decisions_are_pinned(host, name):
    cam, sc, flags = _scene(host, name)
    tol = _mixed_tolerance(sc, cam, flags)
    ad = sc.render_adaptive(cam, NX, NY, NS, MIN, STEP, abs_tol=tol, seed=42, flags=flags)
    spp = ad["spp"]
    counts = sorted(set(int(k) for k in np.unique(spp)))
    print(name, "abs_tol %.4g" % tol, "counts", {k: int((spp == k).sum()) for k in counts}, "samples", ad["stats"]["samples"])
    assert len(counts) >= 3, counts
    assert all(k in range(MIN, NS + 1, STEP) for k in counts), counts
    for k in counts:
        m = spp == k
        # tile equivalence: linear and rgb8 of a tile that stopped at k are those of render(ns = k)
        ref = sc.render(cam, NX, NY, k, seed=42, flags=flags)
        assert _same(ad["linear"][m], ref["linear"][m]), (name, k)
        assert _same(ad["rgb8"][m], ref["rgb8"][m]), (name, k)
        # statistics only at n = k: the same image and, for the tiles that stopped at k, the same standard errors
        so = sc.render_adaptive(cam, NX, NY, k, k, STEP, abs_tol=tol, seed=42, flags=flags)
        assert _same(so["linear"], ref["linear"]) and _same(so["rgb8"], ref["rgb8"]), (name, k)
        assert _same(ad["stderr"][m], so["stderr"][m]), (name, k)
        if k < NS:  # converged at k: a run that starts at k stops those tiles there
            at_k = sc.render_adaptive(cam, NX, NY, NS, k, STEP, abs_tol=tol, seed=42, flags=flags)
            assert np.all(at_k["spp"][m] == k), (name, k)
        if k > MIN:  # not converged at k - step: a run that starts there goes on with those tiles
            before = sc.render_adaptive(cam, NX, NY, NS, k - STEP, STEP, abs_tol=tol, seed=42, flags=flags)
            assert np.all(before["spp"][m] > k - STEP), (name, k)
    assert ad["stats"]["samples"] == int(spp.astype(np.uint64).sum())
    assert ad["stats"]["samples"] < NX * NY * NS


@pytest.mark.gpu
def test_statistics_only_is_the_plain_render_in_one_pass_or_many(host):
    cam, sc, flags = _scene(host, "cornell_box")
    ns = 40
    plain = sc.render(cam, NX, NY, ns, seed=42, flags=flags)
    one = sc.render_adaptive(cam, NX, NY, ns, ns, 1, seed=42, flags=flags)
    per_sample = ((NX + 7) // 8) * ((NY + 7) // 8) * 64 * abi.RTMI_SAMPLE_SLOT_BYTES
    many = sc.render_adaptive(cam, NX, NY, ns, ns, 1, seed=42, flags=flags, sample_buffer_bytes=per_sample * 3)
    for out in (one, many):
        assert _same(out["linear"], plain["linear"]) and _same(out["rgb8"], plain["rgb8"])
        assert np.all(out["spp"] == ns) and out["stats"]["samples"] == NX * NY * ns
    assert _same(one["stderr"], many["stderr"])
    assert np.all(np.isfinite(one["stderr"])) and one["stderr"].max() > 0
    # sub-passes inside steps: the same adaptive render with a buffer of 3 samples per tile
    tol = float(np.median(one["stderr"]))
    a = sc.render_adaptive(cam, NX, NY, 64, 8, 8, abs_tol=tol, seed=42, flags=flags)
    b = sc.render_adaptive(cam, NX, NY, 64, 8, 8, abs_tol=tol, seed=42, flags=flags, sample_buffer_bytes=per_sample * 3)
    for key in ("linear", "rgb8", "stderr", "spp"):
        assert _same(a[key], b[key]), key


@pytest.mark.gpu
def test_estimator_is_exact_on_a_two_valued_light(host):
    """A DiffuseLight sphere seen directly against black, no sky: every sample is 0 or e exactly, so with h = sum / e
    hits out of n the standard error is e * sqrt(h (n - h) / n / (n (n - 1))); Welford's rounding stays far below the
    fp32 output's, so the output is within one fp32 ulp of it.  Interior and background pixels: exactly 0."""
    nx = ny = 64
    n = 64
    e = np.array([4.0, 2.0, 0.5])
    world = host.HittableList()
    world.push(host.Sphere((0.0, 0.0, 0.0), 1.0, host.DiffuseLight(host.SolidTexture(*e))))
    cam = host.Camera((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, nx / ny, 0.0, 5.0, 0.0, 1.0)
    sc = host.lower(world).upload(0)
    out = sc.render_adaptive(cam, nx, ny, n, n, 1, seed=42)
    lin = out["linear"].astype(np.float64)
    h = np.rint(lin * n / e)  # hits: sum = h * e exactly, mean = sum / n
    assert np.all(np.abs(h * e / n - lin) <= 1e-6 * e)
    want = e * np.sqrt(h * (n - h) / n / (n * (n - 1.0)))
    se = out["stderr"].astype(np.float64)
    edge = (h > 0) & (h < n)
    assert edge.sum() > 30 and (h == 0).sum() > 100 and (h == n).sum() > 100
    assert np.all(np.abs(se[edge] - want[edge]) <= 2.0 ** -23 * want[edge])
    assert np.all(se[~edge] == 0.0)


@pytest.mark.gpu
def test_zero_variance_retires_every_tile_at_min_spp(host):
    cam, sc, flags = _scene(host, "final_scene")
    out = sc.render_adaptive(cam, NX, NY, 1000, 4, 16, seed=42, flags=flags)
    assert np.all(out["spp"] == 4) and np.all(out["stderr"] == 0.0)
    assert out["stats"]["samples"] == NX * NY * 4
    ref = sc.render(cam, NX, NY, 4, seed=42, flags=flags)
    assert _same(out["linear"], ref["linear"]) and _same(out["rgb8"], ref["rgb8"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_box", "random_spheres"])
def test_independent_of_kernel_culling_and_repetition(host, name):
    cam, sc, flags = _scene(host, name)
    base = flags & ~FC
    tol = _mixed_tolerance(sc, cam, flags)
    runs = [sc.render_adaptive(cam, NX, NY, 96, 8, 8, abs_tol=tol, rel_tol=0.01, seed=7, flags=f)
            for f in (base | FC, base | FC, base, base | FC | abi.RTMI_FLAG_SYNC, base | abi.RTMI_FLAG_SYNC)]
    kernels = [r["stats"]["kernel"] for r in runs]
    assert kernels[3] == kernels[4] == abi.RTMI_KERNEL_PERLANE, kernels
    if name == "random_spheres":  # (cornell_box's instanced boxes take the per-lane kernel in adaptive mode)
        assert kernels[0] == abi.RTMI_KERNEL_WAVE_COOP, kernels
    for r in runs[1:]:
        for key in ("linear", "rgb8", "stderr", "spp"):
            assert _same(r[key], runs[0][key]), key
    assert len(np.unique(runs[0]["spp"])) >= 2


@pytest.mark.gpu
def test_accounting_and_progress(host):
    cam, sc, flags = _scene(host, "cornell_box")
    seen = []
    tol = _mixed_tolerance(sc, cam, flags)
    out = sc.render_adaptive(cam, NX, NY, NS, MIN, STEP, abs_tol=tol, seed=42, flags=flags,
                             progress=lambda d, t: seen.append((d, t)) and False)
    tiles = ((NX + 7) // 8) * ((NY + 7) // 8)
    assert seen and seen[-1] == (tiles * NS, tiles * NS)
    assert [d for d, _ in seen] == sorted(d for d, _ in seen) and all(d <= t for d, t in seen)
    assert out["stats"]["samples"] == int(out["spp"].astype(np.uint64).sum())
    with pytest.raises(HostError, match="cancelled"):
        sc.render_adaptive(cam, NX, NY, NS, MIN, STEP, abs_tol=tol, seed=42, flags=flags, progress=lambda d, t: True)
    # the handle stays usable after a cancelled call
    again = sc.render_adaptive(cam, NX, NY, NS, MIN, STEP, abs_tol=tol, seed=42, flags=flags)
    assert _same(again["linear"], out["linear"]) and _same(again["spp"], out["spp"])
