"""The numpy restatement of include/rtmi_temporal.h (tests/temporal_ref.py) against known answers, without a GPU, so that
the device (tests/test_gpu_temporal.py) is not merely compared with a twin: running means and their variance under a
standing camera, exact pixel shifts of a plane under a translated camera, the depth, normal and behind-the-camera
rejections, the history cap, alpha_min, reset and the pass-through cases."""
import numpy as np
import pytest

import temporal_ref as ref
from raytracing_rust_amd import abi

F = np.float32
NX, NY = 128, 128
FROM, AT = (278.0, 278.0, -800.0), (278.0, 278.0, 0.0)  # cornell_box's camera; its back wall is 1355 away
WALL = 1355.0


def _camera(shift=(0.0, 0.0, 0.0), at=AT, nx=NX, ny=NY):
    lf = tuple(a + b for a, b in zip(FROM, shift))
    la = tuple(a + b for a, b in zip(at, shift))
    return ref.pinhole(lf, la, aspect=nx / ny)


def _pixel_shift(cam, k, distance, nx=NX):
    """the world translation along `horizontal` that moves a plane at `distance` by k pixels"""
    hor = np.array(list(cam.horizontal), np.float64)
    focus = 10.0
    return tuple(k * (np.linalg.norm(hor) / nx) * (distance / focus) * hor / np.linalg.norm(hor))


def _frames(k, nx=NX, ny=NY, seed=0):
    rng = np.random.default_rng(seed)
    f = []
    for _ in range(k):
        lin = (rng.random((ny, nx, 3)) * 0.8 + 0.3).astype(F)
        se = (lin * (0.05 + 0.3 * rng.random((ny, nx, 1)))).astype(F)
        f.append((lin, se))
    alb = (rng.random((ny, nx, 3)) * 0.9 + 0.05).astype(F)
    nrm = np.zeros((ny, nx, 3), F)
    nrm[..., 2] = -1.0
    return f, alb, nrm


def _flat(nx=NX, ny=NY, value=1.0):
    lin = np.full((ny, nx, 3), value, F)
    nrm = np.zeros((ny, nx, 3), F)
    nrm[..., 2] = -1.0
    return lin, nrm


@pytest.mark.parametrize("K,max_history", [(1, 32), (8, 32), (12, 5)])
def test_standing_camera_is_the_running_mean(K, max_history):
    nx, ny = 40, 24
    cam = _camera(nx=nx, ny=ny)
    frames, alb, nrm = _frames(K, nx, ny)
    z = ref.plane_depth(cam, nx, ny, WALL)
    z[3, 5] = np.inf
    z[7, 9] = np.nan
    surf = np.isfinite(z)
    t = ref.Temporal(nx, ny, max_history=max_history)
    for n, (lin, se) in enumerate(frames):
        out = t.push(cam, lin, alb, nrm, z, stderr=se)
        assert not out["motion"].any()
        assert np.all(out["history"][surf] == min(n + 1, max_history)) and np.all(out["history"][~surf] == 0)
        assert out["linear"][~surf].tobytes() == lin[~surf].tobytes() and out["stderr"][~surf].tobytes() == se[~surf].tobytes()
    if K > max_history:
        return  # past the cap the blend is an exponential average, not the mean
    a = np.fmax(alb, F(1e-3)).astype(np.float64)
    xs = np.stack([lin.astype(np.float64) / a for lin, _ in frames])
    es = np.stack([se.astype(np.float64) / a for _, se in frames])
    got_x = out["linear"].astype(np.float64) / a
    got_e = out["stderr"].astype(np.float64) / a
    err_x = np.abs(got_x - xs.mean(axis=0))[surf] / np.abs(xs).max(axis=0)[surf]
    err_e = np.abs(got_e - np.sqrt((es * es).sum(axis=0)) / K)[surf] / es.max(axis=0)[surf]
    print("K=%d: mean within %.3g, stderr within %.3g of the largest frame value (bound %.3g)" % (
        K, err_x.max(), err_e.max(), ref.mean_bound(K)))
    assert err_x.max() <= ref.mean_bound(K) and err_e.max() <= ref.mean_bound(K)


def test_no_demodulate_first_push_is_the_input():
    nx, ny = 23, 11
    cam = _camera(nx=nx, ny=ny)
    frames, alb, nrm = _frames(1, nx, ny, seed=3)
    lin, se = frames[0]
    alb[2, 3] = 0.0
    z = ref.plane_depth(cam, nx, ny, WALL)
    out = ref.Temporal(nx, ny, demodulate=False).push(cam, lin, alb, nrm, z, stderr=se)
    assert out["linear"].tobytes() == lin.tobytes() and out["stderr"].tobytes() == se.tobytes()
    assert np.all(out["history"] == 1)
    dem = ref.Temporal(nx, ny).push(cam, lin, alb, nrm, z, stderr=se)  # x/a'*a' is the input only up to rounding
    assert np.allclose(dem["linear"], lin, rtol=3e-7, atol=0) and dem["linear"].tobytes() != lin.tobytes()


# fp32 against the exact shift: 2.7e-4 px measured on this geometry at 128x128; the bound is 4 times that, for both
# coordinates (the same fp32 evaluation gives fx and fr, so motion.y is 0 to the same accuracy)
SHIFT_BOUND = 1e-3


@pytest.mark.parametrize("k", [1, 3, -1, -3, 2.5])
def test_translated_camera_shifts_a_plane_by_whole_pixels(k):
    cam0 = _camera()
    cam1 = _camera(_pixel_shift(cam0, k, WALL))
    lin, nrm = _flat()
    z = ref.plane_depth(cam0, NX, NY, WALL)
    t = ref.Temporal(NX, NY)
    t.push(cam0, lin, lin, nrm, z)
    out = t.push(cam1, lin, lin, nrm, ref.plane_depth(cam1, NX, NY, WALL))
    ex, ey = np.abs(out["motion"][..., 0] - k).max(), np.abs(out["motion"][..., 1]).max()
    print("shift %g px: motion.x off by at most %.3g px, motion.y by %.3g px" % (k, ex, ey))
    assert ex <= SHIFT_BOUND and ey <= SHIFT_BOUND
    # a column whose source lies a pixel or more outside the image restarts; the column whose source is the first
    # position outside (within the fp32 error of the guard's edge) may go either way; every other column continues
    src = np.arange(NX) + k
    gone = (src >= NX + 0.5) | (src <= -1.5)
    edge = ~gone & ((src >= NX - 0.5) | (src <= -0.5)) & (np.abs(src - np.round(src)) < 0.25)
    hist = out["history"]
    assert np.all(hist[:, gone] == 1) and gone.sum() == {1: 0, 3: 2, 2.5: 2}[abs(k)]
    assert np.all(hist[:, ~gone & ~edge] == 2) and np.all((hist[:, edge] == 1) | (hist[:, edge] == 2))
    assert np.all(out["linear"] == 1.0)


def test_a_depth_step_stops_the_taps_and_disoccluded_pixels_restart():
    """Left half: a near plane (value 1); right half: the back wall, 1.5 times as far (value 100).  The camera moves one
    wall pixel, so the near plane moves 1.5: the near pixels next to the step look up wall pixels (rejected: they
    restart), the one before straddles the step and must take its near tap only."""
    cam0 = _camera()
    cam1 = _camera(_pixel_shift(cam0, 1, WALL))
    near = WALL / 1.5
    half = NX // 2
    lin, nrm = _flat()
    lin[:, half:] = 100.0

    def depth(cam):
        z = ref.plane_depth(cam, NX, NY, WALL)
        z[:, :half] = ref.plane_depth(cam, NX, NY, near)[:, :half]
        return z

    t = ref.Temporal(NX, NY)
    t.push(cam0, lin, np.ones_like(lin), nrm, depth(cam0))
    out = t.push(cam1, lin, np.ones_like(lin), nrm, depth(cam1))
    m = out["motion"][..., 0]
    assert np.abs(m[:, :half] - 1.5).max() <= 2 * SHIFT_BOUND and np.abs(m[:, half:] - 1.0).max() <= SHIFT_BOUND
    hist = out["history"]
    assert np.all(hist[:, half - 1] == 1)  # both taps on the wall: disoccluded
    assert np.all(hist[:, half - 2] == 2)  # taps half-1 (near) and half (wall): only the near one is used
    assert np.all(hist[:, :half - 2] == 2) and np.all(hist[:, half:NX - 2] == 2)
    assert np.all(out["linear"][:, :half] == 1.0) and np.all(out["linear"][:, half:] == 100.0)  # nothing mixed across
    # with the tolerance opened the straddling pixel mixes in the wall
    t = ref.Temporal(NX, NY, depth_tol=1.0)
    t.push(cam0, lin, np.ones_like(lin), nrm, depth(cam0))
    mixed = t.push(cam1, lin, np.ones_like(lin), nrm, depth(cam1))
    assert np.all(mixed["linear"][:, half - 2] > 10.0) and np.all(mixed["history"][:, half - 1] == 2)


def test_normal_rejection_and_zero_normals():
    nx, ny = 16, 4
    cam = _camera(nx=nx, ny=ny)
    lin, nrm = _flat(nx, ny)
    z = ref.plane_depth(cam, nx, ny, WALL)
    turned = nrm.copy()
    turned[:, 0:4] = (1.0, 0.0, 0.0)      # 90 degrees: rejected
    turned[:, 4:8] = (0.0, 0.0, 0.0)      # zero now: accepted
    c = np.cos(np.radians(25.0))          # 25 degrees: cos = 0.906 >= 0.9, accepted
    turned[:, 8:12] = (np.sin(np.radians(25.0)), 0.0, -c)
    c = np.cos(np.radians(27.0))          # 27 degrees: cos = 0.891 < 0.9, rejected
    turned[:, 12:14] = (np.sin(np.radians(27.0)), 0.0, -c)
    first = nrm.copy()
    first[:, 14:16] = 0.0                 # zero then: accepted
    t = ref.Temporal(nx, ny, normal_min=0.9)
    t.push(cam, lin, lin, first, z)
    out = t.push(cam, lin, lin, turned, z)
    assert out["history"][0].tolist() == [1] * 4 + [2] * 4 + [2] * 4 + [1] * 2 + [2] * 2
    # unnormalised normals: the test is on the cosine, not on the dot product
    t = ref.Temporal(nx, ny, normal_min=0.9)
    t.push(cam, lin, lin, first * F(3.0), z)
    out = t.push(cam, lin, lin, turned * F(0.25), z)
    assert out["history"][0].tolist() == [1] * 4 + [2] * 4 + [2] * 4 + [1] * 2 + [2] * 2


def test_same_camera_depth_change_restarts():
    nx, ny = 8, 2
    cam = _camera(nx=nx, ny=ny)
    lin, nrm = _flat(nx, ny)
    z = np.full((ny, nx), 100.0, F)
    z2 = z.copy()
    z2[:, :2] = 104.0  # within 5 %
    z2[:, 2:4] = 106.0  # beyond
    z2[:, 4] = np.inf
    t = ref.Temporal(nx, ny)
    t.push(cam, lin, lin, nrm, z)
    out = t.push(cam, lin, lin, nrm, z2)
    assert out["history"][0].tolist() == [2, 2, 1, 1, 0, 2, 2, 2]
    out = t.push(cam, lin, lin, nrm, z)  # the pixel that was no surface is no source
    assert out["history"][0].tolist() == [3, 3, 1, 1, 1, 3, 3, 3]


def test_max_history_alpha_min_and_reset():
    nx, ny = 6, 3
    cam = _camera(nx=nx, ny=ny)
    frames, alb, nrm = _frames(6, nx, ny, seed=9)
    z = ref.plane_depth(cam, nx, ny, WALL)
    t = ref.Temporal(nx, ny, max_history=3)
    hist = [t.push(cam, lin, alb, nrm, z, stderr=se)["history"][0, 0] for lin, se in frames]
    assert hist == [1, 2, 3, 3, 3, 3]
    t.reset()
    again = t.push(cam, *frames[0][:1], alb, nrm, z)  # a first push, and the stderr choice is open again
    assert np.all(again["history"] == 1) and again["stderr"] is None
    with pytest.raises(ValueError):
        t.push(cam, frames[1][0], alb, nrm, z, stderr=frames[1][1])
    # alpha_min = 1: every push is a copy of its input (up to the demodulation's rounding: none without it)
    t = ref.Temporal(nx, ny, alpha_min=1.0, demodulate=False)
    for n, (lin, se) in enumerate(frames):
        out = t.push(cam, lin, alb, nrm, z, stderr=se)
        assert out["linear"].tobytes() == lin.tobytes() and out["stderr"].tobytes() == se.tobytes()
        assert np.all(out["history"] == min(n + 1, 32))
    # reset: the same bits as a fresh history
    fresh = ref.Temporal(nx, ny)
    t = ref.Temporal(nx, ny)
    for lin, se in frames[:3]:
        t.push(cam, lin, alb, nrm, z, stderr=se)
    t.reset()
    for lin, se in frames[3:]:
        a, b = t.push(cam, lin, alb, nrm, z, stderr=se), fresh.push(cam, lin, alb, nrm, z, stderr=se)
        assert all(a[k].tobytes() == b[k].tobytes() for k in ("linear", "stderr", "history", "motion"))


def test_a_point_behind_the_previous_camera_has_no_history():
    cam0 = _camera()
    behind = ref.pinhole(FROM, (278.0, 278.0, -1600.0))  # the previous camera looked the other way
    lin, nrm = _flat()
    z = ref.plane_depth(cam0, NX, NY, WALL)
    t = ref.Temporal(NX, NY)
    t.push(behind, lin, lin, nrm, z)
    out = t.push(cam0, lin, lin, nrm, z)
    assert np.all(out["history"] == 1) and not out["motion"].any()


def test_camera_inverse_inverts_and_refuses_singular_cameras():
    cam = _camera((3.0, -2.0, 5.0), at=(100.0, 300.0, 0.0))
    m = ref.camera_inverse(cam).astype(np.float64)
    cols = np.stack([np.array(list(cam.horizontal), np.float64), np.array(list(cam.vertical), np.float64),
                     np.array(list(cam.lower_left_corner), np.float64) - np.array(list(cam.origin), np.float64)], axis=1)
    assert np.abs(m @ cols - np.eye(3)).max() < 1e-6
    flat = _camera()
    flat.vertical = flat.horizontal
    with pytest.raises(ValueError):
        ref.camera_inverse(flat)
    assert abi.RTMI_TEMPORAL_NO_DEMODULATE == 1
