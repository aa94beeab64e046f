"""A numpy restatement of windowed adaptive sampling (include/rtmi_window.h), for the tests.

The lattice, the fold and the own-pixel test are those of tests/pixelwise_ref.py, imported unchanged.  What is added is the
rule that decides who is traced next: after the step that brought the live pixels to count n, fail = live & ~converged &
(n < cap), and a pixel stays live iff it is live and some pixel within the Chebyshev radius r of it, inside the image, fails.
`spread` states that by padded shifts: the fail plane is padded with r zeros on every side and the (2r + 1)^2 shifted views
are ORed, so a window is clipped at the border and never wraps into another row."""
import numpy as np

from denoise_ref import quantise
from pixelwise_ref import decide, fold, lattice


def spread(active, fail, nx, ny, r):
    """active' u8 [ny * nx] (bytes 1 / 0) of active, fail: arrays of ny * nx bytes in any shape, any non-zero byte set."""
    a = np.asarray(active).reshape(ny, nx) != 0
    f = np.zeros((ny + 2 * r, nx + 2 * r), bool)
    f[r:r + ny, r:r + nx] = np.asarray(fail).reshape(ny, nx) != 0
    near = np.zeros((ny, nx), bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            near |= f[dy:dy + ny, dx:dx + nx]
    return (a & near).astype(np.uint8).reshape(-1)


def render(samples, nx, ny, min_spp, step_spp, abs_tol=0.0, rel_tol=0.0, r=0):
    """dict(spp u32 [n], linear f32 [n, 3], stderr f32 [n, 3], rgb8 u8 [n, 3], counts u32 [steps, 2]) of the samples
    float32 [n = ny * nx, cap, 3], row-major from the top row; row k of counts is (traced, traced) of step k."""
    samples = np.asarray(samples, np.float32)
    n_pixels, cap, _ = samples.shape
    assert n_pixels == nx * ny
    x = samples.astype(np.float64)
    state = tuple(np.zeros((n_pixels, 3)) for _ in range(3))
    active = np.ones(n_pixels, bool)
    fail = np.zeros(n_pixels, np.uint8)  # never cleared: a pixel's last write is the 0 of its retirement
    spp = np.zeros(n_pixels, np.uint32)
    linear = np.zeros((n_pixels, 3), np.float32)
    stderr = np.zeros((n_pixels, 3), np.float32)
    rgb8 = np.zeros((n_pixels, 3), np.uint8)
    counts = []
    done = 0
    for n in lattice(cap, min_spp, step_spp):
        counts.append(int(active.sum()))
        for s in range(done, n):  # the retired pixels' state runs on unobserved: their planes are not written again
            fold(state, x[:, s], s + 1)
        done = n
        mean, e, ok = decide(state, n, abs_tol, rel_tol)
        with np.errstate(all="ignore"):
            spp[active] = n
            linear[active] = mean[active].astype(np.float32)
            stderr[active] = e[active].astype(np.float32)
            rgb8[active] = quantise(mean[active])
        fail[active] = (~ok & (n < cap))[active]
        active = spread(active, fail, nx, ny, r) != 0
    c = np.array(counts, np.uint32)
    return {"spp": spp, "linear": linear, "stderr": stderr, "rgb8": rgb8, "counts": np.stack([c, c], axis=1)}


# ---- the inputs the CPU and the GPU tests share -------------------------------------------------------------------------------
VIEW = ((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), 40.0)  # look_from, look_at, vertical fov of the box scenes
# name -> (scene, nx, ny, (min_spp, step_spp, cap), factor): abs_tol = factor * the median over pixels of the max-channel
# stderr at min_spp.  The plain estimator finds the lamp of a closed box by chance, so these start late (tests/test_gpu_pixelwise.py).
PLAIN_INPUTS = {"smoke-plain": ("lit_smoke", 16, 16, (16, 4, 36), 1.5), "cornell-plain": ("cornell_box", 13, 13, (64, 16, 144), 2.0)}


def tolerance(samples, min_spp, factor):
    """factor * median over pixels of the max-channel stderr after min_spp samples, of samples f32 [n, cap, 3]"""
    x = np.asarray(samples, np.float32).astype(np.float64)
    state = tuple(np.zeros((x.shape[0], 3)) for _ in range(3))
    for s in range(min_spp):
        fold(state, x[:, s], s + 1)
    _, e, _ = decide(state, min_spp, 0.0, 0.0)
    return factor * float(np.median(e.max(axis=1)))
