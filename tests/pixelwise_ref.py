"""A numpy restatement of per-pixel adaptive sampling (include/rtmi_pixelwise.h), for the tests.

Input: every pixel's `cap` per-sample radiances, float32 [n_pixels, cap, 3].  They are widened to float64 and folded by a
plain loop over samples, vectorised over pixels: sum += x; d = x - m; m = m + d / k; M2 = M2 + d * (x - m).  At every count of
the lattice min_spp, min_spp + step_spp, ..., cap (the last step shortened) the pixels still active are tested alone:
mean = sum / n, e = sqrt(M2 / (n (n - 1))), converged iff in every channel e and mean are finite and e <= abs_tol + rel_tol
|mean|.  A pixel retires when converged or at n == cap, and stays retired."""
import numpy as np

from denoise_ref import quantise


def lattice(cap, min_spp, step_spp):
    """The counts at which pixels are tested."""
    assert 2 <= min_spp <= cap and step_spp >= 1
    return list(range(min_spp, cap, step_spp)) + [cap]


def fold(state, x, k):
    """One sample x [n, 3] (float64), the pixel's k-th (1-based), into state = (sum, m, M2), each [n, 3]; in place."""
    s, m, M2 = state
    with np.errstate(all="ignore"):
        s += x
        d = x - m
        m += d / float(k)
        M2 += d * (x - m)


def decide(state, n, abs_tol, rel_tol):
    """(mean f64 [n_pixels, 3], e f64 [n_pixels, 3], converged bool [n_pixels]) of the state after n samples."""
    s, _, M2 = state
    with np.errstate(all="ignore"):
        mean = s / float(n)
        e = np.sqrt(M2 / (float(n) * (float(n) - 1.0)))
        ok = np.isfinite(e) & np.isfinite(mean) & (e <= abs_tol + rel_tol * np.abs(mean))
    return mean, e, ok.all(axis=1)


def render(samples, min_spp, step_spp, abs_tol=0.0, rel_tol=0.0):
    """dict(spp u32 [n], linear f32 [n, 3], stderr f32 [n, 3], rgb8 u8 [n, 3], counts u32 [steps, 2]) of the samples
    float32 [n, cap, 3]; row k of counts is (traced, traced) of step k."""
    samples = np.asarray(samples, np.float32)
    n_pixels, cap, _ = samples.shape
    x = samples.astype(np.float64)
    state = tuple(np.zeros((n_pixels, 3)) for _ in range(3))
    active = np.ones(n_pixels, bool)
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
        active &= ~ok & (n < cap)
    c = np.array(counts, np.uint32)
    return {"spp": spp, "linear": linear, "stderr": stderr, "rgb8": rgb8, "counts": np.stack([c, c], axis=1)}


def step(list_, count, samples, state, n_pixels, n_done, decide_, cap, abs_tol, rel_tol, planes):
    """One launch of the step kernel.  list_: u32 [capacity]; count: entries or None; samples: f32 [capacity, pass, 3];
    state: f64 [9, n_pixels] (rows sum r g b | m r g b | M2 r g b), not read when n_done == 0; planes: dict of active u8 [n],
    linear f32 [n, 3], rgb8 u8 [n, 3], stderr f32 [n, 3], spp u32 [n] (each optional).  Returns (state, planes), copies; an
    entry whose pixel lies outside the planes is skipped."""
    lst = np.asarray(list_).astype(np.int64)
    samples = np.asarray(samples, np.float32)
    entries = lst.size if count is None else min(int(count), lst.size)
    state = np.array(state, np.float64, copy=True)
    planes = {k: np.array(v, copy=True) for k, v in planes.items()}
    keep = np.flatnonzero(lst[:entries] < n_pixels)
    px = lst[keep]
    if n_done == 0:
        st = tuple(np.zeros((px.size, 3)) for _ in range(3))
    else:
        st = tuple(state[3 * j:3 * j + 3, px].T.copy() for j in range(3))
    for s in range(samples.shape[1]):
        fold(st, samples[keep, s].astype(np.float64), n_done + s + 1)
    for j in range(3):
        state[3 * j:3 * j + 3, px] = st[j].T
    if decide_:
        n = n_done + samples.shape[1]
        mean, e, ok = decide(st, n, abs_tol, rel_tol)
        with np.errstate(all="ignore"):
            new = {"spp": np.full(px.size, n, np.uint32), "linear": mean.astype(np.float32), "stderr": e.astype(np.float32),
                   "rgb8": quantise(mean), "active": (~ok & (n < cap)).astype(np.uint8)}
        for k in planes:
            planes[k][px] = new[k]
    return state, planes
