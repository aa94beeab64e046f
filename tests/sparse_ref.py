"""A numpy restatement of the select and the patch of include/rtmi_sparse.h, for the tests.

select: pixel p is selected when its byte b satisfies b < 32 and (accept_mask >> b) & 1; the list holds the selected
indices in ascending order, the first `capacity` of them; counts = (written, selected).
patch: for each of the first min(count, capacity) entries k whose pixel p = list[k] lies inside the planes, linear[p] =
mean[k], rgb8[p] = the quantiser of tests/denoise_ref.py on mean[k], bytes[p] = mark; nothing else changes."""
import numpy as np

from denoise_ref import quantise


def mask_of(classes):
    m = 0
    for c in classes:
        assert 0 <= c < 32
        m |= 1 << c
    return m


def select(bytes_, accept_mask, capacity):
    b = np.asarray(bytes_, np.uint8).reshape(-1).astype(np.uint32)
    ok = (b < 32) & (((np.uint32(accept_mask) >> (b & 31)) & 1) == 1)
    idx = np.flatnonzero(ok).astype(np.uint32)
    return idx[:capacity], np.array([min(idx.size, capacity), idx.size], np.uint32)


def patch(list_, count, mean, linear=None, rgb8=None, bytes_=None, mark=4):
    """Patched copies (linear, rgb8, bytes) of the planes given; count = None: every entry of the list."""
    lst = np.asarray(list_).astype(np.int64).reshape(-1)
    entries = lst.size if count is None else min(int(count), lst.size)
    out = [None if a is None else np.array(a, copy=True) for a in (linear, rgb8, bytes_)]
    n_pixels = next(a.size // ch for a, ch in zip(out, (3, 3, 1)) if a is not None)
    flat = [None if a is None else a.reshape((-1, ch) if ch == 3 else (-1,)) for a, ch in zip(out, (3, 3, 1))]
    m = np.asarray(mean, np.float32).reshape(-1, 3)
    for k in range(entries):
        p = lst[k]
        if p >= n_pixels:
            continue
        if flat[0] is not None:
            flat[0][p] = m[k]
        if flat[1] is not None:
            flat[1][p] = quantise(m[k])
        if flat[2] is not None:
            flat[2][p] = mark
    return tuple(out)


def plane(n, density, classes=(3,), seed=0, others=(0, 1, 2, 31, 32, 255)):
    """n bytes: about `density` of them from `classes` (density 0 or 1: exactly none or all), the rest from `others`."""
    rng = np.random.default_rng(seed * 7919 + n)
    pick = rng.random(n) < density if 0.0 < density < 1.0 else np.full(n, density >= 1.0)
    keep = [o for o in others if o not in classes]
    return np.where(pick, rng.choice(np.array(classes, np.uint8), n), rng.choice(np.array(keep, np.uint8), n)).astype(np.uint8)
