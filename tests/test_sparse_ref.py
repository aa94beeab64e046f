"""The numpy restatement of the sparse renders' select and patch (tests/sparse_ref.py), without a GPU: the properties
include/rtmi_sparse.h states, which tests/test_gpu_sparse.py then holds the kernels to word for word."""
import numpy as np
import pytest

import sparse_ref as ref
from denoise_ref import quantise
from raytracing_rust_amd.host import _sparse_mask


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4095, 4096 * 3 + 3])
@pytest.mark.parametrize("density", [0.0, 0.05, 0.5, 1.0])
def test_select_is_ascending_with_both_counts(n, density):
    b = ref.plane(n, density, classes=(2, 3), seed=1)
    mask = ref.mask_of((2, 3))
    full, counts = ref.select(b, mask, n)
    assert counts[0] == counts[1] == full.size == int(((b == 2) | (b == 3)).sum())
    assert (np.diff(full.astype(np.int64)) > 0).all()
    assert set(full.tolist()) == set(np.flatnonzero((b == 2) | (b == 3)).tolist())
    if density == 0.0:
        assert full.size == 0
    if density == 1.0:
        assert full.size == n
    for cap in {1, max(full.size - 1, 1), max(full.size, 1)}:
        cut, c = ref.select(b, mask, cap)
        assert c[1] == full.size and c[0] == min(full.size, cap) == cut.size
        assert (cut == full[:cap]).all()  # the first `cap` in index order


def test_select_mask_rule():
    b = np.arange(256, dtype=np.uint8)
    for mask in (0, 1, 1 << 31, 0xFFFFFFFF, (1 << 3) | (1 << 31)):
        lst, counts = ref.select(b, mask, 256)
        assert lst.tolist() == [k for k in range(32) if (mask >> k) & 1]  # bytes of 32 and above are never selected
        assert counts.tolist() == [len(lst), len(lst)]
    assert ref.select(np.full(100, 3, np.uint8), 0, 100)[1].tolist() == [0, 0]  # accept_mask = 0 selects nothing
    assert ref.mask_of((3,)) == 8 and ref.mask_of((2, 3)) == 12 and ref.mask_of(()) == 0
    for classes in ((), (3,), (2, 3), (0, 31), tuple(range(32))):  # the package builds its masks the same way
        assert _sparse_mask(classes) == ref.mask_of(classes)


def test_patch_touches_only_listed_pixels():
    rng = np.random.default_rng(3)
    ny, nx = 23, 37
    lin = rng.random((ny, nx, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (ny, nx, 3), dtype=np.uint8)
    cls = rng.integers(0, 4, (ny, nx), dtype=np.uint8)
    lst = np.array([5, 850, 0, 400, 5, 10 ** 6, ny * nx], np.uint32)  # a repeat and two entries outside the planes
    mean = rng.random((lst.size, 3)).astype(np.float32) * 1.5
    mean[4] = mean[0]  # a repeat carries the same record
    mean[1, 0] = np.nan
    l2, r2, c2 = ref.patch(lst, None, mean, lin, rgb, cls, mark=4)
    inside = [5, 850, 0, 400]
    touched = np.zeros(ny * nx, bool)
    touched[inside] = True
    assert (l2.reshape(-1, 3)[~touched] == lin.reshape(-1, 3)[~touched]).all()
    assert (r2.reshape(-1, 3)[~touched] == rgb.reshape(-1, 3)[~touched]).all()
    assert (c2.reshape(-1)[~touched] == cls.reshape(-1)[~touched]).all()
    for k, p in enumerate(inside):
        assert l2.reshape(-1, 3)[p].tobytes() == mean[k].tobytes()
        assert (r2.reshape(-1, 3)[p] == quantise(mean[k])).all()
        assert c2.reshape(-1)[p] == 4
    assert r2.reshape(-1, 3)[850, 0] == 0  # NaN -> 0
    # the count cuts the list; each plane alone; the inputs are left alone
    l3, r3, c3 = ref.patch(lst, 2, mean, lin, None, None)
    assert r3 is None and c3 is None and (l3.reshape(-1, 3)[[0, 400]] == lin.reshape(-1, 3)[[0, 400]]).all()
    assert l3.reshape(-1, 3)[5].tobytes() == mean[0].tobytes()
    only = ref.patch(lst, None, mean, None, None, cls, mark=9)
    assert only[0] is None and only[1] is None and (only[2].reshape(-1)[inside] == 9).all()
    assert (cls < 4).all()
