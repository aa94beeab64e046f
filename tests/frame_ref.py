"""numpy restatement of the frame pipeline's un-tiling (include/rtmi_frame.h, step 3).

The lit render leaves its image tiled: texel = tile * 64 + ly * 8 + lx, 8x8 tiles counted row by row from the top-left, the
tiles of the right and bottom edges padded to 8x8.  A texel is four 32-bit words (r, g, b as floats, then rgb8 with
RTMI_TEXEL_POISON in bit 31); its standard errors are three floats at the same index.  The un-tiling copies the texels
of the pixels inside the image to packed row-major planes, bit for bit, and counts the poisoned ones among them."""
import numpy as np

TILE = 8
POISON = 0x80000000


def tiles(nx, ny):
    return (nx + TILE - 1) // TILE, (ny + TILE - 1) // TILE


def texel_count(nx, ny):
    tx, ty = tiles(nx, ny)
    return tx * ty * TILE * TILE


def tiled_index(nx, ny):
    """int64 [ny, nx]: the index of each pixel's texel in the tiled buffers."""
    tx, _ = tiles(nx, ny)
    y, x = np.meshgrid(np.arange(ny, dtype=np.int64), np.arange(nx, dtype=np.int64), indexing="ij")
    return ((y // TILE) * tx + x // TILE) * (TILE * TILE) + (y % TILE) * TILE + x % TILE


def untile(nx, ny, texels, tiled_stderr=None):
    """texels: uint32 [texel_count, 4]; tiled_stderr: float32 [texel_count, 3] or None.  Returns (linear float32
    [ny, nx, 3], stderr float32 [ny, nx, 3] or None, the number of in-image texels with the poison bit)."""
    texels = np.asarray(texels)
    assert texels.dtype == np.uint32 and texels.shape == (texel_count(nx, ny), 4)
    k = tiled_index(nx, ny)
    linear = np.ascontiguousarray(texels[k][..., :3]).view(np.float32)
    poisoned = int(np.count_nonzero(texels[k][..., 3] & np.uint32(POISON)))
    se = None
    if tiled_stderr is not None:
        tiled_stderr = np.asarray(tiled_stderr)
        assert tiled_stderr.dtype == np.float32 and tiled_stderr.shape == (texel_count(nx, ny), 3)
        se = np.ascontiguousarray(tiled_stderr[k])
    return linear, se, poisoned


def padding_texels(nx, ny):
    """The indices of the texels that belong to no pixel (the padding of the edge tiles), sorted."""
    used = np.zeros(texel_count(nx, ny), bool)
    used[tiled_index(nx, ny).ravel()] = True
    return np.flatnonzero(~used)
