"""Independent numpy statement of csrc/vep/clahe.h (int64, whole arrays, a cumulative sum for the
scan), written from the header's text: the oracle of the CPU twin, which is the oracle of the kernels."""
import numpy as np


def luma(p):
    p = p.astype(np.int64)
    return (29 * p[..., 0] + 150 * p[..., 1] + 77 * p[..., 2] + 128) >> 8


def groups(side, tile):
    """[(first pixel, end pixel)] of the groups along a side, and each tile's group index."""
    n = -(-side // tile)
    edges = [(i * tile, min(side, (i + 1) * tile)) for i in range(n)]
    of = list(range(n))
    if n > 1 and 2 * (side - (n - 1) * tile) < tile:  # the thin last tile joins its neighbour
        edges[-2:] = [(edges[-2][0], side)]
        of[-1] = n - 2
    return edges, of


def lut_of(hist, n, clip16, strength):
    h = np.asarray(hist, np.int64)
    v = np.arange(256, dtype=np.int64)
    limit = max(1, clip16 * n // 4096)
    excess = int(np.maximum(h - limit, 0).sum())
    q, r = divmod(excess, 256)
    c = np.cumsum(np.minimum(h, limit) + q + ((((v + 1) * r) >> 8) > ((v * r) >> 8)))
    m = (c * 255 + n // 2) // n
    return ((v * (256 - strength) + m * strength + 128) >> 8).astype(np.uint8)


def luts(y, tile, clip16, strength):
    """(rows, cols, 256) uint8: every tile's LUT (its group's)."""
    h, w = y.shape
    (gx, ox), (gy, oy) = groups(w, tile), groups(h, tile)
    table = [[lut_of(np.bincount(y[y0:y1, x0:x1].ravel(), minlength=256), (y1 - y0) * (x1 - x0), clip16, strength)
              for x0, x1 in gx] for y0, y1 in gy]
    return np.array([[table[j][i] for i in ox] for j in oy], np.uint8)


def axis(side, tile):
    """(i0, i1, a) of every pixel along a side."""
    n = -(-side // tile)
    u = 2 * np.arange(side, dtype=np.int64) + 1 - tile
    i0 = np.where(u < 0, 0, u // (2 * tile))
    a = np.where(u < 0, 0, (u - i0 * 2 * tile) * 128 // tile)
    i1 = np.where(u < 0, 0, np.minimum(i0 + 1, n - 1))
    last = i0 >= n - 1
    return np.where(last, n - 1, i0), np.where(last, n - 1, i1), np.where(last, 0, a)


def corners(p, tile, clip16, strength):
    """Y, the four LUT values a, b, c, d of every pixel, and its weights ax, ay (all int64, (H, W))."""
    y = luma(p)
    t = luts(y, tile, clip16, strength).astype(np.int64)
    (i0, i1, ax), (j0, j1, ay) = axis(p.shape[1], tile), axis(p.shape[0], tile)
    J0, J1, AY = j0[:, None], j1[:, None], ay[:, None]
    return y, t[J0, i0[None], y], t[J0, i1[None], y], t[J1, i0[None], y], t[J1, i1[None], y], ax[None] + 0 * AY, AY + 0 * ax[None]


def clahe(p, tile=128, clip16=32, strength=256):
    y, a, b, c, d, ax, ay = corners(p, tile, clip16, strength)
    y2 = ((256 - ax) * (256 - ay) * a + ax * (256 - ay) * b + (256 - ax) * ay * c + ax * ay * d + 32768) >> 16
    return np.clip(p.astype(np.int64) + (y2 - y)[..., None], 0, 255).astype(np.uint8)
