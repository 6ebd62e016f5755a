"""Independent oracle of the area-average downscale and the wall geometry (docs/WALL.md).

Numpy int64 and Python ints only; nothing from the package. The resampling is written in another
shape than csrc/vep/scale.h: instead of per-sample overlap weights it integrates. A row of ``s``
samples resampled to ``o`` is a step function on an axis of ``s * o`` units, sample ``i`` covering
``[i * o, (i + 1) * o)``. ``F(X)``, its integral from 0 to the integer ``X``, is

    F(X) = o * P[X // o] + (X % o) * a[X // o]        (P = exclusive prefix sums of a)

and output ``j``, which covers ``[j * s, (j + 1) * s)``, is ``F((j + 1) * s) - F(j * s)``. The two
axes are separable and exact in integers; one rounding division by ``sw * sh`` follows.
"""
import math

import numpy as np

BACKGROUND = 16
UNSET = 65535


def _integrate(a: np.ndarray, o: int, axis: int) -> np.ndarray:
    """Sums of the step function of ``a`` along ``axis`` over the ``o`` output intervals."""
    a = np.moveaxis(a.astype(np.int64), axis, 0)
    s = a.shape[0]
    zero = np.zeros((1,) + a.shape[1:], np.int64)
    prefix = np.concatenate([zero, np.cumsum(a, axis=0)])  # P[i] = a[0] + ... + a[i - 1]
    padded = np.concatenate([a, zero])                      # a[s] = 0: F(s * o) needs no sample
    X = np.arange(o + 1, dtype=np.int64) * s
    q, r = X // o, X % o
    shape = (-1,) + (1,) * (a.ndim - 1)
    F = o * prefix[q] + r.reshape(shape) * padded[q]
    return np.moveaxis(np.diff(F, axis=0), 0, axis)


def resize_area(img: np.ndarray, ow: int, oh: int, rows_per_step: int = 256) -> np.ndarray:
    sh, sw = img.shape[:2]
    assert img.dtype == np.uint8 and img.shape[2] == 3 and 1 <= ow <= sw and 1 <= oh <= sh
    # x axis in steps of rows (bounds the int64 temporaries of a large picture), then the y axis
    horiz = np.concatenate([_integrate(img[y:y + rows_per_step], ow, 1) for y in range(0, sh, rows_per_step)])
    total = _integrate(horiz, oh, 0)
    den = sw * sh
    out = (total + den // 2) // den
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def fit(sw: int, sh: int, bw=None, bh=None):
    """(ow, oh) of sw x sh fitted into the box bw x bh, never enlarged (a side not given: 65535)."""
    bw = UNSET if not bw else bw
    bh = UNSET if not bh else bh
    if bw >= sw and bh >= sh:
        return sw, sh
    if sw * bh >= sh * bw:
        ow = min(bw, sw)
        return ow, max(1, min((2 * sh * ow + sw) // (2 * sw), min(bh, sh)))
    oh = min(bh, sh)
    return max(1, min((2 * sw * oh + sh) // (2 * sh), min(bw, sw))), oh


def wall_geometry(n: int, cols=None, tw: int = 320, th: int = 180):
    """(cols, rows, canvas_w, canvas_h)"""
    if not cols:
        cols = math.isqrt(n - 1) + 1 if n > 1 else 1  # ceil(sqrt(n))
    rows = -(-n // cols)
    return cols, rows, cols * tw, rows * th


def place(t: int, cols: int, tw: int, th: int, sw: int, sh: int):
    """(x, y, w, h) of tile t's picture in the canvas."""
    ow, oh = fit(sw, sh, tw, th)
    return (t % cols) * tw + (tw - ow) // 2, (t // cols) * th + (th - oh) // 2, ow, oh


def compose_wall(frames, cols, tw: int, th: int) -> np.ndarray:
    cols, rows, cw, ch = wall_geometry(len(frames), cols, tw, th)
    canvas = np.full((ch, cw, 3), BACKGROUND, np.uint8)
    for t, f in enumerate(frames):
        if f is None:
            continue
        x, y, w, h = place(t, cols, tw, th, f.shape[1], f.shape[0])
        canvas[y:y + h, x:x + w] = resize_area(f, w, h)
    return canvas


def picture(kind: str, w: int, h: int, seed: int = 0) -> np.ndarray:
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "noise":
        img = np.random.default_rng(w * 7919 + h + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif kind == "gradient":
        img = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 255 // max(w + h - 2, 1)],
                       -1).astype(np.uint8)
    elif kind == "checkerboard":
        img = np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[..., None], 3, -1)
    elif kind == "white":
        img = np.full((h, w, 3), 255, np.uint8)
    else:
        img = np.full((h, w, 3), 77, np.uint8)
    return np.ascontiguousarray(img)


KINDS = ["noise", "gradient", "checkerboard", "constant"]
# (sw, sh, ow, oh): identity, integer ratios, one output sample, non-integer ratios both ways,
# nearly 1:1, single-column and single-row sources
SMALL_SHAPES = [(7, 5, 7, 5), (48, 32, 8, 8), (64, 48, 1, 1), (17, 9, 5, 4), (33, 17, 32, 16), (200, 120, 199, 119),
                (1, 9, 1, 4), (9, 1, 4, 1)]
# the 32-bit accumulator's bound: 255 * 4112 * 4096 < 2^32 <= 255 * 4113 * 4096
BOUNDARY_SHAPES = [(4112, 4096, 8, 8), (4113, 4096, 8, 8)]
