"""Float64 oracle of the model-input path: letterbox (BGR), letterbox_nv12 and nv12_to_chw.

numpy only and written from the definitions: it takes no constant and no function from the
package, so a slip in the kernels, in their CPU mirrors or in the torch references of ``ops`` cannot
hide in a shared helper. The one thing it re-derives step by step in float32 is the geometry
(``fill_letterbox_geometry``), because the fitted size is an integer decision; every sample value
after it is plain float64.

Sampling, per axis (align_corners=False): output o of n samples the source at
``s = max((o - pad + 0.5) * r - 0.5, 0)``, between ``i0 = floor(s)`` and ``i1 = min(i0 + 1, src - 1)``
with weight ``s - i0`` on ``i1``; ``r`` is the float32 ratio src / n widened to float64.
"""
from collections import namedtuple

import numpy as np

Geometry = namedtuple("Geometry", "nw nh pad_x pad_y rx ry")


def _lround(x):
    """std::lround of a non-negative float32: half away from zero (exact in float64)."""
    return int(np.floor(np.float64(x) + 0.5))


def geometry(src_w, src_h, S, even=False):
    """The centred aspect-preserving fit of src_w x src_h into S x S, as the launcher derives it:
    float32 scale and products, lround, and for ``even`` (NV12 output) the fitted size and the
    padding rounded down to chroma-sample boundaries. rx, ry: float32 ratios as float64."""
    f = np.float32
    scale = min(f(S) / f(src_w), f(S) / f(src_h))
    nw = max(1, min(S, _lround(f(src_w) * scale)))
    nh = max(1, min(S, _lround(f(src_h) * scale)))
    pad_x, pad_y = (S - nw) // 2, (S - nh) // 2
    if even:
        nw, nh = max(2, nw & ~1), max(2, nh & ~1)
        pad_x, pad_y = ((S - nw) // 2) & ~1, ((S - nh) // 2) & ~1
    return Geometry(nw, nh, pad_x, pad_y, float(f(src_w) / f(nw)), float(f(src_h) / f(nh)))


def is_exact(g):
    """Ratios at which every sample position, weight, product and partial sum of the fp32 kernels
    is exactly representable (weights are multiples of 1/4, samples are 8-bit integers), fused
    multiply-adds or not: there the kernels must reproduce the oracle with no tolerance at all."""
    return g.rx in (0.5, 1.0, 2.0, 4.0) and g.ry in (0.5, 1.0, 2.0, 4.0)


# fp32 error bound of one resampled value, in grey levels: the sample position s carries two
# roundings at magnitude <= src (2 * src * 2^-24), the weights inherit them, the picture's gradient
# is at most 255 per sample, and the four-term sum adds less than 255 * 2^-21.
#
# Measured on an MI355X against this oracle (cases of letterbox_checks.py; the same for the pad
# values 0, 114, 255). "share" = undecidable bytes among the picture's bytes, from the oracle
# alone (cap 5 %); "other" = undecidable bytes that took the neighbour of floor(v + 0.5); no other
# byte differed anywhere. "chw err" = max |got - ref| of the fp32 CHW planes (x 255 x std ~ 58 for
# grey levels): the kernel's real resampling error, e.g. 2.55e-5 -> 1.5e-3 levels at cif against
# delta = 1.07e-2. max |got - v| of the bytes themselves is the rounding's 0.5 (0.5009 at most).
#
#   case              delta     BGR share  other      chw err   NV12 share  other
#   identity          0         0          0          5.3e-7    0           0
#   down2             0         0          0          6.3e-7    0           0
#   down2-portrait    0         0          0          6.2e-7    0           0
#   down2-portrait40  0         0          0          6.3e-7    0           0
#   up2               0         0          0          6.8e-7    0           0
#   up2-portrait      0         0          0          6.8e-7    0           0
#   odd-crop          2.49e-3   0.645 %    1 / 3072   4.3e-6    0.104 %     0
#   cif               1.07e-2   2.875 %    38 / 12288 2.55e-5   2.644 %     14 / 6144
#   wide-crop         1.52e-2   2.292 %    0          6.8e-7    2.500 %     0
#   ragged-block      1.22e-2   0          0          5.3e-7    0           0
#   odd45 (NV12)      2.74e-3   -          -          -         0.812 %     4 / 6144
#   odd41 (NV12)      2.49e-3   -          -          -         0.625 %     0
#   worker 320x240    1.95e-2   0          0          5.3e-7    0           0
#   worker 144x176    1.07e-2   2.965 %    27 / 12288 1.2e-5    2.324 %     14 / 6144
#   worker 200x120    1.22e-2   2.344 %    4 / 12288  1.0e-5    2.467 %     0
#   worker High 10    1.07e-2   2.234 %    26 / 12288 5.1e-6    -           -
#
# (ragged-block, worker 320x240: ratio 5 puts every sample on a source pixel; wide-crop: ratios
# 3.90625 and 4 are exact in fp32. The rules do not rely on either.)
def delta(src_w, src_h):
    return 255.0 * max(src_w, src_h) * 2.0 ** -22


def _axis(n, r, src):
    """(i0, i1, l) of the n picture samples of one axis; float64."""
    s = np.maximum((np.arange(n, dtype=np.float64) + 0.5) * r - 0.5, 0.0)
    i0 = np.floor(s).astype(np.int64)
    assert i0.max() <= src - 1, "sample position outside the source"
    i1 = np.minimum(i0 + 1, src - 1)
    return i0, i1, s - i0


def _bilinear(P, oh, ow, ry, rx):
    """P [h, w, ...] float64 -> [oh, ow, ...]."""
    y0, y1, ly = _axis(oh, ry, P.shape[0])
    x0, x1, lx = _axis(ow, rx, P.shape[1])
    extra = (1,) * (P.ndim - 2)
    ly = ly.reshape((oh, 1) + extra)
    lx = lx.reshape((1, ow) + extra)
    top = (1.0 - lx) * P[y0][:, x0] + lx * P[y0][:, x1]
    bot = (1.0 - lx) * P[y1][:, x0] + lx * P[y1][:, x1]
    return (1.0 - ly) * top + ly * bot


def bt601_bgr(Y, U, V):
    """BT.601 limited range, the project's integer definition: 16.16 fixed point of
    1.164383 / 1.596027 / 0.391762 / 0.812968 / 2.017232, + 0.5 before the floor, clipped.
    Integer arrays in, int64 [..., 3] BGR out."""
    c = (Y.astype(np.int64) - 16) * 76309 + 32768
    d = U.astype(np.int64) - 128
    e = V.astype(np.int64) - 128
    r = (c + 104597 * e) >> 16
    g = (c - 25675 * d - 53279 * e) >> 16
    b = (c + 132201 * d) >> 16
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255)


def bgr_canvas(y, uv, src_w, src_h, crop_left, crop_top, S, pad):
    """float64 [S, S, 3] BGR canvas of ops.letterbox: every luma sample of the coded planes is
    converted with the chroma pair at (row >> 1, column & ~1) of its UNCROPPED position, then the
    window [crop_top, +src_h) x [crop_left, +src_w) is resized bilinearly; pad pixels = pad."""
    g = geometry(src_w, src_h, S, False)
    H, W = y.shape
    rows = np.arange(H) >> 1
    cols = np.arange(W) & ~1
    full = bt601_bgr(y, uv[rows][:, cols], uv[rows][:, cols + 1]).astype(np.float64)
    win = full[crop_top:crop_top + src_h, crop_left:crop_left + src_w]
    assert win.shape[:2] == (src_h, src_w), "window outside the planes"
    out = np.full((S, S, 3), float(pad), dtype=np.float64)
    out[g.pad_y:g.pad_y + g.nh, g.pad_x:g.pad_x + g.nw] = _bilinear(win, g.nh, g.nw, g.ry, g.rx)
    return out


def inside_mask(src_w, src_h, S, even=False):
    """bool [S, S]: True at picture (not pad) pixels."""
    g = geometry(src_w, src_h, S, even)
    m = np.zeros((S, S), dtype=bool)
    m[g.pad_y:g.pad_y + g.nh, g.pad_x:g.pad_x + g.nw] = True
    return m


def nv12_canvas(y, uv, src_w, src_h, crop_left, crop_top, S, pad):
    """float64 (luma [S, S], chroma [S/2, S/2, 2]) of ops.letterbox_nv12: the two planes are
    resized independently, on the even geometry. The chroma plane starts at
    (crop_top // 2, crop_left // 2), is ((src_h + 1) // 2) x ((src_w + 1) // 2) samples and is
    fitted into (nh / 2) x (nw / 2).

    Chroma is sampled with the LUMA ratios rx, ry, not with the ratio of the stored plane sizes:
    one chroma sample spans two luma samples, so the chroma plane of a src_w-wide picture covers
    src_w / 2 chroma samples of picture, also when src_w is odd and the plane stores
    (src_w + 1) / 2 of them. (src_w / 2) / (nw / 2) is the luma ratio. Deriving the scale from
    the stored sizes (as a generic resize call does) gives ((src_w + 1) // 2) / (nw // 2): the same
    for even sizes, but for 41 x 27 into 32 it is 1.3125 / 1.4 against 1.28125 / 1.35, which
    shifts the chroma against the luma towards the right / bottom edge.

    Pad luma = round(16 + pad * 219 / 255) (the limited-range code of grey level pad), pad
    chroma = 128."""
    g = geometry(src_w, src_h, S, True)
    Y = y[crop_top:crop_top + src_h, crop_left:crop_left + src_w].astype(np.float64)
    assert Y.shape == (src_h, src_w), "window outside the planes"
    luma = np.full((S, S), float(int(np.floor(16.0 + pad * 219.0 / 255.0 + 0.5))), dtype=np.float64)
    luma[g.pad_y:g.pad_y + g.nh, g.pad_x:g.pad_x + g.nw] = _bilinear(Y, g.nh, g.nw, g.ry, g.rx)
    ch, cw = (src_h + 1) // 2, (src_w + 1) // 2
    pairs = uv.reshape(uv.shape[0], uv.shape[1] // 2, 2)
    C = pairs[crop_top // 2:crop_top // 2 + ch, crop_left // 2:crop_left // 2 + cw].astype(np.float64)
    assert C.shape == (ch, cw, 2), "chroma window outside the plane"
    chroma = np.full((S // 2, S // 2, 2), 128.0, dtype=np.float64)
    py, px = g.pad_y // 2, g.pad_x // 2
    chroma[py:py + g.nh // 2, px:px + g.nw // 2] = _bilinear(C, g.nh // 2, g.nw // 2, g.ry, g.rx)
    return luma, chroma


def nv12_bytes(luma, chroma):
    """The two float64 planes in the layout of the op's output: [S*S] luma then [S*S/2] UV."""
    return np.concatenate([luma.reshape(-1), chroma.reshape(-1)])


def chw(canvas_bgr, mean, std):
    """float64 [3, S, S] RGB planes: (v / 255 - mean) / std per channel."""
    rgb = np.asarray(canvas_bgr, dtype=np.float64)[..., ::-1].transpose(2, 0, 1)
    m = np.asarray(mean, dtype=np.float64).reshape(3, 1, 1)
    s = np.asarray(std, dtype=np.float64).reshape(3, 1, 1)
    return (rgb / 255.0 - m) / s


def nv12_picture_bgr(batch_row, S):
    """One [S*S*3/2] NV12 picture -> int64 [S, S, 3] BGR (nearest chroma), for nv12_to_chw."""
    yp = batch_row[:S * S].reshape(S, S)
    uvp = batch_row[S * S:].reshape(S // 2, S)
    rows = np.arange(S) >> 1
    cols = np.arange(S) & ~1
    return bt601_bgr(yp, uvp[rows][:, cols], uvp[rows][:, cols + 1])
