"""Independent oracle of the crops (docs/CROPS.md §1). Numpy int64 and Python ints only; nothing
from the package.

It is written in another shape than csrc/vep/crop.h: an axis is a dense integer weight matrix
``o x s`` whose rows sum to ``D``, and a crop is ``Wy @ plane @ Wx.T`` in int64 with one rounding
division by ``Dx * Dy``.
"""
import numpy as np

UNIT = 10000
MAX_OUT = 4096
PAD = (114, 114, 114)


def axis_matrix(s: int, o: int):
    """(D, W): W[j, i] = weight of source sample i in output j."""
    W = np.zeros((o, s), np.int64)
    if o <= s:  # area average on an axis of s * o units
        D = s
        for j in range(o):
            for i in range(j * s // o, ((j + 1) * s - 1) // o + 1):
                W[j, i] = min((i + 1) * o, (j + 1) * s) - max(i * o, j * s)
    else:  # bilinear, half-pixel centres, clamped edges
        D = 2 * o
        for j in range(o):
            t = (2 * j + 1) * s - o
            if t <= 0:
                W[j, 0] = D
                continue
            i0, f = divmod(t, D)
            if i0 >= s - 1:
                W[j, s - 1] = D
            else:
                W[j, i0] = D - f
                W[j, i0 + 1] = f
    assert (W.sum(axis=1) == D).all() and (W >= 0).all()
    return D, W


def taps(s: int, o: int):
    """(D, [(j, i, w)]) as native.crop_taps lists them: the taps the definition names, in order (an
    enlarging axis names its second tap even where its weight is 0)."""
    D, W = axis_matrix(s, o)
    out = []
    for j in range(o):
        if o <= s:
            idx = range(j * s // o, ((j + 1) * s - 1) // o + 1)
        else:
            t = (2 * j + 1) * s - o
            i0 = t // D
            idx = [0] if t <= 0 else [s - 1] if i0 >= s - 1 else [i0, i0 + 1]
        out += [(j, i, int(W[j, i])) for i in idx]
    return D, out


def to_pixels(w: int, h: int, box):
    """(x0, y0, x1, y1) in pixels, rounded outward, never empty, inside the picture."""
    def axis(n, a, b):
        p0, p1 = a * n // UNIT, min(n, -(-b * n // UNIT))
        p0 = max(0, min(p0, n - 1))
        return p0, max(p1, p0 + 1)
    x0, x1 = axis(w, box["x0"], box["x1"])
    y0, y1 = axis(h, box["y0"], box["y1"])
    return x0, y0, x1, y1


def rect_box(w: int, h: int, x0: int, y0: int, x1: int, y1: int) -> dict:
    """The box whose pixel rect in a w x h picture (w, h <= 5000) is [x0, x1) x [y0, y1)."""
    b = {"x0": -(-x0 * UNIT // w), "y0": -(-y0 * UNIT // h), "x1": x1 * UNIT // w, "y1": y1 * UNIT // h}
    assert to_pixels(w, h, b) == (x0, y0, x1, y1), (w, h, x0, y0, x1, y1, b)
    return b


WHOLE = {"x0": 0, "y0": 0, "x1": UNIT, "y1": UNIT}


def fitted(sw: int, sh: int, W: int, H: int, fit: str = "stretch"):
    """(x, y, fw, fh) of the resampled rect in the W x H output."""
    if fit == "stretch":
        return 0, 0, W, H
    assert fit == "letterbox"
    if sw * H >= sh * W:
        fw, fh = W, max(1, min(H, (2 * sh * W + sw) // (2 * sw)))
    else:
        fw, fh = max(1, min(W, (2 * sw * H + sh) // (2 * sh))), H
    return (W - fw) // 2, (H - fh) // 2, fw, fh


def resample(rect: np.ndarray, ow: int, oh: int) -> np.ndarray:
    sh, sw = rect.shape[:2]
    Dx, Wx = axis_matrix(sw, ow)
    Dy, Wy = axis_matrix(sh, oh)
    out = np.empty((oh, ow, 3), np.int64)
    for c in range(3):
        out[:, :, c] = Wy @ rect[:, :, c].astype(np.int64) @ Wx.T
    den = Dx * Dy
    out = (out + den // 2) // den
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def crop_resize(img: np.ndarray, boxes, W: int, H: int, fit: str = "stretch", pad=PAD) -> np.ndarray:
    h, w = img.shape[:2]
    assert img.dtype == np.uint8 and img.shape[2] == 3 and 1 <= W <= MAX_OUT and 1 <= H <= MAX_OUT
    out = np.empty((len(boxes), H, W, 3), np.uint8)
    for k, b in enumerate(boxes):
        x0, y0, x1, y1 = to_pixels(w, h, b)
        fx, fy, fw, fh = fitted(x1 - x0, y1 - y0, W, H, fit)
        out[k] = np.array(pad, np.uint8)
        out[k, fy:fy + fh, fx:fx + fw] = resample(img[y0:y1, x0:x1], fw, fh)
    return out


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


SMALL = [(7, 5), (17, 9), (1, 9), (9, 1), (64, 48), (200, 120)]
SIZES = [(1, 1), (3, 3), (7, 5), (16, 16), (112, 112), (224, 224)]
PADS = [PAD, (1, 2, 250)]


def boxes_of(w: int, h: int) -> list:
    """The whole picture, one pixel, rects starting at x = 1, 2, 3, 5 with widths 1..8, 21, 37, every
    edge and corner."""
    out = [dict(WHOLE), rect_box(w, h, w // 2, h // 2, w // 2 + 1, h // 2 + 1)]
    ya, yb = (1, h - 1) if h > 2 else (0, h)
    for x0 in (1, 2, 3, 5):
        for bw in (1, 2, 3, 4, 5, 6, 7, 8, 21, 37):
            if x0 + bw <= w:
                out.append(rect_box(w, h, x0, ya, x0 + bw, yb))
    ew, eh = max(1, w // 3), max(1, h // 3)
    for cx in (0, w - ew):
        for cy in (0, h - eh):
            out.append(rect_box(w, h, cx, cy, cx + ew, cy + eh))
    out += [rect_box(w, h, 0, 0, w, eh), rect_box(w, h, 0, h - eh, w, h), rect_box(w, h, 0, 0, ew, h),
            rect_box(w, h, w - ew, 0, w, h)]
    return out


def cases(w: int, h: int):
    """(boxes, W, H, fit, pad) covering boxes_of x (SIZES + the rect's size +- 1 on each axis), both
    fits and two pad colours, grouped into few calls: every call takes up to 64 boxes of one
    output size."""
    boxes = boxes_of(w, h)
    by_size = {}
    for k, b in enumerate(boxes):
        x0, y0, x1, y1 = to_pixels(w, h, b)
        sw, sh = x1 - x0, y1 - y0
        sizes = set((a, c) for a in (sw - 1, sw, sw + 1) for c in (sh - 1, sh, sh + 1) if a >= 1 and c >= 1)
        sizes |= set(SIZES[:4]) | (set(SIZES[4:]) if k < 2 or k % 7 == 0 else set())
        for s in sizes:
            by_size.setdefault(s, []).append(b)
    out = []
    for n, ((W, H), bs) in enumerate(sorted(by_size.items())):
        for at in range(0, len(bs), 64):
            out.append((bs[at:at + 64], W, H, "stretch", PADS[0]))
            out.append((bs[at:at + 64], W, H, "letterbox", PADS[n & 1]))
    return out


# enlarge-only shapes of the outside comparison: ((sw, sh), (ow, oh))
ENLARGE = [((5, 7), (16, 16)), ((9, 17), (112, 112)), ((3, 3), (224, 224)), ((37, 21), (64, 48)), ((1, 9), (5, 40)),
           ((9, 1), (40, 5)), ((48, 64), (49, 65)), ((20, 30), (1024, 31))]
