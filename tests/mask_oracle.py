"""Independent numpy oracle of the privacy masks, written from the specification alone (not from
csrc/vep/mask.cpp): slices and means.

A mask is a dict {x0, y0, x1, y1, mode, block, b, g, r}; coordinates in 1/10000 of the picture's
width and height, rounded OUTWARD to pixels:
    px0 = x0 * W // 10000, px1 = (x1 * W + 9999) // 10000   (the same for y)
never empty, never outside the picture. `fill` sets the rect to (b, g, r). `pixelate` cuts the rect
into B x B blocks anchored at (px0, py0), partial at the right and bottom, and sets every pixel of
a block, per channel, to (sum + n // 2) // n with n the block's pixel count. Masks apply in list
order, each on the picture the earlier ones left.
"""
import numpy as np


def to_pixels(w, h, m):
    def axis(n, a, b):
        p0, p1 = a * n // 10000, (b * n + 9999) // 10000
        p1 = min(p1, n)
        p0 = max(0, min(p0, n - 1))
        return p0, max(p1, p0 + 1)

    x0, x1 = axis(w, m["x0"], m["x1"])
    y0, y1 = axis(h, m["y0"], m["y1"])
    return x0, y0, x1, y1


def apply(picture, masks):
    """A new (H, W, 3) uint8 array: `masks` applied in order to `picture`."""
    out = np.array(picture, dtype=np.uint8, copy=True)
    h, w = out.shape[:2]
    for m in masks:
        x0, y0, x1, y1 = to_pixels(w, h, m)
        if m.get("mode", "pixelate") == "fill":
            out[y0:y1, x0:x1] = (m.get("b", 0), m.get("g", 0), m.get("r", 0))
            continue
        B = m.get("block", 16)
        for by in range(y0, y1, B):
            for bx in range(x0, x1, B):
                blk = out[by:min(by + B, y1), bx:min(bx + B, x1)]
                n = blk.shape[0] * blk.shape[1]
                s = blk.reshape(n, 3).astype(np.int64).sum(axis=0)
                blk[...] = ((s + n // 2) // n).astype(np.uint8)
    return out


def levels(w, h, masks):
    """level(k) = 1 + the largest level of the earlier masks whose pixel rects intersect mask k's,
    0 when none does."""
    rects = [to_pixels(w, h, m) for m in masks]
    out = []
    for k, (x0, y0, x1, y1) in enumerate(rects):
        lv = 0
        for e in range(k):
            ex0, ey0, ex1, ey1 = rects[e]
            if x0 < ex1 and ex0 < x1 and y0 < ey1 and ey0 < y1:
                lv = max(lv, out[e] + 1)
        out.append(lv)
    return out


def rect_mask(w, h, px0, py0, px1, py1, strict=True, **kw):
    """A mask whose pixel rect on a w x h picture is exactly [px0, px1) x [py0, py1): the pixel
    edges are scaled up with ceilings for the lower and floors for the upper bound, which the
    outward rounding maps back (checked here). Above 5000 pixels a side a pixel is narrower than
    two units and some rects have no such mask: an error, or None with strict=False."""
    def lo(p, n):
        return -((-p * 10000) // n)

    def hi(p, n):
        return p * 10000 // n

    m = {"x0": lo(px0, w), "y0": lo(py0, h), "x1": hi(px1, w), "y1": hi(py1, h)}
    m.update(kw)
    m.setdefault("mode", "pixelate")
    m.setdefault("block", 16)
    for k in ("b", "g", "r"):
        m.setdefault(k, 0)
    if not strict and (m["x0"] >= m["x1"] or m["y0"] >= m["y1"] or to_pixels(w, h, m) != (px0, py0, px1, py1)):
        return None
    assert to_pixels(w, h, m) == (px0, py0, px1, py1), (to_pixels(w, h, m), (px0, py0, px1, py1))
    return m


def rects(w, h):
    """The pixel rects every picture size is tested with (those that fit it), without repeats:
    the whole picture; one pixel; rects that start at x = 1, 2, 3 (modulo 4) and whose rows end at
    every byte offset modulo 4; a rect smaller than any block; every edge and every corner."""
    out = [(0, 0, w, h), (w // 2, h // 2, w // 2 + 1, h // 2 + 1), (w - 1, h - 1, w, h), (0, 0, 1, 1)]
    for x0 in (1, 2, 3, 5):
        for wd in (1, 2, 3, 4, 5, 6, 7, 8, 21, 37):  # x1 = x0 + wd runs through every residue modulo 4
            out.append((x0, 1, x0 + wd, min(h, 1 + 6)))
    out.append((2, 1, 5, 4))                       # 3 x 3: smaller than the smallest block
    qx, qy = max(1, w // 3), max(1, h // 3)
    out += [(0, qy, qx, h - qy), (w - qx, qy, w, h - qy), (qx, 0, w - qx, qy), (qx, h - qy, w - qx, h),  # edges
            (0, 0, qx, qy), (w - qx, 0, w, qy), (0, h - qy, qx, h), (w - qx, h - qy, w, h),              # corners
            (1, 1, w - 1, h - 1), (3, 0, w, h), (0, 0, w - 3, h)]
    seen, keep = set(), []
    for r in out:
        x0, y0, x1, y1 = r
        if 0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h and r not in seen:
            seen.add(r)
            keep.append(r)
    return keep


def cases(w, h, blocks=(4, 16, 128)):
    """One mask per rect of rects(w, h) and per way of masking: fill, and pixelate at each block size."""
    out = []
    for k, r in enumerate(rects(w, h)):
        if rect_mask(w, h, *r, strict=False) is None:
            continue
        out.append(rect_mask(w, h, *r, mode="fill", b=(k * 40 + 7) % 256, g=(k * 90 + 1) % 256, r=255 - k % 256))
        for b in blocks:
            out.append(rect_mask(w, h, *r, mode="pixelate", block=b))
    return out


KINDS = ("noise", "gradient", "uniform", "checker")


def picture(kind, w, h, seed=0):
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "gradient":
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([(x * 3 + seed) % 256, (y * 5 + x) % 256, (x + y * 7) % 256], axis=-1).astype(np.uint8)
    if kind == "uniform":
        return np.full((h, w, 3), (seed * 37 + 90) % 256, dtype=np.uint8)
    if kind == "checker":  # period 1: 0 / 255 alternating in x and y
        y, x = np.mgrid[0:h, 0:w]
        return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, axis=-1)
    raise ValueError(kind)
