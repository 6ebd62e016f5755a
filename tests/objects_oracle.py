"""numpy and plain Python oracle of the moving-object boxes, written from docs/OBJECTS.md section 1
(not from objects.h): int64 luma and decimation, morphology by explicit neighbourhood loops, labels
by breadth-first flood fill."""
from collections import deque

import numpy as np

BACKGROUND = 0xFFFFFFFF


def luma_plane(bgr, d):
    p = bgr.astype(np.int64)
    y = (29 * p[..., 0] + 150 * p[..., 1] + 77 * p[..., 2] + 128) >> 8
    h, w = y.shape[0] // d, y.shape[1] // d
    s = y[:h * d, :w * d].reshape(h, d, w, d).sum(axis=(1, 3))
    return (s + d * d // 2) >> (2 * {1: 0, 2: 1, 4: 2}[d])


def morph(m, radius, erode):
    """All (erode) or any of the (2 radius + 1)^2 neighbourhood; outside the plane is background."""
    h, w = m.shape
    out = np.zeros_like(m)
    for y in range(h):
        for x in range(w):
            vals = [bool(m[y + dy, x + dx]) if 0 <= y + dy < h and 0 <= x + dx < w else False
                    for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)]
            out[y, x] = all(vals) if erode else any(vals)
    return out


def mask(l0, lg, threshold, open, grow):
    m = np.abs(l0 - lg) > threshold
    if open:
        m = morph(morph(m, 1, True), 1, False)
    return morph(m, grow, False) if grow else m


def label(m):
    """The label plane: the smallest raster index of a sample's 8-connected component."""
    h, w = m.shape
    lab = np.full((h, w), BACKGROUND, np.int64)
    for sy in range(h):
        for sx in range(w):
            if not m[sy, sx] or lab[sy, sx] != BACKGROUND:
                continue
            lab[sy, sx] = sy * w + sx
            todo = deque([(sy, sx)])
            while todo:
                y, x = todo.popleft()
                for yy in range(max(y - 1, 0), min(y + 2, h)):
                    for xx in range(max(x - 1, 0), min(x + 2, w)):
                        if m[yy, xx] and lab[yy, xx] == BACKGROUND:
                            lab[yy, xx] = sy * w + sx
                            todo.append((yy, xx))
    return lab


def records(lab, min_area):
    """(n, 6) int64 of label, area, x0, y0, x1, y1 (exclusive), sorted by label."""
    out = []
    for v in np.unique(lab[lab != BACKGROUND]):
        ys, xs = np.nonzero(lab == v)
        if len(ys) >= min_area:
            out.append((v, len(ys), xs.min(), ys.min(), xs.max() + 1, ys.max() + 1))
    return np.array(out, np.int64).reshape(-1, 6)


def pack(m):
    """The packed mask: (h, ceil(w / 64)) uint64, bit x & 63 of word x >> 6."""
    h, w = m.shape
    out = np.zeros((h, (w + 63) // 64), np.uint64)
    for y, x in zip(*np.nonzero(m)):
        out[y, x >> 6] |= np.uint64(1) << np.uint64(x & 63)
    return out


def objects(newer, older, d, threshold, open, grow, min_area):
    m = mask(luma_plane(newer, d), luma_plane(older, d), threshold, open, grow)
    lab = label(m)
    return records(lab, min_area), lab, pack(m)


def pictures(m, d=1, extra=(0, 0)):
    """(newer, older) whose mask at decimate d, threshold 0, open 0, grow 0 is exactly m: newer grey 255
    where m is set, older all 0, every sample d x d pixels, `extra` trailing pixels the planes do not use."""
    up = np.repeat(np.repeat(m.astype(np.uint8) * 255, d, axis=0), d, axis=1)
    newer = np.zeros((up.shape[0] + extra[1], up.shape[1] + extra[0], 3), np.uint8)
    newer[:up.shape[0], :up.shape[1]] = up[..., None]
    return newer, np.zeros_like(newer)


def summarize(recs, d, max_objects, w, h):
    def px(lo, hi, side):
        a = min(lo * d, side)
        return a, min(hi * d, side) - a

    top = sorted(recs.tolist(), key=lambda r: (-r[1], r[0]))[:max_objects]
    objs = [{"label": r[0], "area": r[1], "box": [px(r[2], r[4], w)[0], px(r[3], r[5], h)[0], px(r[2], r[4], w)[1], px(r[3], r[5], h)[1]]}
            for r in top]
    box = None
    if len(recs):
        x, bw = px(int(recs[:, 2].min()), int(recs[:, 4].max()), w)
        y, bh = px(int(recs[:, 3].min()), int(recs[:, 5].max()), h)
        box = [x, y, bw, bh]
    return {"count": len(recs), "objects": objs, "truncated": len(recs) > max_objects, "area": int(recs[:, 1].sum()) if len(recs) else 0,
            "box": box, "motion": len(recs) >= 1}
