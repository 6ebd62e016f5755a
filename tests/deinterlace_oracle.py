"""Motion-adaptive deinterlacing in numpy, written from the definition in docs/DEINTERLACE.md and
not from csrc/vep/deinterlace.h: whole-picture array arithmetic in int64. Also the moving-bar scene
of the quality tests."""
import numpy as np


def luma(bgr):
    b, g, r = (bgr[..., c].astype(np.int64) for c in range(3))
    return (29 * b + 150 * g + 77 * r + 128) >> 8


def deinterlace(newer, older=None, order="tff", temporal=True):
    """The woven frame ``newer`` (H, W, 3) deinterlaced, against ``older`` where given."""
    f = newer.astype(np.int64)
    h, w = f.shape[:2]
    p = {"tff": 0, "bff": 1}[order]
    rows = np.arange(h)
    up = np.where(rows == 0, 1, rows - 1)
    dn = np.where(rows == h - 1, h - 2, rows + 1)
    yf = luma(newer)
    cols = np.arange(w)

    def at(x):
        return np.clip(x, 0, w - 1)

    def score(j):
        return sum(np.abs(yf[up][:, at(cols + k + j)] - yf[dn][:, at(cols + k - j)]) for k in (-1, 0, 1))

    best, pick = score(0) - 1, np.zeros((h, w), np.int64)
    for sign in (-1, 1):
        s1, s2 = score(sign), score(2 * sign)
        take1 = s1 < best
        take2 = take1 & (s2 < s1)
        pick = np.where(take2, 2 * sign, np.where(take1, sign, pick))
        best = np.where(take2, s2, np.where(take1, s1, best))
    ra, rb = up[:, None], dn[:, None]
    out = (f[ra, at(cols[None] + pick)] + f[rb, at(cols[None] - pick)]) >> 1
    if older is not None and temporal:
        g = older.astype(np.int64)
        t = np.abs(luma(older) - yf)
        diff = np.maximum(t >> 1, (t[up] + t[dn]) >> 1)[..., None]
        d = (g + f) >> 1
        out = np.clip(out, d - diff, d + diff)
    out[rows % 2 == p] = f[rows % 2 == p]
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def bar_scene(w=96, h=48, order="tff", speed=6, seed=5):
    """A textured background with a bright vertical bar moving right by ``speed`` pixels a frame,
    rendered at t - 1/2, t and t + 1/2 and woven into two frames of the given field order.
    -> (newer, older, truth): the frame whose earlier field shows t, the frame before it (whose
    later field shows t - 1/2), and the progressive picture at t."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    back = (96 + 40 * np.sin(xx / 5.0) * np.cos(yy / 7.0))[..., None] + rng.integers(-6, 7, (h, w, 3))

    def render(t2):  # t2: time in half frames
        pic = back.copy()
        x0 = 10 + (speed * t2) // 2
        pic[:, x0:x0 + 9] = (235, 225, 215)
        return np.clip(pic, 0, 255).astype(np.uint8)

    p = {"tff": 0, "bff": 1}[order]
    fields = [render(t2) for t2 in range(4)]  # t - 1, t - 1/2, t, t + 1/2

    def weave(early, late):
        out = early.copy()
        out[1 - p::2] = late[1 - p::2]
        return out

    return weave(fields[2], fields[3]), weave(fields[0], fields[1]), fields[2]


def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
