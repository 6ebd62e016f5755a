"""Independent numpy implementations of the dehazing of docs/DEHAZE.md: `dehaze_int` follows the
document's integer arithmetic step by step (every plane is returned), `dehaze_float` is the same
pipeline in float64 without any rounding, and `hazy_scene` is the synthetic scene of the document's
numbers: coloured blocks with one dark channel each under a veil that thickens across the picture."""
import numpy as np


def window_min(v, r):
    """Minimum over the (2 r + 1)^2 window, clipped to the plane (padding with +inf)."""
    h, w = v.shape
    p = np.pad(v, r, constant_values=v.max())
    rows = np.min([p[:, k:k + w] for k in range(2 * r + 1)], axis=0)
    return np.min([rows[k:k + h] for k in range(2 * r + 1)], axis=0)


def box_sum(v, r):
    """Sum over the cells within r on both axes, clipped to the plane, and the count of them."""
    h, w = v.shape[:2]
    c = np.pad(v, [(r + 1, r), (r + 1, r)] + [(0, 0)] * (v.ndim - 2)).cumsum(0).cumsum(1)
    return c[2 * r + 1:, 2 * r + 1:] - c[:h, 2 * r + 1:] - c[2 * r + 1:, :w] + c[:h, :w]


def axis(n_pix, n_cell):
    """Per pixel: the two cells it lies between and the weight (in 1/8) of the second."""
    u = 2 * np.arange(n_pix) - 3
    i0 = np.where(u < 0, 0, u >> 3)
    wx = np.where(u < 0, 0, u & 7)
    edge = i0 >= n_cell - 1
    i0 = np.where(edge, n_cell - 1, i0)
    return i0, np.minimum(i0 + 1, n_cell - 1), np.where(edge, 0, wx)


def cell_sums(v, cw, ch):
    """Sums over cells of 4 x 4 pixels (the right and bottom ones partial)."""
    h, w = v.shape
    return np.pad(v, ((0, ch * 4 - h), (0, cw * 4 - w))).reshape(ch, 4, cw, 4).sum((1, 3))


def air_light(img, dark):
    """The walk from bin 255 down in whole bins -> (sums of B, G, R, count n)."""
    h, w = dark.shape
    target = max(1, w * h // 1000)
    count = np.bincount(dark.ravel(), minlength=256)
    above = count[::-1].cumsum()[::-1] - count  # pixels in the bins above v
    take = (above < target)[dark]
    return img[take].astype(np.int64).sum(0), int(take.sum())


def lerp(plane, i0, i1, wx, j0, j1, wy):
    wx, wy = wx[None, :], wy[:, None]
    return ((8 - wx) * (8 - wy) * plane[j0][:, i0] + wx * (8 - wy) * plane[j0][:, i1] + (8 - wx) * wy * plane[j1][:, i0] +
            wx * wy * plane[j1][:, i1])


def dehaze_int(img, patch, omega, t0, radius, strength):
    """img (H, W, 3) uint8; omega in 1/256, t0 in 1/1024, strength in 1/256 -> dict of every plane."""
    h, w = img.shape[:2]
    i = img.astype(np.int64)
    r = patch // 2
    dark = window_min(i.min(2), r)
    table = np.zeros((256, 4), np.int64)
    np.add.at(table, dark.ravel(), np.concatenate([np.ones((h * w, 1), np.int64), i.reshape(-1, 3)], 1))
    s, n = air_light(i, dark)
    air = np.maximum(1, (s + n // 2) // n)
    norm = np.minimum(255, (255 * np.arange(256)[None, :] + air[:, None] // 2) // air[:, None])
    dn = window_min(np.min([norm[c][i[..., c]] for c in range(3)], axis=0), r)
    t_raw = 1024 - (4 * omega * dn + 127) // 255
    y = (29 * i[..., 0] + 150 * i[..., 1] + 77 * i[..., 2] + 128) >> 8
    cw, ch = -(-w // 4), -(-h // 4)
    cnt = cell_sums(np.ones((h, w), np.int64), cw, ch)
    yc = (4 * cell_sums(y, cw, ch) + cnt // 2) // cnt
    tc = (cell_sums(t_raw, cw, ch) + cnt // 2) // cnt
    k = box_sum(np.ones((ch, cw), np.int64), radius)
    sy, st, syt, syy = (box_sum(v, radius) for v in (yc, tc, yc * tc, yc * yc))
    den = k * syy - sy * sy + 1024 * k * k
    a = (1024 * (k * syt - sy * st) + den // 2) // den  # (numpy's // is the floor division)
    b = (1024 * st - a * sy + k // 2) // k
    mean_a, mean_b = (box_sum(a, radius) + k // 2) // k, (box_sum(b, radius) + k // 2) // k
    ax, ay = axis(w, cw), axis(h, ch)
    t = np.clip((lerp(mean_a, *ax, *ay) * 4 * y + lerp(mean_b, *ax, *ay) + 32768) >> 16, t0, 1024)
    recip = ((1 << 22) + t // 2) // t
    j = np.clip(air + (((i - air) * recip[..., None] + 2048) >> 12), 0, 255)
    out = (i * (256 - strength) + j * strength + 128) >> 8
    return {"table": table, "air": np.append(air, n), "norm": norm, "cell": yc | tc << 16, "ab": np.stack([a, b], 2),
            "mean": np.stack([mean_a, mean_b], 2), "t": t, "out": out.astype(np.uint8)}


def dehaze_float(img, patch, omega, t0, radius, strength):
    """The same pipeline in float64, nothing rounded: omega, t0, strength as fractions ->
    (out float (H, W, 3), t (H, W), air (3,))."""
    h, w = img.shape[:2]
    i = img.astype(np.float64)
    r = patch // 2
    s, n = air_light(img, window_min(img.min(2).astype(np.int64), r))
    air = np.maximum(1.0, s / n)
    t_raw = 1 - omega * window_min(np.minimum(1.0, i / air).min(2), r)
    y = (29 * i[..., 0] + 150 * i[..., 1] + 77 * i[..., 2]) / 256
    cw, ch = -(-w // 4), -(-h // 4)
    cnt = cell_sums(np.ones((h, w)), cw, ch)
    yc, tc = cell_sums(y, cw, ch) / cnt, cell_sums(t_raw, cw, ch) / cnt
    k = box_sum(np.ones((ch, cw)), radius)
    my, mt, myt, myy = (box_sum(v, radius) / k for v in (yc, tc, yc * tc, yc * yc))
    a = (myt - my * mt) / (myy - my * my + 1024 / 16)  # (eps: 1024 in luma of 1/4 levels squared)
    b = mt - a * my
    ax, ay = axis(w, cw), axis(h, ch)
    t = np.clip(lerp(box_sum(a, radius) / k, *ax, *ay) / 64 * y + lerp(box_sum(b, radius) / k, *ax, *ay) / 64, t0, 1.0)
    j = np.clip((i - air) / t[..., None] + air, 0, 255)
    return i * (1 - strength) + j * strength, t, air


def hazy_scene(w=160, h=96, air=(230, 225, 220), t_lo=0.35, t_hi=0.9, block=8, seed=7):
    """-> (haze-free scene, hazy picture, true t per column): blocks of `block` pixels, each with
    one channel dark (0..20) and two bright ones, under I = J t + A (1 - t)."""
    rng = np.random.default_rng(seed)
    by, bx = -(-h // block), -(-w // block)
    cols = rng.integers(60, 256, (by, bx, 3))
    cols[np.arange(by)[:, None], np.arange(bx)[None, :], rng.integers(0, 3, (by, bx))] = rng.integers(0, 21, (by, bx))
    clear = np.kron(cols, np.ones((block, block, 1), np.int64))[:h, :w].astype(np.float64)
    t = np.linspace(t_lo, t_hi, w)
    hazy = clear * t[None, :, None] + np.array(air, np.float64) * (1 - t[None, :, None])
    return clear.astype(np.uint8), np.rint(hazy).astype(np.uint8), t
