"""The temporal denoise of docs/DENOISE.md, section 1, in plain numpy int64: written from the text,
not from csrc/vep/denoise.h. frames: (K, H, W, 3) uint8, frames[0] the newest."""
import numpy as np


def luma(p):
    p = p.astype(np.int64)
    return (29 * p[..., 0] + 150 * p[..., 1] + 77 * p[..., 2] + 128) >> 8


def denoise(frames, level=8, strength=256):
    """-> (picture (H, W, 3) uint8, weights (K, H, W) int64)."""
    f = np.asarray(frames).astype(np.int64)
    k, h, w = f.shape[:3]
    y = luma(f)
    weights = np.empty((k, h, w), np.int64)
    weights[0] = 16
    for i in range(1, k):
        ad = np.pad(np.abs(y[0] - y[i]), 1, mode="edge")
        d = sum(ad[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
        s = d * 16 // (9 * level)
        wk = np.where(s <= 16, 16, np.where(s >= 32, 0, 32 - s))
        weights[i] = (wk * strength) >> 8
    total = weights.sum(0)
    out = ((weights[..., None] * f).sum(0) + (total // 2)[..., None]) // total[..., None]
    return out.astype(np.uint8), weights
