"""What the CPU and GPU dewarp tests share: the from-scratch numpy transcription of the arithmetic
(csrc/vep/dewarp.h, docs/DEWARP.md section 1) and the meshes both are run on."""
import numpy as np

LO, HI = -8192 * 256, 2 * 8192 * 256
OUT_SIZES = [(w, h) for w in (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 130) for h in (1, 8, 9, 16, 17, 33)]
SOURCES = [(1, 1), (17, 9), (200, 120)]
MESHES = ["identity", "half", "rot90", "outside", "half_inside", "minify6", "smooth", "garbage"]
PAD = (7, 200, 90)


def picture(w, h, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def oracle(src, mesh, ow, oh, pad=(0, 0, 0)):
    h, w = src.shape[:2]
    n = np.clip(mesh.astype(np.int64), LO, HI - 1)
    j, k = np.meshgrid(np.arange(ow), np.arange(oh))
    m, a, r, b = j >> 3, j & 7, k >> 3, k & 7
    s = ((8 - a) * (8 - b))[..., None] * n[r, m] + (a * (8 - b))[..., None] * n[r, m + 1] \
        + ((8 - a) * b)[..., None] * n[r + 1, m] + (a * b)[..., None] * n[r + 1, m + 1]
    assert np.abs(s).max() <= 2 ** 28
    p = (s + 32) >> 6
    px, py = p[..., 0], p[..., 1]
    outside = (px < -128) | (px >= w * 256 - 128) | (py < -128) | (py >= h * 256 - 128)
    fx, fy = (px & 255)[..., None], (py & 255)[..., None]
    x0, x1 = np.clip(px >> 8, 0, w - 1), np.clip((px >> 8) + 1, 0, w - 1)
    y0, y1 = np.clip(py >> 8, 0, h - 1), np.clip((py >> 8) + 1, 0, h - 1)
    v = src.astype(np.int64)
    out = ((256 - fx) * (256 - fy) * v[y0, x0] + fx * (256 - fy) * v[y0, x1] + (256 - fx) * fy * v[y1, x0]
           + fx * fy * v[y1, x1] + 32768) >> 16
    out[outside] = pad
    return out.astype(np.uint8)


def mesh_of(kind, w, h, ow, oh, seed=0):
    """int32[mh, mw, 2] for an ow x oh view of a w x h picture. On the GPU (64 x 16 tiles): identity,
    half and half_inside have footprints of the tile's own size (taps from global memory, not
    staged; half_inside also has tiles wholly right of the picture: pad); outside is pad tiles only;
    rot90 of the 200 x 120 picture has footprints 17 wide and 65 high, and smooth stretches it to
    about 100 x 60 a tile (both staged in LDS); minify6 spans 385 x 97 source pixels a full tile,
    above the staging buffer (global), a narrow last tile (staged) and pad tiles past the picture;
    garbage has boxes as large as the clamp allows (global or pad)."""
    mh, mw = (oh + 7) // 8 + 1, (ow + 7) // 8 + 1
    x, y = np.meshgrid(np.arange(mw, dtype=np.int64) * 8, np.arange(mh, dtype=np.int64) * 8)
    rng = np.random.default_rng(seed + 1000 * ow + oh)
    if kind == "identity":
        sx, sy = x * 256, y * 256
    elif kind == "half":
        sx, sy = x * 256 - 128, y * 256
    elif kind == "rot90":  # out(j, k) = src(k, h - 1 - j)
        sx, sy = y * 256, (h - 1 - x) * 256
    elif kind == "outside":
        sx, sy = np.full_like(x, -100000), y * 256
    elif kind == "half_inside":
        sx, sy = x * 256 + w * 128, y * 256
    elif kind == "minify6":
        sx, sy = x * 6 * 256 + 640, y * 6 * 256 + 640
    elif kind == "smooth":  # the output stretched over the picture, every node moved by up to 3 px
        sx = x * 256 * w // max(ow, 1) + rng.integers(-768, 769, x.shape)
        sy = y * 256 * h // max(oh, 1) + rng.integers(-768, 769, x.shape)
    else:  # garbage: INT32_MIN / INT32_MAX and anything between
        pool = np.array([-2 ** 31, 2 ** 31 - 1, 0, 256 * w, -129, 5 * 10 ** 6], np.int64)
        sx, sy = rng.choice(pool, x.shape), rng.choice(pool, x.shape)
        some = rng.random(x.shape) < 0.3
        sx = np.where(some, rng.integers(-2 ** 31, 2 ** 31, x.shape), sx)
    return np.ascontiguousarray(np.stack([sx, sy], -1).astype(np.int32))
