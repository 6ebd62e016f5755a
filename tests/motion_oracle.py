"""Independent oracle of the motion detector (docs/MOTION.md §1): numpy int64 and Python ints
only, nothing from the package, and written in another shape than csrc/vep/motion.h: the luma of
the whole picture by one matrix product, the shift as a floor division, the changed pixels as a
boolean plane, the cell counts by padding and reshaping, the summary restated from the text."""
import numpy as np

LUMA = np.array([29, 150, 77], dtype=np.int64)  # B, G, R; the weights sum to 256


def picture(kind: str, w: int, h: int, seed: int = 0) -> np.ndarray:
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "gradient":
        y, x = np.mgrid[0:h, 0:w].astype(np.int64)
        return np.stack([(x * 7 + seed * 97) % 256, (y * 5 + x + seed * 89) % 256, (x + y * 3 + seed * 101) % 256],
                        axis=-1).astype(np.uint8)
    raise ValueError(kind)


def grey(v: int, w: int, h: int) -> np.ndarray:
    """A constant v, v, v picture: its luma is v exactly."""
    return np.full((h, w, 3), v, dtype=np.uint8)


def blob(base: int, w: int, h: int, x: int, y: int, bw: int, bh: int, delta: int) -> np.ndarray:
    """A grey picture with the rectangle (x, y, bw, bh) raised by delta."""
    p = grey(base, w, h)
    p[y:y + bh, x:x + bw] = base + delta
    return p


def luma(bgr: np.ndarray) -> np.ndarray:
    return (bgr.astype(np.int64) @ LUMA + 128) // 256


def grid(w: int, h: int, cell: int):
    return -(-w // cell), -(-h // cell)  # cols, rows


def update(bgr: np.ndarray, bg, cell: int, threshold: int, learn_shift: int):
    """(counts int64 (rows, cols), background int64 (h, w)); bg None: prime."""
    h, w = bgr.shape[:2]
    cols, rows = grid(w, h, cell)
    y = luma(bgr)
    if bg is None:
        return np.zeros((rows, cols), dtype=np.int64), y * 256
    bg = np.asarray(bg).astype(np.int64)
    ref = (bg + 128) // 256
    mask = np.abs(y - ref) > threshold
    new = bg + (y * 256 - bg) // (2 ** learn_shift)  # floor, also below zero
    padded = np.zeros((rows * cell, cols * cell), dtype=np.int64)
    padded[:h, :w] = mask
    counts = padded.reshape(rows, cell, cols, cell).sum(axis=(1, 3))
    return counts, new


def summarize(counts, w: int, h: int, cell: int, cell_percent: int, min_cells: int) -> dict:
    cols, rows = grid(w, h, cell)
    changed, active, xs, ys = 0, [], [], []
    for gy in range(rows):
        for gx in range(cols):
            n = int(counts[gy][gx])
            changed += n
            pixels = (min((gx + 1) * cell, w) - gx * cell) * (min((gy + 1) * cell, h) - gy * cell)
            if n * 100 >= pixels * cell_percent:
                active.append((gx, gy))
    box = None
    if active:
        x0, y0 = min(g[0] for g in active) * cell, min(g[1] for g in active) * cell
        x1, y1 = min((max(g[0] for g in active) + 1) * cell, w), min((max(g[1] for g in active) + 1) * cell, h)
        box = (x0, y0, x1 - x0, y1 - y0)
    return {"changed": changed, "active": len(active), "box": box, "motion": len(active) >= min_cells}
