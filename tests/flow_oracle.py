"""numpy int64 oracle of the block matching, written from docs/FLOW.md section 1 (not from flow.h)."""
import numpy as np


def luma_plane(bgr, d):
    p = bgr.astype(np.int64)
    y = (29 * p[..., 0] + 150 * p[..., 1] + 77 * p[..., 2] + 128) >> 8
    h, w = y.shape[0] // d, y.shape[1] // d
    s = y[:h * d, :w * d].reshape(h, d, w, d).sum(axis=(1, 3))
    return (s + d * d // 2) >> (2 * {1: 0, 2: 1, 4: 2}[d])


def match(l0, lg, R):
    """(rows, cols, 4) int64 of vx, vy, best, zero."""
    h, w = l0.shape
    rows, cols = h // 8, w // 8
    out = np.zeros((rows, cols, 4), np.int64)
    for by in range(rows):
        for bx in range(cols):
            x0, y0 = bx * 8, by * 8
            blk, best = l0[y0:y0 + 8, x0:x0 + 8], None
            for vy in range(-R, R + 1):
                for vx in range(-R, R + 1):
                    x, y = x0 - vx, y0 - vy
                    if x < 0 or y < 0 or x + 8 > w or y + 8 > h:
                        continue
                    sad = int(np.abs(blk - lg[y:y + 8, x:x + 8]).sum())
                    key = sad << 15 | (abs(vx) + abs(vy)) << 10 | (vy + R) << 5 | (vx + R)
                    if best is None or key < best[0]:
                        best = (key, vx, vy, sad)
                    if vx == 0 and vy == 0:
                        zero = sad
            out[by, bx] = (best[1], best[2], best[3], zero)
    return out


def flow(newer, older, d, R):
    l0, lg = luma_plane(newer, d), luma_plane(older, d)
    return np.stack([l0, lg]), match(l0, lg, R)


def direction(vx, vy):
    a, b = abs(vx), abs(vy)
    if 12 * b < 5 * a:
        return 0 if vx > 0 else 4
    if 12 * a < 5 * b:
        return 2 if vy > 0 else 6
    return (1 if vx > 0 else 3) if vy > 0 else (7 if vx > 0 else 5)


def summarize(grid, d, min_gain, min_blocks, global_percent):
    rows, cols = grid.shape[:2]
    moving = [(bx, by, int(g[0]), int(g[1])) for by in range(rows) for bx in range(cols) for g in [grid[by, bx]]
              if (g[0] or g[1]) and g[3] - g[2] >= 64 * min_gain]
    dirs = [0] * 8
    for _, _, vx, vy in moving:
        dirs[direction(vx, vy)] += 1
    box = None
    if moving:
        xs, ys = [m[0] for m in moving], [m[1] for m in moving]
        box = (min(xs) * 8 * d, min(ys) * 8 * d, (max(xs) - min(xs) + 1) * 8 * d, (max(ys) - min(ys) + 1) * 8 * d)
    votes = {}
    for g in grid.reshape(-1, 4):
        votes[(int(g[0]), int(g[1]))] = votes.get((int(g[0]), int(g[1])), 0) + 1
    n = rows * cols
    gv, count = (0, 0), 0
    if votes:
        gv, count = min(votes.items(), key=lambda kv: (-kv[1], abs(kv[0][0]) + abs(kv[0][1]), kv[0][1], kv[0][0]))
    return {"moving": len(moving), "sum_vx": sum(m[2] for m in moving), "sum_vy": sum(m[3] for m in moving), "dirs": dirs,
            "box": box, "motion": len(moving) >= min_blocks,
            "global": {"vx": gv[0], "vy": gv[1], "count": count, "percent": count * 100 // n if n else 0},
            "camera_moved": bool(n) and gv != (0, 0) and count * 100 >= n * global_percent}
