"""Independent oracle of the tamper detector (docs/TAMPER.md §1): numpy int64 and Python ints
only, nothing from the package, and written in another shape than csrc/vep/tamper.h: the luma of
the whole picture by one matrix product, the histogram by np.bincount, the energy from np.diff
planes with the pairs that cross a cell boundary masked out by index arithmetic, the cell sums by
padding and reshaping, the summary restated from the text."""
import numpy as np

LUMA = np.array([29, 150, 77], dtype=np.int64)  # B, G, R; the weights sum to 256

DEFAULTS = {"cell": 32, "dark_level": 32, "bright_level": 224, "spread_min": 24, "focus_percent": 50,
            "shift_level": 24, "shift_percent": 50}
FLAGS = ("dark", "bright", "flat", "defocused", "moved")


def picture(kind: str, w: int, h: int, seed: int = 0) -> np.ndarray:
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "gradient":
        return np.stack([(x * 7 + seed * 97) % 256, (y * 5 + x + seed * 89) % 256, (x + y * 3 + seed * 101) % 256],
                        axis=-1).astype(np.uint8)
    if kind == "uniform":
        return grey(128 + seed, w, h)
    if kind == "checker":  # 0 / 255, one pixel per field
        return levels(((x + y + seed) % 2) * 255)
    if kind == "vstripes":  # columns 0 / 255: horizontal pairs only
        return levels(((x + seed) % 2) * 255 + y * 0)
    if kind == "hstripes":  # rows 0 / 255: vertical pairs only
        return levels(((y + seed) % 2) * 255 + x * 0)
    raise ValueError(kind)


KINDS = ("noise", "gradient", "uniform", "checker", "vstripes", "hstripes")


def grey(v: int, w: int, h: int) -> np.ndarray:
    """A constant v, v, v picture: its luma is v exactly."""
    return np.full((h, w, 3), v, dtype=np.uint8)


def levels(plane) -> np.ndarray:
    """The grey picture whose luma is `plane` exactly."""
    p = np.asarray(plane).astype(np.uint8)
    return np.ascontiguousarray(np.stack([p, p, p], axis=-1))


def luma(bgr: np.ndarray) -> np.ndarray:
    return (bgr.astype(np.int64) @ LUMA + 128) // 256


def grid(w: int, h: int, cell: int):
    return -(-w // cell), -(-h // cell)  # cols, rows


def _cell_sums(plane, w, h, cell):
    cols, rows = grid(w, h, cell)
    padded = np.zeros((rows * cell, cols * cell), dtype=np.int64)
    padded[:h, :w] = plane
    return padded.reshape(rows, cell, cols, cell).sum(axis=(1, 3))


def stats(bgr: np.ndarray, cell: int):
    """(hist int64 (256,), sum_y int64 (rows, cols), energy int64 (rows, cols))"""
    h, w = bgr.shape[:2]
    y = luma(bgr)
    hist = np.bincount(y.ravel(), minlength=256).astype(np.int64)
    # a pair is booked on its first pixel; one that ends in column / row k * cell crosses a boundary
    dx = np.zeros((h, w), dtype=np.int64)
    dx[:, :-1] = np.diff(y, axis=1) ** 2
    dx[:, np.arange(w) % cell == cell - 1] = 0
    dy = np.zeros((h, w), dtype=np.int64)
    dy[:-1, :] = np.diff(y, axis=0) ** 2
    dy[np.arange(h) % cell == cell - 1, :] = 0
    return hist, _cell_sums(y, w, h, cell), _cell_sums(dx + dy, w, h, cell)


def summarize(hist, sum_y, energy, w: int, h: int, params=None, reference=None) -> dict:
    """reference: None or (w, h, cell, sum_y, energy) of the frame declared normal."""
    p = dict(DEFAULTS, **(params or {}))
    cell = p["cell"]
    cols, rows = grid(w, h, cell)
    n = w * h
    if reference is not None and tuple(reference[:3]) != (w, h, cell):
        reference = None
    mean_sum = sum(int(v) for v in np.asarray(sum_y).ravel())
    energy_total = sum(int(v) for v in np.asarray(energy).ravel())
    pairs_total, shifted = 0, 0
    for gy in range(rows):
        ch = min((gy + 1) * cell, h) - gy * cell
        for gx in range(cols):
            cw = min((gx + 1) * cell, w) - gx * cell
            pairs_total += (cw - 1) * ch + cw * (ch - 1)
            if reference is not None and abs(int(sum_y[gy][gx]) - int(reference[3][gy][gx])) > p["shift_level"] * cw * ch:
                shifted += 1

    def pct(k):
        cum = 0
        for v in range(256):
            cum += int(hist[v])
            if cum * 100 >= k * n:
                return v
        raise AssertionError("the histogram does not hold the picture")

    out = {"mean": mean_sum / n, "mean_sum": mean_sum, "p5": pct(5), "p95": pct(95), "energy_total": energy_total,
           "pairs_total": pairs_total, "sharpness": energy_total / pairs_total if pairs_total else 0.0,
           "has_reference": reference is not None, "cells": cols * rows, "shifted": shifted}
    out["dark"] = mean_sum <= p["dark_level"] * n
    out["bright"] = mean_sum >= p["bright_level"] * n
    out["flat"] = out["p95"] - out["p5"] < p["spread_min"]
    out["defocused"] = out["moved"] = False
    if reference is not None:
        ref_energy = sum(int(v) for v in np.asarray(reference[4]).ravel())
        out["defocused"] = p["focus_percent"] > 0 and energy_total * 100 < p["focus_percent"] * ref_energy
        out["moved"] = shifted * 100 >= p["shift_percent"] * cols * rows
    out["causes"] = [f for f in FLAGS if out[f]]
    out["tampered"] = bool(out["causes"])
    return out


def box_blur(bgr: np.ndarray, k: int = 5) -> np.ndarray:
    """k x k box blur with the edges replicated."""
    r = k // 2
    p = np.pad(bgr.astype(np.int64), ((r, r), (r, r), (0, 0)), mode="edge")
    h, w = bgr.shape[:2]
    acc = np.zeros(bgr.shape, dtype=np.int64)
    for dy in range(k):
        for dx in range(k):
            acc += p[dy:dy + h, dx:dx + w]
    return (acc // (k * k)).astype(np.uint8)
