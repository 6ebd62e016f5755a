"""numpy oracle of the on-screen display, written from docs/OVERLAY.md section 1 alone and in another
shape than csrc/vep/overlay.h: every primitive becomes a whole-picture boolean coverage array (glyph
runs by np.kron of the glyph bitmaps), and the blend runs vectorised in int64 over that array.

The font is data, not arithmetic: the oracle takes the (95, 8) table as an argument
(native.overlay_font()); tests/test_overlay.py checks the table's properties on their own.

Also the pictures and the item lists every size is tested with.
"""
from __future__ import annotations

import datetime

import numpy as np

UNIT = 10000
MAX_PRIMS = 256
MAX_TEXT = 64
FILL, TEXT = 0, 1


def blend(d, c, a):
    d, c, a = (np.asarray(v, dtype=np.int64) for v in (d, c, a))
    return (d * (255 - a) + c * a + 127) // 255


def auto_k(rows: int) -> int:
    return max(1, min(8, rows // 270))


def time_text(timestamp: int) -> str:
    """FrameMeta::timestamp counts 90 kHz ticks; shown as UTC from 1970-01-01."""
    ms = max(0, timestamp) // 90
    t = datetime.datetime(1970, 1, 1) + datetime.timedelta(milliseconds=ms)
    return t.strftime("%Y-%m-%d %H:%M:%S.") + "%03d" % (ms % 1000)


def final_text(raw, name: str = "", meta=None) -> bytes:
    meta = meta or {}
    if isinstance(raw, str):
        raw = raw.encode("latin-1")
    s = raw.replace(b"{name}", name.encode("latin-1"))
    s = s.replace(b"{seq}", str(int(meta.get("seq", 0))).encode())
    s = s.replace(b"{time}", time_text(int(meta.get("timestamp", 0))).encode())
    s = s[:MAX_TEXT]
    return bytes(b if 0x20 <= b <= 0x7E else ord("?") for b in s)


def axis_pixels(n, a, b):
    p0, p1 = a * n // UNIT, -(-b * n // UNIT)
    p1 = min(p1, n)
    p0 = max(0, min(p0, n - 1))
    return p0, max(p1, p0 + 1)


def _fill(out, x0, y0, x1, y1, W, H, colour, a):
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)
    if x0 < x1 and y0 < y1:
        out.append((FILL, x0, y0, x1, y1, tuple(colour), a))


def expand(items, W: int, H: int, name: str = "", meta=None) -> list:
    """The primitives in the format of native.overlay_expand."""
    out = []
    ak = auto_k(H)
    for it in items:
        kind = it.get("type", "box" if "x0" in it else "text")
        if kind == "box":
            x0, x1 = axis_pixels(W, it["x0"], it["x1"])
            y0, y1 = axis_pixels(H, it["y0"], it["y1"])
            col, a = tuple(it.get("color", (0, 255, 0))), it.get("alpha", 255)
            t = it.get("thickness", 0) or ak
            if it.get("fill", False) or 2 * t >= min(x1 - x0, y1 - y0):
                _fill(out, x0, y0, x1, y1, W, H, col, a)
            else:
                _fill(out, x0, y0, x1, y0 + t, W, H, col, a)
                _fill(out, x0, y1 - t, x1, y1, W, H, col, a)
                _fill(out, x0, y0 + t, x0 + t, y1 - t, W, H, col, a)
                _fill(out, x1 - t, y0 + t, x1, y1 - t, W, H, col, a)
            s = final_text(it.get("label") or "", name, meta)
            if s:
                sw, sh = 6 * ak * len(s) + ak, 9 * ak
                sy = y0 - sh if y0 - sh >= 0 else y0
                _fill(out, x0, sy, x0 + sw, sy + sh, W, H, col, a)
                b, g, r = col
                ink = 255 if 2 * r + 5 * g + b < 1024 else 0
                out.append((TEXT, x0 + ak, sy + ak, ak, (ink, ink, ink), 255, s))
        else:
            s = final_text(it["text"], name, meta)
            if not s:
                continue
            k = it.get("scale", 0) or ak
            ox, oy = it["x"] * W // UNIT, it["y"] * H // UNIT
            if it.get("bg") is not None:
                _fill(out, ox - k, oy - k, ox + 6 * k * len(s), oy + 8 * k, W, H, it["bg"], it.get("bg_alpha", 255))
            out.append((TEXT, ox, oy, k, tuple(it.get("color", (255, 255, 255))), it.get("alpha", 255), s))
        if len(out) > MAX_PRIMS:
            raise ValueError("the list expands to more than 256 primitives")
    return out


def coverage(prim, W: int, H: int, font) -> np.ndarray:
    """(H, W) bool: the pixels of the picture the primitive covers."""
    cov = np.zeros((H, W), dtype=bool)
    if prim[0] == FILL:
        _, x0, y0, x1, y1 = prim[:5]
        cov[y0:y1, x0:x1] = True
        return cov
    _, ox, oy, k, _, _, s = prim
    bits = (np.asarray(font)[np.frombuffer(s, np.uint8) - 0x20][:, :, None] >> np.arange(6)) & 1  # (len, 8, 6)
    run = np.kron(np.concatenate(list(bits), axis=1), np.ones((k, k), dtype=np.int64)).astype(bool)  # (8k, 6k len)
    h, w = min(run.shape[0], H - oy), min(run.shape[1], W - ox)
    if h > 0 and w > 0:
        cov[oy:oy + h, ox:ox + w] = run[:h, :w]
    return cov


def colour_alpha(prim):
    return (prim[5], prim[6]) if prim[0] == FILL else (prim[4], prim[5])


def draw(img: np.ndarray, prims, font) -> np.ndarray:
    H, W = img.shape[:2]
    out = img.astype(np.int64)
    for p in prims:
        cov = coverage(p, W, H, font)
        col, a = colour_alpha(p)
        out = np.where(cov[:, :, None], blend(out, np.asarray(col, np.int64)[None, None, :], a), out)
    return out.astype(np.uint8)


def apply(img: np.ndarray, items, font, name: str = "", meta=None) -> np.ndarray:
    H, W = img.shape[:2]
    return draw(img, expand(items, W, H, name, meta), font)


# ------------------------------------------------------------------------ pictures and lists

SMALL = [(1, 1), (7, 5), (17, 9), (64, 16), (65, 17), (200, 120)]  # (W, H)


def picture(W: int, H: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(1000 * W + H + seed)
    return rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)


FILLS = [{"x0": 0, "y0": 0, "x1": 7000, "y1": 6000, "color": [250, 10, 20], "alpha": 100, "fill": True},
         {"x0": 3000, "y0": 2000, "x1": 10000, "y1": 9000, "color": [5, 240, 90], "alpha": 180, "fill": True},
         {"x0": 1000, "y0": 4000, "x1": 9000, "y1": 10000, "color": [60, 70, 255], "alpha": 33, "fill": True}]
LONG = "The quick brown fox jumps over the lazy dog 0123456789 ~!@#$%^&*"


def lists() -> dict:
    """name -> items: what twin == oracle and kernel == twin are checked with at every size."""
    ones = [{"type": "text", "x": (37 * i) % 10001, "y": (91 * i) % 10001, "text": chr(0x21 + i % 94), "scale": 1,
             "color": [i % 256, (3 * i) % 256, 255 - i % 256], "alpha": 255 - i // 2} for i in range(64)]
    pixels = [{"x0": (61 * i) % 10000, "y0": (29 * i) % 10000, "x1": (61 * i) % 10000 + 1, "y1": (29 * i) % 10000 + 1,
               "color": [255 - i, i, 7 * i % 256], "alpha": 128 + i, "thickness": 1, "label": "#"} for i in range(64)]
    return {
        "empty": [],
        "full": [{"x0": 0, "y0": 0, "x1": 10000, "y1": 10000, "color": [1, 2, 3], "alpha": 200, "fill": True}],
        "three": FILLS,
        "three_reversed": FILLS[::-1],
        "text_k1": [{"type": "text", "x": 300, "y": 2000, "text": LONG, "scale": 1, "alpha": 210}],
        "text_k8": [{"type": "text", "x": 1500, "y": 100, "text": LONG, "scale": 8, "color": [0, 255, 255],
                     "bg": [30, 30, 30], "bg_alpha": 99}],
        "text_edges": [{"type": "text", "x": 9700, "y": 4000, "text": "right edge", "scale": 2},
                       {"type": "text", "x": 2000, "y": 9800, "text": "bottom edge", "scale": 3, "bg": [0, 0, 255]},
                       {"type": "text", "x": 0, "y": 0, "text": "corner", "scale": 1, "bg": [9, 9, 9], "bg_alpha": 140},
                       {"type": "text", "x": 10000, "y": 10000, "text": "outside", "bg": [1, 1, 1]},
                       {"type": "text", "x": 9990, "y": 9990, "text": "last pixel", "scale": 4, "alpha": 77}],
        "outlines": [{"x0": 500, "y0": 500, "x1": 9500, "y1": 9500, "alpha": 120, "label": "person 87%"},
                     {"x0": 2000, "y0": 0, "x1": 6000, "y1": 5000, "color": [255, 0, 0], "thickness": 3,
                      "label": "top {seq}"},
                     {"x0": 8000, "y0": 6000, "x1": 10000, "y1": 10000, "color": [0, 0, 0], "alpha": 200,
                      "thickness": 32, "label": "runs off the right edge"}],
        "ones": ones,        # 64 one-glyph texts
        "pixels": pixels,    # 64 one-pixel boxes, each a fill, a strip and a text: 192 primitives
        "dense": dense(),    # 256 primitives where the picture is large enough
    }


def dense() -> list:
    """A list that expands to exactly 256 primitives on any picture of at least 200 x 120: 42
    labelled outlines one pixel thick (four fills, a strip and a text each: 252, the side fills one
    pixel wide) and two texts on a background (4). Primitives arise from items only, so this is how
    the interface reaches the kernel's full set of 256."""
    a = [{"x0": 100 + 1400 * (i % 7), "y0": 1200 + 1450 * (i // 7), "x1": 700 + 1400 * (i % 7),
          "y1": 2000 + 1450 * (i // 7), "thickness": 1, "alpha": 255 - 3 * i, "color": [40 * (i % 7), 255 - 6 * i, 5 * i],
          "label": "%d" % i} for i in range(42)]
    a += [{"type": "text", "x": 50, "y": 50, "text": "{name} {time}", "scale": 1, "bg": [0, 0, 0], "bg_alpha": 128},
          {"type": "text", "x": 5000, "y": 9000, "text": "seq {seq}", "scale": 2, "bg": [255, 255, 255], "bg_alpha": 60,
           "color": [0, 0, 0]}]
    return a
