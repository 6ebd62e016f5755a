"""On-screen display items as the public interface spells them (csrc/vep/overlay.h has the
arithmetic, docs/OVERLAY.md the reasoning).

An item is a dict. Coordinates are in 1/10000 of the picture, so a list drawn on a scaled picture
lands in the same place. A picture takes at most 64 items.

``{"type": "box", "x0", "y0", "x1", "y1", "color": [b, g, r], "alpha", "thickness", "fill", "label"}``
    ``0 <= x0 < x1 <= 10000``, likewise y; ``color`` defaults to ``[0, 255, 0]``, ``alpha`` (0..255)
    to 255, ``thickness`` is 1..32 or 0 for auto, ``fill`` defaults to false, ``label`` is optional.
``{"type": "text", "x", "y", "text", "scale", "color", "alpha", "bg": [b, g, r], "bg_alpha"}``
    ``0 <= x, y <= 10000``; ``scale`` is 1..8 or 0 for auto, ``color`` defaults to white, ``bg`` is
    optional with ``bg_alpha`` defaulting to 255.

``type`` may be left out: an item with ``x0`` is a box, any other a text. In a text or a label
``{name}``, ``{seq}`` and ``{time}`` are replaced from the frame that is drawn on; the result is cut
at 64 bytes and every byte outside 0x20..0x7E becomes ``?``.

The native layer takes tuples ``(kind, x0, y0, x1, y1, b, g, r, alpha, thickness, fill, scale, has_bg,
bg_b, bg_g, bg_r, bg_alpha, text)``: the functions below validate (``ValueError`` on a bad value)
and convert.
"""
from __future__ import annotations

MAX_ITEMS = 64
MAX_PRIMS = 256
MAX_TEXT = 64
MAX_RAW_TEXT = 256
MAX_SCALE = 8
MAX_THICKNESS = 32
UNIT = 10000
BOX, TEXT = 0, 1
STAMP = {"type": "text", "x": 100, "y": 100, "text": "{name} {time}", "bg": [0, 0, 0], "bg_alpha": 128}



class Refused(ValueError):
    """A valid list that cannot be drawn: it expands to more than 256 primitives."""


_BOX_FIELDS = ("type", "x0", "y0", "x1", "y1", "color", "alpha", "thickness", "fill", "label")
_TEXT_FIELDS = ("type", "x", "y", "text", "scale", "color", "alpha", "bg", "bg_alpha")


def _int(v, what, lo, hi):
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f"{what} must be an integer {lo}..{hi}, got {v!r}")
    return v


def _colour(v, what):
    if isinstance(v, (str, bytes, dict)) or not hasattr(v, "__iter__"):
        raise ValueError(f"{what} must be [b, g, r]")
    v = list(v)
    if len(v) != 3:
        raise ValueError(f"{what} must be [b, g, r]")
    return [_int(c, f"{what} component", 0, 255) for c in v]


def _text(v, what) -> str:
    if isinstance(v, bytes):
        v = v.decode("latin-1")
    if not isinstance(v, str):
        raise ValueError(f"{what} must be a string")
    if len(_bytes(v)) > MAX_RAW_TEXT:
        raise ValueError(f"{what} has more than {MAX_RAW_TEXT} bytes")
    return v


def _bytes(s: str) -> bytes:
    """A text as the native layer gets it: code points below 256 as one byte each (so bytes given
    as latin-1 survive), anything else as UTF-8; every byte outside 0x20..0x7E is drawn as ``?``."""
    try:
        return s.encode("latin-1")
    except UnicodeEncodeError:
        return s.encode("utf-8")


def normalize(item) -> dict:
    """One item as a dict with every field present; ``ValueError`` unless it is valid."""
    if not isinstance(item, dict):
        raise ValueError(f"an overlay item must be a dict, got {type(item).__name__}")
    kind = item.get("type", "box" if "x0" in item else "text")
    if kind not in ("box", "text"):
        raise ValueError(f"an overlay item's type is 'box' or 'text', got {kind!r}")
    fields = _BOX_FIELDS if kind == "box" else _TEXT_FIELDS
    unknown = set(item) - set(fields)
    if unknown:
        raise ValueError(f"unknown {kind} field(s): {sorted(unknown, key=str)}")
    out = {"type": kind}
    if kind == "box":
        for k in ("x0", "y0", "x1", "y1"):
            if k not in item:
                raise ValueError(f"box field {k} is missing")
            out[k] = _int(item[k], f"box {k}", 0, UNIT)
        if not out["x0"] < out["x1"]:
            raise ValueError("box needs 0 <= x0 < x1 <= 10000")
        if not out["y0"] < out["y1"]:
            raise ValueError("box needs 0 <= y0 < y1 <= 10000")
        out["color"] = _colour(item.get("color", [0, 255, 0]), "color")
        out["alpha"] = _int(item.get("alpha", 255), "alpha", 0, 255)
        out["thickness"] = _int(item.get("thickness", 0), "thickness", 0, MAX_THICKNESS)
        fill = item.get("fill", False)
        if not isinstance(fill, bool):
            raise ValueError("fill must be true or false")
        out["fill"] = fill
        label = item.get("label")
        out["label"] = "" if label is None else _text(label, "label")
        return out
    for k in ("x", "y"):
        if k not in item:
            raise ValueError(f"text field {k} is missing")
        out[k] = _int(item[k], f"text {k}", 0, UNIT)
    if "text" not in item:
        raise ValueError("text field text is missing")
    out["text"] = _text(item["text"], "text")
    out["scale"] = _int(item.get("scale", 0), "scale", 0, MAX_SCALE)
    out["color"] = _colour(item.get("color", [255, 255, 255]), "color")
    out["alpha"] = _int(item.get("alpha", 255), "alpha", 0, 255)
    bg = item.get("bg")
    out["bg"] = None if bg is None else _colour(bg, "bg")
    out["bg_alpha"] = _int(item.get("bg_alpha", 255), "bg_alpha", 0, 255)
    return out


def normalize_list(items, max_items: int = MAX_ITEMS) -> list:
    if items is None or isinstance(items, (dict, str, bytes)) or not hasattr(items, "__iter__"):
        raise ValueError("items must be a list of overlay items")
    out = [normalize(i) for i in items]
    if len(out) > max_items:
        raise ValueError(f"at most {max_items} overlay items per picture")
    return out


def _native(it: dict) -> tuple:
    b, g, r = it["color"]
    if it["type"] == "box":
        return (BOX, it["x0"], it["y0"], it["x1"], it["y1"], b, g, r, it["alpha"], it["thickness"], int(it["fill"]),
                0, 0, 0, 0, 0, 255, _bytes(it["label"]))
    bg = it["bg"] or [0, 0, 0]
    return (TEXT, it["x"], it["y"], 0, 0, b, g, r, it["alpha"], 0, 0, it["scale"], int(it["bg"] is not None),
            bg[0], bg[1], bg[2], it["bg_alpha"], _bytes(it["text"]))


def to_native(items, max_items: int = MAX_ITEMS) -> list:
    return [_native(i) for i in normalize_list(items, max_items)]


def public(it: dict) -> dict:
    """A normalised item as the interface shows it again (JSON-ready)."""
    out = dict(it)
    if out["type"] == "box" and not out["label"]:
        del out["label"]
    if out["type"] == "text" and out["bg"] is None:
        del out["bg"], out["bg_alpha"]
    return out


def from_pixel_box(left: int, top: int, right: int, bottom: int, width: int, height: int) -> tuple:
    """A pixel box ``[left, right) x [top, bottom)`` of a ``width x height`` picture in 1/10000,
    rounded outward (so its pixel rect never loses a pixel of the box) and clamped to the picture."""
    if width <= 0 or height <= 0:
        raise ValueError("width and height must be positive")
    x0 = max(0, min(UNIT - 1, left * UNIT // width))
    y0 = max(0, min(UNIT - 1, top * UNIT // height))
    x1 = max(x0 + 1, min(UNIT, -(-right * UNIT // width)))
    y1 = max(y0 + 1, min(UNIT, -(-bottom * UNIT // height)))
    return x0, y0, x1, y1


def from_annotation(req) -> dict | None:
    """The box item of an ``AnnotateRequest`` that names a bounding box and the size of the picture
    it was found in (``width`` / ``height`` non-zero), else None. The label is ``object_type`` and
    the confidence in percent."""
    if not req.HasField("object_bouding_box") or req.width <= 0 or req.height <= 0:
        return None
    bb = req.object_bouding_box
    if bb.width <= 0 or bb.height <= 0:
        return None
    x0, y0, x1, y1 = from_pixel_box(bb.left, bb.top, bb.left + bb.width, bb.top + bb.height, req.width, req.height)
    conf = req.confidence if req.confidence > 1.0 else req.confidence * 100.0
    label = f"{req.object_type} {int(round(max(0.0, min(100.0, conf))))}%".strip()
    return {"type": "box", "x0": x0, "y0": y0, "x1": x1, "y1": y1, "label": label}
