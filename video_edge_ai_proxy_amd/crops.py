"""Crop requests as the public interface spells them (csrc/vep/crop.h has the arithmetic).

A box is a dict ``{"x0", "y0", "x1", "y1"}``: the rectangle in 1/10000 of the picture's width and
height (``0 <= x0 < x1 <= 10000``, likewise y), rounded outward to pixels. A picture has at most 64
boxes; an output side is 1..4096. ``fit`` is ``"stretch"`` (the box fills the output) or
``"letterbox"`` (the aspect is kept, the rest is the pad colour ``(b, g, r)``).

The native layer takes tuples ``(x0, y0, x1, y1)`` of ints, the fit as its index and the pad colour
as a tuple: the functions below validate (``ValueError`` on a bad value) and convert.
"""
from __future__ import annotations

MAX_BOXES = 64
MAX_OUT = 4096
UNIT = 10000
FITS = ("stretch", "letterbox")  # the native enum's order
DEFAULT_PAD = (114, 114, 114)
_FIELDS = ("x0", "y0", "x1", "y1")


def _int(v, what):
    if isinstance(v, bool) or not isinstance(v, int):
        raise ValueError(f"{what} must be an integer, got {v!r}")
    return v


def normalize(box) -> dict:
    """One box as a dict of ints; ``ValueError`` unless it is valid."""
    if isinstance(box, (tuple, list)):
        if len(box) != len(_FIELDS):
            raise ValueError("a box tuple is (x0, y0, x1, y1)")
        box = dict(zip(_FIELDS, box))
    if not isinstance(box, dict):
        raise ValueError(f"a box must be a dict, got {type(box).__name__}")
    unknown = set(box) - set(_FIELDS)
    if unknown:
        raise ValueError(f"unknown box field(s): {sorted(unknown)}")
    for k in _FIELDS:
        if k not in box:
            raise ValueError(f"box field {k} is missing")
    out = {k: _int(box[k], f"box {k}") for k in _FIELDS}
    if not 0 <= out["x0"] < out["x1"] <= UNIT:
        raise ValueError("box needs 0 <= x0 < x1 <= 10000")
    if not 0 <= out["y0"] < out["y1"] <= UNIT:
        raise ValueError("box needs 0 <= y0 < y1 <= 10000")
    return out


def normalize_list(boxes, max_boxes: int = MAX_BOXES) -> list:
    if boxes is None or isinstance(boxes, (dict, str, bytes)) or not hasattr(boxes, "__iter__"):
        raise ValueError("boxes must be a list of boxes")
    out = [normalize(b) for b in boxes]
    if len(out) > max_boxes:
        raise ValueError(f"at most {max_boxes} boxes per picture")
    return out


def to_native(boxes, max_boxes: int = MAX_BOXES) -> list:
    return [(b["x0"], b["y0"], b["x1"], b["y1"]) for b in normalize_list(boxes, max_boxes)]


def size(width, height) -> tuple:
    for v, what in ((width, "width"), (height, "height")):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= MAX_OUT:
            raise ValueError(f"{what} must be an integer 1..{MAX_OUT}")
    return width, height


def fit_index(fit) -> int:
    if fit is None:
        return 0
    if fit not in FITS:
        raise ValueError(f"fit must be one of {FITS}, got {fit!r}")
    return FITS.index(fit)


def pad_tuple(pad) -> tuple:
    if pad is None:
        return DEFAULT_PAD
    if isinstance(pad, (str, bytes, dict)) or not hasattr(pad, "__iter__"):
        raise ValueError("pad must be (b, g, r)")
    pad = tuple(pad)
    if len(pad) != 3:
        raise ValueError("pad must be (b, g, r)")
    for v in pad:
        if _int(v, "pad component") < 0 or v > 255:
            raise ValueError("pad components must be 0..255")
    return pad


def seq_args(after, seq) -> tuple:
    for v, what in ((after, "after"), (seq, "seq")):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"{what} must be an integer >= 0")
    return after, seq
