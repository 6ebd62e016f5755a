"""Privacy masks as the public interface spells them (csrc/vep/mask.h has the arithmetic).

A mask is a dict ``{"x0", "y0", "x1", "y1", "mode", "block", "b", "g", "r"}``: the rectangle in
1/10000 of the picture's width and height (``0 <= x0 < x1 <= 10000``, likewise y), ``mode``
``"fill"`` (every pixel becomes ``(b, g, r)``) or ``"pixelate"`` (blocks of ``block`` x ``block``
pixels, 4..128, become their mean). ``mode`` defaults to ``"pixelate"``, ``block`` to 16, the
colour to black. A camera has at most 8 masks, applied in list order.

The native layer takes tuples ``(x0, y0, x1, y1, mode, block, b, g, r)`` of ints: :func:`to_native`
validates a list (``ValueError`` on a bad one) and converts it, :func:`from_native` converts back.
"""
from __future__ import annotations

MAX_MASKS = 8
UNIT = 10000
MIN_BLOCK, MAX_BLOCK, DEFAULT_BLOCK = 4, 128, 16
MODES = ("fill", "pixelate")  # the native enum's order
_FIELDS = ("x0", "y0", "x1", "y1", "mode", "block", "b", "g", "r")


def _int(v, what):
    if isinstance(v, bool) or not isinstance(v, int):
        raise ValueError(f"mask {what} must be an integer, got {v!r}")
    return v


def normalize(mask) -> dict:
    """One mask as a complete dict; ``ValueError`` unless it is valid."""
    if isinstance(mask, (tuple, list)):
        if len(mask) != len(_FIELDS):
            raise ValueError("a mask tuple is (x0, y0, x1, y1, mode, block, b, g, r)")
        mask = dict(zip(_FIELDS, mask))
    if not isinstance(mask, dict):
        raise ValueError(f"a mask must be a dict, got {type(mask).__name__}")
    unknown = set(mask) - set(_FIELDS)
    if unknown:
        raise ValueError(f"unknown mask field(s): {sorted(unknown)}")
    for k in ("x0", "y0", "x1", "y1"):
        if k not in mask:
            raise ValueError(f"mask field {k} is missing")
    mode = mask.get("mode", "pixelate")
    if isinstance(mode, int) and not isinstance(mode, bool) and 0 <= mode < len(MODES):
        mode = MODES[mode]
    if mode not in MODES:
        raise ValueError(f"mask mode must be one of {MODES}, got {mode!r}")
    out = {k: _int(mask[k], k) for k in ("x0", "y0", "x1", "y1")}
    out["mode"] = mode
    out["block"] = _int(mask.get("block", DEFAULT_BLOCK), "block")
    for k in ("b", "g", "r"):
        out[k] = _int(mask.get(k, 0), k)
    if not 0 <= out["x0"] < out["x1"] <= UNIT:
        raise ValueError("mask needs 0 <= x0 < x1 <= 10000")
    if not 0 <= out["y0"] < out["y1"] <= UNIT:
        raise ValueError("mask needs 0 <= y0 < y1 <= 10000")
    if not MIN_BLOCK <= out["block"] <= MAX_BLOCK:
        raise ValueError("mask block must be 4..128")
    for k in ("b", "g", "r"):
        if not 0 <= out[k] <= 255:
            raise ValueError(f"mask colour component {k} must be 0..255")
    return out


def normalize_list(masks) -> list:
    """A camera's list as complete dicts (``None`` = no masks); ``ValueError`` on a bad list."""
    if masks is None:
        return []
    if isinstance(masks, (dict, str, bytes)) or not hasattr(masks, "__iter__"):
        raise ValueError("masks must be a list of masks")
    out = [normalize(m) for m in masks]
    if len(out) > MAX_MASKS:
        raise ValueError(f"at most {MAX_MASKS} masks per camera")
    return out


def to_native(masks) -> list:
    return [(m["x0"], m["y0"], m["x1"], m["y1"], MODES.index(m["mode"]), m["block"], m["b"], m["g"], m["r"])
            for m in normalize_list(masks)]


def from_native(tuples) -> list:
    return [normalize(tuple(t)) for t in tuples]
