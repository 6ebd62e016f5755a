"""Contrast enhancement of dark scenes (CLAHE on luma; csrc/vep/clahe.h, docs/ENHANCE.md): the
parameters as clients give them, and as the native layer takes them.

``tile``      side of a tile in pixels, 32..256 and a multiple of 8 (default 128)
``clip``      clip limit in multiples of the mean bin height, 1.0..256.0 (default 2.0; 256 never clips)
``strength``  0..1: how much of the equalised luma is taken (default 1.0; 0 is the identity)
"""
from __future__ import annotations

DEFAULTS = {"tile": 128, "clip": 2.0, "strength": 1.0}


def _number(v, what: str) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
        raise ValueError(f"{what} must be a number")
    return float(v)


def to_native(tile=None, clip=None, strength=None, defaults=None) -> tuple:
    """``(tile, clip16, strength256)`` of the three parameters (None: ``defaults``' value, which
    itself defaults to :data:`DEFAULTS`); a bad value is a ``ValueError``."""
    d = dict(DEFAULTS, **(defaults or {}))
    tile = d["tile"] if tile is None else tile
    if isinstance(tile, bool) or not isinstance(tile, int) or not 32 <= tile <= 256 or tile % 8:
        raise ValueError("tile must be an integer 32..256 and a multiple of 8")
    clip = _number(d["clip"] if clip is None else clip, "clip")
    if not 1.0 <= clip <= 256.0:
        raise ValueError("clip must be 1.0..256.0")
    strength = _number(d["strength"] if strength is None else strength, "strength")
    if not 0.0 <= strength <= 1.0:
        raise ValueError("strength must be 0..1")
    return tile, int(round(clip * 16)), int(round(strength * 256))


def from_request(enhance, defaults=None):
    """A call's ``enhance`` argument as the native tuple, or None for no enhancement: ``None`` /
    ``False``, ``True`` (the defaults) or a dict with any of ``tile``, ``clip``, ``strength``."""
    if enhance is None or enhance is False:
        return None
    if enhance is True:
        return to_native(defaults=defaults)
    if not isinstance(enhance, dict) or set(enhance) - set(DEFAULTS):
        raise ValueError("enhance must be true, false or a dict of tile, clip and strength")
    return to_native(enhance.get("tile"), enhance.get("clip"), enhance.get("strength"), defaults)
