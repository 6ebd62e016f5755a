"""Upright pictures of cameras mounted sideways, upside down or behind a mirror
(csrc/vep/orient.h, docs/ORIENT.md): the orientation as clients give it, and as the native layer
takes it.

``rotate``  0 (the default), 90, 180 or 270 degrees clockwise
``flip``    ``"none"`` (the default), ``"h"`` (left-right) or ``"v"`` (top-bottom), applied to the
            rotated picture
"""
from __future__ import annotations

DEFAULTS = {"rotate": 0, "flip": "none"}
ROTATES = (0, 90, 180, 270)
FLIPS = {"none": 0, "h": 1, "v": 2}


def to_native(rotate=None, flip=None) -> tuple:
    """``(rotate, flip)`` as two ints (None: the default); a bad value is a ``ValueError``."""
    rotate = DEFAULTS["rotate"] if rotate is None else rotate
    if isinstance(rotate, bool) or not isinstance(rotate, int) or rotate not in ROTATES:
        raise ValueError("rotate must be 0, 90, 180 or 270")
    flip = DEFAULTS["flip"] if flip is None else flip
    if not isinstance(flip, str) or flip not in FLIPS:
        raise ValueError("flip must be none, h or v")
    return rotate, FLIPS[flip]


def from_request(orient, mounting=None):
    """A call's ``orient`` argument as the native tuple, or None where the sensor picture is served:
    ``None`` takes the camera's ``mounting`` (its entry of the config's ``orient:`` section, if any);
    a dict with ``rotate`` and / or ``flip`` is the request's own orientation, the identity
    included, whatever the mounting."""
    if orient is None:
        orient = mounting or {}
    if not isinstance(orient, dict) or set(orient) - set(DEFAULTS):
        raise ValueError("orient must be a dict of rotate and flip")
    native = to_native(orient.get("rotate"), orient.get("flip"))
    return None if native == (0, 0) else native


def header(native) -> str:
    """``<rotate>[,<flip>]`` of a native tuple (``X-Vep-Orient``, ``meta["orient"]``)."""
    flip = next(k for k, v in FLIPS.items() if v == native[1])
    return str(native[0]) if flip == "none" else f"{native[0]},{flip}"


def check_mountings(cameras) -> None:
    """The config's ``orient.cameras``: ``{name: {rotate, flip}}``; a bad entry is a ``ValueError``."""
    if not isinstance(cameras, dict):
        raise ValueError("cameras must map a camera's name to its rotate and flip")
    for name, entry in cameras.items():
        if not isinstance(entry, dict) or set(entry) - set(DEFAULTS):
            raise ValueError(f"cameras.{name} must be a dict of rotate and flip")
        try:
            to_native(entry.get("rotate"), entry.get("flip"))
        except ValueError as e:
            raise ValueError(f"cameras.{name}: {e}") from None
