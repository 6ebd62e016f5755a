"""Temporal denoising of served frames from a camera's history (csrc/vep/denoise.h,
docs/DENOISE.md): the parameters as clients give them, and as the native layer takes them.

``frames``    how many of the ring's newest frames are blended, 2..8 (default 4)
``level``     the noise floor in luma levels, 1..64 (default 8): an earlier frame counts fully where
              it differs from the newest by at most this on average, not at all from twice this
``strength``  0..1: how much an earlier frame may weigh (default 1.0; 0 is the identity)
"""
from __future__ import annotations

DEFAULTS = {"frames": 4, "level": 8, "strength": 1.0}


def _integer(v, what: str, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f"{what} must be an integer {lo}..{hi}")
    return v


def to_native(frames=None, level=None, strength=None, defaults=None) -> tuple:
    """``(frames, level, strength256)`` of the three parameters (None: ``defaults``' value, which
    itself defaults to :data:`DEFAULTS`); a bad value is a ``ValueError``."""
    d = dict(DEFAULTS, **(defaults or {}))
    frames = _integer(d["frames"] if frames is None else frames, "frames", 2, 8)
    level = _integer(d["level"] if level is None else level, "level", 1, 64)
    strength = d["strength"] if strength is None else strength
    if isinstance(strength, bool) or not isinstance(strength, (int, float)) or not 0.0 <= strength <= 1.0:
        raise ValueError("strength must be a number 0..1")
    return frames, level, int(round(float(strength) * 256))


def from_request(denoise, defaults=None):
    """A call's ``denoise`` argument as the native tuple, or None for no denoising: ``None`` /
    ``False``, ``True`` (the defaults) or a dict with any of ``frames``, ``level``, ``strength``."""
    if denoise is None or denoise is False:
        return None
    if denoise is True:
        return to_native(defaults=defaults)
    if not isinstance(denoise, dict) or set(denoise) - set(DEFAULTS):
        raise ValueError("denoise must be true, false or a dict of frames, level and strength")
    return to_native(denoise.get("frames"), denoise.get("level"), denoise.get("strength"), defaults)
