"""Dehazing of fog, haze and smoke (dark-channel prior; csrc/vep/dehaze.h, docs/DEHAZE.md): the
parameters as clients give them, and as the native layer takes them.

``patch``     side of the dark channel's window in pixels, odd, 3..31 (default 15)
``omega``     0..1: how much of the veil is taken off (default 0.95)
``t0``        0.05..1: the floor of the transmission, which bounds the gain (default 0.1)
``radius``    radius of the edge-aware refinement in cells of 4 x 4 pixels, 1..16 (default 8)
``strength``  0..1: how much of the dehazed picture is taken (default 1.0; 0 is the identity)
"""
from __future__ import annotations

from .enhance import _number

DEFAULTS = {"patch": 15, "omega": 0.95, "t0": 0.1, "radius": 8, "strength": 1.0}


def _integer(v, what: str, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f"{what} must be an integer {lo}..{hi}")
    return v


def to_native(patch=None, omega=None, t0=None, radius=None, strength=None, defaults=None) -> tuple:
    """``(patch, omega256, t0_1024, radius, strength256)`` of the five parameters (None:
    ``defaults``' value, which itself defaults to :data:`DEFAULTS`); a bad value is a ``ValueError``."""
    d = dict(DEFAULTS, **(defaults or {}))
    patch = _integer(d["patch"] if patch is None else patch, "patch", 3, 31)
    if patch % 2 == 0:
        raise ValueError("patch must be odd")
    omega = _number(d["omega"] if omega is None else omega, "omega")
    if not 0.0 <= omega <= 1.0:
        raise ValueError("omega must be 0..1")
    t0 = _number(d["t0"] if t0 is None else t0, "t0")
    if not 0.05 <= t0 <= 1.0:
        raise ValueError("t0 must be 0.05..1")
    radius = _integer(d["radius"] if radius is None else radius, "radius", 1, 16)
    strength = _number(d["strength"] if strength is None else strength, "strength")
    if not 0.0 <= strength <= 1.0:
        raise ValueError("strength must be 0..1")
    return patch, int(round(omega * 256)), int(round(t0 * 1024)), radius, int(round(strength * 256))


def from_request(dehaze, defaults=None):
    """A call's ``dehaze`` argument as the native tuple, or None for no dehazing: ``None`` /
    ``False``, ``True`` (the defaults) or a dict with any of the five parameters."""
    if dehaze is None or dehaze is False:
        return None
    if dehaze is True:
        return to_native(defaults=defaults)
    if not isinstance(dehaze, dict) or set(dehaze) - set(DEFAULTS):
        raise ValueError("dehaze must be true, false or a dict of patch, omega, t0, radius and strength")
    return to_native(*(dehaze.get(k) for k in DEFAULTS), defaults)


def split_planes(words, width: int, height: int) -> dict:
    """The five planes of one picture out of its buffer of u32 words (a numpy array or a tensor,
    as ``native.dehaze_cpu`` and ``ops.dehaze_batch(planes=True)`` return it): ``table``
    ``[256, 4]`` (count and the sums of B, G and R per bin), ``air`` ``[4]`` (A and the pixel count),
    ``norm`` (196 - 4 words: the three tables' bytes), ``ab`` and ``mean`` ``[ch, cw, 2]`` (signed),
    ``cell`` ``[ch, cw]`` (Yc | Tc << 16)."""
    cw, ch = -(-width // 4), -(-height // 4)
    n, at, out = cw * ch, 0, {}
    for name, count, shape in (("table", 1024, (256, 4)), ("air", 4, (4,)), ("norm", 192, (192,)), ("ab", 2 * n, (ch, cw, 2)),
                               ("mean", 2 * n, (ch, cw, 2)), ("cell", n, (ch, cw))):
        out[name] = words[at:at + count].reshape(shape)
        at += count
    return out
