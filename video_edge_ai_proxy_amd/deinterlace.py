"""Motion-adaptive deinterlacing of interlaced cameras (csrc/vep/deinterlace.h, docs/DEINTERLACE.md):
the parameters as clients give them, and as the native layer takes them.

``order``     ``"tff"`` (top field first, the default: the even rows are the earlier field) or ``"bff"``
``temporal``  true (the default): bound the spatial prediction by the frame before; false: spatial only
"""
from __future__ import annotations

DEFAULTS = {"order": "tff", "temporal": True}
ORDERS = {"tff": 0, "bff": 1}


def to_native(order=None, temporal=None, defaults=None) -> tuple:
    """``(order, temporal)`` as two ints (None: ``defaults``' value, which itself defaults to
    :data:`DEFAULTS`); a bad value is a ``ValueError``."""
    d = dict(DEFAULTS, **(defaults or {}))
    order = d["order"] if order is None else order
    if not isinstance(order, str) or order not in ORDERS:
        raise ValueError("order must be tff or bff")
    temporal = d["temporal"] if temporal is None else temporal
    if temporal not in (True, False, 0, 1) or isinstance(temporal, float):
        raise ValueError("temporal must be true or false")
    return ORDERS[order], int(temporal)


def from_request(deinterlace, defaults=None):
    """A call's ``deinterlace`` argument as the native tuple, or None for no deinterlacing:
    ``None`` / ``False``, ``True`` (the defaults) or a dict with ``order`` and / or ``temporal``."""
    if deinterlace is None or deinterlace is False:
        return None
    if deinterlace is True:
        return to_native(defaults=defaults)
    if not isinstance(deinterlace, dict) or set(deinterlace) - set(DEFAULTS):
        raise ValueError("deinterlace must be true, false or a dict of order and temporal")
    return to_native(deinterlace.get("order"), deinterlace.get("temporal"), defaults)
