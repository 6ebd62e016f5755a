"""Per-camera motion vectors by block matching (csrc/vep/flow.h, docs/FLOW.md): the parameters of
the ``flow:`` config section, checked as the native layer checks them.

``decimate``        the luma plane's decimation, 1, 2 or 4 (default 2)
``range``           the search range in samples of the plane, 1..15 (default 7)
``gap``             how many frames the earlier frame lies before the newest, 1..7 (default 1)
``min_gain``        a block moves when its SAD fell by this much per sample, 0..255 (default 4)
``min_blocks``      moving blocks that make ``motion`` true, >= 1 (default 4)
``global_percent``  the share of one vector that makes ``camera_moved`` true, 1..100 (default 60)

The defaults are design choices, not measured thresholds.
"""
from __future__ import annotations

DEFAULTS = {"decimate": 2, "range": 7, "gap": 1, "min_gain": 4, "min_blocks": 4, "global_percent": 60}
_RANGES = {"range": (1, 15), "gap": (1, 7), "min_gain": (0, 255), "min_blocks": (1, 1 << 30), "global_percent": (1, 100)}


def _integer(v, what: str, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f"flow: {what} must be an integer {lo}..{hi}")
    return v


def check_match(decimate, range) -> tuple:
    """``(decimate, range)`` checked; a bad value is a ``ValueError``."""
    if isinstance(decimate, bool) or decimate not in (1, 2, 4):
        raise ValueError("flow: decimate must be 1, 2 or 4")
    return int(decimate), _integer(range, "range", *_RANGES["range"])


def to_native(params=None) -> dict:
    """The section (None or a dict with any of :data:`DEFAULTS`' keys) as the keyword arguments of
    ``Worker.set_flow_params``; an unknown key or a bad value is a ``ValueError``."""
    params = dict(params or {})
    if set(params) - set(DEFAULTS):
        raise ValueError(f"flow: unknown parameter {sorted(set(params) - set(DEFAULTS))[0]}")
    d = dict(DEFAULTS, **params)
    check_match(d["decimate"], d["range"])
    for k, (lo, hi) in _RANGES.items():
        _integer(d[k], k, lo, hi)
    return d


def response(r: dict, grid: bool = False) -> dict:
    """A native flow answer as the REST response (docs/FLOW.md)."""
    g = r["grid"]
    out = {
        "seq": r["seq"], "prev_seq": r["prev_seq"], "primed": r["primed"], "blocks": [r["cols"], r["rows"]],
        "block_px": r["block_px"], "moving": r["moving"], "mean": [round(v, 3) for v in r["mean"]], "dirs": list(r["dirs"]),
        "box": None if r["box"] is None else list(r["box"]), "motion": r["motion"],
        "global": {k: r["global"][k] for k in ("vx", "vy", "percent")}, "camera_moved": r["camera_moved"],
    }
    if grid:
        for i, k in enumerate(("vx", "vy", "best", "zero")):
            out[k] = g[:, :, i].ravel().tolist()
    return out
