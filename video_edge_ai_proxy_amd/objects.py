"""Per-camera moving-object boxes (csrc/vep/objects.h, docs/OBJECTS.md): the parameters of the
``objects:`` config section, checked as the native layer checks them.

``decimate``     the luma plane's decimation, 1, 2 or 4 (default 2)
``threshold``    a sample differs when its lumas are further apart than this, 0..255 (default 24)
``gap``          how many frames the earlier frame lies before the newest, 1..7 (default 1)
``open``         1: a 3 x 3 erosion and dilation remove specks, 0: none (default 1)
``grow``         the radius of the final square dilation, 0..3 (default 1)
``min_area``     samples a region needs to be reported, 4..65535 (default 64)
``max_objects``  the largest regions listed in an answer, 1..1024 (default 32)

The defaults are design choices, not measured thresholds.
"""
from __future__ import annotations

DEFAULTS = {"decimate": 2, "threshold": 24, "gap": 1, "open": 1, "grow": 1, "min_area": 64, "max_objects": 32}
_RANGES = {"threshold": (0, 255), "gap": (1, 7), "open": (0, 1), "grow": (0, 3), "min_area": (4, 65535),
           "max_objects": (1, 1024)}
LABEL_KEYS = ("decimate", "threshold", "open", "grow", "min_area")


def _integer(v, what: str, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f"objects: {what} must be an integer {lo}..{hi}")
    return v


def check_label(decimate, threshold, open, grow, min_area) -> tuple:
    """The labelling's parameters checked; a bad value is a ``ValueError``."""
    if isinstance(decimate, bool) or decimate not in (1, 2, 4):
        raise ValueError("objects: decimate must be 1, 2 or 4")
    vals = {"threshold": threshold, "open": open, "grow": grow, "min_area": min_area}
    return (int(decimate),) + tuple(_integer(v, k, *_RANGES[k]) for k, v in vals.items())


def to_native(params=None) -> dict:
    """The section (None or a dict with any of :data:`DEFAULTS`' keys) as the keyword arguments of
    ``Worker.set_objects_params``; an unknown key or a bad value is a ``ValueError``."""
    params = dict(params or {})
    if set(params) - set(DEFAULTS):
        raise ValueError(f"objects: unknown parameter {sorted(set(params) - set(DEFAULTS))[0]}")
    d = dict(DEFAULTS, **params)
    check_label(*(d[k] for k in LABEL_KEYS))
    for k, (lo, hi) in _RANGES.items():
        _integer(d[k], k, lo, hi)
    return d


def response(r: dict) -> dict:
    """A native objects answer as the REST response (docs/OBJECTS.md): boxes are ``[x, y, w, h]`` in
    picture pixels, areas in samples of the decimated plane."""
    return {
        "seq": r["seq"], "prev_seq": r["prev_seq"], "primed": r["primed"], "width": r["width"], "height": r["height"],
        "decimate": r["decimate"], "count": r["count"], "truncated": r["truncated"], "area": r["area"],
        "objects": [{"label": o["label"], "area": o["area"], "box": list(o["box"])} for o in r["objects"]],
        "box": None if r["box"] is None else list(r["box"]), "motion": r["motion"],
    }


def crop_boxes(answer: dict) -> list:
    """The answer's boxes as ``x0,y0,x1,y1`` strings in 1/10000 of the picture, the form ``vep crop
    --box`` takes: rounded outwards, so a crop never loses a sample of its region."""
    pw, ph = max(int(answer.get("width") or 0), 1), max(int(answer.get("height") or 0), 1)
    out = []
    for o in answer.get("objects") or []:
        x, y, w, h = o["box"]
        out.append("{},{},{},{}".format(x * 10000 // pw, y * 10000 // ph, min(10000, -(-(x + w) * 10000 // pw)),
                                        min(10000, -(-(y + h) * 10000 // ph))))
    return out
