"""Views of a fisheye or wide-angle camera as the public interface spells them, and the meshes the
native layer samples a frame through (csrc/vep/dewarp.h has the arithmetic, docs/DEWARP.md the
reasoning). Control plane: numpy float64, built once per (lens, view, source size).

A **lens** is a dict. ``model`` is ``"equidistant"`` (r = f theta), ``"equisolid"``
(r = 2 f sin(theta / 2)), ``"stereographic"`` (r = 2 f tan(theta / 2)) or ``"brown"`` (the
Brown-Conrady polynomial). ``cx, cy`` is the optical centre in 1/10000 of the picture's width and
height (default 5000, 5000), so a lens survives a resolution change. The fisheye models take
``radius``, the image circle's radius in 1/10000 of the picture's WIDTH (default 5000), and
``fov_deg``, the field of view across that circle (default 180): f follows from r(fov / 2) = radius.
``brown`` takes ``fx, fy`` (focal lengths in 1/10000 of the width and height) and the coefficients
``k1, k2, k3, p1, p2`` (default 0).

A **view** is a dict with ``width`` and ``height`` (1..4096) and a ``type``:

* ``"ptz"``: a rectilinear virtual camera looking ``pan`` degrees right and ``tilt`` degrees up,
  rolled by ``roll``, with a horizontal field of view ``fov`` (degrees, 0 < fov < 180, default 90).
  ``mount`` is ``"wall"`` (pan turns about the vertical, angles 0: along the lens axis) or
  ``"ceiling"`` (the lens looks down, pan turns about the lens axis, tilt 0 is the horizon and
  -90 straight down). With zero angles on a ``brown`` lens this is the undistorted picture.
* ``"panorama"``: azimuth ``pan0 .. pan1`` linear in the column, elevation ``tilt0`` (top row)
  ``.. tilt1`` linear in the row, ``mount`` as above.

Rays that leave the lens's field land outside the picture and become the pad colour.

A mesh is ``int32[mesh_h, mesh_w, 2]``: node ``(n, m)`` holds the source position ``(sx, sy)`` of
the centre of output pixel ``(8 m, 8 n)`` in 1/256 of a source pixel, 0 the centre of pixel 0.
"""
from __future__ import annotations

import math

import numpy as np

CELL = 8
MAX_OUT = 4096
MAX_SRC = 8192
UNIT = 10000
SUB = 256                                  # mesh units per source pixel
NODE_LO, NODE_HI = -MAX_SRC * SUB, 2 * MAX_SRC * SUB  # [lo, hi): the native clamp
FISHEYE = ("equidistant", "equisolid", "stereographic")
MODELS = FISHEYE + ("brown",)
MOUNTS = ("wall", "ceiling")
_LENS_DEFAULTS = {"cx": 5000, "cy": 5000, "radius": 5000, "fov_deg": 180.0}
_BROWN_DEFAULTS = {"cx": 5000, "cy": 5000, "k1": 0.0, "k2": 0.0, "k3": 0.0, "p1": 0.0, "p2": 0.0}
_PTZ_DEFAULTS = {"pan": 0.0, "tilt": 0.0, "roll": 0.0, "fov": 90.0, "mount": "wall"}
_PANO_DEFAULTS = {"mount": "wall"}


def _num(v, what, lo=-math.inf, hi=math.inf):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not lo <= v <= hi:
        raise ValueError(f"{what} must be a number in [{lo}, {hi}], got {v!r}")
    return float(v)


def _fields(d, what, required, defaults):
    if not isinstance(d, dict):
        raise ValueError(f"a {what} must be a dict, got {type(d).__name__}")
    unknown = set(d) - set(required) - set(defaults)
    if unknown:
        raise ValueError(f"unknown {what} field(s): {sorted(unknown)}")
    for k in required:
        if k not in d:
            raise ValueError(f"{what} field {k} is missing")
    return {**defaults, **d}


def mesh_shape(width: int, height: int) -> tuple:
    return ((height + CELL - 1) // CELL + 1, (width + CELL - 1) // CELL + 1, 2)


def size(width, height, limit=MAX_OUT, what="view") -> tuple:
    for v, name in ((width, "width"), (height, "height")):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= limit:
            raise ValueError(f"{what} {name} must be an integer 1..{limit}")
    return width, height


def check_lens(lens) -> dict:
    """The lens with its defaults filled in; ``ValueError`` unless it is valid."""
    model = lens.get("model") if isinstance(lens, dict) else None
    if model not in MODELS:
        raise ValueError(f"lens model must be one of {MODELS}, got {model!r}")
    if model == "brown":
        out = _fields(lens, "lens", ("model", "fx", "fy"), _BROWN_DEFAULTS)
        for k in ("fx", "fy"):
            out[k] = _num(out[k], f"lens {k}", 1, 100 * UNIT)
        for k in ("k1", "k2", "k3", "p1", "p2"):
            out[k] = _num(out[k], f"lens {k}", -1e6, 1e6)
    else:
        out = _fields(lens, "lens", ("model",), _LENS_DEFAULTS)
        out["radius"] = _num(out["radius"], "lens radius", 1, 10 * UNIT)
        out["fov_deg"] = _num(out["fov_deg"], "lens fov_deg", 1, 360 if model != "stereographic" else 359)
    for k in ("cx", "cy"):
        out[k] = _num(out[k], f"lens {k}", -UNIT, 2 * UNIT)
    return out


def check_view(view) -> dict:
    """The view with its defaults filled in; ``ValueError`` unless it is valid."""
    kind = view.get("type") if isinstance(view, dict) else None
    if kind == "ptz":
        out = _fields(view, "view", ("type", "width", "height"), _PTZ_DEFAULTS)
        for k in ("pan", "tilt", "roll"):
            out[k] = _num(out[k], f"view {k}", -360, 360)
        out["fov"] = _num(out["fov"], "view fov", 0.1, 179.9)
    elif kind == "panorama":
        out = _fields(view, "view", ("type", "width", "height", "pan0", "pan1", "tilt0", "tilt1"), _PANO_DEFAULTS)
        for k in ("pan0", "pan1"):
            out[k] = _num(out[k], f"view {k}", -360, 360)
        for k in ("tilt0", "tilt1"):
            out[k] = _num(out[k], f"view {k}", -90, 90)
        if out["pan0"] == out["pan1"] or out["tilt0"] == out["tilt1"]:
            raise ValueError("a panorama needs pan0 != pan1 and tilt0 != tilt1")
    else:
        raise ValueError(f"view type must be 'ptz' or 'panorama', got {kind!r}")
    if out["mount"] not in MOUNTS:
        raise ValueError(f"view mount must be one of {MOUNTS}, got {out['mount']!r}")
    size(out["width"], out["height"])
    return out


def check_views(views) -> dict:
    """A camera's stored views ``{name: view}``, each checked."""
    if not isinstance(views, dict):
        raise ValueError("views must be a dict {name: view}")
    for n in views:
        if not isinstance(n, str) or not n:
            raise ValueError("a view's name must be a non-empty string")
    return {n: check_view(v) for n, v in views.items()}


def radius_of(lens: dict, theta, src_w: int):
    """r(theta) of a fisheye lens in source pixels."""
    big = lens["radius"] / UNIT * src_w
    half = math.radians(lens["fov_deg"]) / 2
    if lens["model"] == "equidistant":
        return big / half * theta
    if lens["model"] == "equisolid":
        return big / math.sin(half / 2) * np.sin(theta / 2)
    return big / math.tan(half / 2) * np.tan(np.minimum(theta, math.pi - 1e-6) / 2)  # stereographic


def _rot(axis: str, deg: float) -> np.ndarray:
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array({"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]],
                     "z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis], np.float64)


def rays(view: dict, xs, ys) -> np.ndarray:
    """``[len(ys), len(xs), 3]``: the unit-free rays, in the lens's frame (x right, y down, z along
    the lens axis), through the centres of output pixels ``xs`` x ``ys`` of a checked view."""
    x, y = np.meshgrid(np.asarray(xs, np.float64) + 0.5, np.asarray(ys, np.float64) + 0.5)
    w, h, ceiling = view["width"], view["height"], view["mount"] == "ceiling"
    if view["type"] == "ptz":
        f = w / 2 / math.tan(math.radians(view["fov"]) / 2)
        d = np.stack([x - w / 2, y - h / 2, np.full_like(x, f)], -1)
        turn = (_rot("z", view["pan"]) @ _rot("x", view["tilt"] + 90)) if ceiling else (
            _rot("y", view["pan"]) @ _rot("x", view["tilt"]))
        return d @ (turn @ _rot("z", view["roll"])).T
    az = np.radians(view["pan0"] + x / w * (view["pan1"] - view["pan0"]))
    el = np.radians(view["tilt0"] + y / h * (view["tilt1"] - view["tilt0"]))
    if ceiling:  # azimuth about the lens axis, elevation 0 the horizon (image-up at azimuth 0)
        return np.stack([np.cos(el) * np.sin(az), -np.cos(el) * np.cos(az), -np.sin(el)], -1)
    return np.stack([np.cos(el) * np.sin(az), -np.sin(el), np.cos(el) * np.cos(az)], -1)


def project(lens: dict, d: np.ndarray, src_w: int, src_h: int) -> np.ndarray:
    """``[..., 2]`` float64: where rays ``d`` of the lens's frame land, in source pixels (0 the
    centre of pixel 0). A ray a ``brown`` lens cannot see (z <= 0) is NaN."""
    cx, cy = lens["cx"] / UNIT * src_w - 0.5, lens["cy"] / UNIT * src_h - 0.5
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    if lens["model"] == "brown":
        with np.errstate(divide="ignore", invalid="ignore"):
            a, b = np.where(z > 0, x / z, np.nan), np.where(z > 0, y / z, np.nan)
        r2 = a * a + b * b
        rad = 1 + r2 * (lens["k1"] + r2 * (lens["k2"] + r2 * lens["k3"]))
        u = a * rad + 2 * lens["p1"] * a * b + lens["p2"] * (r2 + 2 * a * a)
        v = b * rad + lens["p1"] * (r2 + 2 * b * b) + 2 * lens["p2"] * a * b
        return np.stack([cx + lens["fx"] / UNIT * src_w * u, cy + lens["fy"] / UNIT * src_h * v], -1)
    rho = np.hypot(x, y)
    r = radius_of(lens, np.arctan2(rho, z), src_w)
    with np.errstate(divide="ignore", invalid="ignore"):
        ux, uy = np.where(rho > 0, x / rho, 0.0), np.where(rho > 0, y / rho, 0.0)
    return np.stack([cx + r * ux, cy + r * uy], -1)


def positions(lens, view, src_w: int, src_h: int, xs, ys) -> np.ndarray:
    """The exact source positions (float64 pixels) of output pixels ``xs`` x ``ys``."""
    return project(check_lens(lens), rays(check_view(view), xs, ys), src_w, src_h)


def quantize(pos: np.ndarray) -> np.ndarray:
    """Float positions in pixels as mesh words: rounded to 1/256, clamped as the native layer
    clamps, NaN far outside."""
    q = np.rint(np.nan_to_num(pos * SUB, nan=NODE_LO, posinf=NODE_HI, neginf=NODE_LO))
    return np.clip(q, NODE_LO, NODE_HI - 1).astype(np.int32)


def build_mesh(lens, view, src_w: int, src_h: int) -> np.ndarray:
    """``int32[mesh_h, mesh_w, 2]``: the mesh of ``view`` through ``lens`` for a ``src_w x src_h``
    picture."""
    size(src_w, src_h, MAX_SRC, "source")
    view = check_view(view)
    mh, mw, _ = mesh_shape(view["width"], view["height"])
    return quantize(positions(lens, view, src_w, src_h, np.arange(mw) * CELL, np.arange(mh) * CELL))


def identity_mesh(width: int, height: int) -> np.ndarray:
    """The mesh under which a ``width x height`` view of a picture of that size is the picture."""
    size(width, height)
    mh, mw, _ = mesh_shape(width, height)
    x, y = np.meshgrid(np.arange(mw) * CELL * SUB, np.arange(mh) * CELL * SUB)
    return np.stack([x, y], -1).astype(np.int32)


def interpolate(mesh: np.ndarray, width: int, height: int) -> np.ndarray:
    """``int64[height, width, 2]``: the position of every output pixel as the native layer
    interpolates the mesh (dewarp.h), in 1/256 px."""
    n = np.clip(mesh.astype(np.int64), NODE_LO, NODE_HI - 1)
    j, k = np.meshgrid(np.arange(width), np.arange(height))
    m, a, r, b = j // CELL, (j % CELL)[..., None], k // CELL, (k % CELL)[..., None]
    s = (CELL - a) * (CELL - b) * n[r, m] + a * (CELL - b) * n[r, m + 1] + (CELL - a) * b * n[r + 1, m] + a * b * n[r + 1, m + 1]
    return (s + CELL * CELL // 2) // (CELL * CELL)


def mesh_error(lens, view, src_w: int, src_h: int) -> float:
    """The largest distance, in source pixels, between the mesh-interpolated and the exact position
    over the output pixels whose exact position lies inside the picture."""
    view = check_view(view)
    w, h = view["width"], view["height"]
    exact = positions(lens, view, src_w, src_h, np.arange(w), np.arange(h))
    got = interpolate(build_mesh(lens, view, src_w, src_h), w, h) / SUB
    inside = (exact[..., 0] >= -0.5) & (exact[..., 0] < src_w - 0.5) & (exact[..., 1] >= -0.5) & (exact[..., 1] < src_h - 0.5)
    return float(np.hypot(*np.moveaxis(got - exact, -1, 0))[inside].max()) if inside.any() else 0.0


def to_native(mesh, width: int, height: int) -> np.ndarray:
    """A mesh as the native layer takes it: C-contiguous int32 of ``mesh_shape(width, height)``."""
    size(width, height)
    if not isinstance(mesh, np.ndarray) or mesh.dtype != np.int32 or mesh.shape != mesh_shape(width, height):
        raise ValueError(f"the mesh must be an int32 array of shape {mesh_shape(width, height)}")
    return np.ascontiguousarray(mesh)
