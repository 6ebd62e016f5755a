"""REST API (``/api/v1``), static portal and Prometheus metrics.

Reference parity: server/router/config_routes.go:25-50 (CORS ``*`` + six routes),
server/api/rtsp_process.go:39-106, api/settings.go:38-62, api/error.go:20-31:

  POST   /api/v1/process          400 bad JSON / missing rtsp_endpoint, 409 start failure, 200
  DELETE /api/v1/process/{name}   400 / 409 / 200
  GET    /api/v1/process/{name}   400 / 200 + StreamProcess JSON
  GET    /api/v1/processlist      500 / 200 + [StreamProcess]
  GET    /api/v1/settings         500 / 200 + Settings
  POST   /api/v1/settings         400 / 500 / 202
Errors are ``{"code": int, "message": str}``. New: ``/metrics`` (Prometheus), ``/healthz``,
``GET /api/v1/process/{name}/frame`` (latest frame as PPM), ``.../frame.jpg`` (the same frame
as a JPEG, encoded on the camera's GPU) and ``.../stream.mjpg`` (live MJPEG, one part per new
frame), both with ``?width=&height=`` for a picture fitted into that box and downscaled on the GPU,
``/api/v1/wall.jpg`` / ``wall.mjpg`` / ``wall`` (one picture of many cameras and its geometry,
docs/WALL.md), ``/api/v1/process/{name}/motion`` and ``/api/v1/motion`` (did anything change:
motion detection on the GPU, docs/MOTION.md; ``DELETE .../motion`` resets the background),
``/api/v1/process/{name}/tamper`` and ``/api/v1/tamper`` (does the camera still show what it should:
tamper detection on the GPU, docs/TAMPER.md; ``PUT .../tamper/reference`` declares the newest frame
normal, ``DELETE .../tamper`` forgets it), ``POST /api/v1/process/{name}/crops`` and
``GET .../crop.jpg`` (boxes of a frame cut and resized on the GPU, docs/CROPS.md),
``PUT / GET / DELETE /api/v1/process/{name}/overlay`` (a camera's stored on-screen display list,
drawn with ``frame.jpg?overlay=1&stamp=1`` and ``wall.jpg?labels=1``, docs/OVERLAY.md), and the portal itself at ``/`` (replaces the Angular build, which needs a node
toolchain).
"""
from __future__ import annotations

import json
import logging
import time
from pathlib import Path

from fastapi import FastAPI, Request
from fastapi.middleware.cors import CORSMiddleware
from fastapi.responses import HTMLResponse, JSONResponse, Response, StreamingResponse

from .. import overlay as overlay_items
from ..models import Settings, StreamProcess
from ..services.process_manager import ProcessError, ProcessManager
from ..services.settings import SettingsManager

log = logging.getLogger("vep.rest")
PORTAL = Path(__file__).with_name("portal.html")
MJPEG_BOUNDARY = "vepframe"
MJPEG_IDLE_S = 10.0  # a stream whose camera publishes nothing for this long ends


def err(code: int, message: str) -> JSONResponse:
    return JSONResponse(status_code=code, content={"code": code, "message": message})


def create_app(pm: ProcessManager, sm: SettingsManager, metrics=None) -> FastAPI:
    app = FastAPI(title="vep", docs_url=None, redoc_url=None, openapi_url=None)
    app.add_middleware(CORSMiddleware, allow_origins=["*"], allow_methods=["*"], allow_headers=["*"],
                       allow_credentials=False)

    async def body_json(request: Request):
        raw = await request.body()
        try:
            data = json.loads(raw or b"null")
        except ValueError as e:
            raise ValueError(f"invalid JSON: {e}")
        if not isinstance(data, dict):
            raise ValueError("JSON object expected")
        return data

    @app.post("/api/v1/process")
    async def start_process(request: Request):
        try:
            sp = StreamProcess.from_json(await body_json(request))
        except ValueError as e:
            return err(400, str(e))
        if not sp.rtsp_endpoint:
            return err(400, "RTSP endpoint required")
        from ..models import RTMPStreamStatus

        sp.rtmp_stream_status = RTMPStreamStatus(streaming=True, storing=False)
        try:
            pm.start(sp)
        except ProcessError as e:
            return err(409, str(e))
        return Response(status_code=200)

    @app.delete("/api/v1/process/{name}")
    def stop_process(name: str):
        if not name:
            return err(400, "required device_id")
        try:
            pm.stop(name)
        except ProcessError as e:
            return err(409, str(e))
        return Response(status_code=200)

    @app.get("/api/v1/process/{name}")
    def info(name: str):
        try:
            return pm.info(name).to_json()
        except ProcessError as e:
            return err(400, str(e))

    @app.get("/api/v1/process/{name}/frame")
    def frame(name: str):
        try:
            pm.hub.touch(name)
            r = pm.hub.latest_frame(name, 0)
        except KeyError:
            return err(404, f"process {name!r} not found")
        if r is None:
            return err(404, "no frame decoded yet")
        meta, img = r
        h, w = img.shape[:2]
        ppm = f"P6 {w} {h} 255\n".encode() + img[:, :, ::-1].tobytes()  # BGR -> RGB
        return Response(content=ppm, media_type="image/x-portable-pixmap")

    def jpeg_quality(quality):
        if quality is None:
            return None
        if not 1 <= quality <= 100:
            raise ValueError("quality must be 1..100")
        return quality

    def box(width, height) -> dict:
        """The scaling arguments of latest_jpeg: none when the request names no size, so an
        unscaled request calls the hub exactly as before."""
        for v, what in ((width, "width"), (height, "height")):
            if v is not None and not 1 <= v <= 65535:
                raise ValueError(f"{what} must be 1..65535")
        if width is None and height is None:
            return {}
        return {"width": width, "height": height}

    def osd(overlay, stamp) -> dict:
        """The overlay arguments of latest_jpeg: none when the request names neither, so such a
        request calls the hub exactly as before."""
        for v, what in ((overlay, "overlay"), (stamp, "stamp")):
            if v not in (0, 1):
                raise ValueError(f"{what} must be 0 or 1")
        if not (overlay or stamp):
            return {}
        return {"overlay": True if overlay else None, "stamp": bool(stamp)}

    @app.get("/api/v1/process/{name}/frame.jpg")
    def frame_jpg(name: str, quality: int | None = None, after: int = 0, width: int | None = None,
                  height: int | None = None, overlay: int = 0, stamp: int = 0):
        try:
            q = jpeg_quality(quality)
            size = box(width, height)
            size.update(osd(overlay, stamp))
        except ValueError as e:
            return err(400, str(e))
        try:
            pm.hub.touch(name)
            r = pm.hub.latest_jpeg(name, after, q, **size)
        except KeyError:
            return err(404, f"process {name!r} not found")
        except NotImplementedError as e:
            return err(501, str(e))
        except ValueError as e:
            return err(422, str(e))
        if r is None:
            return err(404, "no frame decoded yet")
        meta, jpg = r
        return Response(content=jpg, media_type="image/jpeg", headers={"X-Vep-Seq": str(meta["seq"])})

    @app.get("/api/v1/process/{name}/stream.mjpg")
    def stream_mjpg(name: str, fps: float = 10.0, frames: int | None = None, quality: int | None = None,
                    width: int | None = None, height: int | None = None, overlay: int = 0, stamp: int = 0):
        try:
            q = jpeg_quality(quality)
            size = box(width, height)
            size.update(osd(overlay, stamp))
            if not 0 < fps <= 1000:
                raise ValueError("fps must be in (0, 1000]")
            if frames is not None and frames < 1:
                raise ValueError("frames must be >= 1")
        except ValueError as e:
            return err(400, str(e))
        try:
            pm.hub.touch(name)
        except KeyError:
            return err(404, f"process {name!r} not found")
        if "stamp" in size:
            _, bad = overlay_call(pm.hub.overlay, name)  # (501 before the stream starts)
            if bad is not None:
                return bad

        def parts():
            # one part per NEW frame (the seq cursor), at most `fps` a second; every part touches
            # the camera, so its lazy decoder stays awake while someone watches
            seq, sent, last_new = 0, 0, time.monotonic()
            due = last_new
            while frames is None or sent < frames:
                try:
                    pm.hub.touch(name)
                    wait = getattr(pm.hub, "wait_frame", None)
                    if wait is not None:
                        if pm.hub.published(name) < seq:
                            seq = 0  # the camera started a new ring (restart, resolution change)
                        wait(name, seq, 500)
                    r = pm.hub.latest_jpeg(name, seq, q, **size)
                except (KeyError, ValueError):
                    return  # the camera was removed (or its stored overlay can no longer be drawn)
                now = time.monotonic()
                if r is None:
                    if now - last_new > MJPEG_IDLE_S:
                        return
                    if wait is None:
                        time.sleep(min(0.05, 1.0 / fps))
                    continue
                meta, jpg = r
                seq, last_new = meta["seq"], now
                yield (f"--{MJPEG_BOUNDARY}\r\nContent-Type: image/jpeg\r\nContent-Length: {len(jpg)}\r\n"
                       f"X-Vep-Seq: {seq}\r\n\r\n").encode() + jpg + b"\r\n"
                sent += 1
                due = max(due + 1.0 / fps, now)
                if (frames is None or sent < frames) and due > now:
                    time.sleep(due - now)

        return StreamingResponse(parts(), media_type=f"multipart/x-mixed-replace; boundary={MJPEG_BOUNDARY}")

    # ---- camera wall: one picture of many cameras, scaled and composed on the GPU (docs/WALL.md)
    def wall_args(names, cols, tile, quality, labels=0) -> dict:
        from ..config import parse_tile

        a = {"names": None, "cols": None, "tile_width": None, "tile_height": None, "quality": jpeg_quality(quality)}
        if labels not in (0, 1):
            raise ValueError("labels must be 0 or 1")
        if labels:
            a["labels"] = True  # (absent otherwise: the hub is called exactly as before)
        if names is not None:
            a["names"] = [n for n in names.split(",") if n]
            if not a["names"]:
                raise ValueError("names must list at least one camera")
        if cols is not None:
            if not 1 <= cols <= 65535:
                raise ValueError("cols must be 1..65535")
            a["cols"] = cols
        if tile is not None:
            a["tile_width"], a["tile_height"] = parse_tile(tile)
        return a

    def wall_call(fn, *args, **kw):
        """(result, None) or (None, error response) of a hub wall call."""
        try:
            return fn(*args, **kw), None
        except NotImplementedError as e:
            return None, err(501, str(e))
        except KeyError as e:
            return None, err(404, f"process {e.args[0] if e.args else ''!r} not found")
        except overlay_items.Refused as e:
            return None, err(422, str(e))
        except ValueError as e:
            # no camera running is "nothing to show" (404); everything else is a bad argument
            return None, err(404 if not pm.hub.cameras else 400, str(e))

    def wall_header(order, seqs) -> str:
        return ",".join(f"{n}:{seqs.get(n, 0)}" for n in order)

    @app.get("/api/v1/wall.jpg")
    def wall_jpg(names: str | None = None, cols: int | None = None, tile: str | None = None,
                 quality: int | None = None, labels: int = 0):
        try:
            a = wall_args(names, cols, tile, quality, labels)
        except ValueError as e:
            return err(400, str(e))
        lay, bad = wall_call(pm.hub.wall_layout, a["names"], a["cols"], a["tile_width"], a["tile_height"])
        if bad is not None:
            return bad
        a["names"] = lay[0]
        r, bad = wall_call(pm.hub.wall_jpeg, **a)
        if bad is not None:
            return bad
        seqs, jpg = r
        return Response(content=jpg, media_type="image/jpeg", headers={"X-Vep-Wall": wall_header(lay[0], seqs)})

    @app.get("/api/v1/wall")
    def wall_info(names: str | None = None, cols: int | None = None, tile: str | None = None):
        try:
            a = wall_args(names, cols, tile, None)
        except ValueError as e:
            return err(400, str(e))
        lay, bad = wall_call(pm.hub.wall_layout, a["names"], a["cols"], a["tile_width"], a["tile_height"])
        if bad is not None:
            return bad
        order, gc, gr, tw, th = lay
        tiles = []
        for t, n in enumerate(order):
            try:
                seq = int(pm.hub.published(n))
            except KeyError:
                seq = 0
            tiles.append({"name": n, "x": (t % gc) * tw, "y": (t // gc) * th, "w": tw, "h": th, "seq": seq})
        return {"cols": gc, "rows": gr, "tile": [tw, th], "tiles": tiles}

    @app.get("/api/v1/wall.mjpg")
    def wall_mjpg(names: str | None = None, cols: int | None = None, tile: str | None = None,
                  quality: int | None = None, fps: float = 10.0, frames: int | None = None, labels: int = 0):
        try:
            a = wall_args(names, cols, tile, quality, labels)
            if not 0 < fps <= 1000:
                raise ValueError("fps must be in (0, 1000]")
            if frames is not None and frames < 1:
                raise ValueError("frames must be >= 1")
        except ValueError as e:
            return err(400, str(e))
        lay, bad = wall_call(pm.hub.wall_layout, a["names"], a["cols"], a["tile_width"], a["tile_height"])
        if bad is not None:
            return bad
        a["names"] = order = lay[0]  # the cameras of the first part stay the stream's cameras

        def parts():
            # one part whenever any tile has a newer frame, at most `fps` a second; every part
            # touches the cameras it shows (Hub.wall_jpeg), so their lazy decoders stay awake
            shown, sent, last_new = None, 0, time.monotonic()
            due = last_new
            while frames is None or sent < frames:
                now = time.monotonic()
                try:
                    cur = {n: int(pm.hub.published(n)) for n in order}
                except KeyError:
                    return  # a camera was removed
                if shown is not None and all(cur[n] == shown.get(n, 0) or cur[n] == 0 for n in order):
                    if now - last_new > MJPEG_IDLE_S:
                        return
                    try:
                        for n in order:
                            pm.hub.touch(n)
                    except KeyError:
                        return
                    time.sleep(min(0.05, 1.0 / fps))
                    continue
                try:
                    seqs, jpg = pm.hub.wall_jpeg(**a)
                except (KeyError, ValueError, NotImplementedError):
                    return
                if shown is not None and seqs == shown:
                    # (published() moved for a frame the wall does not show yet)
                    time.sleep(min(0.05, 1.0 / fps))
                    if now - last_new > MJPEG_IDLE_S:
                        return
                    continue
                shown, last_new = seqs, now
                yield (f"--{MJPEG_BOUNDARY}\r\nContent-Type: image/jpeg\r\nContent-Length: {len(jpg)}\r\n"
                       f"X-Vep-Wall: {wall_header(order, seqs)}\r\n\r\n").encode() + jpg + b"\r\n"
                sent += 1
                due = max(due + 1.0 / fps, now)
                if (frames is None or sent < frames) and due > now:
                    time.sleep(due - now)

        return StreamingResponse(parts(), media_type=f"multipart/x-mixed-replace; boundary={MJPEG_BOUNDARY}")

    # ---- motion detection: evaluated on the GPU where the frames lie (docs/MOTION.md)
    @app.get("/api/v1/process/{name}/motion")
    def motion(name: str, after: int = 0, grid: int = 0):
        if after < 0 or grid not in (0, 1):
            return err(400, "after must be >= 0 and grid 0 or 1")
        try:
            r = pm.hub.motion(name, after, bool(grid))
        except KeyError:
            return err(404, f"process {name!r} not found")
        if r is None:
            return err(404, "no newer frame decoded yet")
        return JSONResponse(content=r, headers={"X-Vep-Seq": str(r["seq"])})

    @app.delete("/api/v1/process/{name}/motion")
    def motion_reset(name: str):
        try:
            pm.hub.motion_reset(name)
        except KeyError:
            return err(404, f"process {name!r} not found")
        return Response(status_code=204)

    @app.get("/api/v1/motion")
    def motion_many(names: str | None = None, grid: int = 0):
        if grid not in (0, 1):
            return err(400, "grid must be 0 or 1")
        order = None
        if names is not None:
            order = [n for n in names.split(",") if n]
            if not order:
                return err(400, "names must list at least one camera")
        elif not pm.hub.cameras:
            return err(404, "no camera running")
        try:
            res = pm.hub.motion_many(order, bool(grid))
        except KeyError as e:
            return err(404, f"process {e.args[0] if e.args else ''!r} not found")
        cams = []
        for n, r in res.items():
            cams.append({"name": n, **(r if r is not None else {"seq": 0, "motion": False})})
        return {"cameras": cams}

    # ---- tamper detection: dark, bright, flat, defocused, moved, from the ring slots (docs/TAMPER.md)
    @app.get("/api/v1/process/{name}/tamper")
    def tamper(name: str, after: int = 0, grid: int = 0, wake: int = 1):
        if after < 0 or grid not in (0, 1) or wake not in (0, 1):
            return err(400, "after must be >= 0, grid and wake 0 or 1")
        try:
            r = pm.hub.tamper(name, after, bool(grid), bool(wake))
        except KeyError:
            return err(404, f"process {name!r} not found")
        if r is None:
            return err(404, "no newer frame decoded yet")
        return JSONResponse(content=r, headers={"X-Vep-Seq": str(r["seq"])})

    @app.put("/api/v1/process/{name}/tamper/reference")
    def tamper_reference(name: str):
        try:
            ok = pm.hub.tamper_reference(name)
        except KeyError:
            return err(404, f"process {name!r} not found")
        if not ok:
            return err(404, "no frame decoded yet")
        return Response(status_code=204)

    @app.delete("/api/v1/process/{name}/tamper")
    def tamper_reset(name: str):
        try:
            pm.hub.tamper_reset(name)
        except KeyError:
            return err(404, f"process {name!r} not found")
        return Response(status_code=204)

    # ---- privacy masks: written into the ring slot before a frame is published (docs/PRIVACY.md)
    @app.get("/api/v1/process/{name}/privacy")
    def privacy_get(name: str):
        try:
            return {"masks": pm.privacy_masks(name), "unmasked_outputs": pm.unmasked_outputs(name)}
        except (KeyError, ProcessError):
            return err(404, f"process {name!r} not found")

    @app.put("/api/v1/process/{name}/privacy")
    async def privacy_put(name: str, request: Request):
        try:
            masks = json.loads(await request.body() or b"null")
            if not isinstance(masks, list):
                raise ValueError("a JSON list of masks expected")
            pm.set_privacy_masks(name, masks)
        except ValueError as e:  # (invalid JSON included)
            return err(422, str(e))
        except (KeyError, ProcessError):
            return err(404, f"process {name!r} not found")
        return Response(status_code=204)

    @app.delete("/api/v1/process/{name}/privacy")
    def privacy_delete(name: str):
        try:
            pm.set_privacy_masks(name, [])
        except (KeyError, ProcessError):
            return err(404, f"process {name!r} not found")
        return Response(status_code=204)

    # ---- on-screen display: a camera's stored list, drawn on served JPEGs (docs/OVERLAY.md)
    def overlay_call(fn, name, *args):
        try:
            return fn(name, *args), None
        except KeyError:
            return None, err(404, f"process {name!r} not found")
        except NotImplementedError as e:
            return None, err(501, str(e))
        except ValueError as e:
            return None, err(422, str(e))

    @app.get("/api/v1/process/{name}/overlay")
    def overlay_get(name: str):
        items, bad = overlay_call(pm.hub.overlay, name)
        return bad if bad is not None else {"items": items}

    @app.put("/api/v1/process/{name}/overlay")
    async def overlay_put(name: str, request: Request):
        try:
            body = json.loads(await request.body() or b"null")
            if not isinstance(body, dict) or "items" not in body or set(body) - {"items", "ttl_ms"}:
                raise ValueError('a JSON object {"items": [...], "ttl_ms": N} expected')
        except ValueError as e:
            return err(422, str(e))
        _, bad = overlay_call(pm.hub.set_overlay, name, body["items"], body.get("ttl_ms", 0))
        return bad if bad is not None else Response(status_code=204)

    @app.delete("/api/v1/process/{name}/overlay")
    def overlay_delete(name: str):
        _, bad = overlay_call(pm.hub.clear_overlay, name)
        return bad if bad is not None else Response(status_code=204)

    # ---- crops: boxes of a frame, cut and resized on the GPU in its ring slot (docs/CROPS.md)
    @app.post("/api/v1/process/{name}/crops")
    async def crops_post(name: str, request: Request):
        from starlette.concurrency import run_in_threadpool

        try:
            body = json.loads(await request.body() or b"null")
            if not isinstance(body, dict):
                raise ValueError("a JSON object expected")
            unknown = set(body) - {"boxes", "width", "height", "fit", "pad", "after", "seq"}
            if unknown:
                raise ValueError(f"unknown field(s): {sorted(unknown)}")
            for k in ("boxes", "width", "height"):
                if k not in body:
                    raise ValueError(f"field {k} is missing")
            r = await run_in_threadpool(pm.hub.crops, name, body["boxes"], body["width"], body["height"],
                                        body.get("after", 0), body.get("seq", 0), body.get("fit", "stretch"),
                                        body.get("pad"))
        except ValueError as e:  # (invalid JSON included)
            return err(422, str(e))
        except NotImplementedError as e:
            return err(501, str(e))
        except KeyError:
            return err(404, f"process {name!r} not found")
        if r is None:
            return err(404, "no such frame")
        seq, px = r
        return Response(content=px.tobytes(), media_type="application/octet-stream",
                        headers={"X-Vep-Seq": str(seq), "X-Vep-Crops": f"{px.shape[0]},{px.shape[2]},{px.shape[1]}"})

    @app.get("/api/v1/process/{name}/crop.jpg")
    def crop_jpg(name: str, box: str, width: int, height: int, fit: str = "stretch", quality: int | None = None,
                 after: int = 0, seq: int = 0):
        try:
            try:
                rect = [int(v) for v in box.split(",")]
            except ValueError:
                raise ValueError("box must be x0,y0,x1,y1") from None
            if len(rect) != 4:
                raise ValueError("box must be x0,y0,x1,y1")
            r = pm.hub.crop_jpeg(name, rect, width, height, after, seq, quality, fit)
        except ValueError as e:
            return err(422, str(e))
        except NotImplementedError as e:
            return err(501, str(e))
        except KeyError:
            return err(404, f"process {name!r} not found")
        if r is None:
            return err(404, "no such frame")
        return Response(content=r[1], media_type="image/jpeg", headers={"X-Vep-Seq": str(r[0])})

    @app.get("/api/v1/tamper")
    def tamper_many(names: str | None = None, grid: int = 0, wake: int = 1):
        if grid not in (0, 1) or wake not in (0, 1):
            return err(400, "grid and wake must be 0 or 1")
        order = None
        if names is not None:
            order = [n for n in names.split(",") if n]
            if not order:
                return err(400, "names must list at least one camera")
        elif not pm.hub.cameras:
            return err(404, "no camera running")
        try:
            res = pm.hub.tamper_many(order, bool(grid), bool(wake))
        except KeyError as e:
            return err(404, f"process {e.args[0] if e.args else ''!r} not found")
        cams = []
        for n, r in res.items():
            cams.append({"name": n, **(r if r is not None else {"seq": 0, "tampered": False, "causes": []})})
        return {"cameras": cams}

    @app.get("/api/v1/processlist")
    def plist():
        try:
            return [p.to_json() for p in pm.list()]
        except Exception as e:
            return err(500, str(e))

    @app.get("/api/v1/settings")
    def get_settings():
        try:
            return sm.get().to_json()
        except Exception as e:
            return err(500, str(e))

    @app.post("/api/v1/settings")
    async def put_settings(request: Request):
        try:
            s = Settings.from_json(await body_json(request))
        except (ValueError, TypeError) as e:
            return err(400, str(e))
        try:
            sm.overwrite(s)
        except Exception as e:
            return err(500, str(e))
        return Response(status_code=202)

    @app.get("/healthz")
    def healthz():
        from .._native import native

        out = {"ok": True, "cameras": len(pm.hub.cameras), "devices": pm.hub.devices,
               "decoder_backends": [w.decoder for w in pm.hub.workers],
               "vcn_available": bool(native.rocdecode_available()),
               "direct_host_reads": [bool(w.direct_reads) for w in pm.hub.workers],
               # per-GPU host data plane: each worker's CPU list, NUMA node and parse threads
               "host_plane": pm.hub.host_plane() if hasattr(pm.hub, "host_plane") else []}
        if metrics is not None and metrics.consumer is not None:
            out["consumer"] = metrics.consumer.stats()
        return out

    @app.get("/metrics")
    def prom():
        if metrics is None:
            return Response(status_code=404)
        body, ctype = metrics.render()
        return Response(content=body, media_type=ctype)

    @app.get("/", response_class=HTMLResponse)
    def portal():
        return PORTAL.read_text()

    return app
